"""The small d128 LLaVA and VILA models of tests/test_generate_gpu.py and tests/test_generate_vila_gpu.py, with the prompts and images of
their goldens (generate_d128.npz / generate_vila.npz), for further generation tests."""
import math

import torch

from golden_util import load_npz, meta_of, tensors
from model_util import build_product_models

LLAVA_PROMPT_LENS = (20, 33, 47)


def pad_batch(rows, pad=0):
    T = max(len(r) for r in rows)
    ids = torch.full((len(rows), T), pad, dtype=torch.long)
    mask = torch.zeros(len(rows), T, dtype=torch.bool)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
        mask[i, :len(r)] = True
    return ids, mask


def build_llava(device="cuda:0"):
    """-> (model, prompts, images [3, 3, H, W] bf16): dpa_step_d128_init's policy (2 layers, 2 heads x 128, vocab 160, LoRA r = 4)."""
    z = load_npz("dpa_step_d128_init.npz")
    model, _, _ = build_product_models(z, device=device)
    model.eval()
    ids = torch.as_tensor(z["batch.input_ids"][:3])
    prompts = [ids[i, :n].clone() for i, n in enumerate(LLAVA_PROMPT_LENS)]
    return model, prompts, torch.as_tensor(z["batch.images"][:3]).to(device, torch.bfloat16)


def build_vila(device="cuda:0"):
    """-> (model, prompts, images): vila_step_init's weights as one head of 128 with generate_vila's decoder config (scaled RoPE), LoRA
    r = 4 unmerged."""
    from halva_amd.llama import LlamaConfig, add_lora, load_hf_llama_weights
    from halva_amd.siglip import SiglipVisionConfig, SiglipVisionTower
    from halva_amd.vila_model import LlamaForCausalLM, MultimodalProjector, VilaConfig, VilaLlavaLlamaModel
    z, g = load_npz("vila_step_init.npz"), load_npz("generate_vila.npz")
    cfg_d, vis_d = meta_of(g, "llama_cfg"), meta_of(z, "vis_cfg")
    factor = float(math.ceil(int(g["model_max_length"]) / int(g["max_position_embeddings"])))
    cfg = VilaConfig(mm_hidden_size=vis_d["hidden_size"], hidden_size=cfg_d["hidden_size"], mm_vision_select_layer=-2,
                     mm_vision_select_feature="cls_patch")
    llm = LlamaForCausalLM(LlamaConfig(**cfg_d, rope_scaling={"type": "linear", "factor": factor}), torch.bfloat16, device)
    load_hf_llama_weights(llm, tensors(z, "llm."))
    llm.config.tokenizer_model_max_length, llm.config.tokenizer_padding_side = int(g["model_max_length"]), "right"
    vt = SiglipVisionTower("fixture", args=cfg, delay_load=True, config=SiglipVisionConfig(**vis_d), device=device)
    vt._alloc()
    vt.load_hf_state_dict(tensors(z, "vis."))
    vt.requires_grad_(False)
    vt.is_loaded = True
    proj = MultimodalProjector("mlp_downsample", cfg, device=device)
    proj.load_state_dict(tensors(z, "proj."))
    m = VilaLlavaLlamaModel(cfg, llm=llm, vision_tower=vt, mm_projector=proj, device=device)
    for p in m.parameters():
        p.requires_grad_(False)
    r, alpha, fac = int(z["lora_cfg"][0]), float(z["lora_cfg"][1]), tensors(z, "lora.")
    add_lora(m.llm, r, alpha)
    with torch.no_grad():
        for i, layer in enumerate(m.llm.model.layers):
            for sub, grp in layer.groups():
                for gi, n in enumerate(grp.names):
                    key = "model.layers.%d.%s.%s" % (i, sub, n)
                    grp.A_cat[gi * r:(gi + 1) * r].copy_(fac[key + ".A"])
                    getattr(grp, n).lora_B["default"].weight.copy_(fac[key + ".B"])
    m.eval()
    prompts = [torch.as_tensor(g["prompt.%d" % i]) for i in range(3)]
    return m, prompts, torch.as_tensor(z["batch.images"][:3, 0]).to(device, torch.bfloat16)
