#!/usr/bin/env python3
"""Generate tests/golden/generate_vila.npz: greedy decoding of the REFERENCE's VILA LlavaLlamaModel (CPU, fp32): its SigLIP tower,
the mlp_downsample projector and the vendored transformers-4.31 Llama as `.llm`, loaded through make_golden_vila.py's import shims.

Weights: those of vila_step_init.npz (vocab 160, d = 128, F = 192, 2 layers; SigLIP 144 wide, 48 px -> 4 image tokens), with the
LoRA factors merged (W + (alpha / r) B A).  The decoder runs them as ONE head of 128 instead of the fixture's two of 64 (the same
weights: the head split only regroups the attention), the head width the HIP decode kernels serve.  Linear RoPE scaling is on:
max_position_embeddings = 32 with model_max_length = 64 gives factor ceil(64 / 32) = 2 (vila/model/language_model/builder.py's
context_length_extension), and every prompt's decoded positions run past 32.

3 prompts (prefixes of the fixture's rows, one image each), 24 greedy steps per prompt.  Each step runs the reference's own forward
on the whole prefix (no cache, use_cache=False): the arithmetic that a cached `generate(use_cache=True)` is defined to match, without
HF generation internals.  Only inputs and outputs are stored: the config, the prompt ids, the generated ids, every step's last-row
logits and their top-1 / top-2 gap; the weights stay in vila_step_init.npz.

Usage:  python tests/golden/make_golden_generate_vila.py          (runs where the reference tree is mounted, like make_golden_vila.py)
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_vila as MGV  # noqa: E402  (imports the reference's VILA files through its shims)

PROMPT_LENS = (12, 16, 21)
STEPS = 24
MAX_POS, MODEL_MAX_LEN = 32, 64


def _f32(a):
    a = np.asarray(a)
    if a.dtype == np.uint16:
        return torch.from_numpy(a.astype(np.uint32) << 16).view(torch.float32)
    return torch.from_numpy(np.array(a, dtype=np.float32))


def llama_cfg(z):
    d = json.loads(bytes(z["llama_cfg"]).decode())
    d.update(num_attention_heads=1, num_key_value_heads=1, max_position_embeddings=MAX_POS)
    return d


def build_reference(z):
    from transformers import LlamaConfig
    from make_golden_vila import V
    sig = json.loads(bytes(z["vis_cfg"]).decode())
    tower = MGV.build_tower(71, sig)
    missing, unexpected = tower.vision_tower.load_state_dict({k[len("vis."):]: _f32(z[k]) for k in z.files if k.startswith("vis.")},
                                                             strict=False)
    assert not unexpected, unexpected
    assert all("position_ids" in k or ".head." in k or "post_layernorm" in k for k in missing), missing
    lc = LlamaConfig(**llama_cfg(z))
    lc.pretraining_tp = 1
    lc._attn_implementation = "eager"
    lc.rope_scaling = {"type": "linear", "factor": float(np.ceil(MODEL_MAX_LEN / MAX_POS))}
    llm = MGV._Llm(lc)
    missing, unexpected = llm.load_state_dict({k[len("llm."):]: _f32(z[k]) for k in z.files if k.startswith("llm.")}, strict=False)
    assert not unexpected and all("rotary" in k for k in missing), (missing, unexpected)
    assert type(llm.model.layers[0].self_attn.rotary_emb).__name__ == "LlamaLinearScalingRotaryEmbedding"
    r, alpha = int(z["lora_cfg"][0]), float(z["lora_cfg"][1])
    mods = dict(llm.named_modules())
    with torch.no_grad():
        for k in z.files:
            if k.startswith("lora.") and k.endswith(".A"):
                name = k[len("lora."):-len(".A")]
                mods[name].weight.add_((alpha / r) * (_f32(z["lora." + name + ".B"]) @ _f32(z[k])))
    cfg = type("C", (), dict(mm_hidden_size=sig["hidden_size"], hidden_size=lc.hidden_size))()
    proj = V.BP.MultimodalProjector(V.BP.MultimodalProjectorConfig("mlp_downsample"), cfg)
    proj.load_state_dict({k[len("proj."):]: _f32(z[k]) for k in z.files if k.startswith("proj.")})
    llm.config.tokenizer_model_max_length = MODEL_MAX_LEN
    llm.config.tokenizer_padding_side = "right"
    m = MGV.RefVila(llm, tower, proj, type("C", (), {})())
    m.eval()
    return m


@torch.no_grad()
def greedy(m, prompt, image):
    ids = prompt.clone()
    toks, logits, gaps = [], [], []
    for _ in range(STEPS):
        out = m(input_ids=ids[None], images=image[None], attention_mask=torch.ones(1, len(ids), dtype=torch.bool), use_cache=False)
        lg = out.logits[0, -1].float()
        top2 = lg.topk(2).values
        nxt = int(lg.argmax())
        toks.append(nxt)
        logits.append(lg.numpy())
        gaps.append(float(top2[0] - top2[1]))
        ids = torch.cat([ids, torch.tensor([nxt], dtype=ids.dtype)])
    return np.array(toks, np.int64), np.stack(logits), np.array(gaps, np.float32), out.logits.shape[1]


def main():
    torch.set_num_threads(4)
    z = np.load(os.path.join(HERE, "vila_step_init.npz"))
    m = build_reference(z)
    ids = torch.from_numpy(z["batch.input_ids"][:3].astype(np.int64))
    images = torch.from_numpy(z["batch.images"][:3, 0].astype(np.float32))
    packs = {"prompt_lens": np.array(PROMPT_LENS, np.int64), "max_position_embeddings": np.array(MAX_POS),
             "model_max_length": np.array(MODEL_MAX_LEN),
             "llama_cfg": np.frombuffer(json.dumps(llama_cfg(z)).encode(), dtype=np.uint8)}
    for i, n in enumerate(PROMPT_LENS):
        toks, logits, gaps, last_len = greedy(m, ids[i, :n], images[i])
        assert last_len > MAX_POS, (i, last_len)              # the scaled positions are exercised past max_position_embeddings
        packs["prompt.%d" % i] = ids[i, :n].numpy()
        packs["tokens.%d" % i] = toks
        packs["logits.%d" % i] = logits
        packs["gap.%d" % i] = gaps
        print("   prompt %d (%d ids, %d rows at the last step): tokens %s, min top-2 gap %.3e"
              % (i, n, last_len, toks.tolist(), float(gaps.min())))
    MGV.save_npz("generate_vila.npz", **packs)


if __name__ == "__main__":
    main()
