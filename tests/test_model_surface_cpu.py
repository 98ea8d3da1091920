"""The Python surface between the C ABI and the step engine (no GPU): parameter names and their order for both towers, every
projector type and both model wrappers - the lists below are those of the commit before the wrappers, the ViT block and the
projector Function were each made one copy - the per-layer HF-name loader with padded heads, and the frozen-projector view."""
from types import SimpleNamespace

import pytest
import torch

CLIP_CFG = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=14)
SIGLIP_CFG = dict(hidden_size=144, intermediate_size=160, num_hidden_layers=2, num_attention_heads=2, image_size=42, patch_size=14)
LLAVA_LLM = dict(vocab_size=160, hidden_size=64, intermediate_size=96, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=4,
                 max_position_embeddings=128, rms_norm_eps=1e-05, pad_token_id=0)
VILA_LLM = dict(vocab_size=64, hidden_size=128, intermediate_size=192, num_hidden_layers=2, num_attention_heads=1,
                max_position_embeddings=64)

CLIP_NAMES = [
    "patch_w", "class_embedding", "position_embedding", "pre_ln_w", "pre_ln_b", "layers.0.ln1_w", "layers.0.ln1_b",
    "layers.0.ln2_w", "layers.0.ln2_b", "layers.0.qkv_w", "layers.0.qkv_b", "layers.0.out_w", "layers.0.out_b",
    "layers.0.fc1_w", "layers.0.fc1_b", "layers.0.fc2_w", "layers.0.fc2_b", "layers.1.ln1_w", "layers.1.ln1_b",
    "layers.1.ln2_w", "layers.1.ln2_b", "layers.1.qkv_w", "layers.1.qkv_b", "layers.1.out_w", "layers.1.out_b",
    "layers.1.fc1_w", "layers.1.fc1_b", "layers.1.fc2_w", "layers.1.fc2_b",
]

SIGLIP_NAMES = [
    "patch_w", "patch_b", "position_embedding", "layers.0.ln1_w", "layers.0.ln1_b", "layers.0.ln2_w", "layers.0.ln2_b",
    "layers.0.qkv_w", "layers.0.qkv_b", "layers.0.out_w", "layers.0.out_b", "layers.0.fc1_w", "layers.0.fc1_b",
    "layers.0.fc2_w", "layers.0.fc2_b", "layers.1.ln1_w", "layers.1.ln1_b", "layers.1.ln2_w", "layers.1.ln2_b",
    "layers.1.qkv_w", "layers.1.qkv_b", "layers.1.out_w", "layers.1.out_b", "layers.1.fc1_w", "layers.1.fc1_b",
    "layers.1.fc2_w", "layers.1.fc2_b",
]

LLAVA_POLICY_NAMES = [
    "model.embed_tokens.weight", "model.layers.0.qkv.weight_cat", "model.layers.0.qkv.A_cat",
    "model.layers.0.qkv.q_proj.lora_B.default.weight", "model.layers.0.qkv.k_proj.lora_B.default.weight",
    "model.layers.0.qkv.v_proj.lora_B.default.weight", "model.layers.0.o.weight_cat", "model.layers.0.o.A_cat",
    "model.layers.0.o.o_proj.lora_B.default.weight", "model.layers.0.gate_up.weight_cat", "model.layers.0.gate_up.A_cat",
    "model.layers.0.gate_up.gate_proj.lora_B.default.weight", "model.layers.0.gate_up.up_proj.lora_B.default.weight",
    "model.layers.0.down.weight_cat", "model.layers.0.down.A_cat", "model.layers.0.down.down_proj.lora_B.default.weight",
    "model.layers.0.input_layernorm.weight", "model.layers.0.post_attention_layernorm.weight", "model.layers.1.qkv.weight_cat",
    "model.layers.1.qkv.A_cat", "model.layers.1.qkv.q_proj.lora_B.default.weight",
    "model.layers.1.qkv.k_proj.lora_B.default.weight", "model.layers.1.qkv.v_proj.lora_B.default.weight",
    "model.layers.1.o.weight_cat", "model.layers.1.o.A_cat", "model.layers.1.o.o_proj.lora_B.default.weight",
    "model.layers.1.gate_up.weight_cat", "model.layers.1.gate_up.A_cat",
    "model.layers.1.gate_up.gate_proj.lora_B.default.weight", "model.layers.1.gate_up.up_proj.lora_B.default.weight",
    "model.layers.1.down.weight_cat", "model.layers.1.down.A_cat", "model.layers.1.down.down_proj.lora_B.default.weight",
    "model.layers.1.input_layernorm.weight", "model.layers.1.post_attention_layernorm.weight", "model.norm.weight",
    "model.vision_tower.patch_w", "model.vision_tower.class_embedding", "model.vision_tower.position_embedding",
    "model.vision_tower.pre_ln_w", "model.vision_tower.pre_ln_b", "model.vision_tower.layers.0.ln1_w",
    "model.vision_tower.layers.0.ln1_b", "model.vision_tower.layers.0.ln2_w", "model.vision_tower.layers.0.ln2_b",
    "model.vision_tower.layers.0.qkv_w", "model.vision_tower.layers.0.qkv_b", "model.vision_tower.layers.0.out_w",
    "model.vision_tower.layers.0.out_b", "model.vision_tower.layers.0.fc1_w", "model.vision_tower.layers.0.fc1_b",
    "model.vision_tower.layers.0.fc2_w", "model.vision_tower.layers.0.fc2_b", "model.vision_tower.layers.1.ln1_w",
    "model.vision_tower.layers.1.ln1_b", "model.vision_tower.layers.1.ln2_w", "model.vision_tower.layers.1.ln2_b",
    "model.vision_tower.layers.1.qkv_w", "model.vision_tower.layers.1.qkv_b", "model.vision_tower.layers.1.out_w",
    "model.vision_tower.layers.1.out_b", "model.vision_tower.layers.1.fc1_w", "model.vision_tower.layers.1.fc1_b",
    "model.vision_tower.layers.1.fc2_w", "model.vision_tower.layers.1.fc2_b", "model.mm_projector.0.weight",
    "model.mm_projector.0.bias", "model.mm_projector.2.weight", "model.mm_projector.2.bias", "lm_head.weight",
]

LLAVA_REFERENCE_NAMES = [
    "model.embed_tokens.weight", "model.norm.weight", "model.vision_tower.patch_w", "model.vision_tower.class_embedding",
    "model.vision_tower.position_embedding", "model.vision_tower.pre_ln_w", "model.vision_tower.pre_ln_b",
    "model.vision_tower.layers.0.ln1_w", "model.vision_tower.layers.0.ln1_b", "model.vision_tower.layers.0.ln2_w",
    "model.vision_tower.layers.0.ln2_b", "model.vision_tower.layers.0.qkv_w", "model.vision_tower.layers.0.qkv_b",
    "model.vision_tower.layers.0.out_w", "model.vision_tower.layers.0.out_b", "model.vision_tower.layers.0.fc1_w",
    "model.vision_tower.layers.0.fc1_b", "model.vision_tower.layers.0.fc2_w", "model.vision_tower.layers.0.fc2_b",
    "model.vision_tower.layers.1.ln1_w", "model.vision_tower.layers.1.ln1_b", "model.vision_tower.layers.1.ln2_w",
    "model.vision_tower.layers.1.ln2_b", "model.vision_tower.layers.1.qkv_w", "model.vision_tower.layers.1.qkv_b",
    "model.vision_tower.layers.1.out_w", "model.vision_tower.layers.1.out_b", "model.vision_tower.layers.1.fc1_w",
    "model.vision_tower.layers.1.fc1_b", "model.vision_tower.layers.1.fc2_w", "model.vision_tower.layers.1.fc2_b",
    "lm_head.weight",
]

VILA_POLICY_NAMES = [
    "llm.model.embed_tokens.weight", "llm.model.layers.0.qkv.weight_cat", "llm.model.layers.0.qkv.A_cat",
    "llm.model.layers.0.qkv.q_proj.lora_B.default.weight", "llm.model.layers.0.qkv.k_proj.lora_B.default.weight",
    "llm.model.layers.0.qkv.v_proj.lora_B.default.weight", "llm.model.layers.0.o.weight_cat", "llm.model.layers.0.o.A_cat",
    "llm.model.layers.0.o.o_proj.lora_B.default.weight", "llm.model.layers.0.gate_up.weight_cat",
    "llm.model.layers.0.gate_up.A_cat", "llm.model.layers.0.gate_up.gate_proj.lora_B.default.weight",
    "llm.model.layers.0.gate_up.up_proj.lora_B.default.weight", "llm.model.layers.0.down.weight_cat",
    "llm.model.layers.0.down.A_cat", "llm.model.layers.0.down.down_proj.lora_B.default.weight",
    "llm.model.layers.0.input_layernorm.weight", "llm.model.layers.0.post_attention_layernorm.weight",
    "llm.model.layers.1.qkv.weight_cat", "llm.model.layers.1.qkv.A_cat", "llm.model.layers.1.qkv.q_proj.lora_B.default.weight",
    "llm.model.layers.1.qkv.k_proj.lora_B.default.weight", "llm.model.layers.1.qkv.v_proj.lora_B.default.weight",
    "llm.model.layers.1.o.weight_cat", "llm.model.layers.1.o.A_cat", "llm.model.layers.1.o.o_proj.lora_B.default.weight",
    "llm.model.layers.1.gate_up.weight_cat", "llm.model.layers.1.gate_up.A_cat",
    "llm.model.layers.1.gate_up.gate_proj.lora_B.default.weight", "llm.model.layers.1.gate_up.up_proj.lora_B.default.weight",
    "llm.model.layers.1.down.weight_cat", "llm.model.layers.1.down.A_cat",
    "llm.model.layers.1.down.down_proj.lora_B.default.weight", "llm.model.layers.1.input_layernorm.weight",
    "llm.model.layers.1.post_attention_layernorm.weight", "llm.model.norm.weight", "llm.lm_head.weight", "vision_tower.patch_w",
    "vision_tower.patch_b", "vision_tower.position_embedding", "vision_tower.layers.0.ln1_w", "vision_tower.layers.0.ln1_b",
    "vision_tower.layers.0.ln2_w", "vision_tower.layers.0.ln2_b", "vision_tower.layers.0.qkv_w", "vision_tower.layers.0.qkv_b",
    "vision_tower.layers.0.out_w", "vision_tower.layers.0.out_b", "vision_tower.layers.0.fc1_w", "vision_tower.layers.0.fc1_b",
    "vision_tower.layers.0.fc2_w", "vision_tower.layers.0.fc2_b", "vision_tower.layers.1.ln1_w", "vision_tower.layers.1.ln1_b",
    "vision_tower.layers.1.ln2_w", "vision_tower.layers.1.ln2_b", "vision_tower.layers.1.qkv_w", "vision_tower.layers.1.qkv_b",
    "vision_tower.layers.1.out_w", "vision_tower.layers.1.out_b", "vision_tower.layers.1.fc1_w", "vision_tower.layers.1.fc1_b",
    "vision_tower.layers.1.fc2_w", "vision_tower.layers.1.fc2_b", "mm_projector.layers.1.weight", "mm_projector.layers.1.bias",
    "mm_projector.layers.2.weight", "mm_projector.layers.2.bias", "mm_projector.layers.4.weight", "mm_projector.layers.4.bias",
]

VILA_REFERENCE_NAMES = [
    "llm.model.embed_tokens.weight", "llm.model.norm.weight", "llm.lm_head.weight", "vision_tower.patch_w",
    "vision_tower.patch_b", "vision_tower.position_embedding", "vision_tower.layers.0.ln1_w", "vision_tower.layers.0.ln1_b",
    "vision_tower.layers.0.ln2_w", "vision_tower.layers.0.ln2_b", "vision_tower.layers.0.qkv_w", "vision_tower.layers.0.qkv_b",
    "vision_tower.layers.0.out_w", "vision_tower.layers.0.out_b", "vision_tower.layers.0.fc1_w", "vision_tower.layers.0.fc1_b",
    "vision_tower.layers.0.fc2_w", "vision_tower.layers.0.fc2_b", "vision_tower.layers.1.ln1_w", "vision_tower.layers.1.ln1_b",
    "vision_tower.layers.1.ln2_w", "vision_tower.layers.1.ln2_b", "vision_tower.layers.1.qkv_w", "vision_tower.layers.1.qkv_b",
    "vision_tower.layers.1.out_w", "vision_tower.layers.1.out_b", "vision_tower.layers.1.fc1_w", "vision_tower.layers.1.fc1_b",
    "vision_tower.layers.1.fc2_w", "vision_tower.layers.1.fc2_b",
]

PROJECTOR_NAMES = {
    "linear": ["weight", "bias"],
    "mlp2x_gelu": ["0.weight", "0.bias", "2.weight", "2.bias"],
    "mlp3x_gelu": ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"],
}
VILA_PROJECTOR_NAMES = {
    "mlp_downsample": ["layers.1.weight", "layers.1.bias", "layers.2.weight", "layers.2.bias", "layers.4.weight", "layers.4.bias"],
    "mlp2x_gelu": ["layers.0.weight", "layers.0.bias", "layers.2.weight", "layers.2.bias"],
}


def _names(m):
    return [n for n, _ in m.named_parameters()]


def _clip():
    from halva_amd.clip import CLIPVisionConfig, CLIPVisionTower
    vt = CLIPVisionTower("fixture", delay_load=True, config=CLIPVisionConfig(**CLIP_CFG), device="cpu")
    vt._alloc()
    return vt


def _siglip():
    from halva_amd.siglip import SiglipVisionConfig, SiglipVisionTower
    vt = SiglipVisionTower("fixture", delay_load=True, config=SiglipVisionConfig(**SIGLIP_CFG), device="cpu")
    vt._alloc()
    return vt


def test_tower_parameter_names_and_order():
    assert _names(_clip()) == CLIP_NAMES
    vt = _siglip()
    assert _names(vt) == SIGLIP_NAMES
    assert (vt.head_dim, vt.head_pad) == (72, 128)
    L = vt.layers[0]
    assert L.qkv_w.shape == (3 * 2 * 128, 144) and L.qkv_b.shape == (3 * 2 * 128,) and L.out_w.shape == (144, 2 * 128)


def test_projector_parameter_names_and_order():
    from halva_amd.clip import build_vision_projector
    from halva_amd.vila_model import MultimodalProjector
    cfg = SimpleNamespace(mm_hidden_size=32, hidden_size=64)
    for kind, want in PROJECTOR_NAMES.items():
        cfg.mm_projector_type = kind
        assert _names(build_vision_projector(cfg, device="cpu")) == want, kind
    for kind, want in VILA_PROJECTOR_NAMES.items():
        assert _names(MultimodalProjector(kind, cfg, device="cpu")) == want, kind


def test_wrapper_parameter_names_and_order():
    """build_random_llava / build_random_vila run on the CPU without a kernel call: the policy and the reference that shares its base."""
    from halva_amd.llava_model import build_random_llava
    from halva_amd.vila_model import build_random_vila
    pol = build_random_llava(LLAVA_LLM, dict(CLIP_CFG, layer_norm_eps=1e-5), lora_r=4, lora_alpha=8, seed=1, device="cpu", max_len=64)
    assert _names(pol) == LLAVA_POLICY_NAMES
    ref = build_random_llava(LLAVA_LLM, dict(CLIP_CFG, layer_norm_eps=1e-5), seed=1, device="cpu", max_len=64, share_base_from=pol)
    assert _names(ref) == LLAVA_REFERENCE_NAMES
    assert [n for n, p in pol.named_parameters() if p.requires_grad] == [n for n in LLAVA_POLICY_NAMES if "A_cat" in n or "lora_B" in n
                                                                         or "mm_projector" in n]
    pol = build_random_vila(VILA_LLM, SIGLIP_CFG, lora_r=4, lora_alpha=8, seed=1, device="cpu", max_len=64)
    assert _names(pol) == VILA_POLICY_NAMES
    ref = build_random_vila(VILA_LLM, SIGLIP_CFG, seed=1, device="cpu", max_len=64, share_base_from=pol)
    assert _names(ref) == VILA_REFERENCE_NAMES
    assert pol.causal_lm() == (pol.llm, "llm.") and pol.projector() == (pol.mm_projector, "mm_projector.")


def _hf_state(cfg, siglip, seed):
    """A synthetic HF-named state dict (bf16-representable values, so that the bf16 tensors must hold them exactly)."""
    g = torch.Generator().manual_seed(seed)
    d, f, p = cfg["hidden_size"], cfg["intermediate_size"], cfg["patch_size"]
    n_tok = (cfg["image_size"] // p) ** 2
    rnd = lambda *s: torch.randn(*s, generator=g).bfloat16().float()
    sd = {"embeddings.patch_embedding.weight": rnd(d, 3, p, p),
          "embeddings.position_embedding.weight": rnd(n_tok + (0 if siglip else 1), d)}
    if siglip:
        sd["embeddings.patch_embedding.bias"] = rnd(d)
    else:
        sd.update({"embeddings.class_embedding": rnd(d), "pre_layrnorm.weight": rnd(d), "pre_layrnorm.bias": rnd(d)})
    for i in range(cfg["num_hidden_layers"]):
        pre = "encoder.layers.%d." % i
        for n in ("layer_norm1", "layer_norm2"):
            sd[pre + n + ".weight"], sd[pre + n + ".bias"] = rnd(d), rnd(d)
        for n in ("q_proj", "k_proj", "v_proj", "out_proj"):
            sd[pre + "self_attn.%s.weight" % n], sd[pre + "self_attn.%s.bias" % n] = rnd(d, d), rnd(d)
        sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"] = rnd(f, d), rnd(f)
        sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"] = rnd(d, f), rnd(d)
    return {"vision_model." + k: v for k, v in sd.items()}


@pytest.mark.parametrize("tower", ["clip", "siglip"])
def test_hf_loader_fills_real_lanes_and_zeroes_pad_lanes(tower):
    siglip = tower == "siglip"
    cfg = SIGLIP_CFG if siglip else CLIP_CFG
    vt = _siglip() if siglip else _clip()
    with torch.no_grad():
        for p in vt.parameters():
            p.fill_(7.0)                                            # garbage that the load must not leave behind anywhere
    sd = _hf_state(cfg, siglip, seed=3)
    vt.load_hf_state_dict(sd)
    src = {k[len("vision_model."):]: v for k, v in sd.items()}
    d, H = cfg["hidden_size"], cfg["num_attention_heads"]
    D = d // H
    Dp = vt.head_pad if siglip else D
    eq = lambda got, want: torch.equal(got.float(), want)
    w = src["embeddings.patch_embedding.weight"].reshape(d, -1)
    assert eq(vt.patch_w[:, :w.shape[1]], w) and not vt.patch_w[:, w.shape[1]:].any()
    assert eq(vt.position_embedding, src["embeddings.position_embedding.weight"])
    if siglip:
        assert eq(vt.patch_b, src["embeddings.patch_embedding.bias"])
    else:
        assert eq(vt.class_embedding, src["embeddings.class_embedding"])
        assert eq(vt.pre_ln_w, src["pre_layrnorm.weight"]) and eq(vt.pre_ln_b, src["pre_layrnorm.bias"])
    for i, L in enumerate(vt.layers):
        pre = "encoder.layers.%d." % i
        for mine, theirs in (("ln1", "layer_norm1"), ("ln2", "layer_norm2"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2")):
            assert eq(getattr(L, mine + "_w"), src[pre + theirs + ".weight"]), (i, mine)
            assert eq(getattr(L, mine + "_b"), src[pre + theirs + ".bias"]), (i, mine)
        qkv_w, qkv_b, out_w = L.qkv_w.view(3, H, Dp, d), L.qkv_b.view(3, H, Dp), L.out_w.view(d, H, Dp)
        for j, n in enumerate(("q_proj", "k_proj", "v_proj")):
            assert eq(qkv_w[j, :, :D], src[pre + "self_attn.%s.weight" % n].view(H, D, d)), (i, n)
            assert eq(qkv_b[j, :, :D], src[pre + "self_attn.%s.bias" % n].view(H, D)), (i, n)
        assert eq(out_w[:, :, :D], src[pre + "self_attn.out_proj.weight"].view(d, H, D))
        assert eq(L.out_b, src[pre + "self_attn.out_proj.bias"])
        if siglip:
            assert Dp == 128 and D == 72
            assert not qkv_w[:, :, D:].any() and not qkv_b[:, :, D:].any() and not out_w[:, :, D:].any()


def test_frozen_projector_view_forwards_what_the_projector_has():
    from halva_amd.clip import build_vision_projector
    from halva_amd.multimodal import FrozenProjectorView
    from halva_amd.vila_model import MultimodalProjector
    cfg = SimpleNamespace(mm_hidden_size=32, hidden_size=64, mm_projector_type="mlp2x_gelu")
    proj = MultimodalProjector("mlp_downsample", cfg, device="cpu")
    view = FrozenProjectorView(proj)
    assert view.kind == "mlp_downsample" and view.config is proj.config
    assert view.tokens_per_image(729) == proj.tokens_per_image(729) == 196
    assert list(view.parameters()) == []                           # the tensors stay the policy's
    plain = FrozenProjectorView(build_vision_projector(cfg, device="cpu"))
    assert not any(hasattr(plain, a) for a in ("kind", "config", "tokens_per_image"))
    seen = []
    plain._p[0].forward = lambda x: seen.append(torch.is_grad_enabled()) or x
    x = torch.ones(2, 3, requires_grad=True)
    assert plain(x) is x and seen == [False]                       # run under no_grad
