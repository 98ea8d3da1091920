"""The host side of merged export, without a GPU: the name mapping of the exported checkpoint (fused qkv / gate_up rows split into the HF
per-projection names and fused again by the loader's load_hf_llama_weights: the identity), what save_pretrained writes and refuses, and
the refusal to merge a model a trainer has bound."""
import pytest
import torch

from golden_util import load_json

VIS = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=28, patch_size=14, layer_norm_eps=1e-5)


def _tiny(seed, lora=False):
    from halva_amd.llava_model import build_random_llava
    d = load_json("peft_state_names.json")
    m = build_random_llava(d["llama_cfg"], VIS, lora_r=d["lora_r"] if lora else 0, lora_alpha=8, seed=seed, device="cpu", max_len=64)
    if lora:
        with torch.no_grad():
            for layer in m.model.layers:
                for _, grp in layer.groups():
                    for B in grp._Bs():
                        B.normal_(0.0, 0.05)
    return m


def _groups(m):
    return [grp for layer in m.model.layers for _, grp in layer.groups()]


def test_split_names_fused_again_through_the_loader_mapping_are_the_identity(tmp_path):
    from halva_amd.clip import _read_checkpoint
    from halva_amd.llama import load_hf_llama_weights
    src, dst = _tiny(1), _tiny(2)
    assert any(not torch.equal(a.weight, b.weight) for a, b in zip(_groups(src), _groups(dst)))
    sd = src.hf_state_dict()
    n, cfg = src.config.num_hidden_layers, src.config
    want = {"model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"}
    for i in range(n):
        want |= {"model.layers.%d.self_attn.%s.weight" % (i, t) for t in ("q_proj", "k_proj", "v_proj", "o_proj")}
        want |= {"model.layers.%d.mlp.%s.weight" % (i, t) for t in ("gate_proj", "up_proj", "down_proj")}
        want |= {"model.layers.%d.%s.weight" % (i, t) for t in ("input_layernorm", "post_attention_layernorm")}
    proj = {k for k in sd if k.startswith("model.mm_projector.")}
    assert set(sd) == want | proj and len(proj) == 4
    d, F = cfg.hidden_size, cfg.intermediate_size
    for i in range(n):
        for t in ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj"):
            assert sd["model.layers.%d.%s.%s.weight" % (i, "mlp" if t == "down_proj" else "self_attn", t)].shape == ((d, F) if t == "down_proj" else (d, d))
        for t in ("gate_proj", "up_proj"):
            assert sd["model.layers.%d.mlp.%s.weight" % (i, t)].shape == (F, d)
    # the rows of a fused weight, in the order of the group's names
    qkv = src.model.layers[0].qkv
    assert torch.equal(torch.cat([sd["model.layers.0.self_attn.%s.weight" % t] for t in qkv.names]), qkv.weight)
    # written and read back, then fused again by the loader: every tensor of the source, bit for bit
    out = str(tmp_path / "full")
    src.save_pretrained(out)
    back = _read_checkpoint(out)
    assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    load_hf_llama_weights(dst, back, strict=True)
    dst.model.mm_projector.load_state_dict({k.split("mm_projector.")[1]: v for k, v in back.items() if "mm_projector." in k})
    for a, b in zip(_groups(src), _groups(dst)):
        assert torch.equal(a.weight, b.weight)
    again = dst.hf_state_dict()
    assert set(again) == set(sd) and all(torch.equal(again[k], sd[k]) for k in sd)
    import json
    import os
    saved = json.load(open(os.path.join(out, "config.json")))
    assert saved["model_type"] == "llava" and saved["hidden_size"] == d and saved["num_hidden_layers"] == n


def test_save_pretrained_refuses_a_model_that_still_carries_factors(tmp_path):
    m = _tiny(3, lora=True)
    with pytest.raises(RuntimeError, match="merge_and_unload"):
        m.save_pretrained(str(tmp_path / "x"))
    assert not (tmp_path / "x").exists()


def test_merging_a_model_with_a_bound_gradient_sink_is_refused():
    from halva_amd import dpa, hip
    m = _tiny(4, lora=True)
    dpa.set_grad_sink(m, True)
    state = {k: v.clone() for grp in _groups(m) for k, v in grp.lora_state().items()}
    weights = [grp.weight_cat.clone() for grp in _groups(m)]
    with pytest.raises(RuntimeError, match="gradient sink"):
        m.merge_and_unload()
    with pytest.raises(RuntimeError, match="gradient sink"):
        m.get_model().merge_and_unload()
    with pytest.raises(RuntimeError, match="gradient sink"):
        m.model.layers[0].qkv.merge_()
    assert m.decode_stack().use_lora is True
    assert all(torch.equal(w, grp.weight_cat) for w, grp in zip(weights, _groups(m)))
    assert all(torch.equal(v, dict(kv for grp in _groups(m) for kv in grp.lora_state().items())[k]) for k, v in state.items())
    # without the sink the merge goes to the HIP kernel, and only there: host tensors are an error, not a slow path
    dpa.set_grad_sink(m, False)
    with pytest.raises(hip.HalvaHipError, match="no CPU fallback"):
        m.merge_and_unload()
    # a model that never had factors: nothing to do
    plain = _tiny(5)
    w0 = [grp.weight_cat.clone() for grp in _groups(plain)]
    assert plain.merge_and_unload() is plain
    assert all(torch.equal(w, grp.weight_cat) for w, grp in zip(w0, _groups(plain)))
