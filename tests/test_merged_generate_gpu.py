"""merge_and_unload() (halva_amd/llama.py:LoraGroup.merge_ on halva_lora_merge), merged loading and the export tool.

The merged models are held to the same goldens as the unmerged ones - tests/golden/generate_d128.npz and generate_vila.npz hold the
REFERENCE's forward with the LoRA factors merged in fp32 - under the bound tests/test_generate_gpu.py / test_generate_vila_gpu.py apply
to the unmerged path (their helpers are imported, not copied): 1.5 x the distance of the unmerged model's cache-free forward from the
golden, per prompt.  Greedy tokens agree with the unmerged model's up to a step whose top-2 gap is within 4 x the row-grouping bound.

The cross-check at 2 layers, d = 256, r = 8 bounds merged-vs-unmerged logits by twice what the two existing orderings of the LoRA
arithmetic (HALVA_LORA_TWO_GEMM = 1 / 0) differ by on the same input, measured in the test: the factor 2 is for the one extra rounding
of W.  Loading with merge_lora=True, and loading what tools/merge_lora_weights.py wrote as a plain full checkpoint, give the logits of
the in-memory merged model bit for bit."""
import importlib.util
import json
import math
import os
import sys
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_generate_gpu as TG  # noqa: E402
import test_generate_vila_gpu as TV  # noqa: E402
from golden_util import load_npz, meta_of, tensors  # noqa: E402
from model_util import batch_of, build_product_models  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NEW = TG.N_NEW


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _groups(lm):
    return [grp for layer in lm.layers for _, grp in layer.groups()]


def _lora_free(model, merged=True):
    """what merge_and_unload leaves: no factor anywhere, the LoRA-free weight layout, decode without the LoRA path"""
    lm = model.get_model()
    for grp in _groups(lm):
        assert grp.lora_state() == {} and grp.A_cat is None and grp.weight_cat_t is None and grp.r == 0
        assert grp.weight_cat.shape[1] == grp.in_features + (64 if grp.in_features % 1024 == 0 else 0)
        assert all(len(t.lora_B) == 0 for t in grp.targets())
    assert not merged or model.decode_stack().use_lora is False
    assert not any("lora" in n or "A_cat" in n for n, _ in model.named_parameters())


def _row_grouping_bound(full_last_logits, model, prompts, images, long_row, long_image):
    """the `bound` fixture of the two generate test files: what two bf16 forwards that differ in row grouping disagree by"""
    together = full_last_logits(model, prompts + [long_row], torch.cat([images, long_image]))[:3]
    alone = torch.cat([full_last_logits(model, [p], images[i:i + 1]) for i, p in enumerate(prompts)])
    floor = 2.0 ** (math.floor(math.log2(float(together.abs().max()))) - 7)
    return max(float((together - alone).abs().max()), floor)


def _check_against_golden(M, unmerged, merged, prompts, images, g, bound, new_tokens):
    """M: the generate test module whose helpers and rule apply (TG: LLaVA, TV: VILA)"""
    for i in range(3):
        p, toks = prompts[i], torch.as_tensor(g["tokens.%d" % i])
        glog = torch.as_tensor(g["logits.%d" % i]).double()
        with torch.no_grad():
            cached = M._teacher_forced(merged, p, images[i], toks[:-1].tolist()).double().cpu()
        full_u = torch.stack([M._full_last_logits(unmerged, [torch.cat([p, toks[:s]])], images[i:i + 1])[0] for s in range(N_NEW)]).double().cpu()
        d_cached, d_full = (cached - glog).abs().amax(-1), (full_u - glog).abs().amax(-1)
        bound_i = 1.5 * float(d_full.max())
        print("prompt %d: |merged cached - golden| max %.3e, |unmerged full - golden| max %.3e, bound %.3e"
              % (i, float(d_cached.max()), float(d_full.max()), bound_i))
        assert (d_cached <= bound_i).all(), (d_cached, d_full)
        a = new_tokens(merged.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[]), p)
        b = new_tokens(unmerged.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[]), p)
        ref = M._teacher_forced(unmerged, p, images[i], b[:-1])
        assert M._agree_until_close(a, b, ref, 4 * bound), (i, a, b)


# ------------------------------------------------------------------------------------------------
def test_llava_merged_against_the_reference_golden():
    _dev()
    z, g = load_npz("dpa_step_d128_init.npz"), load_npz("generate_d128.npz")
    unmerged = build_product_models(z, device="cuda:0")[0].eval()
    merged = build_product_models(z, device="cuda:0")[0].eval()
    before = [grp.weight.clone() for grp in _groups(merged.model)]
    assert merged.merge_and_unload() is merged
    _lora_free(merged)
    assert any(not torch.equal(b, grp.weight) for b, grp in zip(before, _groups(merged.model)))
    after = [grp.weight_cat.clone() for grp in _groups(merged.model)]
    assert merged.merge_and_unload() is merged                     # a second merge: nothing to do
    assert all(torch.equal(a, grp.weight_cat) for a, grp in zip(after, _groups(merged.model)))
    ids = torch.as_tensor(z["batch.input_ids"][:3])
    prompts = [ids[i, :n].clone() for i, n in enumerate(TG.PROMPT_LENS)]
    images = torch.as_tensor(z["batch.images"][:3]).to("cuda:0", torch.bfloat16)
    bound = _row_grouping_bound(TG._full_last_logits, unmerged, prompts, images, torch.as_tensor(z["batch.input_ids"][3]), images[:1])
    _check_against_golden(TG, unmerged, merged, prompts, images, g, bound, lambda out, p: out[0, len(p):].tolist())


def test_vila_merged_against_the_reference_golden():
    _dev()
    z, g = load_npz("vila_step_init.npz"), load_npz("generate_vila.npz")
    unmerged, merged = TV._build(z, g), TV._build(z, g)
    assert merged.merge_and_unload() is merged
    _lora_free(merged)
    assert merged.merge_and_unload() is merged
    prompts = [torch.as_tensor(g["prompt.%d" % i]) for i in range(3)]
    images = torch.as_tensor(z["batch.images"][:3, 0]).to("cuda:0", torch.bfloat16)
    long_row = torch.as_tensor(z["batch.input_ids"][2][:int(z["batch.attention_mask"][2].sum())])
    bound = _row_grouping_bound(TV._full_last_logits, unmerged, prompts, images, long_row, images[2:3])
    _check_against_golden(TV, unmerged, merged, prompts, images, g, bound, lambda out, p: out[0].tolist())


def test_merged_forward_within_twice_the_spread_of_the_two_lora_orderings(monkeypatch):
    """2 layers, d = 256 (2 heads x 128), r = 8, non-zero B: |merged - unmerged| logits <= 2 x |two-GEMM form - K-concatenated form|."""
    _dev()
    from halva_amd import llama
    from halva_amd.llava_model import build_random_llava
    z = load_npz("dpa_step_d128_init.npz")
    cfg = dict(vocab_size=160, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
               max_position_embeddings=256, rms_norm_eps=1e-5, pad_token_id=0)

    def make():
        m = build_random_llava(cfg, meta_of(z, "clip_cfg"), lora_r=8, lora_alpha=16, seed=3, device="cuda", max_len=256)
        gen = torch.Generator(device="cuda").manual_seed(4)
        with torch.no_grad():
            for grp in _groups(m.model):
                for B in grp._Bs():
                    B.normal_(0.0, 0.02, generator=gen)
        return m.eval()
    a, b = make(), make()
    rows = torch.as_tensor(z["batch.input_ids"][:3])
    ids, mask = (t.cuda() for t in TG._pad_batch([rows[i, :n].clone() for i, n in enumerate(TG.PROMPT_LENS)]))
    images = torch.as_tensor(z["batch.images"][:3]).to("cuda:0", torch.bfloat16)

    @torch.no_grad()
    def logits(m):
        out = m.forward(input_ids=ids, attention_mask=mask, images=images).logits
        keep = m._last_plan.mask.to(out.device)
        return out[keep].double()
    one = logits(a)
    monkeypatch.setattr(llama, "LORA_TWO_GEMM", True)
    two = logits(a)
    monkeypatch.setattr(llama, "LORA_TWO_GEMM", False)
    assert torch.equal(logits(b), one)                            # the twin computes the same bits before it is merged
    b.merge_and_unload()
    spread, diff = float((two - one).abs().max()), float((logits(b) - one).abs().max())
    print("two-GEMM vs K-concatenated: %.3e;  merged vs unmerged: %.3e  (bound %.3e)" % (spread, diff, 2 * spread))
    assert spread > 0 and diff > 0
    assert diff <= 2 * spread


# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """A trained run on disk, written as tests/test_generate_gpu.py:test_adapter_round_trip_through_load_pretrained_model writes it:
    three DPA steps move the LoRA factors and the projector; base / vision / run-lora directories."""
    _dev()
    from safetensors.torch import save_file
    import llava.train.train_halva as TH
    from halva_amd import dpa
    tmp = tmp_path_factory.mktemp("merged")
    z = load_npz("dpa_step_d128_init.npz")
    model, ref, _ = build_product_models(z, device="cuda:0")
    flat = dpa.FlatTrainables(dpa.trainable_named_parameters(model))
    dpa.bind_model(flat, model)
    dpa.set_grad_sink(model, True)
    opt = dpa.AdamWFlat(flat, lr=2e-3, weight_decay=0.0, mm_projector_lr=2e-3)
    eng = dpa.DPAEngine(model, ref, float(z["alpha"]), 2, 2)
    for _ in range(3):
        flat.zero_grad()
        eng.loss(batch_of(z), backward=True)
        opt.step()
    torch.cuda.synchronize()
    base, vis, out = (str(tmp / d) for d in ("base", "vision", "run-lora"))
    os.makedirs(base)
    os.makedirs(vis)
    cfg = dict(meta_of(z, "llama_cfg"), model_type="llava", mm_vision_tower=vis, mm_projector_type="mlp2x_gelu",
               mm_hidden_size=meta_of(z, "clip_cfg")["hidden_size"], mm_vision_select_layer=-2, mm_vision_select_feature="patch",
               tokenizer_model_max_length=int(z["max_len"]), tokenizer_padding_side="right")
    json.dump(cfg, open(os.path.join(base, "config.json"), "w"))
    save_file({k: v.to(torch.bfloat16).contiguous() for k, v in tensors(z, "base.").items()}, os.path.join(base, "model.safetensors"))
    json.dump({"vision_config": meta_of(z, "clip_cfg")}, open(os.path.join(vis, "config.json"), "w"))
    save_file({"vision_model." + k: v.to(torch.bfloat16).contiguous() for k, v in tensors(z, "clip.").items()},
              os.path.join(vis, "model.safetensors"))
    model.config.mm_vision_tower = vis
    grp = model.model.layers[0].qkv
    TH.save_lora_outputs(model, types.SimpleNamespace(output_dir=out, lora_bias="none", lora_r=grp.r, lora_alpha=grp.scale * grp.r,
                                                      lora_dropout=0.0))
    ids = torch.as_tensor(z["batch.input_ids"][2, :TG.PROMPT_LENS[2]]).clone()
    image = torch.as_tensor(z["batch.images"][2]).to("cuda:0", torch.bfloat16)

    def logits(m):
        with torch.no_grad():
            return TG._teacher_forced(m, ids, image, [3, 4, 5])
    unmerged_logits = logits(model)
    # the trainer has bound this model: merging it is refused, and nothing has changed after the refusal
    with pytest.raises(RuntimeError, match="gradient sink"):
        model.merge_and_unload()
    assert torch.equal(logits(model), unmerged_logits) and model.model.layers[0].qkv.A_cat is not None
    dpa.set_grad_sink(model, False)
    model.merge_and_unload()
    _lora_free(model)
    return types.SimpleNamespace(base=base, out=out, tmp=str(tmp), logits=logits, unmerged=unmerged_logits, merged=logits(model))


def test_loader_with_merge_lora_gives_the_in_memory_merged_model(run, capsys):
    from llava.model.builder import load_pretrained_model
    _, plain, _, _ = load_pretrained_model(run.out, run.base, "run-lora")
    assert plain.model.layers[0].qkv.A_cat is not None and plain.decode_stack().use_lora is True
    assert torch.equal(run.logits(plain), run.unmerged)                       # the default load: unmerged, bitwise as before
    assert "Merging" not in capsys.readouterr().out
    _, loaded, _, _ = load_pretrained_model(run.out, run.base, "run-lora", merge_lora=True)
    assert "Merging LoRA weights..." in capsys.readouterr().out
    _lora_free(loaded)
    assert torch.equal(run.logits(loaded), run.merged)
    assert not torch.equal(run.merged, run.unmerged)
    # a merged, loaded policy has nothing to train: the step engine's flat buffer still refuses it
    from halva_amd import dpa
    with pytest.raises(ValueError, match="no trainable parameters"):
        dpa.FlatTrainables(dpa.trainable_named_parameters(loaded))


def test_export_tool_writes_a_full_checkpoint_that_loads_without_lora(run, monkeypatch):
    from safetensors import safe_open
    from llava.model.builder import load_pretrained_model
    spec = importlib.util.spec_from_file_location("merge_lora_weights", os.path.join(ROOT, "tools", "merge_lora_weights.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    dst = os.path.join(run.tmp, "merged-full")
    monkeypatch.setattr(sys, "argv", ["merge_lora_weights.py", "--model-path", run.out, "--model-base", run.base, "--save-model-path", dst])
    tool.main()
    assert sorted(os.listdir(dst)) == ["config.json", "model.safetensors"]
    with safe_open(os.path.join(dst, "model.safetensors"), "pt") as f:
        keys = set(f.keys())
    assert not any("lora_" in k for k in keys)
    n_layers = json.load(open(os.path.join(dst, "config.json")))["num_hidden_layers"]
    want = {"model.embed_tokens.weight", "model.norm.weight", "lm_head.weight"}
    for i in range(n_layers):
        want |= {"model.layers.%d.self_attn.%s.weight" % (i, n) for n in ("q_proj", "k_proj", "v_proj", "o_proj")}
        want |= {"model.layers.%d.mlp.%s.weight" % (i, n) for n in ("gate_proj", "up_proj", "down_proj")}
        want |= {"model.layers.%d.%s.weight" % (i, n) for n in ("input_layernorm", "post_attention_layernorm")}
    assert want <= keys and all(k.startswith("model.mm_projector.") for k in keys - want) and len(keys - want) == 4
    _, full, _, _ = load_pretrained_model(dst, None, "merged-full")
    _lora_free(full, merged=False)                                # (never had factors: a plain checkpoint)
    assert torch.equal(run.logits(full), run.merged)
