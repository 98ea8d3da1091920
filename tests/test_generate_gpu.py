"""KV-cached greedy generation (halva_amd/decode.py, LlavaLlamaForCausalLM.generate) on the dpa_step_d128_init weights (2 layers,
2 heads x 128, vocab 160, LoRA r = 4 with non-zero factors), against the product's own full forward without a cache.

Against the reference itself: tests/golden/generate_d128.npz (tests/golden/make_golden_generate.py).

The bound of the comparisons with the product's own forward is measured, not set: BOUND is what two bf16 full forwards that differ only in row grouping (the
three prompts in one batch with a long fourth row against each alone) disagree by on the last-row logits, floored at one bf16 ulp of the
largest of those logits (the row-wise GEMMs often give the same bits in both groupings)."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_npz  # noqa: E402
from model_util import build_product_models  # noqa: E402

PROMPT_LENS = (20, 33, 47)
N_NEW = 24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


@pytest.fixture(scope="module")
def setup():
    _dev()
    z = load_npz("dpa_step_d128_init.npz")
    pol, _, _ = build_product_models(z, device="cuda:0")
    pol.eval()
    ids = torch.as_tensor(z["batch.input_ids"][:3])
    prompts = [ids[i, :n].clone() for i, n in enumerate(PROMPT_LENS)]
    images = torch.as_tensor(z["batch.images"][:3]).to("cuda:0", torch.bfloat16)
    return pol, prompts, images


def _pad_batch(rows, pad=0):
    T = max(len(r) for r in rows)
    ids = torch.full((len(rows), T), pad, dtype=torch.long)
    mask = torch.zeros(len(rows), T, dtype=torch.bool)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
        mask[i, :len(r)] = True
    return ids, mask


@torch.no_grad()
def _full_last_logits(model, rows, images):
    """forward() on right-padded rows (no cache): the logits of each row's last token [len(rows), V]."""
    ids, mask = _pad_batch(rows)
    out = model.forward(input_ids=ids.cuda(), attention_mask=mask.cuda(), images=images).logits
    n = model._last_plan.seq_len.long()
    return out[torch.arange(len(rows)), n - 1].float()


@pytest.fixture(scope="module")
def bound(setup):
    model, prompts, images = setup
    z = load_npz("dpa_step_d128_init.npz")
    long_row = torch.as_tensor(z["batch.input_ids"][3])            # 139 tokens: the batch's GEMMs run at several times the rows
    together = _full_last_logits(model, prompts + [long_row], torch.cat([images, images[:1]]))[:3]
    alone = torch.cat([_full_last_logits(model, [p], images[i:i + 1]) for i, p in enumerate(prompts)])
    d = float((together - alone).abs().max())
    floor = 2.0 ** (math.floor(math.log2(float(together.abs().max()))) - 7)       # one bf16 ulp of the largest logit
    b = max(d, floor)
    print("row-grouping difference %.3e, bf16 floor %.3e -> bound %.3e" % (d, floor, b))
    return b


def _teacher_forced(model, prompt, image, tokens):
    """logits of the prompt's last row and of each forced token, through prefill + decode_step."""
    from halva_amd import decode as DEC
    embeds, plan = model._splice(prompt[None].cuda(), None, None, None, image[None])
    cache = DEC.KVCache(model, 1, embeds.shape[1] + len(tokens) + 1)
    out = [DEC.prefill(model, embeds, plan.seq_len, cache)]
    for t in tokens:
        out.append(DEC.decode_step(model, cache, torch.tensor([t], device="cuda")))
    return torch.cat(out)


def test_cached_decode_matches_full_forward(setup, bound):
    model, prompts, images = setup
    worst = 0.0
    for i, p in enumerate(prompts):
        gen = model.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[])
        toks = gen[0, len(p):].tolist()
        assert len(toks) == N_NEW
        cached = _teacher_forced(model, p, images[i], toks[:-1])
        for s in range(N_NEW):
            full = _full_last_logits(model, [torch.cat([p, torch.tensor(toks[:s], dtype=torch.long)])], images[i:i + 1])[0]
            worst = max(worst, float((cached[s] - full).abs().max()))
    print("cached vs full forward: max |logit diff| %.3e (bound %.3e)" % (worst, bound))
    # the cached path runs every GEMM at M = 1 (other kernels, other accumulation orders than at M = T) and attends in another order, so
    # its bf16 intermediates round differently: measured 2.0 x the bound on MI355X (7.8e-3 against one ulp, 3.9e-3); 3 x leaves one ulp
    assert worst <= 3 * bound


def test_against_the_reference_golden(setup):
    """tests/golden/generate_d128.npz (make_golden_generate.py): 24 greedy steps of the REFERENCE's own forward (fp32, LoRA merged, no
    cache) on the same weights and prompts.  Teacher-forced through prefill + decode_step, every step's logits sit no further from the
    golden than the product's cache-free full forward gets over the prompt's steps, x 1.5; greedy generate() emits the golden's tokens up
    to the first step whose golden top-2 gap is below 4 x that bound."""
    model, prompts, images = setup
    g = load_npz("generate_d128.npz")
    for i in range(3):
        p, toks = torch.as_tensor(g["prompt.%d" % i]), torch.as_tensor(g["tokens.%d" % i])
        glog, gap = torch.as_tensor(g["logits.%d" % i]).double(), torch.as_tensor(g["gap.%d" % i])
        assert torch.equal(p, prompts[i]) and len(toks) == N_NEW
        with torch.no_grad():
            cached = _teacher_forced(model, p, images[i], toks[:-1].tolist()).double().cpu()
        full = torch.stack([_full_last_logits(model, [torch.cat([p, toks[:s]])], images[i:i + 1])[0] for s in range(N_NEW)]).double().cpu()
        d_cached, d_full = (cached - glog).abs().amax(-1), (full - glog).abs().amax(-1)
        print("prompt %d: |cached - golden| max %.3e, |full - golden| max %.3e, worst step ratio %.2f"
              % (i, float(d_cached.max()), float(d_full.max()), float((d_cached / d_full).max())))
        # the bound: 1.5 x how far the product's full forward gets from the golden over the 24 steps (one number per prompt, also the unit
        # of the token rule below).  Per step the two distances are a few bf16 ulps each and move by one ulp from step to step: the
        # step-wise ratio measured up to 1.65 on MI355X while the cached path's worst step stayed within 1.33 x the full forward's worst.
        bound_i = 1.5 * float(d_full.max())
        assert (d_cached <= bound_i).all(), (d_cached, d_full)
        gen = model.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[])[0, len(p):].cpu()
        for s in range(N_NEW):
            if float(gap[s]) < 4 * bound_i:
                break
            assert int(gen[s]) == int(toks[s]), (i, s, gen.tolist(), toks.tolist())


def _agree_until_close(a, b, logits_ref, gap):
    """token lists a, b equal up to the first step whose top-2 gap (of logits_ref) is below `gap`."""
    for s in range(min(len(a), len(b))):
        top2 = logits_ref[s].topk(2).values
        if float(top2[0] - top2[1]) < gap:
            return True
        if a[s] != b[s]:
            return False
    return True


def test_batched_ragged_equals_one_at_a_time(setup, bound):
    model, prompts, images = setup
    ids, mask = _pad_batch(prompts)
    batched = model.generate(ids, images=images, attention_mask=mask, max_new_tokens=N_NEW, eos_token_id=[])
    assert batched.shape == (3, ids.shape[1] + N_NEW)
    for i, p in enumerate(prompts):
        single = model.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[])
        a, b = batched[i, ids.shape[1]:].tolist(), single[0, len(p):].tolist()
        ref = _teacher_forced(model, p, images[i], b[:-1])
        assert _agree_until_close(a, b, ref, 4 * bound), (i, a, b)


def test_prefill_fills_the_cache_with_the_forward_rotated_kv(setup, monkeypatch):
    """The cache after prefill holds the rotated k / v that the ordinary forward() (no hook, every row in every layer) computes: they
    are captured there by wrapping the attention call of the decoder layers."""
    from halva_amd import decode as DEC
    from halva_amd import kernels as K
    model, prompts, images = setup
    ids, mask = _pad_batch(prompts)
    seen = []
    attention = K.attention

    def capture(qkv, *a, **k):
        out = attention(qkv, *a, **k)               # rotates q, k of qkv in place
        seen.append(qkv.detach().clone())
        return out
    monkeypatch.setattr(K, "attention", capture)
    with torch.no_grad():
        model.forward(input_ids=ids.cuda(), attention_mask=mask.cuda(), images=images)
    monkeypatch.setattr(K, "attention", attention)
    assert len(seen) == model.config.num_hidden_layers
    embeds, plan = model._splice(ids.cuda(), mask.cuda(), None, None, images)
    cache = DEC.KVCache(model, 3, embeds.shape[1] + 4)
    DEC.prefill(model, embeds, plan.seq_len, cache)
    H, D = cache.H, cache.D
    for i in range(model.config.num_hidden_layers):
        assert cache.lens[i].cpu().tolist() == plan.seq_len.tolist()
        kv = seen[i].view(3, -1, 3, H, D)
        for b, n in enumerate(plan.seq_len.tolist()):
            assert torch.equal(cache.k[i][b, :, :n], kv[b, :n, 1].transpose(0, 1))
            assert torch.equal(cache.v[i][b, :, :n], kv[b, :n, 2].transpose(0, 1))


def test_full_cache_is_refused(setup):
    from halva_amd import decode as DEC
    model, prompts, images = setup
    p = prompts[0]
    embeds, plan = model._splice(p[None].cuda(), None, None, None, images[:1])
    cache = DEC.KVCache(model, 1, embeds.shape[1] + 1)
    DEC.prefill(model, embeds, plan.seq_len, cache)
    DEC.decode_step(model, cache, torch.tensor([3], device="cuda"))
    with pytest.raises(RuntimeError, match="KV cache full"):
        DEC.decode_step(model, cache, torch.tensor([4], device="cuda"))


def test_output_contract(setup):
    model, prompts, images = setup
    p = prompts[1]
    out = model.generate(p[None], images=images[1:2], max_new_tokens=5, eos_token_id=[])
    assert out.dtype == torch.long and out.shape == (1, len(p) + 5)
    assert torch.equal(out[0, :len(p)].cpu(), p)                     # the prompt echoed as given, image token included
    assert int(out[0, 5]) == -200
    # fp16 images: the same tokens as bf16 ones that hold the same values
    out16 = model.generate(p[None], images=images[1:2].half(), max_new_tokens=5, eos_token_id=[])
    assert torch.equal(out16, model.generate(p[None], images=images[1:2].half().bfloat16(), max_new_tokens=5, eos_token_id=[]))
    # EOS: make the first generated token of row 0 the EOS id; that row stops and is padded, the other runs on
    ids, mask = _pad_batch(prompts[:2])
    free = model.generate(ids, images=images[:2], attention_mask=mask, max_new_tokens=6, eos_token_id=[])
    T = ids.shape[1]
    eos = int(free[0, T])
    stopped = model.generate(ids, images=images[:2], attention_mask=mask, max_new_tokens=6, eos_token_id=eos, pad_token_id=0)
    assert int(stopped[0, T]) == eos and (stopped[0, T + 1:] == 0).all()
    if eos not in free[1, T:].tolist():
        assert stopped.shape[1] == T + 6 and torch.equal(stopped[1], free[1])
    # every row done at once: the loop ends early
    one = model.generate(p[None], images=images[1:2], max_new_tokens=6, eos_token_id=int(out[0, len(p)]))
    assert one.shape == (1, len(p) + 1)
    # not implemented
    with pytest.raises(NotImplementedError):
        model.generate(p[None], images=images[1:2], num_beams=2, max_new_tokens=2)
    with pytest.raises(NotImplementedError):
        model.generate(p[None], images=images[1:2], do_sample=True, max_new_tokens=2)


def test_adapter_round_trip_through_load_pretrained_model(setup, tmp_path):
    """Train three DPA steps (LoRA factors and projector move), write the base model and the run's outputs as training writes them
    (save_lora_outputs), load them back with llava.model.builder.load_pretrained_model, and decode: the same logits as the trained
    in-memory model, bitwise.  The projector of the run differs from the base checkpoint's, so the non_lora_trainables.bin path counts."""
    import json
    import types
    from safetensors.torch import save_file
    import llava.train.train_halva as TH
    from golden_util import meta_of, tensors
    from halva_amd import dpa
    from llava.model.builder import load_pretrained_model
    from model_util import batch_of
    _, prompts, images = setup
    z = load_npz("dpa_step_d128_init.npz")
    model, ref, _ = build_product_models(z, device="cuda:0")
    flat = dpa.FlatTrainables(dpa.trainable_named_parameters(model))
    dpa.bind_model(flat, model)
    dpa.set_grad_sink(model, True)
    opt = dpa.AdamWFlat(flat, lr=2e-3, weight_decay=0.0, mm_projector_lr=2e-3)
    eng = dpa.DPAEngine(model, ref, float(z["alpha"]), 2, 2)
    proj0 = {k: v.clone() for k, v in model.model.mm_projector.state_dict().items()}
    for _ in range(3):
        flat.zero_grad()
        eng.loss(batch_of(z), backward=True)
        opt.step()
    torch.cuda.synchronize()
    assert any(not torch.equal(proj0[k], v) for k, v in model.model.mm_projector.state_dict().items())
    base, vis, out = (str(tmp_path / d) for d in ("base", "vision", "run-lora"))
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
    args = types.SimpleNamespace(output_dir=out, lora_bias="none", lora_r=grp.r, lora_alpha=grp.scale * grp.r, lora_dropout=0.0)
    TH.save_lora_outputs(model, args)
    tok, loaded, proc, ctx = load_pretrained_model(out, base, "run-lora")
    assert tok is None and ctx > 0
    for k, v in model.model.mm_projector.state_dict().items():
        assert torch.equal(loaded.model.mm_projector.state_dict()[k], v)
    p = prompts[2]
    with torch.no_grad():
        a = _teacher_forced(model, p, images[2], [3, 4, 5])
        b = _teacher_forced(loaded, p, images[2], [3, 4, 5])
    assert torch.equal(a, b)
