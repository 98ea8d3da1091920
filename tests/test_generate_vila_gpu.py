"""KV-cached greedy generation of the VILA wrapper (VilaLlavaLlamaModel.generate, halva_amd/decode.py on `.llm`).

Tiny geometry: the weights of vila_step_init.npz (LoRA r = 4 unmerged) run as ONE head of 128 (the width of the decode kernels) with
max_position_embeddings 32, model_max_length 64 -> linear RoPE factor 2; tests/golden/generate_vila.npz holds 24 greedy steps of the
REFERENCE's own VILA forward on them (make_golden_generate_vila.py).  Bounds follow tests/test_generate_gpu.py: BOUND is what two bf16
forwards that differ only in row grouping disagree by on the last-row logits, floored at one bf16 ulp of the largest logit.

13B geometry (2 layers, as tests/test_fullsize_13b_vila_gpu.py): d = 5120, 40 heads x 128, F = 13824, vocab 32000, linear RoPE
factor 2, a prompt of about 4090 rows and a cache past 4096 slots."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load_npz, meta_of, tensors  # noqa: E402

N_NEW = 24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _build(z, g, lora=True, device="cuda:0"):
    """The product's VILA on vila_step_init's weights with generate_vila's decoder config (one head of 128, scaled RoPE)."""
    from halva_amd.llama import LlamaConfig, add_lora, load_hf_llama_weights
    from halva_amd.siglip import SiglipVisionConfig, SiglipVisionTower
    from halva_amd.vila_model import LlamaForCausalLM, MultimodalProjector, VilaConfig, VilaLlavaLlamaModel
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
    if lora:
        r, alpha, fac = int(z["lora_cfg"][0]), float(z["lora_cfg"][1]), tensors(z, "lora.")
        add_lora(m.llm, r, alpha)
        with torch.no_grad():
            for i, layer in enumerate(m.llm.model.layers):
                for sub, grp in layer.groups():
                    for gi, n in enumerate(grp.names):
                        key = "model.layers.%d.%s.%s" % (i, sub, n)
                        grp.A_cat[gi * r:(gi + 1) * r].copy_(fac[key + ".A"])
                        getattr(grp, n).lora_B["default"].weight.copy_(fac[key + ".B"])
    else:
        m._use_lora = False
    m.eval()
    return m


@pytest.fixture(scope="module")
def setup():
    _dev()
    z, g = load_npz("vila_step_init.npz"), load_npz("generate_vila.npz")
    model = _build(z, g)
    prompts = [torch.as_tensor(g["prompt.%d" % i]) for i in range(3)]
    images = torch.as_tensor(z["batch.images"][:3, 0]).to("cuda:0", torch.bfloat16)
    return model, prompts, images, g


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


@torch.no_grad()
def _teacher_forced(model, prompt, image, tokens):
    """logits of the prompt's last row and of each forced token, through prefill + decode_step on the VILA wrapper."""
    from halva_amd import decode as DEC
    embeds, plan = model._splice(prompt[None].cuda(), None, None, None, image[None])
    cache = DEC.KVCache(model, 1, embeds.shape[1] + len(tokens) + 1)
    out = [DEC.prefill(model, embeds, plan.seq_len, cache)]
    for t in tokens:
        out.append(DEC.decode_step(model, cache, torch.tensor([t], device="cuda")))
    return torch.cat(out)


@pytest.fixture(scope="module")
def bound(setup):
    model, prompts, images, _ = setup
    z = load_npz("vila_step_init.npz")
    long_row = torch.as_tensor(z["batch.input_ids"][2][:int(z["batch.attention_mask"][2].sum())])
    together = _full_last_logits(model, prompts + [long_row], torch.cat([images, images[2:3]]))[:3]
    alone = torch.cat([_full_last_logits(model, [p], images[i:i + 1]) for i, p in enumerate(prompts)])
    d = float((together - alone).abs().max())
    floor = 2.0 ** (math.floor(math.log2(float(together.abs().max()))) - 7)
    b = max(d, floor)
    print("row-grouping difference %.3e, bf16 floor %.3e -> bound %.3e" % (d, floor, b))
    return b


def test_the_fixture_runs_past_max_position_embeddings(setup):
    model, prompts, images, g = setup
    rope = model.llm.config.rope_scaling
    assert rope == {"type": "linear", "factor": 2.0}
    for i, p in enumerate(prompts):
        embeds, _ = model._splice(p[None].cuda(), None, None, None, images[i:i + 1])
        assert embeds.shape[1] + N_NEW - 1 > int(g["max_position_embeddings"])


def test_against_the_reference_golden(setup):
    """Teacher-forced through prefill + decode_step, every step's logits sit no further from the golden than 1.5 x the distance of the
    product's own cache-free forward from it; greedy generate() emits the golden's tokens up to the first step whose golden top-2 gap is
    below 4 x that bound (tests/test_generate_gpu.py's rule).  The steps past max_position_embeddings run on the scaled RoPE tables."""
    model, prompts, images, g = setup
    for i in range(3):
        p, toks = prompts[i], torch.as_tensor(g["tokens.%d" % i])
        glog, gap = torch.as_tensor(g["logits.%d" % i]).double(), torch.as_tensor(g["gap.%d" % i])
        assert len(toks) == N_NEW
        cached = _teacher_forced(model, p, images[i], toks[:-1].tolist()).double().cpu()
        full = torch.stack([_full_last_logits(model, [torch.cat([p, toks[:s]])], images[i:i + 1])[0] for s in range(N_NEW)]).double().cpu()
        d_cached, d_full = (cached - glog).abs().amax(-1), (full - glog).abs().amax(-1)
        print("prompt %d: |cached - golden| max %.3e, |full - golden| max %.3e" % (i, float(d_cached.max()), float(d_full.max())))
        bound_i = 1.5 * float(d_full.max())
        assert (d_cached <= bound_i).all(), (d_cached, d_full)
        gen = model.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[])[0].cpu()
        assert gen.shape == (N_NEW,)
        for s in range(N_NEW):
            if float(gap[s]) < 4 * bound_i:
                break
            assert int(gen[s]) == int(toks[s]), (i, s, gen.tolist(), toks.tolist())


def test_cached_decode_matches_full_forward(setup, bound):
    model, prompts, images, _ = setup
    worst = 0.0
    for i, p in enumerate(prompts):
        toks = model.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[])[0].tolist()
        cached = _teacher_forced(model, p, images[i], toks[:-1])
        for s in range(N_NEW):
            full = _full_last_logits(model, [torch.cat([p, torch.tensor(toks[:s], dtype=torch.long)])], images[i:i + 1])[0]
            worst = max(worst, float((cached[s] - full).abs().max()))
    print("cached vs full forward: max |logit diff| %.3e (bound %.3e)" % (worst, bound))
    assert worst <= 3 * bound          # the factor of tests/test_generate_gpu.py (GEMMs at M = 1 round differently than at M = T)


def _agree_until_close(a, b, logits_ref, gap):
    for s in range(min(len(a), len(b))):
        top2 = logits_ref[s].topk(2).values
        if float(top2[0] - top2[1]) < gap:
            return True
        if a[s] != b[s]:
            return False
    return True


def test_batched_ragged_equals_one_at_a_time(setup, bound):
    """A right-padded batch of three prompts gives each row the tokens of that prompt alone (up to a step whose top-2 gap is within the
    row-grouping noise: the batched GEMMs may round differently)."""
    model, prompts, images, _ = setup
    ids, mask = _pad_batch(prompts)
    batched = model.generate(ids, images=images, attention_mask=mask, max_new_tokens=N_NEW, eos_token_id=[])
    assert batched.shape == (3, N_NEW)
    for i, p in enumerate(prompts):
        single = model.generate(p[None], images=images[i:i + 1], max_new_tokens=N_NEW, eos_token_id=[])[0].tolist()
        ref = _teacher_forced(model, p, images[i], single[:-1])
        assert _agree_until_close(batched[i].tolist(), single, ref, 4 * bound), (i, batched[i].tolist(), single)


class _Tok:
    """Enough of a tokenizer for KeywordsStoppingCriteria: one keyword word -> one id."""
    bos_token_id = 1

    def __init__(self, word, tid):
        self.word, self.tid = word, tid

    def __call__(self, text):
        return type("E", (), {"input_ids": [1] + [self.tid if w == self.word else 3 for w in text.split()]})()

    def batch_decode(self, ids, skip_special_tokens=True):
        return [" ".join(self.word if i == self.tid else "x" for i in row) for row in ids.tolist()]


def test_output_contract(setup):
    from vila.mm_utils import KeywordsStoppingCriteria
    model, prompts, images, _ = setup
    p = prompts[1]
    free = model.generate(p[None], images=images[1:2], max_new_tokens=6, eos_token_id=[])
    assert free.dtype == torch.long and free.shape == (1, 6)                 # the new tokens only
    assert model.generate(p[None], images=images[1:2], max_new_tokens=3, eos_token_id=[]).shape == (1, 3)
    # fp16 images, a list and [B, n, 3, H, W] give the same tokens
    im = images[1:2]
    assert torch.equal(model.generate(p[None], images=im.half(), max_new_tokens=6, eos_token_id=[]),
                       model.generate(p[None], images=im.half().bfloat16(), max_new_tokens=6, eos_token_id=[]))
    assert torch.equal(model.generate(p[None], images=[im[0]], max_new_tokens=6, eos_token_id=[]), free)
    assert torch.equal(model.generate(p[None], images=im[:, None], max_new_tokens=6, eos_token_id=[]), free)
    # EOS: row 0's first token made the EOS id; that row is padded after it, the other runs on
    ids, mask = _pad_batch(prompts[:2])
    both = model.generate(ids, images=images[:2], attention_mask=mask, max_new_tokens=6, eos_token_id=[])
    eos = int(both[0, 0])
    stopped = model.generate(ids, images=images[:2], attention_mask=mask, max_new_tokens=6, eos_token_id=eos, pad_token_id=0)
    assert int(stopped[0, 0]) == eos and (stopped[0, 1:] == 0).all()
    if eos not in both[1].tolist():
        assert stopped.shape == (2, 6) and torch.equal(stopped[1], both[1])
    assert model.generate(p[None], images=im, max_new_tokens=6, eos_token_id=int(free[0, 0])).shape == (1, 1)
    # stopping criteria: a list; the sequence handed over is the new tokens only; any True stops the batch
    seen = []

    def spy(seq, scores):
        seen.append(seq.clone())
        return False
    stop_at = [lambda seq, scores: seq.shape[1] == 3]
    assert model.generate(p[None], images=im, max_new_tokens=6, eos_token_id=[], stopping_criteria=[spy]).shape == (1, 6)
    assert [s.shape[1] for s in seen] == [1, 2, 3, 4, 5, 6] and torch.equal(seen[-1], free)
    assert model.generate(p[None], images=im, max_new_tokens=6, eos_token_id=[], stopping_criteria=[spy] + stop_at).shape == (1, 3)
    tid = int(free[0, 2])
    k = free[0].tolist().index(tid)
    crit = KeywordsStoppingCriteria(["stop"], _Tok("stop", tid), p[None])
    out = model.generate(p[None], images=im, max_new_tokens=6, eos_token_id=[], stopping_criteria=[crit])
    assert out.shape == (1, k + 1) and torch.equal(out[0], free[0, :k + 1])
    # not implemented
    with pytest.raises(NotImplementedError):
        model.generate(p[None], images=im, num_beams=2, max_new_tokens=2)
    with pytest.raises(NotImplementedError):
        model.generate(p[None], images=im, do_sample=True, max_new_tokens=2)
    with pytest.raises(NotImplementedError):
        model.forward(input_ids=p[None].cuda(), images=im, use_cache=True)
    left = torch.zeros(1, len(p) + 2, dtype=torch.long)
    left[0, 2:] = p
    lmask = left != 0
    with pytest.raises(NotImplementedError):
        model.generate(left, images=im, attention_mask=lmask, max_new_tokens=2)


def test_full_cache_is_refused(setup):
    from halva_amd import decode as DEC
    model, prompts, images, _ = setup
    embeds, plan = model._splice(prompts[0][None].cuda(), None, None, None, images[:1])
    cache = DEC.KVCache(model, 1, embeds.shape[1] + 1)
    DEC.prefill(model, embeds, plan.seq_len, cache)
    DEC.decode_step(model, cache, torch.tensor([3], device="cuda"))
    with pytest.raises(RuntimeError, match="KV cache full"):
        DEC.decode_step(model, cache, torch.tensor([4], device="cuda"))


def _save_base(model, z, root):
    """A VILA checkpoint directory of the model's base weights: config.json naming llm / vision_tower / mm_projector sub-folders."""
    import json
    from safetensors.torch import save_file
    from halva_amd.llama import hf_llama_state_dict
    llm_dir, vt_dir, pj_dir = (os.path.join(root, d) for d in ("llm", "vision_tower", "mm_projector"))
    os.makedirs(llm_dir)
    os.makedirs(vt_dir)
    model.llm.config.save_pretrained(llm_dir)
    save_file({k: v.detach().cpu().contiguous() for k, v in hf_llama_state_dict(model.llm).items()}, os.path.join(llm_dir, "model.safetensors"))
    json.dump(dict(meta_of(z, "vis_cfg"), architectures=["SiglipVisionModel"]), open(os.path.join(vt_dir, "config.json"), "w"))
    save_file({k: v.to(torch.bfloat16).contiguous() for k, v in tensors(z, "vis.").items()}, os.path.join(vt_dir, "model.safetensors"))
    model.mm_projector.save_pretrained(pj_dir)
    json.dump({"llm_cfg": llm_dir, "vision_tower_cfg": vt_dir, "mm_projector_cfg": pj_dir, "mm_vision_select_layer": -2,
               "mm_vision_select_feature": "cls_patch", "model_type": "llava_llama"}, open(os.path.join(root, "config.json"), "w"))


def test_adapter_round_trip_through_load_pretrained_model(setup, tmp_path):
    """Random LoRA B factors and projector, written by the VILA trainer's save_lora_outputs over a base checkpoint, loaded back with
    vila.model.builder_halva.load_pretrained_model: generate() gives the in-memory model's tokens and logits, bitwise."""
    import types
    import vila.train.train_halva as TV
    from vila.model.builder_halva import load_pretrained_model
    _, prompts, images, g = setup
    z = load_npz("vila_step_init.npz")
    base = _build(z, g, lora=False)
    base_dir, out = str(tmp_path / "base"), str(tmp_path / "run-lora")
    _save_base(base, z, base_dir)
    model = _build(z, g)
    gen = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():
        for layer in model.llm.model.layers:
            for _, grp in layer.groups():
                for n in grp.names:
                    getattr(grp, n).lora_B["default"].weight.normal_(0.0, 0.05, generator=gen)
        for p in model.mm_projector.parameters():
            p.add_(torch.randn(p.shape, device=p.device, generator=gen).to(p.dtype) * 0.01)
            p.requires_grad_(True)
    grp = model.llm.model.layers[0].qkv
    args = types.SimpleNamespace(output_dir=out, lora_bias="none", lora_r=grp.r, lora_alpha=grp.scale * grp.r, lora_dropout=0.0)
    TV.save_lora_outputs(model, args)
    tok, loaded, proc, ctx = load_pretrained_model(out, "run-lora", base_dir)
    assert ctx > 0 and loaded.llm.config.rope_scaling == model.llm.config.rope_scaling
    for k, v in model.mm_projector.state_dict().items():
        assert torch.equal(loaded.mm_projector.state_dict()[k], v)
    p = prompts[2]
    a = model.generate(p[None], images=images[2:3], max_new_tokens=N_NEW, eos_token_id=[])
    b = loaded.generate(p[None], images=images[2:3], max_new_tokens=N_NEW, eos_token_id=[])
    assert torch.equal(a, b)
    assert torch.equal(_teacher_forced(model, p, images[2], a[0, :5].tolist()), _teacher_forced(loaded, p, images[2], a[0, :5].tolist()))


# ------------------------------------------------------------------------------------------------
# the VILA-13B geometry, 2 decoder layers
@pytest.fixture(scope="module")
def vila13b():
    _dev()
    import bench
    from halva_amd.vila_model import build_random_vila
    geo = dict(bench.LLAMA_13B, num_hidden_layers=2, rope_scaling={"type": "linear", "factor": 2.0})
    sig = dict(bench.SIGLIP_SO400M_384, num_hidden_layers=2)
    m = build_random_vila(geo, sig, lora_r=128, lora_alpha=256, seed=7, device="cuda", max_len=5120)
    gen = torch.Generator(device="cuda").manual_seed(8)
    with torch.no_grad():
        for layer in m.llm.model.layers:
            for _, grp in layer.groups():
                grp.weight_cat_t = None
                for n in grp.names:
                    getattr(grp, n).lora_B["default"].weight.normal_(0.0, 0.01, generator=gen)
    m.eval()
    g = torch.Generator().manual_seed(9)
    prompt = torch.randint(3, 32000, (3900,), generator=g)
    prompt[0], prompt[5] = 1, -200
    image = torch.randn(1, 3, 384, 384, generator=g).to("cuda", torch.bfloat16)
    return m, prompt, image


def test_13b_cached_logits_match_the_cache_free_forward_past_4096(vila13b):
    from halva_amd import decode as DEC
    model, prompt, image = vila13b
    n_new = 16
    toks = model.generate(prompt[None], images=image, max_new_tokens=n_new, eos_token_id=[])[0].tolist()
    assert len(toks) == n_new
    embeds, plan = model._splice(prompt[None].cuda(), None, None, None, image)
    T = embeds.shape[1]
    assert T == 3900 - 1 + 196 and T + n_new > 4096 and model.llm.model.rope(T + n_new, "cuda")[0].shape[0] >= T + n_new
    cached = _teacher_forced(model, prompt, image[0], toks[:-1])
    # bound: the row-grouping difference of two cache-free forwards of the prompt (alone / next to a second row)
    alone = _full_last_logits(model, [prompt], image)[0]
    pair = _full_last_logits(model, [prompt, prompt[:2000]], torch.cat([image, image]))[0]
    floor = 2.0 ** (math.floor(math.log2(float(alone.abs().max()))) - 7)
    bound = max(float((alone - pair).abs().max()), floor)
    worst = float((cached[0] - alone).abs().max())
    for s in (1, n_new // 2, n_new - 1):                       # positions up to T + 15 > 4096
        full = _full_last_logits(model, [torch.cat([prompt, torch.tensor(toks[:s], dtype=torch.long)])], image)[0]
        worst = max(worst, float((cached[s] - full).abs().max()))
    print("13B: cached vs full forward max |logit diff| %.3e, bound %.3e" % (worst, bound))
    assert worst <= 3 * bound
    # poison every cache slot at or beyond lens[b] with NaN / Inf: the decoded logits do not change
    cache = DEC.KVCache(model, 1, T + n_new)
    first = DEC.prefill(model, embeds, plan.seq_len, cache)
    for i in range(len(cache.k)):
        cache.k[i][:, :, T:].fill_(float("nan"))
        cache.v[i][:, :, T:].fill_(float("inf"))
    poisoned = [first] + [DEC.decode_step(model, cache, torch.tensor([t], device="cuda")) for t in toks[:-1]]
    assert torch.equal(torch.cat(poisoned), cached)


def test_13b_decode_kernels_row_invariance_and_scaled_positions():
    """At H = 40, Lcap = 5120, B = 16 (0.84 GB per K or V): row b of halva_decode_attn is bitwise the same as row b alone (B = 1), and
    slots beyond lens[b] (NaN / Inf) are never read.  halva_decode_rope_append takes the position only through the cos / sin rows: at
    p > 4096 with factor-2 tables it equals the rotation by those rows."""
    _dev()
    from halva_amd import kernels as K
    B, H, D, L = 16, 40, 128, 5120
    g = torch.Generator(device="cuda").manual_seed(3)
    kc = torch.randn(B, H, L, D, device="cuda", generator=g).to(torch.bfloat16)
    vc = torch.randn(B, H, L, D, device="cuda", generator=g).to(torch.bfloat16)
    q = torch.randn(B, 3 * H * D, device="cuda", generator=g).to(torch.bfloat16)
    lens_l = [L, L - 1, 4097, 4096, 4095, 257, 256, 1, 5000, 3000, 2048, 4500, 5119, 100, 4200, 4800]
    lens = torch.tensor(lens_l, dtype=torch.int32, device="cuda")
    for b, n in enumerate(lens_l):
        kc[b, :, n:] = float("nan")
        vc[b, :, n:] = float("inf")
    ws = torch.empty(K.decode_ws_bytes(B, H, L), dtype=torch.uint8, device="cuda")
    assert ws.numel() == B * H * ((L + K.decode_kc() - 1) // K.decode_kc()) * 130 * 4
    out = K.decode_attention(q, kc, vc, lens, ws, H, D)
    assert torch.isfinite(out.float()).all()
    ws1 = torch.empty(K.decode_ws_bytes(1, H, L), dtype=torch.uint8, device="cuda")
    for b in (0, 2, 3, 7, 12, 15):
        one = K.decode_attention(q[b:b + 1].contiguous(), kc[b:b + 1], vc[b:b + 1], lens[b:b + 1].clone(), ws1, H, D)
        assert torch.equal(one, out[b:b + 1]), b
    # fp64 check of one long row (L - 1 keys)
    b = 1
    n = lens_l[b]
    qh = q[b, :H * D].view(H, D).double()
    s = torch.einsum("hd,hld->hl", qh, kc[b, :, :n].double()) / math.sqrt(D)
    ref = torch.einsum("hl,hld->hd", s.softmax(-1), vc[b, :, :n].double()).reshape(-1)
    assert float((out[b, :H * D].double() - ref).abs().max()) < 2e-2
    del kc, vc
    # RoPE + append at a position past 4096 through factor-2 tables
    cos, sin = K.rope_tables(D, L, 10000.0, "cuda", 2.0)
    Bq = 2
    kc2 = torch.zeros(Bq, H, L, D, dtype=torch.bfloat16, device="cuda")
    vc2 = torch.zeros_like(kc2)
    qkv = torch.randn(Bq, 3 * H * D, device="cuda", generator=g).to(torch.bfloat16)
    x = qkv.clone()
    pos = [4100, 5119]
    lens2 = torch.tensor(pos, dtype=torch.int32, device="cuda")
    K.decode_rope_append(qkv, cos, sin, kc2, vc2, lens2, H, D)
    assert lens2.tolist() == [p + 1 for p in pos]
    for b, p in enumerate(pos):
        c, s_ = cos[p].float(), sin[p].float()
        for part in (0, 1):
            v = x[b, part * H * D:(part + 1) * H * D].view(H, D).float()
            x1, x2 = v[:, :D // 2], v[:, D // 2:]
            rot = torch.cat([x1 * c - x2 * s_, x2 * c + x1 * s_], -1).to(torch.bfloat16)
            got = qkv[b, :H * D].view(H, D) if part == 0 else kc2[b, :, p]
            assert torch.allclose(got.float(), rot.float(), rtol=2 ** -7, atol=1e-3), (b, p, part)
        assert torch.equal(vc2[b, :, p], x[b, 2 * H * D:].view(H, D))
        assert not kc2[b, :, :p].any() and not kc2[b, :, p + 1:].any()
