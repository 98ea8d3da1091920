#!/usr/bin/env python3
"""KV-cached greedy decoding on a random-weight LLaVA-1.5-7B geometry (32 layers, 32 x 128 heads, LoRA r = 128 unmerged, CLIP ViT-L/14 at
336 px): prefill ms of one image + 64 text tokens, decode ms per step and tokens/s at B = 1 and B = 16, and the split-KV decode-attention
kernel alone at B = 16, H = 32, L = 2048 as effective TB/s (bytes = sum_b 2 L_b H D 2) for each chunk size KC.  Not part of bench.py.

--model vila13b: the VILA-13B geometry instead (40 layers, 40 x 128 heads, d = 5120, F = 13824, LoRA r = 128 unmerged, SigLIP-so400m at
384 px -> 196 image tokens after mlp_downsample, linear RoPE factor 2): one image + 60 text tokens, the attention kernel at H = 40,
L = 4096.

--merged: after the unmerged measurement the same model is merged in place (merge_and_unload: halva_lora_merge once per target) and
the same decode steps are timed again; the record gains `merged` = {merge_s, weights_GB, decode}, next to the unmerged `weights_GB` /
`decode` of the same run on the same box.

--sample: the record gains `sample`: at V = 32000 and B = 1 and 16, us per call of the native token select (halva_sample_top_k_top_p)
and of the torch composition it stands in for (softmax, sort, cumsum, scatter, softmax, multinomial, as HF's warpers run them) on the same
logits, and ms per step of the whole sampled loop (decode.sample) beside the greedy loop (decode.greedy) on the same prompts.

--extend: the record gains `extend` (7B geometry, H = 32, B = 1 and 16): us per call of the extend attention (halva_extend_attn) at
past = 0, n = 639 beside halva_sdpa_causal_fwd_ld on the same rows (the prompt pass's attention), of the extend attention at past = 639,
n = 32, and - with the model - ms of a second turn of 32 ids through session.append beside a fresh start_session (vision tower, splice,
prompt pass) on the concatenated prompt.  Measurement only, no gate.

--fork: the record gains `fork` (7B geometry, H = 32, 16 members).  `attention`: us, bytes moved and TB/s of halva_fork_decode_attn at
prefix 2048 and at prefix 639, own = 32, beside halva_decode_attn on 16 materialised caches of the same logical keys, the two timed
alternately in one process and their outputs compared.  With the model: `sampled_loop`, generate's num_return_sequences=16 path
(decode.sample_fork) beside decode.sample on the prompt repeated 16 times - ms/step, prefill ms, cache GB; `questions`, 16 questions of 32
ids forked from one 639-row prompt and appended beside a fresh B = 16 start_session on the concatenated prompts.  Measurement only, no gate.

--beam: the record gains `beam` (7B geometry, H = 32, K = 5 beams, B = 1 and 4 prompts, prefix 639, own rows 32 and 512).  `attention`: us
of halva_beam_decode_attn beside halva_fork_decode_attn on the same rows with an identity ancestry table, timed alternately, outputs compared
bitwise.  `reorder`: us per step of halva_beam_advance beside the index_select of all layers' own K / V by the parents that the table
replaces, and the bytes either moves.  `select`: us of halva_beam_select beside log_softmax + topk over [B, K * V] in torch, V = 32000, and whether the two return the same
candidates - on the fp32 logits that are timed, on the same logits rounded to bf16 and on their roundings to multiples of 0.5 (ties inside a
row), with every differing place and its float64 score gap.
With the model: `loop`, ms/step of the beam loop beside the greedy loop on the same prompts.  Measurement only, no gate.

--contrast: the record gains `contrast`: at V = 32000 and B = 1 and 16, us per call of the contrast select (halva_contrast_select) beside
halva_sample_top_k_top_p on one of its two inputs and beside the torch composition of the same rule (max, compare, two products, a
difference, masked_fill, then torch_select) - and, with the model, ms per step of the contrast loop (decode.contrast: 2 B rows) beside the
greedy loop at B on the same prompts.  Measurement only, no gate.  Without --out it writes profiles/r14_contrast.json.

    python tools/bench_decode.py [--model llava7b | vila13b] [--merged] [--sample] [--extend] [--fork] [--beam] [--contrast] [--out profiles/r07_decode.json] [--steps 32]
"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _time(fn, reps, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def attn_kernel(kc_values=(64, 128, 256), B=16, H=32, L=2048, D=128, reps=50):
    from halva_amd import kernels as K
    dev = "cuda"
    kc = torch.randn(B, H, L, D, device=dev).to(torch.bfloat16)
    vc = torch.randn(B, H, L, D, device=dev).to(torch.bfloat16)
    q = torch.randn(B, 3 * H * D, device=dev).to(torch.bfloat16)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    nbytes = 2 * B * L * H * D * 2
    res = {}
    for c in kc_values:
        ws = torch.empty(K.decode_ws_bytes(B, H, L, c), dtype=torch.uint8, device=dev)
        ms = _time(lambda: K.decode_attention(q, kc, vc, lens, ws, H, D, kc=c), reps, warmup=5)
        res[str(c)] = {"us": round(ms * 1e3, 2), "TB_s": round(nbytes / (ms * 1e-3) / 1e12, 3)}
    return {"B": B, "H": H, "L": L, "D": D, "bytes": nbytes, "kc_shipped": K.decode_kc(), "by_kc": res}


def model_7b():
    from halva_amd.llava_model import build_random_llava
    cfg = dict(vocab_size=32000, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
               max_position_embeddings=4096, rms_norm_eps=1e-5, pad_token_id=0)
    vis = dict(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16, image_size=336, patch_size=14,
               layer_norm_eps=1e-5)
    m = build_random_llava(cfg, vis, lora_r=128, lora_alpha=256, seed=0, device="cuda", max_len=2048)
    with torch.no_grad():
        for layer in m.model.layers:
            for _, grp in layer.groups():
                grp.weight_cat_t = None          # (training-only copy; inference does not keep it)
                for Bf in grp._Bs():
                    Bf.normal_(0.0, 0.02)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def model_vila13b():
    import bench
    from halva_amd.vila_model import build_random_vila
    cfg = dict(bench.LLAMA_13B, rope_scaling={"type": "linear", "factor": 2.0})
    m = build_random_vila(cfg, dict(bench.SIGLIP_SO400M_384), lora_r=128, lora_alpha=256, seed=0, device="cuda", max_len=4096)
    with torch.no_grad():
        for layer in m.llm.model.layers:
            for _, grp in layer.groups():
                grp.weight_cat_t = None
                for Bf in grp._Bs():
                    Bf.normal_(0.0, 0.02)
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def decode_numbers(m, steps, text=64, image=336):
    from halva_amd import decode as DEC
    g = torch.Generator().manual_seed(0)
    res = {}
    for B in (1, 16):
        ids = torch.randint(3, 32000, (B, text), generator=g)
        ids[:, 0] = 1
        ids[:, 6] = -200
        images = torch.randn(B, 3, image, image, generator=g).to("cuda", torch.bfloat16)
        with torch.no_grad():
            embeds, plan = m._splice(ids.cuda(), None, None, None, images)
            T = embeds.shape[1]
            state = {}

            def do_prefill():
                state["cache"] = DEC.KVCache(m, B, T + steps + 8)
                state["logits"] = DEC.prefill(m, embeds, plan.seq_len, state["cache"])
            pre_ms = _time(do_prefill, 3, warmup=1)
            tok = state["logits"].argmax(-1)

            def do_steps():
                cache = state["cache"]
                cache.lens.copy_(torch.full_like(cache.lens, T))          # every timed pass decodes from the same position
                cache.filled = T
                for _ in range(steps):
                    DEC.decode_step(m, cache, tok)
            step_ms = _time(do_steps, 3, warmup=1) / steps
        res["B%d" % B] = {"prompt_rows": T, "prefill_ms": round(pre_ms, 2), "decode_ms_per_step": round(step_ms, 3),
                          "tokens_per_s": round(B * 1000.0 / step_ms, 1)}
    return res


SAMPLE_SETTINGS = ((0.2, 50, 0.7), (1.0, 0, 0.9))      # (temperature, top_k, top_p): the scripts' call with HF's top_k, and top-p alone


def torch_select(logits, temperature, top_k, top_p):
    """HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> softmax -> multinomial, restated in torch."""
    s = logits / temperature
    if top_k > 0:
        s = s.masked_fill(s < torch.topk(s, top_k)[0][..., -1, None], -float("inf"))
    if top_p < 1.0:
        sl, si = torch.sort(s, descending=False)
        remove = sl.softmax(-1).cumsum(-1) <= 1 - top_p
        remove[..., -1:] = False
        s = s.masked_fill(remove.scatter(1, si, remove), -float("inf"))
    return torch.multinomial(s.softmax(-1), 1).squeeze(1)


def select_numbers(V=32000, reps=200):
    from halva_amd import kernels as K
    res = {}
    for B in (1, 16):
        logits = (8.0 * torch.randn(B, V, device="cuda")).bfloat16().float()
        u = torch.rand(B, device="cuda")
        for T, k, p in SAMPLE_SETTINGS:
            native = _time(lambda: K.sample_top_k_top_p(logits, u, T, k, p), reps, warmup=10)
            composed = _time(lambda: torch_select(logits, T, k, p), reps, warmup=10)
            res["B%d_T%g_k%d_p%g" % (B, T, k, p)] = {"native_us": round(native * 1e3, 2), "torch_us": round(composed * 1e3, 2)}
    return {"V": V, "by_setting": res}


def loop_numbers(m, steps, text=64, image=336):
    """ms per step of the whole loop, host syncs included: (a run of steps + 1 tokens - a run of 1 token) / steps."""
    import time
    from halva_amd import decode as DEC
    g = torch.Generator().manual_seed(0)
    T_, k, p = SAMPLE_SETTINGS[0]
    none = torch.empty(0, dtype=torch.long, device="cuda")
    res = {}
    for B in (1, 16):
        ids = torch.randint(3, 32000, (B, text), generator=g)
        ids[:, 0] = 1
        ids[:, 6] = -200
        images = torch.randn(B, 3, image, image, generator=g).to("cuda", torch.bfloat16)
        with torch.no_grad():
            embeds, plan = m._splice(ids.cuda(), None, None, None, images)

        def wall(fn, n):
            best = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(n)
                torch.cuda.synchronize()
                best.append(time.perf_counter() - t0)
            return statistics.median(best) * 1e3

        def greedy(n):
            DEC.greedy(m, embeds, plan.seq_len, n, none, 0)

        def sampled(n):
            DEC.sample(m, embeds, plan.seq_len, n, none, 0, T_, k, p)
        greedy(2), sampled(2)
        res["B%d" % B] = {"greedy_ms_per_step": round((wall(greedy, steps + 1) - wall(greedy, 1)) / steps, 3),
                          "sampled_ms_per_step": round((wall(sampled, steps + 1) - wall(sampled, 1)) / steps, 3)}
    return {"temperature": T_, "top_k": k, "top_p": p, "loop": res}


CONTRAST = (0.5, 0.1)          # (alpha, beta): VCD's defaults


def torch_contrast_select(logits, logits_cd, alpha, beta, temperature, top_k, top_p):
    """halva_contrast_select's rule composed in torch, then torch_select."""
    cut = logits.max(-1, keepdim=True)[0] + math.log(beta)
    x = ((1 + alpha) * logits - alpha * logits_cd).masked_fill(logits < cut, -float("inf"))
    return torch_select(x, temperature, top_k, top_p)


def contrast_select_numbers(V=32000, reps=200):
    from halva_amd import kernels as K
    alpha, beta = CONTRAST
    res = {}
    for B in (1, 16):
        logits = (8.0 * torch.randn(B, V, device="cuda")).bfloat16().float()
        logits_cd = (logits + 2.0 * torch.randn(B, V, device="cuda")).bfloat16().float()
        u = torch.rand(B, device="cuda")
        for T, k, p in SAMPLE_SETTINGS:
            native = _time(lambda: K.contrast_select(logits, logits_cd, u, alpha, beta, T, k, p), reps, warmup=10)
            plain = _time(lambda: K.sample_top_k_top_p(logits, u, T, k, p), reps, warmup=10)
            composed = _time(lambda: torch_contrast_select(logits, logits_cd, alpha, beta, T, k, p), reps, warmup=10)
            res["B%d_T%g_k%d_p%g" % (B, T, k, p)] = {"contrast_us": round(native * 1e3, 2), "sample_us": round(plain * 1e3, 2),
                                                     "torch_us": round(composed * 1e3, 2)}
    return {"V": V, "alpha": alpha, "beta": beta, "by_setting": res}


def contrast_loop_numbers(m, steps, text=64, image=336):
    """ms per step of the greedy contrast loop (2 B rows in one cache) beside the greedy loop at B, host syncs included."""
    import time
    from halva_amd import decode as DEC
    from halva_amd.contrast import add_diffusion_noise
    g = torch.Generator().manual_seed(0)
    alpha, beta = CONTRAST
    none = torch.empty(0, dtype=torch.long, device="cuda")
    res = {}
    for B in (1, 16):
        ids = torch.randint(3, 32000, (B, text), generator=g)
        ids[:, 0] = 1
        ids[:, 6] = -200
        images = torch.randn(B, 3, image, image, generator=g).to("cuda", torch.bfloat16)
        with torch.no_grad():
            embeds, plan = m._splice(ids.cuda(), None, None, None, images)
            embeds_cd, plan_cd = m._splice(ids.cuda(), None, None, None, add_diffusion_noise(images, 500))

        def wall(fn, n):
            best = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(n)
                torch.cuda.synchronize()
                best.append(time.perf_counter() - t0)
            return statistics.median(best) * 1e3

        def greedy(n):
            DEC.greedy(m, embeds, plan.seq_len, n, none, 0)

        def contrast(n):
            DEC.contrast(m, embeds, plan.seq_len, embeds_cd, plan_cd.seq_len, n, none, 0, alpha, beta)
        greedy(2), contrast(2)
        res["B%d" % B] = {"greedy_ms_per_step": round((wall(greedy, steps + 1) - wall(greedy, 1)) / steps, 3),
                          "contrast_ms_per_step": round((wall(contrast, steps + 1) - wall(contrast, 1)) / steps, 3)}
    return res


def extend_kernel_numbers(H=32, D=128, T=639, n2=32, reps=20):
    from halva_amd import hip
    from halva_amd import kernels as K
    dev = "cuda"
    res = {}
    for B in (1, 16):
        L = T + n2
        qkv = torch.randn(B, T, 3 * H * D, device=dev).to(torch.bfloat16)
        kc = torch.randn(B, H, L, D, device=dev).to(torch.bfloat16)
        vc = torch.randn(B, H, L, D, device=dev).to(torch.bfloat16)
        zero = torch.zeros(B, dtype=torch.int32, device=dev)
        full = torch.full((B,), T, dtype=torch.int32, device=dev)
        out = torch.empty(B, T, H * D, dtype=torch.bfloat16, device=dev)
        lse = torch.empty(B, H, T, dtype=torch.float32, device=dev)
        ext0 = _time(lambda: K.extend_attention(qkv, kc, vc, zero, full, None, H, D, out=out), reps, warmup=3)
        sdpa = _time(lambda: hip.call("halva_sdpa_causal_fwd_ld", hip.ptr(qkv), hip.ptr(out), H * D, hip.ptr(lse), hip.ptr(zero), hip.ptr(full),
                                      B, T, H, D, 0.0, hip.stream_ptr()), reps, warmup=3)
        q2 = qkv[:, :n2].contiguous()
        out2 = torch.empty(B, n2, H * D, dtype=torch.bfloat16, device=dev)
        few = torch.full((B,), n2, dtype=torch.int32, device=dev)
        ext1 = _time(lambda: K.extend_attention(q2, kc, vc, full, few, None, H, D, out=out2), reps, warmup=3)
        res["B%d" % B] = {"extend_past0_n%d_us" % T: round(ext0 * 1e3, 1), "sdpa_causal_fwd_T%d_us" % T: round(sdpa * 1e3, 1),
                          "extend_past%d_n%d_us" % (T, n2): round(ext1 * 1e3, 1)}
    return res


def extend_turn_numbers(m, text=64, image=336, turn=32):
    g = torch.Generator().manual_seed(0)
    res = {}
    for B in (1, 16):
        ids = torch.randint(3, 32000, (B, text), generator=g)
        ids[:, 0] = 1
        ids[:, 6] = -200
        more = torch.randint(3, 32000, (B, turn), generator=g)
        images = torch.randn(B, 3, image, image, generator=g).to("cuda", torch.bfloat16)
        state = {}

        def first():
            state["ses"] = m.start_session(ids, images=images, max_len=2 * (text + turn) + 1024)

        def second():
            ses = state["ses"]
            ses.lens = list(state["lens"])          # every timed pass appends at the same position
            ses._set_lens()
            ses.append(more)
        first()
        state["lens"] = list(state["ses"].lens)
        app_ms = _time(second, 3, warmup=1)
        both = torch.cat([ids, more], 1)
        fresh_ms = _time(lambda: m.start_session(both, images=images, max_len=2 * (text + turn) + 1024), 3, warmup=1)
        res["B%d" % B] = {"prompt_rows": state["lens"][0], "turn_ids": turn, "append_ms": round(app_ms, 2), "fresh_prefill_ms": round(fresh_ms, 2)}
    return res


FORK_N, FORK_OWN = 16, 32


def fork_attn_bytes(prefix, own, n, H, D=128):
    """K and V bytes the two attentions have to read for n members of `prefix` shared and `own` private bf16 key rows each: (the fork:
    the prefix once per block of 16 members, the own rows per member; n materialised caches: everything per member)."""
    row = 2 * H * D * 2
    return (-(-n // 16) * prefix + n * own) * row, n * (prefix + own) * row


def fork_kernel_numbers(H=32, D=128, reps=50, rounds=3):
    from halva_amd import kernels as K
    dev = "cuda"
    n, own = FORK_N, FORK_OWN
    res = {}
    for prefix in (2048, 639):
        Lown = 2 * own
        pk = torch.randn(1, H, prefix, D, device=dev).to(torch.bfloat16)
        pv = torch.randn(1, H, prefix, D, device=dev).to(torch.bfloat16)
        kc = torch.randn(n, H, Lown, D, device=dev).to(torch.bfloat16)
        vc = torch.randn(n, H, Lown, D, device=dev).to(torch.bfloat16)
        q = torch.randn(n, 3 * H * D, device=dev).to(torch.bfloat16)
        plens = torch.tensor([prefix], dtype=torch.int32, device=dev)
        of = torch.zeros(n, dtype=torch.int32, device=dev)
        olens = torch.full((n,), own, dtype=torch.int32, device=dev)
        ws = torch.empty(K.fork_ws_bytes(n, H, prefix, Lown), dtype=torch.uint8, device=dev)
        # the same logical keys as n caches of their own
        L = prefix + own
        km = torch.cat([pk.expand(n, -1, -1, -1), kc[:, :, :own]], 2).contiguous()
        vm = torch.cat([pv.expand(n, -1, -1, -1), vc[:, :, :own]], 2).contiguous()
        lens = torch.full((n,), L, dtype=torch.int32, device=dev)
        ws1 = torch.empty(K.decode_ws_bytes(n, H, L), dtype=torch.uint8, device=dev)
        fork = lambda: K.fork_decode_attention(q, pk, pv, plens, of, kc, vc, olens, ws, H, D)      # noqa: E731
        flat = lambda: K.decode_attention(q, km, vm, lens, ws1, H, D)                                # noqa: E731
        diff = float((fork().float() - flat().float()).abs().max())
        tf, tm = [], []
        for _ in range(rounds):                   # alternately: other work shares the machine
            tf.append(_time(fork, reps, warmup=5))
            tm.append(_time(flat, reps, warmup=5))
        bf, bm = fork_attn_bytes(prefix, own, n, H, D)
        f_ms, m_ms = statistics.median(tf), statistics.median(tm)
        res["prefix%d" % prefix] = {
            "members": n, "own": own, "max_abs_diff": diff,
            "fork": {"us": round(f_ms * 1e3, 2), "bytes": bf, "TB_s": round(bf / (f_ms * 1e-3) / 1e12, 3), "us_rounds": [round(t * 1e3, 2) for t in tf]},
            "materialised": {"us": round(m_ms * 1e3, 2), "bytes": bm, "TB_s": round(bm / (m_ms * 1e-3) / 1e12, 3),
                             "us_rounds": [round(t * 1e3, 2) for t in tm]}}
    return res


def _cache_gb(m, rows):
    cfg = m.decode_stack().lm.config
    return round(cfg.num_hidden_layers * 2 * rows * cfg.hidden_size * 2 / 1e9, 3)


def fork_loop_numbers(m, steps, text=64, image=336):
    """The sampled loop with 16 continuations of one prompt: one prompt pass and a fork, beside the prompt repeated 16 times."""
    import time
    from halva_amd import decode as DEC
    g = torch.Generator().manual_seed(0)
    T_, k, p = SAMPLE_SETTINGS[0]
    n = FORK_N
    none = torch.empty(0, dtype=torch.long, device="cuda")
    ids = torch.randint(3, 32000, (1, text), generator=g)
    ids[:, 0] = 1
    ids[:, 6] = -200
    images = torch.randn(1, 3, image, image, generator=g).to("cuda", torch.bfloat16)
    with torch.no_grad():
        e1, plan1 = m._splice(ids.cuda(), None, None, None, images)
        e16, plan16 = m._splice(ids.repeat(n, 1).cuda(), None, None, None, images.repeat(n, 1, 1, 1))
    T = e1.shape[1]

    def wall(fn, cnt):
        best = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(cnt)
            torch.cuda.synchronize()
            best.append(time.perf_counter() - t0)
        return statistics.median(best) * 1e3

    def forked(cnt):
        DEC.sample_fork(m, e1, plan1.seq_len, n, cnt, none, 0, T_, k, p)

    def repeated(cnt):
        DEC.sample(m, e16, plan16.seq_len, cnt, none, 0, T_, k, p)
    forked(2), repeated(2)
    with torch.no_grad():
        pre1 = _time(lambda: DEC.prefill(m, e1, plan1.seq_len, DEC.KVCache(m, 1, T)), 3, warmup=1)
        pre16 = _time(lambda: DEC.prefill(m, e16, plan16.seq_len, DEC.KVCache(m, n, T + steps + 1)), 3, warmup=1)
    return {"prompt_rows": T, "members": n, "steps": steps, "temperature": T_, "top_k": k, "top_p": p,
            "fork": {"ms_per_step": round((wall(forked, steps + 1) - wall(forked, 1)) / steps, 3), "prefill_ms": round(pre1, 2),
                     "cache_GB": _cache_gb(m, T + n * (steps + 1))},
            "repeated_prompt": {"ms_per_step": round((wall(repeated, steps + 1) - wall(repeated, 1)) / steps, 3), "prefill_ms": round(pre16, 2),
                                "cache_GB": _cache_gb(m, n * (T + steps + 1))}}


def fork_question_numbers(m, text=64, image=336, turn=32):
    """16 questions of `turn` ids about one image: forked from one session and appended, beside a fresh B = 16 start_session."""
    g = torch.Generator().manual_seed(0)
    n = FORK_N
    ids = torch.randint(3, 32000, (1, text), generator=g)
    ids[:, 0] = 1
    ids[:, 6] = -200
    more = torch.randint(3, 32000, (n, turn), generator=g)
    images = torch.randn(1, 3, image, image, generator=g).to("cuda", torch.bfloat16)
    ses = m.start_session(ids, images=images, max_len=text + 1024)

    def forked():
        ses.fork(n, max_new=2 * turn).append(more)
    both, images16 = torch.cat([ids.repeat(n, 1), more], 1), images.repeat(n, 1, 1, 1)
    f_ms = _time(forked, 3, warmup=1)
    fresh_ms = _time(lambda: m.start_session(both, images=images16, max_len=text + turn + 1024), 3, warmup=1)
    return {"prompt_rows": ses.lens[0], "questions": n, "turn_ids": turn, "fork_append_ms": round(f_ms, 2), "fresh_prefill_ms": round(fresh_ms, 2)}


BEAM_K, BEAM_PREFIX, BEAM_OWN = 5, 639, (32, 512)


def _alternately(a, b, reps, rounds):
    ta, tb = [], []
    for _ in range(rounds):                       # alternately: other work shares the machine
        ta.append(_time(a, reps, warmup=5))
        tb.append(_time(b, reps, warmup=5))
    return statistics.median(ta), statistics.median(tb), ta, tb


def _select_compare(K, logits, scores, B, Kb, C, V):
    """halva_beam_select beside log_softmax + topk on the same inputs: whether the candidate lists are equal, and for every place where they
    differ the two flat indices and the float64 gap between their scores (0 = a tie that each side's tie rule ordered its own way)."""
    s, t, b = K.beam_select(logits, scores, Kb, C)
    mine = (b.long() * V + t.long()).cpu()
    theirs = (torch.log_softmax(logits, -1) + scores[:, None]).view(B, Kb * V).topk(C, 1).indices.cpu()
    x = logits.double().cpu()
    flat = (scores.double().cpu()[:, None] + (x - torch.logsumexp(x, 1)[:, None])).view(B, Kb * V)
    diff = []
    for p, r in (mine != theirs).nonzero().tolist():
        a, o = int(mine[p, r]), int(theirs[p, r])
        diff.append({"prompt": p, "rank": r, "native": a, "torch": o, "score_gap_f64": abs(float(flat[p, a] - flat[p, o])),
                     "logits_equal": bool(logits.view(B, Kb * V)[p, a] == logits.view(B, Kb * V)[p, o]), "same_beam": a // V == o // V})
    return {"same_candidates": not diff, "same_candidate_sets": all(sorted(mine[p].tolist()) == sorted(theirs[p].tolist()) for p in range(B)),
            "differing": diff[:16]}


def beam_kernel_numbers(H=32, D=128, layers=32, V=32000, reps=50, rounds=3):
    from halva_amd import kernels as K
    dev = "cuda"
    Kb, prefix = BEAM_K, BEAM_PREFIX
    att, reorder, select = {}, {}, {}
    for B in (1, 4):
        M = B * Kb
        pk = torch.randn(B, H, prefix, D, device=dev).to(torch.bfloat16)
        pv = torch.randn(B, H, prefix, D, device=dev).to(torch.bfloat16)
        plens = torch.full((B,), prefix, dtype=torch.int32, device=dev)
        of = torch.arange(B, dtype=torch.int32, device=dev).repeat_interleave(Kb)
        q = torch.randn(M, 3 * H * D, device=dev).to(torch.bfloat16)
        parents = (torch.arange(B, device=dev).repeat_interleave(Kb) * Kb + torch.randint(0, Kb, (M,), device=dev)).to(torch.int32)
        for own in BEAM_OWN:
            Lown = own + 1
            kc = torch.randn(M, H, Lown, D, device=dev).to(torch.bfloat16)
            vc = torch.randn(M, H, Lown, D, device=dev).to(torch.bfloat16)
            olens = torch.full((M,), own, dtype=torch.int32, device=dev)
            ws = torch.empty(K.fork_ws_bytes(M, H, prefix, Lown), dtype=torch.uint8, device=dev)
            anc = torch.arange(M, dtype=torch.int32, device=dev)[:, None].expand(M, Lown).contiguous()
            beam = lambda: K.beam_decode_attention(q, pk, pv, plens, of, kc, vc, olens, anc, ws, H, D)      # noqa: E731
            fork = lambda: K.fork_decode_attention(q, pk, pv, plens, of, kc, vc, olens, ws, H, D)           # noqa: E731
            same = bool(torch.equal(beam().view(torch.int16), fork().view(torch.int16)))
            b_ms, f_ms, tb, tf = _alternately(beam, fork, reps, rounds)
            att["B%d_own%d" % (B, own)] = {"members": M, "prefix": prefix, "own": own, "bitwise_equal": same,
                                           "beam_us": round(b_ms * 1e3, 2), "fork_us": round(f_ms * 1e3, 2),
                                           "beam_us_rounds": [round(t * 1e3, 2) for t in tb], "fork_us_rounds": [round(t * 1e3, 2) for t in tf]}
            # what the table replaces: every layer's own K and V gathered by the parents, each step
            ks = [torch.randn(M, H, Lown, D, device=dev).to(torch.bfloat16) for _ in range(2 * layers)]
            idx = parents.long()
            anc2 = torch.zeros(2, M, Lown, dtype=torch.int32, device=dev)
            anc2[0] = anc
            hold = {}

            def gather():
                hold["out"] = [t.index_select(0, idx) for t in ks]

            def advance():
                K.beam_advance(anc2[0], anc2[1], parents, olens)
            g_ms, a_ms, tg, ta = _alternately(gather, advance, max(reps // 5, 5), rounds)
            reorder["B%d_own%d" % (B, own)] = {"layers": layers, "index_select_us_per_step": round(g_ms * 1e3, 1),
                                               "index_select_bytes": 2 * 2 * layers * M * H * own * D * 2,
                                               "beam_advance_us_per_step": round(a_ms * 1e3, 2), "beam_advance_bytes": 2 * 4 * M * own}
            del ks, hold
        scores = -torch.rand(M, device=dev) * 4
        C = 2 * Kb
        raw = 8.0 * torch.randn(M, V, device=dev)
        # timed on fp32 logits; compared on those, on the same logits rounded to bf16 and on their roundings to multiples of 0.5, where equal
        # values inside a row leave the order to each side's tie rule (the kernel's: lower flat index; torch.topk's: unspecified)
        rec = {"K": Kb, "C": C, "V": V}
        for name, logits in (("fp32_logits", raw), ("bf16_rounded_logits", raw.bfloat16().float()),
                             ("half_integer_logits", torch.round(raw * 2) / 2)):
            rec[name] = _select_compare(K, logits, scores, B, Kb, C, V)
        logits = raw
        native = lambda: K.beam_select(logits, scores, Kb, C)                                                # noqa: E731
        composed = lambda: (torch.log_softmax(logits, -1) + scores[:, None]).view(B, Kb * V).topk(C, 1)     # noqa: E731
        n_ms, c_ms, _, _ = _alternately(native, composed, reps, rounds)
        rec.update({"native_us": round(n_ms * 1e3, 2), "torch_us": round(c_ms * 1e3, 2)})
        select["B%d" % B] = rec
    return {"attention": att, "reorder": reorder, "select": select}


def beam_loop_numbers(m, steps, text=64, image=336):
    """ms per step of the whole beam loop (select, host sync, BeamState, advance, layers) beside the greedy loop on the same prompts:
    (a run of steps + 1 tokens - a run of 1 token) / steps; no EOS id, so every run takes all its steps."""
    import time
    from halva_amd import decode as DEC
    g = torch.Generator().manual_seed(0)
    none = torch.empty(0, dtype=torch.long, device="cuda")
    res = {}
    for B in (1, 4):
        ids = torch.randint(3, 32000, (B, text), generator=g)
        ids[:, 0] = 1
        ids[:, 6] = -200
        images = torch.randn(B, 3, image, image, generator=g).to("cuda", torch.bfloat16)
        with torch.no_grad():
            embeds, plan = m._splice(ids.cuda(), None, None, None, images)

        def wall(fn, n):
            best = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(n)
                torch.cuda.synchronize()
                best.append(time.perf_counter() - t0)
            return statistics.median(best) * 1e3

        def greedy(n):
            DEC.greedy(m, embeds, plan.seq_len, n, none, 0)

        def beams(n):
            cache = DEC.KVCache(m, B, embeds.shape[1])
            logits = DEC.prefill(m, embeds, plan.seq_len, cache)
            cache.filled = int(plan.seq_len.max())
            ses = DEC.DecodeSession(m, cache, logits, plan.seq_len.tolist(), m._lm_config())
            ses.beam_search(BEAM_K, n, eos_token_id=[], early_stopping="never")
        greedy(2), beams(2)
        res["B%d" % B] = {"prompt_rows": embeds.shape[1], "beams": BEAM_K, "steps": steps,
                          "greedy_ms_per_step": round((wall(greedy, steps + 1) - wall(greedy, 1)) / steps, 3),
                          "beam_ms_per_step": round((wall(beams, steps + 1) - wall(beams, 1)) / steps, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--model", choices=("llava7b", "vila13b"), default="llava7b")
    ap.add_argument("--merged", action="store_true", help="also time the decode step after merge_and_unload() on the same model")
    ap.add_argument("--sample", action="store_true", help="also time the native token select, its torch composition and the sampled loop")
    ap.add_argument("--extend", action="store_true", help="also time the extend attention beside the prompt pass's, and a session's second turn")
    ap.add_argument("--fork", action="store_true",
                    help="also time the fork decode attention beside 16 materialised caches, the num_return_sequences=16 loop beside the "
                         "repeated prompt, and 16 forked questions beside a fresh prefill")
    ap.add_argument("--beam", action="store_true",
                    help="also time the beam decode attention beside the fork attention (identity table), halva_beam_advance beside the "
                         "index_select it replaces, halva_beam_select beside log_softmax + topk, and the beam loop beside the greedy loop")
    ap.add_argument("--contrast", action="store_true",
                    help="also time the contrast select beside the plain select and its torch composition, and the contrast loop (2 B rows) "
                         "beside the greedy loop")
    a = ap.parse_args()
    if a.contrast and a.out is None:
        a.out = os.path.join(ROOT, "profiles", "r14_contrast.json")
    from halva_amd import hip
    hip.load()
    torch.cuda.set_device(0)
    vila = a.model == "vila13b"
    rec = {"device": torch.cuda.get_device_name(0), "model": a.model,
           "decode_attn": attn_kernel(H=40, L=4096) if vila else attn_kernel()}
    if a.sample:
        rec["sample"] = select_numbers()
    if a.contrast:
        rec["contrast"] = contrast_select_numbers()
    if a.extend:
        rec["extend"] = extend_kernel_numbers()
    if a.fork:
        rec["fork"] = {"attention": fork_kernel_numbers(H=40 if vila else 32)}
    if a.beam:
        rec["beam"] = beam_kernel_numbers(H=40 if vila else 32, layers=40 if vila else 32)
    if not a.skip_model:
        m = model_vila13b() if vila else model_7b()
        def weights_gb():
            return round(sum(p.numel() * p.element_size() for n, p in m.named_parameters() if "vision_tower" not in n) / 1e9, 2)

        def numbers():
            return decode_numbers(m, a.steps, text=60, image=384) if vila else decode_numbers(m, a.steps)
        rec["weights_GB"] = weights_gb()
        rec["decode"] = numbers()
        if a.sample:
            rec["sample"].update(loop_numbers(m, a.steps, text=60, image=384) if vila else loop_numbers(m, a.steps))
        if a.contrast:
            rec["contrast"]["loop"] = contrast_loop_numbers(m, a.steps, text=60, image=384) if vila else contrast_loop_numbers(m, a.steps)
        if a.extend:
            rec["extend"]["second_turn"] = extend_turn_numbers(m, text=60, image=384) if vila else extend_turn_numbers(m)
        if a.fork:
            rec["fork"]["sampled_loop"] = fork_loop_numbers(m, a.steps, text=60, image=384) if vila else fork_loop_numbers(m, a.steps)
            rec["fork"]["questions"] = fork_question_numbers(m, text=60, image=384) if vila else fork_question_numbers(m)
        if a.beam:
            rec["beam"]["loop"] = beam_loop_numbers(m, a.steps, text=60, image=384) if vila else beam_loop_numbers(m, a.steps)
        if a.merged:
            import time
            torch.cuda.synchronize()
            t0 = time.time()
            m.merge_and_unload()
            torch.cuda.synchronize()
            rec["merged"] = {"merge_s": round(time.time() - t0, 3), "weights_GB": weights_gb(), "decode": numbers()}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
