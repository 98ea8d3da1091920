"""The kernels that extend a kept KV cache by a block of rows (halva_amd/csrc/kvcache.hip: halva_extend_rope_append, halva_extend_attn,
halva_extend_advance), alone: H = 2, D = 128, Lcap = 320.

past = [0, 37, 130, 255], n_new = [65, 1, 33, 64], n = 65: key counts on both sides of the 64- and 256-boundaries, query blocks of 1, 32 + 1
and 64 + 1 rows, an empty cache.  Cache slots at or beyond past + n_new, q rows at or beyond n_new and the workspace hold NaN / Inf; out
rows at or beyond n_new (and out's columns beyond H*D) hold a sentinel that must survive.

The attention's bound is the one tests/test_sdpa_rowwise_gpu.py applies to the rows of the causal forward's `out` (its module docstring):
    |out_kernel[r] - out_ref[r]|  <=  C |out_model[r] - out_ref[r]|  +  F |out_ref[r]|  +  G rms_r' |out_ref[r']|,   C = 2, F = 2^-8, G = 2^-14
per (sequence, row, head) row norm; out_ref is the fp64 softmax over the bf16 values actually stored, out_model the same computation in
fp32 with P rounded to bf16 before P V and the output rounded to bf16.  The constants are restated from there, not chosen here
(tests/extend_ref_util.py holds them, with the references; tests/test_extend_ref_util_cpu.py checks those on the host).

Behind the single-block case, the same bound at what it does not reach (second half of this file):
  * a boundary sweep (extend_ref_util.SWEEP_*: n = 257, Lcap = 448, one launch): every past mod 64 under two or three query blocks, last
    blocks of 1 .. 4 live waves, a cache filled to the brim, an empty block, a block clipped by the capacity; guards around the caches;
  * wide scores (extend_ref_util.wide_inputs, up to ~290 nats): the exponent reference moves, or P runs up to 2^46 without a move;
  * a long cache (past = 4031: 66 tiles), strides with gaps through the C ABI, a three-block sequence alone against the batch, and three
    input mismatches that the row-wise check must report on the affected rows only."""
import math

import pytest
import torch

import extend_ref_util as E
from extend_ref_util import C_OUT, F_OUT, G_OUT

pytestmark = pytest.mark.gpu

B, H, D, LCAP, N = 4, 2, 128, 320, 65
PAST = [0, 37, 130, 255]
N_NEW = [65, 1, 33, 64]
SENTINEL = 7.5


def _i16(t):
    return t.contiguous().view(torch.int16)


@pytest.fixture(scope="module")
def run():
    """One append + attention + advance on the poisoned operands, and the row-by-row halva_decode_rope_append reference of the append."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from halva_amd import kernels as K
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(11)
    cos, sin = K.rope_tables(D, LCAP, device=dev)
    x = torch.randn(B, N, 3 * H * D, device=dev, generator=g).to(torch.bfloat16)
    k0 = torch.randn(B, H, LCAP, D, device=dev, generator=g).to(torch.bfloat16)
    v0 = torch.randn(B, H, LCAP, D, device=dev, generator=g).to(torch.bfloat16)
    for b in range(B):
        x[b, N_NEW[b]:] = float("nan")
        k0[b, :, PAST[b]:] = float("nan")
        v0[b, :, PAST[b]:] = float("inf")
        v0[b, :, PAST[b]::2] = float("nan")
    past = torch.tensor(PAST, dtype=torch.int32, device=dev)
    n_new = torch.tensor(N_NEW, dtype=torch.int32, device=dev)
    # reference of the append: n successive single-row appends per sequence
    kref, vref, xref = k0.clone(), v0.clone(), x.clone()
    for b in range(B):
        lens_b = past[b:b + 1].clone()
        for i in range(N_NEW[b]):
            row = x[b, i][None].clone()
            K.decode_rope_append(row, cos, sin, kref[b:b + 1], vref[b:b + 1], lens_b, H, D)
            xref[b, i] = row[0]
        assert int(lens_b) == PAST[b] + N_NEW[b]
    kc, vc, qkv, lens = k0.clone(), v0.clone(), x.clone(), past.clone()
    K.extend_rope_append(qkv, cos, sin, kc, vc, lens, n_new, H, D)
    lens_after_append = lens.clone()
    ws = torch.full((64,), 0xFF, dtype=torch.uint8, device=dev)
    width = H * D + 8
    out = torch.full((B, N, width), SENTINEL, dtype=torch.bfloat16, device=dev)
    K.extend_attention(qkv, kc, vc, lens, n_new, ws, H, D, out_width=width, out=out)
    lens_after_attn = lens.clone()
    K.extend_advance(lens, n_new, LCAP)
    torch.cuda.synchronize()
    return dict(cos=cos, sin=sin, x=x, k0=k0, v0=v0, kref=kref, vref=vref, xref=xref, kc=kc, vc=vc, qkv=qkv, out=out, lens=lens,
                lens_after_append=lens_after_append, lens_after_attn=lens_after_attn, n_new=n_new, past=past)


def test_append_is_bitwise_n_single_row_appends(run):
    r = run
    # rotated q (in place), rotated k in the cache, v a plain copy; rows >= n_new (NaN) and every slot outside [past, past + n_new) keep their bits
    assert torch.equal(_i16(r["qkv"]), _i16(r["xref"]))
    assert torch.equal(_i16(r["kc"]), _i16(r["kref"]))
    assert torch.equal(_i16(r["vc"]), _i16(r["vref"]))
    for b in range(B):
        p, m = PAST[b], N_NEW[b]
        assert torch.equal(_i16(r["vc"][b, :, p:p + m]), _i16(r["x"][b, :m, 2 * H * D:].view(m, H, D).transpose(0, 1)))
        assert torch.equal(_i16(r["kc"][b, :, :p]), _i16(r["k0"][b, :, :p])) and torch.equal(_i16(r["kc"][b, :, p + m:]), _i16(r["k0"][b, :, p + m:]))
        assert torch.isfinite(r["kc"][b, :, p:p + m].float()).all()
    assert r["lens_after_append"].tolist() == PAST and r["lens_after_attn"].tolist() == PAST
    assert r["lens"].tolist() == [p + m for p, m in zip(PAST, N_NEW)]


def test_attention_rows_against_float64(run):
    r = run
    out, q = r["out"], r["qkv"][..., :H * D].view(B, N, H, D)
    scale = 1.0 / math.sqrt(D)
    errs, bounds_model, refs = [], [], []
    for b in range(B):
        p, m = PAST[b], N_NEW[b]
        L = p + m
        Kb, Vb = r["kc"][b, :, :L], r["vc"][b, :, :L]                        # [H, L, D], finite
        qb = q[b, :m].transpose(0, 1)                                         # [H, m, D]
        vis = torch.arange(L, device="cuda")[None, :] <= (p + torch.arange(m, device="cuda"))[:, None]      # key j visible to row i
        s64 = torch.einsum("hid,hjd->hij", qb.double(), Kb.double()) * scale
        ref = torch.einsum("hij,hjd->hid", s64.masked_fill(~vis, -math.inf).softmax(-1), Vb.double())
        s32 = (torch.einsum("hid,hjd->hij", qb.float(), Kb.float()) * (scale * 1.4426950408889634)).masked_fill(~vis, -math.inf)
        p32 = torch.exp2(s32 - s32.amax(-1, keepdim=True))
        model = (torch.einsum("hij,hjd->hid", p32.to(torch.bfloat16).float(), Vb.float()) / p32.sum(-1, keepdim=True)).to(torch.bfloat16)
        got = out[b, :m, :H * D].view(m, H, D).transpose(0, 1)
        assert torch.isfinite(got.float()).all(), b
        errs.append((got.double() - ref).norm(dim=-1).flatten())
        bounds_model.append((model.double() - ref).norm(dim=-1).flatten())
        refs.append(ref.norm(dim=-1).flatten())
        # rows at or beyond n_new and the columns beyond H*D keep the sentinel
        assert (out[b, m:] == SENTINEL).all() and (out[b, :, H * D:] == SENTINEL).all()
    ek, em, nr = torch.cat(errs), torch.cat(bounds_model), torch.cat(refs)
    bound = C_OUT * em + F_OUT * nr + G_OUT * float(nr.pow(2).mean().sqrt())
    ratio = ek / bound
    print("extend attention: worst row error / bound %.3f over %d rows (worst row error %.3e)" % (float(ratio.max()), ek.numel(), float(ek.max())))
    assert bool((ek <= bound).all()), "row-wise bound exceeded: worst error / bound %.3f at flat row %d" % (float(ratio.max()), int(ratio.argmax()))


def test_sequence_alone_equals_its_rows_in_the_batch(run):
    from halva_amd import kernels as K
    r = run
    b = 2
    m = N_NEW[b]
    kc, vc, qkv = r["k0"][b:b + 1].clone(), r["v0"][b:b + 1].clone(), r["x"][b:b + 1].clone()
    lens, n_new = r["past"][b:b + 1].clone(), r["n_new"][b:b + 1].clone()
    K.extend_rope_append(qkv, r["cos"], r["sin"], kc, vc, lens, n_new, H, D)
    out = K.extend_attention(qkv, kc, vc, lens, n_new, None, H, D)
    assert torch.equal(_i16(kc), _i16(r["kc"][b:b + 1])) and torch.equal(_i16(qkv), _i16(r["qkv"][b:b + 1]))
    assert torch.equal(_i16(out[0, :m]), _i16(r["out"][b, :m, :H * D]))
    assert not out[0, m:].any()                   # a fresh out is zero outside the new rows


def test_argument_checks_launch_nothing(run):
    from halva_amd import hip
    r = run
    lib = hip.load()
    P = hip.ptr
    kc, vc, qkv, lens, n_new, out = r["kc"], r["vc"], r["qkv"].clone(), r["lens"].clone(), r["n_new"], r["out"].clone()
    before = (_i16(out).clone(), _i16(qkv).clone(), lens.clone())
    ld, ldo = qkv.shape[-1], out.shape[-1]
    need = lib.halva_extend_attn_ws_bytes(B, N, H, LCAP)
    assert need >= 0

    def attn(q=P(qkv), n=N, d=D, ws_bytes=need):
        return lib.halva_extend_attn(q, ld, N * ld, P(kc), P(vc), P(lens), P(n_new), P(out), ldo, N * ldo, None if need == 0 else P(qkv), ws_bytes,
                                     B, n, H, d, LCAP, 0.0, hip.stream_ptr())

    def app(q=P(qkv), n=N, d=D):
        return lib.halva_extend_rope_append(q, ld, N * ld, P(r["cos"]), P(r["sin"]), LCAP, P(kc), P(vc), P(lens), P(n_new), B, n, H, d, LCAP,
                                            hip.stream_ptr())
    assert attn(d=64) == -1 and b"head_dim" in lib.halva_last_error()
    assert attn(q=P(qkv) + 2) == -1 and b"aligned" in lib.halva_last_error()
    assert attn(ws_bytes=need - 1) == -1 and b"workspace" in lib.halva_last_error()
    assert attn(n=0) == -1
    assert app(d=64) == -1 and app(q=P(qkv) + 2) == -1 and app(n=0) == -1
    assert lib.halva_extend_advance(None, P(n_new), B, LCAP, hip.stream_ptr()) == -1
    torch.cuda.synchronize()
    assert torch.equal(_i16(out), before[0]) and torch.equal(_i16(qkv), before[1]) and torch.equal(lens, before[2])


# ------------------------------------------------------------------------------------------------
# Several query blocks, wide scores, long caches, strides.  One bound (extend_ref_util.row_bound), one reference.
def _rows_vs_float64(out, q, kc, vc, pasts, rows, Hh):
    """Per sequence b: rows[b] new rows of out / q [B, n, >= Hh*D] against the float64 reference over the cache as stored.  Returns the
    list of [Hh, rows[b]] error / bound ratios (the bound's RMS term over every row of the call) and the worst row error."""
    eks, ems, nrs = [], [], []
    for b, (p, m) in enumerate(zip(pasts, rows)):
        if m == 0:
            eks.append(torch.zeros(0, device=out.device, dtype=torch.float64)), ems.append(eks[-1]), nrs.append(eks[-1])
            continue
        qb = q[b, :m, :Hh * D].view(m, Hh, D).transpose(0, 1)
        got = out[b, :m, :Hh * D].view(m, Hh, D).transpose(0, 1)
        assert torch.isfinite(got.float()).all(), "sequence %d: non-finite output" % b
        assert torch.isfinite(kc[b, :, :p + m].float()).all() and torch.isfinite(vc[b, :, :p + m].float()).all(), b
        ek, em, nr = E.row_errors(got, E.reference(qb, kc[b], vc[b], p, m), E.model(qb, kc[b], vc[b], p, m))
        eks.append(ek), ems.append(em), nrs.append(nr)
    bound = E.row_bound(torch.cat(ems), torch.cat(nrs))
    ratio = torch.cat(eks) / bound
    split = torch.split(ratio, [Hh * m for m in rows])
    return [r.view(Hh, m) for r, m in zip(split, rows)], float(torch.cat(eks).max())


def _assert_rows(name, ratios, worst, pasts):
    top = max((float(r.max()), b) for b, r in enumerate(ratios) if r.numel())
    print("%s: worst row error / bound %.3f over %d rows (sequence %d; worst row error %.3e)"
          % (name, top[0], sum(r.numel() for r in ratios), top[1], worst))
    for b, r in enumerate(ratios):
        if r.numel() and float(r.max()) > 1.0:
            h, i = divmod(int(r.argmax()), r.shape[1])
            raise AssertionError("%s: row-wise bound exceeded at sequence %d (past %d), row %d, head %d: error / bound %.3f; %d rows over in "
                                 "this sequence" % (name, b, pasts[b], i, h, float(r.max()), int((r > 1).sum())))


SW_H, SW_GUARD = 2, 4096


def _guarded(shape, dev):
    """A contiguous bf16 tensor of `shape` inside a larger buffer, SW_GUARD sentinel elements before its first and after its last one."""
    numel = math.prod(shape)
    buf = torch.full((numel + 2 * SW_GUARD,), SENTINEL, dtype=torch.bfloat16, device=dev)
    return buf, buf[SW_GUARD:SW_GUARD + numel].view(shape)


@pytest.fixture(scope="module")
def sweep():
    """The boundary sweep: one append + attention + advance over extend_ref_util's layout, poisoned as `run` above, the caches inside
    guarded buffers; and the append's reference, row by row through halva_decode_rope_append (one launch per row index, every sequence)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from halva_amd import kernels as K
    dev = "cuda"
    n, Lcap, Hh = E.SWEEP_N, E.SWEEP_LCAP, SW_H
    pasts, nns = E.SWEEP_PAST, E.SWEEP_N_NEW
    Bs = len(pasts)
    rows = [E.ext_rows(p, m, n, Lcap) for p, m in zip(pasts, nns)]
    g = torch.Generator(device=dev).manual_seed(23)
    cos, sin = K.rope_tables(D, Lcap, device=dev)
    x = torch.randn(Bs, n, 3 * Hh * D, device=dev, generator=g).to(torch.bfloat16)
    kbuf, kc = _guarded((Bs, Hh, Lcap, D), dev)
    vbuf, vc = _guarded((Bs, Hh, Lcap, D), dev)
    kc.copy_(torch.randn(Bs, Hh, Lcap, D, device=dev, generator=g))
    vc.copy_(torch.randn(Bs, Hh, Lcap, D, device=dev, generator=g))
    for b in range(Bs):
        x[b, nns[b]:] = float("nan")
        kc[b, :, pasts[b]:] = float("nan")
        vc[b, :, pasts[b]:] = float("inf")
        vc[b, :, pasts[b]::2] = float("nan")
    k0, v0 = kc.clone(), vc.clone()
    past = torch.tensor(pasts, dtype=torch.int32, device=dev)
    n_new = torch.tensor(nns, dtype=torch.int32, device=dev)
    rows_t = torch.tensor(rows, dtype=torch.int32, device=dev)
    # reference of the append: row i of every sequence that has one, by the single-row kernel (a full cache is left as it is)
    kref, vref, xref = k0.clone(), v0.clone(), x.clone()
    for i in range(max(rows)):
        lens_i = torch.where(rows_t > i, past + i, torch.full_like(past, Lcap))
        row = x[:, i].contiguous()
        K.decode_rope_append(row, cos, sin, kref, vref, lens_i, Hh, D)
        xref[:, i] = row
    qkv, lens = x.clone(), past.clone()
    K.extend_rope_append(qkv, cos, sin, kc, vc, lens, n_new, Hh, D)
    width = Hh * D + 8
    out = torch.full((Bs, n, width), SENTINEL, dtype=torch.bfloat16, device=dev)
    K.extend_attention(qkv, kc, vc, lens, n_new, None, Hh, D, out_width=width, out=out)
    lens_before_advance = lens.clone()
    K.extend_advance(lens, n_new, Lcap)
    torch.cuda.synchronize()
    return dict(cos=cos, sin=sin, x=x, k0=k0, v0=v0, kref=kref, vref=vref, xref=xref, kc=kc, vc=vc, kbuf=kbuf, vbuf=vbuf, qkv=qkv, out=out,
                lens=lens, lens_before_advance=lens_before_advance, past=past, n_new=n_new, rows=rows, pasts=pasts, nns=nns)


def test_sweep_rows_against_float64(sweep):
    r = sweep
    ratios, worst = _rows_vs_float64(r["out"], r["qkv"], r["kc"], r["vc"], r["pasts"], r["rows"], SW_H)
    by_blocks = {}
    for m, q in zip(r["rows"], ratios):
        if m:
            k = (m + E.BM - 1) // E.BM
            by_blocks[k] = max(by_blocks.get(k, 0.0), float(q.max()))
    print("sweep: worst row error / bound by live query blocks %s" % {k: round(v, 3) for k, v in sorted(by_blocks.items())})
    _assert_rows("extend attention, boundary sweep", ratios, worst, r["pasts"])
    out = r["out"]
    for b, m in enumerate(r["rows"]):      # rows at or beyond the new ones and the columns beyond H*D keep the sentinel
        assert (out[b, m:] == SENTINEL).all() and (out[b, :, SW_H * D:] == SENTINEL).all(), b


def test_sweep_append_guards_lens_empty_and_clipped_sequences(sweep):
    r = sweep
    n, Lcap, Hh = E.SWEEP_N, E.SWEEP_LCAP, SW_H
    assert torch.equal(_i16(r["qkv"]), _i16(r["xref"]))
    assert torch.equal(_i16(r["kc"]), _i16(r["kref"])) and torch.equal(_i16(r["vc"]), _i16(r["vref"]))
    for b, (p, m) in enumerate(zip(r["pasts"], r["rows"])):
        assert torch.equal(_i16(r["vc"][b, :, p:p + m]), _i16(r["x"][b, :m, 2 * Hh * D:].view(m, Hh, D).transpose(0, 1))), b
        assert torch.equal(_i16(r["kc"][b, :, :p]), _i16(r["k0"][b, :, :p])) and torch.equal(_i16(r["kc"][b, :, p + m:]), _i16(r["k0"][b, :, p + m:])), b
        assert torch.equal(_i16(r["vc"][b, :, :p]), _i16(r["v0"][b, :, :p])) and torch.equal(_i16(r["vc"][b, :, p + m:]), _i16(r["v0"][b, :, p + m:])), b
        assert torch.isfinite(r["kc"][b, :, p:p + m].float()).all(), b
    for buf in (r["kbuf"], r["vbuf"]):
        assert (buf[:SW_GUARD] == SENTINEL).all() and (buf[-SW_GUARD:] == SENTINEL).all()
    assert r["lens_before_advance"].tolist() == r["pasts"]
    assert r["lens"].tolist() == [min(p + m, Lcap) for p, m in zip(r["pasts"], r["nns"])]
    assert r["lens"][E.SWEEP_FULL].item() == Lcap and r["rows"][E.SWEEP_FULL] == n
    # n_new = 0: nothing of the sequence is touched
    b = E.SWEEP_EMPTY
    assert r["nns"][b] == 0 and r["lens"][b].item() == r["pasts"][b]
    assert torch.equal(_i16(r["kc"][b]), _i16(r["k0"][b])) and torch.equal(_i16(r["vc"][b]), _i16(r["v0"][b]))
    assert torch.equal(_i16(r["qkv"][b]), _i16(r["x"][b])) and (r["out"][b] == SENTINEL).all()
    # past = Lcap - 5, n_new = 9: five slots and five out rows, the four rows without a slot are left as they were
    b = E.SWEEP_CLIP
    p = r["pasts"][b]
    assert r["nns"][b] == 9 and r["rows"][b] == 5 and p + 5 == Lcap and r["lens"][b].item() == Lcap
    assert torch.isfinite(r["kc"][b, :, p:].float()).all() and torch.isfinite(r["vc"][b, :, p:].float()).all()
    assert torch.equal(_i16(r["qkv"][b, 5:]), _i16(r["x"][b, 5:])) and torch.isfinite(r["x"][b, 5:9].float()).all()
    assert not torch.equal(_i16(r["qkv"][b, :5, :Hh * D]), _i16(r["x"][b, :5, :Hh * D]))
    assert torch.isfinite(r["out"][b, :5, :Hh * D].float()).all() and (r["out"][b, 5:] == SENTINEL).all()


@pytest.mark.parametrize("b", [3, E.SWEEP_FULL])
def test_sweep_sequence_alone_equals_its_rows_in_the_batch(sweep, b):
    """Two and three query blocks (n_new = 161 at past = 3; 257 rows up to the brim of the cache): B and the neighbours do not reach a row's bits."""
    from halva_amd import kernels as K
    r = sweep
    m = r["rows"][b]
    assert m >= 161 and m == r["nns"][b]
    kc, vc, qkv = r["k0"][b:b + 1].clone(), r["v0"][b:b + 1].clone(), r["x"][b:b + 1].clone()
    lens, n_new = r["past"][b:b + 1].clone(), r["n_new"][b:b + 1].clone()
    K.extend_rope_append(qkv, r["cos"], r["sin"], kc, vc, lens, n_new, SW_H, D)
    out = K.extend_attention(qkv, kc, vc, lens, n_new, None, SW_H, D)
    assert torch.equal(_i16(kc), _i16(r["kc"][b:b + 1])) and torch.equal(_i16(qkv), _i16(r["qkv"][b:b + 1]))
    assert torch.equal(_i16(out[0, :m]), _i16(r["out"][b, :m, :SW_H * D]))
    assert not out[0, m:].any()


def _direct_case(q, Kc, Vc, pasts, nns, Lcap, poison=True):
    """q [B, n, Hh, D], Kc / Vc [B, Hh, L_b.., D] lists of bf16 CPU or device tensors written straight into a cache (no RoPE).  Returns the
    device operands of extend_attention."""
    dev = "cuda"
    Bq, n, Hh = len(pasts), max(nns), q[0].shape[0]
    kc = torch.full((Bq, Hh, Lcap, D), float("nan") if poison else 0.0, dtype=torch.bfloat16, device=dev)
    vc = torch.full((Bq, Hh, Lcap, D), float("inf") if poison else 0.0, dtype=torch.bfloat16, device=dev)
    qq = torch.full((Bq, n, Hh * D), float("nan") if poison else 0.0, dtype=torch.bfloat16, device=dev)
    for b in range(Bq):
        L = pasts[b] + nns[b]
        kc[b, :, :L] = Kc[b][:, :L].to(dev)
        vc[b, :, :L] = Vc[b][:, :L].to(dev)
        qq[b, :nns[b]] = q[b][:, :nns[b]].to(dev).transpose(0, 1).reshape(nns[b], Hh * D)
    return qq, kc, vc, torch.tensor(pasts, dtype=torch.int32, device=dev), torch.tensor(nns, dtype=torch.int32, device=dev)


def test_wide_scores_against_float64():
    """The five profiles of extend_ref_util (past = 37, 300 new rows, H = 1, scores up to ~290 nats), one sequence each, one launch: `up`
    moves the exponent reference once per tile with P up to 2^46 in between, `spike_late` moves it by 216 log2 units at once, `down` and
    `spike_first` never move it and underflow.  tests/test_extend_ref_util_cpu.py: the documented arithmetic meets this bound on these
    inputs at <= 0.54, and breaks it 200-fold without the rescale."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from halva_amd import kernels as K
    past, m = 37, 300
    ins = [E.wide_inputs(name, past + m, m, seed=E.WIDE_SEEDS[0]) for name in E.WIDE_PROFILES]
    qq, kc, vc, lens, n_new = _direct_case([i[0] for i in ins], [i[1] for i in ins], [i[2] for i in ins], [past] * 5, [m] * 5, past + m + 7)
    out = K.extend_attention(qq, kc, vc, lens, n_new, None, 1, D)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    ratios, worst = _rows_vs_float64(out, qq, kc, vc, [past] * 5, [m] * 5, 1)
    print("extend attention, wide scores: worst row error / bound %s" % {n_: round(float(r.max()), 3) for n_, r in zip(E.WIDE_PROFILES, ratios)})
    _assert_rows("extend attention, wide scores", ratios, worst, [past] * 5)


def test_long_cache_against_float64():
    """past = 4031, 130 new rows: 66 key tiles, two query blocks, the second of one live wave."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from halva_amd import kernels as K
    past, m = 4031, 130
    g = torch.Generator().manual_seed(31)
    q = torch.randn(1, m, D, generator=g).to(torch.bfloat16)
    Kc, Vc = torch.randn(1, past + m, D, generator=g).to(torch.bfloat16), torch.randn(1, past + m, D, generator=g).to(torch.bfloat16)
    qq, kc, vc, lens, n_new = _direct_case([q], [Kc], [Vc], [past], [m], 4224)
    out = K.extend_attention(qq, kc, vc, lens, n_new, None, 1, D)
    torch.cuda.synchronize()
    ratios, worst = _rows_vs_float64(out, qq, kc, vc, [past], [m], 1)
    _assert_rows("extend attention, long cache", ratios, worst, [past])


def test_strides_with_gaps_through_the_c_abi():
    """ldseq > n ldrow and ld_out_seq > n ld_out_row (the Python wrappers cannot produce them): the gaps hold NaN on the q side and the
    sentinel on the out side; append and attention equal the contiguous call's, bit for bit, and leave the gaps alone."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from halva_amd import hip, kernels as K
    lib, P, dev = hip.load(), hip.ptr, "cuda"
    Bq, n, Hh, Lcap = 2, 130, 2, 256
    pasts, nns = [3, 70], [130, 97]
    g = torch.Generator(device=dev).manual_seed(41)
    cos, sin = K.rope_tables(D, Lcap, device=dev)
    x = torch.randn(Bq, n, 3 * Hh * D, device=dev, generator=g).to(torch.bfloat16)
    k0 = torch.randn(Bq, Hh, Lcap, D, device=dev, generator=g).to(torch.bfloat16)
    v0 = torch.randn(Bq, Hh, Lcap, D, device=dev, generator=g).to(torch.bfloat16)
    for b in range(Bq):
        x[b, nns[b]:] = float("nan")
        k0[b, :, pasts[b]:] = float("nan")
        v0[b, :, pasts[b]:] = float("nan")
    lens = torch.tensor(pasts, dtype=torch.int32, device=dev)
    n_new = torch.tensor(nns, dtype=torch.int32, device=dev)
    # contiguous
    kc, vc, qkv = k0.clone(), v0.clone(), x.clone()
    K.extend_rope_append(qkv, cos, sin, kc, vc, lens, n_new, Hh, D)
    out = torch.full((Bq, n, Hh * D), SENTINEL, dtype=torch.bfloat16, device=dev)
    K.extend_attention(qkv, kc, vc, lens, n_new, None, Hh, D, out=out)
    # strided
    ldrow = 3 * Hh * D + 8
    ldseq = n * ldrow + 16
    ldo = Hh * D + 8
    ldos = n * ldo + 24
    qbuf = torch.full((Bq * ldseq,), float("nan"), dtype=torch.bfloat16, device=dev)
    obuf = torch.full((Bq * ldos,), SENTINEL, dtype=torch.bfloat16, device=dev)
    qv = qbuf.as_strided((Bq, n, 3 * Hh * D), (ldseq, ldrow, 1))
    ov = obuf.as_strided((Bq, n, Hh * D), (ldos, ldo, 1))
    qv.copy_(x)
    qgap = torch.ones(Bq * ldseq, dtype=torch.bool, device=dev)
    qgap.as_strided((Bq, n, 3 * Hh * D), (ldseq, ldrow, 1)).fill_(False)
    ogap = torch.ones(Bq * ldos, dtype=torch.bool, device=dev)
    ogap.as_strided((Bq, n, Hh * D), (ldos, ldo, 1)).fill_(False)
    assert int(qgap.sum()) == Bq * (n * 8 + 16) and int(ogap.sum()) == Bq * (n * 8 + 24)
    k2, v2 = k0.clone(), v0.clone()
    assert lib.halva_extend_rope_append(P(qbuf), ldrow, ldseq, P(cos), P(sin), cos.shape[0], P(k2), P(v2), P(lens), P(n_new), Bq, n, Hh, D, Lcap,
                                        hip.stream_ptr()) == 0, lib.halva_last_error()
    assert lib.halva_extend_attn(P(qbuf), ldrow, ldseq, P(k2), P(v2), P(lens), P(n_new), P(obuf), ldo, ldos, None, 0, Bq, n, Hh, D, Lcap, 0.0,
                                 hip.stream_ptr()) == 0, lib.halva_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_i16(k2), _i16(kc)) and torch.equal(_i16(v2), _i16(vc))
    assert torch.equal(_i16(qv.contiguous()), _i16(qkv))
    assert torch.equal(_i16(ov.contiguous()), _i16(out))
    assert torch.isnan(qbuf[qgap].float()).all() and (obuf[ogap] == SENTINEL).all()
    for b in range(Bq):
        assert torch.isfinite(out[b, :nns[b]].float()).all() and (out[b, nns[b]:] == SENTINEL).all()
    # a sequence stride one element short of n rows is refused
    assert lib.halva_extend_attn(P(qbuf), ldrow, n * ldrow - 8, P(k2), P(v2), P(lens), P(n_new), P(obuf), ldo, ldos, None, 0, Bq, n, Hh, D, Lcap,
                                 0.0, hip.stream_ptr()) == -1 and b"sequence stride" in lib.halva_last_error()


# ---- input mismatches: the kernel is given an input that differs from the reference's; the row-wise check must report the affected rows only
MM_PAST, MM_N, MM_H, MM_LCAP = [37, 5], [200, 200], 2, 256


@pytest.fixture(scope="module")
def mm():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    g = torch.Generator().manual_seed(53)
    q = [torch.randn(MM_H, MM_N[b], D, generator=g).to(torch.bfloat16) for b in range(2)]
    Kc = [torch.randn(MM_H, MM_PAST[b] + MM_N[b] + 1, D, generator=g).to(torch.bfloat16) for b in range(2)]      # (+ 1: the slot a lens off by one reaches)
    Vc = [torch.randn(MM_H, MM_PAST[b] + MM_N[b] + 1, D, generator=g).to(torch.bfloat16) for b in range(2)]
    qq, kc, vc, lens, n_new = _direct_case(q, Kc, Vc, MM_PAST, MM_N, MM_LCAP, poison=False)
    for b in range(2):
        L = MM_PAST[b] + MM_N[b]
        kc[b, :, L] = Kc[b][:, L].cuda()
        vc[b, :, L] = Vc[b][:, L].cuda()
    return qq, kc, vc, lens, n_new


def _mm_violations(mm, kc=None, vc=None, lens=None):
    """Run the kernel on the (changed) operands, check against the reference of the unchanged ones: [H, rows] violation masks per sequence."""
    from halva_amd import kernels as K
    qq, kc0, vc0, lens0, n_new = mm
    out = K.extend_attention(qq, kc0 if kc is None else kc, vc0 if vc is None else vc, lens0 if lens is None else lens, n_new, None, MM_H, D)
    torch.cuda.synchronize()
    ratios, _ = _rows_vs_float64(out, qq, kc0, vc0, MM_PAST, MM_N, MM_H)
    return [r > 1.0 for r in ratios]


def test_mismatch_control_has_no_violation(mm):
    assert not any(bool(v.any()) for v in _mm_violations(mm))


def test_mismatch_swapped_key_rows_is_caught_rowwise_only(mm):
    """keys (k and v) t and t + 1 of sequence 0 swapped for the kernel only, t = past + 150 in the second query block: only row 150's
    visible set changes (the rows behind it see the same set in another order)"""
    i = 150
    t = MM_PAST[0] + i
    kc, vc = mm[1].clone(), mm[2].clone()
    kc[0, :, [t, t + 1]] = mm[1][0][:, [t + 1, t]]
    vc[0, :, [t, t + 1]] = mm[2][0][:, [t + 1, t]]
    v0, v1 = _mm_violations(mm, kc=kc, vc=vc)
    assert bool(v0.any()), "the row-wise check missed the swapped keys"
    assert set(v0.nonzero()[:, 1].tolist()) == {i} and not bool(v1.any())


def test_mismatch_lens_off_by_one_is_caught_rowwise_only(mm):
    """lens[0] one too large for the kernel: every row of sequence 0 sees one key more; sequence 1 is untouched"""
    lens = mm[3].clone()
    lens[0] += 1
    v0, v1 = _mm_violations(mm, lens=lens)
    print("lens off by one: %d of %d rows reported" % (int(v0.sum()), v0.numel()))
    assert bool(v0[:, 128:].any()) and bool(v0[:, :128].any()), "the row-wise check missed the shifted lens"
    assert not bool(v1.any())


def test_mismatch_scaled_value_row_is_caught_rowwise_only(mm):
    """V row t = past + 140 of sequence 0 scaled by 1.5 for the kernel only: the rows from 140 on see it"""
    i = 140
    vc = mm[2].clone()
    vc[0, :, MM_PAST[0] + i] = (vc[0, :, MM_PAST[0] + i].float() * 1.5).to(torch.bfloat16)
    v0, v1 = _mm_violations(mm, vc=vc)
    print("scaled V row: %d of %d rows that see it reported" % (int(v0.sum()), v0[:, i:].numel()))
    assert bool(v0.any()), "the row-wise check missed the scaled V row"
    assert min(v0.nonzero()[:, 1].tolist()) >= i and not bool(v1.any())
