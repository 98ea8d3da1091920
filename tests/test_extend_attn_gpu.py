"""The kernels that extend a kept KV cache by a block of rows (halva_amd/csrc/extend.hip: halva_extend_rope_append, halva_extend_attn,
halva_extend_advance), alone: H = 2, D = 128, Lcap = 320.

past = [0, 37, 130, 255], n_new = [65, 1, 33, 64], n = 65: key counts on both sides of the 64- and 256-boundaries, query blocks of 1, 32 + 1
and 64 + 1 rows, an empty cache.  Cache slots at or beyond past + n_new, q rows at or beyond n_new and the workspace hold NaN / Inf; out
rows at or beyond n_new (and out's columns beyond H*D) hold a sentinel that must survive.

The attention's bound is the one tests/test_sdpa_rowwise_gpu.py applies to the rows of the causal forward's `out` (its module docstring):
    |out_kernel[r] - out_ref[r]|  <=  C |out_model[r] - out_ref[r]|  +  F |out_ref[r]|  +  G rms_r' |out_ref[r']|,   C = 2, F = 2^-8, G = 2^-14
per (sequence, row, head) row norm; out_ref is the fp64 softmax over the bf16 values actually stored, out_model the same computation in
fp32 with P rounded to bf16 before P V and the output rounded to bf16.  The constants are restated from there, not chosen here."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C_OUT, F_OUT, G_OUT = 2.0, 2.0 ** -8, 2.0 ** -14      # tests/test_sdpa_rowwise_gpu.py: C_X["out"], F_X["out"], G_X["out"]
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
