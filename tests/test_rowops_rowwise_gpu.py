"""Elementwise checks of the decoder layer's row kernels (halva_amd/csrc/rowops.hip) against float64, with poisoned padding.

test_hip_kernels.py takes one relative Frobenius error per tensor (tolerances 2e-3 to 8e-3): a wrong 8-element chunk in a
50 x 11008 tensor moves it by far less.  Here every element is held, on the kernel's own bf16 inputs (and bf16 cos / sin tables), to

    |X_kernel - X_ref|  <=  C |X_model - X_ref|  +  F |X_ref|  +  2 delta  +  G

X_ref: float64.  X_model: the rounding model - X_ref rounded to bf16 where the kernel rounds.  U = 2^-24.
  * C = 1: a kernel whose fp32 value y' lies within delta of X_ref rounds to X_model, or - when X_ref lies within delta of a rounding
    midpoint - to its neighbour, which is |X_model - X_ref| + 2 |X_ref - midpoint| <= |X_model - X_ref| + 2 delta away.
  * delta, the fp32 pre-rounding error (absolute):
      RMSNorm rstd   E_r = U (LAMBDA / 2 sqrt(n) + C_FN) relative, n = 8 ceil(d / 512) + 6 terms along a lane's sum of squares and the
                     wave shuffles (LAMBDA = 8: the probabilistic bound of tests/loss_ref_util.py), half of it through the square
                     root; C_FN = 4: the products with 1/d, + eps, and rsqrtf (v_rsq_f32, 1 ulp).  rstd itself is held to E_r.
      RMSNorm y      (E_r + 2 U) |y|: two products, w (x r).
      RMSNorm dx     r (U |g| + |n| (|dot| (2 U + 2 E_r) + e_dot) + U |g - n dot|) + (U + E_r) |dx|, g = dy w, n = x r, with
                     e_dot = (E_r + (4 + LAMBDA sqrt(n)) U) mean |dy w x r|: the cancelling difference is bounded by its terms.
      SwiGLU         sigmoid through __expf(-g) = v_exp_f32(-g log2e): relative e_s = U (|g| + 6) (the product's rounding of
                     |g| log2e, v_exp_f32, 1 + e, the division); du = dout g s: (e_s + 2 U) |du|;
                     dg = dout u s (1 + g (1 - s)): |dout u s| (|1 + g (1 - s)| (e_s + 3 U) + U (1 + 2 |g|) + |g| s e_s) + 3 U |dg|.
      RoPE           U |y|: x c and x s are exact in fp32 (bf16 x bf16), one rounding of their sum or difference.
  * F = 0 where the kernel rounds once.  F = 2^-7 where it rounds twice - SwiGLU's forward bf16(bf16(silu(g)) u) and the residual
    backward bf16(bf16(dx) + dres): a flip of the inner rounding moves the result by up to one inner bf16 ulp (2^-7 of the value)
    before the outer rounding; the outer product / sum of two bf16 values is exact in fp32.
  * G = 2^-100 (1 + |a|)(1 + |b|)(1 + |c|) of the operands: the floor of results below fp32's normal range - __expf overflows for
    |g| > 88.7, and silu / sigmoid of those gates is ~1e-38 in float64 and 0 in the kernel.

Contracts checked bit for bit: columns [d, ldy) of a wider y and [F, ldo) of a wider SwiGLU output keep a sentinel; NaN in the
columns [d, lddy) of dy / [F, lddo) of dout changes nothing; rmsnorm_fwd_fork's x_copy is x and its y / rstd those of rmsnorm_fwd_ld;
rmsnorm_bwd_res_ld is bf16(bwd_ld + dres) (the sum autograd forms); RoPE leaves the v third untouched.  Paths: RMSNorm's 10-chunk
instantiation (d <= 5120) and 16-chunk one (d = 5128, 8192), row counts that are not a multiple of its 4 rows per workgroup.
Entry points go through the C ABI (halva_amd.hip.call).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from halva_amd.hip import call, ptr, stream_ptr  # noqa: E402
from sdpa_ref_util import branch_positions  # noqa: E402

DEV = "cuda"
bf16 = torch.bfloat16
U = 2.0 ** -24
LAMBDA = 8.0
C_FN = 4.0
F2 = 2.0 ** -7
EPS = 1e-5
SENT = 12.5
REPORT = {}


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _bf(x):
    return x.to(bf16).double()


def _floor(*ops):
    g = torch.full_like(ops[0].double(), 2.0 ** -100)
    for o in ops:
        g = g * (1 + o.double().abs())
    return g


def held(name, got, ref, model, delta, F=0.0, G=None):
    got, ref, model = got.double(), ref.double(), model.double()
    assert bool(torch.isfinite(got).all()), (name, "non-finite results")
    bound = (model - ref).abs() + F * ref.abs() + 2 * delta + (0 if G is None else G)
    err = (got - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        raise AssertionError("%s: %d elements outside the bound, first %s, got %s want %s" % (
            name, int(bad.sum()), idx, got[bad][:4].tolist(), ref[bad][:4].tolist()))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(r.max()) if r.numel() else 0.0
    REPORT[name] = max(REPORT.get(name, 0.0), worst)
    return worst


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def padded(x, ld, fill):
    """x [R, n] in a [R, ld] buffer whose columns [n, ld) hold fill ('nan' cycles NaN / +-Inf)"""
    R, n = x.shape
    buf = torch.full((R, ld), SENT if fill == "sent" else 0.0, dtype=x.dtype, device=DEV)
    if fill == "nan":
        buf[:] = torch.tensor([float("nan"), float("inf"), float("-inf")], device=DEV).repeat(R * ld // 3 + 1)[:R * ld].view(R, ld).to(x.dtype)
    elif isinstance(fill, float):
        buf.fill_(fill)
    buf[:, :n] = x
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------
# RMSNorm
RMS = [(d, rows, ld_i) for d in (64, 4096, 5120, 5128, 8192) for rows in (1, 3, 5, 4099) for ld_i in range(3)]


def _rms_inputs(rows, d, seed):
    g = _gen(seed)
    x = torch.randn(rows, d, generator=g, device=DEV)
    r = torch.arange(rows, device=DEV)[:, None]
    x = torch.where(r % 4 == 2, x * 1e3, x)
    x = torch.where(r % 4 == 3, x * 1e-3, x)
    if rows > 1:
        x[1] = 0                                                  # an all-zero row: y = 0 exactly, dx finite
    w = (1 + 0.1 * torch.randn(d, generator=g, device=DEV)).to(bf16)
    dy = torch.randn(rows, d, generator=g, device=DEV).to(bf16)
    dres = torch.randn(rows, d, generator=g, device=DEV).to(bf16)
    return x.to(bf16), w, dy, dres


@pytest.mark.parametrize("d,rows,ld_i", RMS, ids=["d%d-r%d-ld%d" % c for c in RMS])
def test_rmsnorm_elementwise(d, rows, ld_i):
    ldy = (d, d + 8, d + 384)[ld_i]
    x, w, dy, dres = _rms_inputs(rows, d, seed=d + rows + ld_i)
    st = stream_ptr()
    # forward, _ld: y into a sentinel-filled [rows, ldy] buffer
    y = padded(torch.full((rows, d), float("nan"), device=DEV).to(bf16), ldy, "sent")
    rstd = torch.full((rows,), float("nan"), device=DEV)
    call("halva_rmsnorm_fwd_ld", ptr(x), ptr(w), ptr(y), ldy, ptr(rstd), rows, d, EPS, st)
    x64, w64 = x.double(), w.double()
    eps32 = float(torch.tensor(EPS, dtype=torch.float32))
    r64 = 1.0 / torch.sqrt((x64 * x64).mean(-1) + eps32)
    n = 8 * math.ceil(d / 512) + 6
    E_r = U * (LAMBDA / 2 * math.sqrt(n) + C_FN)
    rr = float(((rstd.double() - r64).abs() / (E_r * r64)).max())
    assert rr <= 1.0, ("rstd", rr)
    REPORT["rmsnorm rstd"] = max(REPORT.get("rmsnorm rstd", 0.0), rr)
    yref = w64 * x64 * r64[:, None]
    a = held("rmsnorm y", y[:, :d], yref, _bf(yref), (E_r + 2 * U) * yref.abs(), G=_floor(x, w))
    assert bool((y[:, d:] == SENT).all()), "columns [d, ldy) of y were written"
    if rows > 1:
        assert bool((y[1, :d] == 0).all())
    # fork: the same y / rstd, and x_copy = x
    y2 = padded(torch.zeros(rows, d, device=DEV).to(bf16), ldy, "sent")
    rstd2 = torch.empty(rows, device=DEV)
    xc = torch.full_like(x, float("nan"))
    call("halva_rmsnorm_fwd_fork_ld", ptr(x), ptr(w), ptr(y2), ldy, ptr(rstd2), ptr(xc), rows, d, EPS, st)
    assert same_bits(y2, y) and torch.equal(rstd2, rstd) and same_bits(xc, x)
    # backward, _ld: dy rows of width ldy; NaN in their columns [d, ldy) changes nothing
    lddy = ldy
    dyc = padded(dy, lddy, 3.0)
    dx = torch.full_like(x, float("nan"))
    call("halva_rmsnorm_bwd_ld", ptr(dyc), lddy, ptr(x), ptr(w), ptr(rstd), ptr(dx), rows, d, st)
    g64 = dy.double() * w64
    n64 = x64 * r64[:, None]
    dot = (g64 * n64).mean(-1, keepdim=True)
    dxref = r64[:, None] * (g64 - n64 * dot)
    e_dot = (E_r + (4 + LAMBDA * math.sqrt(n)) * U) * (g64 * n64).abs().mean(-1, keepdim=True)
    delta = r64[:, None] * (U * g64.abs() + n64.abs() * (dot.abs() * (2 * U + 2 * E_r) + e_dot) + U * (g64 - n64 * dot).abs()) \
        + (U + E_r) * dxref.abs()
    b = held("rmsnorm dx", dx, dxref, _bf(dxref), delta, G=_floor(dy, x, w) * r64[:, None] ** 2)
    dyp = padded(dy, lddy, "nan")
    dxp = torch.full_like(x, float("nan"))
    call("halva_rmsnorm_bwd_ld", ptr(dyp), lddy, ptr(x), ptr(w), ptr(rstd), ptr(dxp), rows, d, st)
    assert same_bits(dxp, dx), "NaN in dy[:, d:lddy] changed dx"
    # backward with the residual gradient: bf16(bwd + dres), bit for bit, and held to float64
    dxr = torch.full_like(x, float("nan"))
    call("halva_rmsnorm_bwd_res_ld", ptr(dyp), lddy, ptr(x), ptr(w), ptr(rstd), ptr(dres), ptr(dxr), rows, d, st)
    assert same_bits(dxr, (dx.float() + dres.float()).to(bf16)), "bwd_res is not bf16(bwd + dres)"
    ref_res = dxref + dres.double()
    c = held("rmsnorm dx+res", dxr, ref_res, _bf(_bf(dxref) + dres.double()), delta, F=F2, G=_floor(dy, x, w, dres) * r64[:, None] ** 2)
    print("[rmsnorm d=%d rows=%d ldy=%d] worst error / bound: rstd %.3f, y %.3f, dx %.3f, dx+res %.3f" % (d, rows, ldy, rr, a, b, c))


# ---------------------------------------------------------------------------------------------------------------------------------
# SwiGLU
SWI = [(F, rows, ld_i) for F in (8, 1032, 11008, 13824) for rows in (1, 7, 4099) for ld_i in range(3)]
GATES = [0.0, -0.0, 1e-3, -1e-3, 20.0, -20.0, 88.5, -88.5, 89.0, -89.0, 95.0, -95.0, 100.0, -100.0]


def _gates(rows, F, g):
    x = torch.randn(rows, F, generator=g, device=DEV) * 3
    special = torch.tensor(GATES, device=DEV)
    pick = torch.randint(0, len(GATES), (rows, F), generator=g, device=DEV)
    use = torch.rand(rows, F, generator=g, device=DEV) < 0.25
    x = torch.where(use, special[pick], x)
    x[0, :min(F, len(GATES))] = special[:min(F, len(GATES))]
    return x.to(bf16)


@pytest.mark.parametrize("F,rows,ld_i", SWI, ids=["F%d-r%d-ld%d" % c for c in SWI])
def test_swiglu_elementwise(F, rows, ld_i):
    ldo = (F, F + 8, F + 128)[ld_i]
    g = _gen(F + rows + ld_i)
    gate = _gates(rows, F, g)
    up = torch.randn(rows, F, generator=g, device=DEV).to(bf16)
    gu = torch.cat([gate, up], 1).contiguous()
    dout = torch.randn(rows, F, generator=g, device=DEV).to(bf16)
    st = stream_ptr()
    out = padded(torch.full((rows, F), float("nan"), device=DEV).to(bf16), ldo, "sent")
    call("halva_swiglu_fwd_ld", ptr(gu), ptr(out), ldo, rows, F, st)
    assert bool((out[:, F:] == SENT).all()), "columns [F, ldo) of the output were written"
    g64, u64 = gate.double(), up.double()
    s64 = torch.sigmoid(g64)
    silu = g64 * s64
    e_s = U * (g64.abs() + 6)
    ref = silu * u64
    a = held("swiglu out", out[:, :F], ref, _bf(_bf(silu) * u64), (e_s + U) * silu.abs() * u64.abs(), F=F2, G=_floor(gate, up))
    # backward: dout rows of width ldo; NaN in [F, ldo) changes nothing
    dgu = torch.full_like(gu, float("nan"))
    call("halva_swiglu_bwd_ld", ptr(padded(dout, ldo, 3.0)), ldo, ptr(gu), ptr(dgu), rows, F, st)
    d64 = dout.double()
    du = d64 * g64 * s64
    inner = 1 + g64 * (1 - s64)
    dg = d64 * u64 * s64 * inner
    b = held("swiglu du", dgu[:, F:], du, _bf(du), (e_s + 2 * U) * du.abs(), G=_floor(dout, gate))
    c = held("swiglu dg", dgu[:, :F], dg, _bf(dg),
             (d64 * u64 * s64).abs() * (inner.abs() * (e_s + 3 * U) + U * (1 + 2 * g64.abs()) + g64.abs() * s64 * e_s) + 3 * U * dg.abs(),
             G=_floor(dout, gate, up))
    dgp = torch.full_like(gu, float("nan"))
    call("halva_swiglu_bwd_ld", ptr(padded(dout, ldo, "nan")), ldo, ptr(gu), ptr(dgp), rows, F, st)
    assert same_bits(dgp, dgu), "NaN in dout[:, F:lddo] changed dgu"
    print("[swiglu F=%d rows=%d ldo=%d] worst error / bound: out %.3f, du %.3f, dg %.3f" % (F, rows, ldo, a, b, c))


# ---------------------------------------------------------------------------------------------------------------------------------
# RoPE
ROPE = [(D, H, mode) for D in (64, 128) for H in (1, 32, 40) for mode in ("table", "pos", "branch")]


@pytest.mark.parametrize("D,H,mode", ROPE, ids=["D%d-H%d-%s" % c for c in ROPE])
def test_rope_elementwise(D, H, mode):
    from halva_amd import kernels
    S, T = 2, 333                                                    # T not a multiple of 8
    g = _gen(D + H)
    qkv = torch.randn(S * T, 3, H, D, generator=g, device=DEV).to(bf16)
    st = stream_ptr()
    if mode == "table":
        max_pos = T                                                  # row T - 1 of the table is used
        pos = torch.arange(T).repeat(S)
    elif mode == "pos":
        max_pos = 512
        pos = torch.randint(0, max_pos, (S * T,), generator=torch.Generator().manual_seed(D + H))
        pos[:2] = torch.tensor([max_pos - 1, 0])
    else:
        max_pos = T
        br_a, br_b = [63, T], [192, T]                               # sequence 1: no branch point
        pos = branch_positions(T, br_a, br_b, S).reshape(-1)
    cos, sin = kernels.rope_tables(D, max_pos, device=DEV)
    c = cos.double()[pos.to(DEV)][:, None]                           # [rows, 1, D/2]
    s = sin.double()[pos.to(DEV)][:, None]
    report = []
    for inverse in (0, 1):
        work = qkv.clone()
        if mode == "branch":
            a32, b32 = (torch.tensor(v, dtype=torch.int32, device=DEV) for v in (br_a, br_b))      # (held across the launch)
            call("halva_rope_qk_branch", ptr(work), ptr(cos), ptr(sin), ptr(a32), ptr(b32), S * T, T, H, D, max_pos, inverse, st)
        else:
            p32 = pos.int().to(DEV) if mode == "pos" else None
            call("halva_rope_qk", ptr(work), ptr(cos), ptr(sin), ptr(p32), S * T, T, H, D, max_pos, inverse, st)
        assert same_bits(work[:, 2], qkv[:, 2]), "the v third was written"
        x = qkv[:, :2].double()
        x1, x2 = x[..., :D // 2], x[..., D // 2:]
        sg = -1.0 if inverse else 1.0
        ref = torch.cat([x1 * c[:, None] - x2 * sg * s[:, None], x2 * c[:, None] + x1 * sg * s[:, None]], -1)
        r = held("rope" + (" inverse" if inverse else ""), work[:, :2], ref, _bf(ref), U * ref.abs(), G=_floor(ref))
        report.append(r)
    print("[rope D=%d H=%d %s] worst error / bound: forward %.3f, inverse %.3f" % (D, H, mode, report[0], report[1]))


def test_zz_report_worst_ratios():
    """(runs last in the file) the worst ratio error / bound of every quantity over the tests above"""
    print("worst error / bound per quantity: " + ", ".join("%s %.3g" % kv for kv in sorted(REPORT.items())))
    for k, v in REPORT.items():
        assert v <= 1.0, k
