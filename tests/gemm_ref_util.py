"""Float64 references, input generators, poison / sentinel embedding and per-element error bounds for the elementwise checks of
the MFMA GEMM, the LoRA weight gradients and the vision row kernels (tests/test_gemm_elementwise_gpu.py,
tests/test_vision_rowwise_gpu.py).  Nothing here calls a project kernel: the module imports without a GPU and works wherever its
tensors live (tests/test_gemm_ref_util_cpu.py proves it on the CPU).

Two input regimes.

EXACT: operands are bf16-exact integers in [-8, 8], a prior C holds integers |C| <= 1024, alpha is a power of two.  Every product
and every partial sum - in whatever order the MFMA, the k-slabs and the reduction take them - is then an integer (a multiple of
alpha after the scale) below 2^24, so every fp32 operation on the way is exact and the fp32 result IS the float64 one: fp32 outputs
are compared bit for bit, bf16 outputs with the float64 result rounded to nearest-even.  No error model, no tolerance: a dropped,
doubled or misplaced term changes an integer.  `assert_exact_headroom` checks the 2^24 premise on the actual sum of magnitudes
S = |A|^T |B| (+ |bias| + |C| / alpha), which bounds every partial sum.

RANDOM: randn-scaled operands with rows scaled by 1e3 and 1e-3 and an all-zero row.  Every element is held to the form of
tests/test_rowops_rowwise_gpu.py (restated here, because that module needs a GPU at import):

    |X_kernel - X_ref|  <=  |X_model - X_ref|  +  F |X_ref|  +  2 delta  +  G

X_ref: float64 on the kernel's own inputs.  X_model: X_ref rounded to bf16 where the kernel rounds (X_ref itself for fp32 outputs).
delta: the fp32 pre-rounding error, from S (the sum of the magnitudes of the terms) and n = K + 2 (+ splits) operations:
  * `delta_det` = 2 n U S, U = 2^-24: first-order gamma_n of any summation order and any rounding mode inside the MFMA (twice U:
    a truncating accumulator is admitted).  Used for bf16 outputs, where it is compared with the bf16 rounding itself.
  * `delta_prob` = U (LAMBDA sqrt(n) + 4) S, LAMBDA = 8 of tests/loss_ref_util.py (Higham & Mary 2019).  Used for fp32 outputs.
What the random regime can see: an error above 2 delta.  At K = 27 424 unit-variance rows 2 delta is about the size of ONE product,
so there it sees a wrong term only in the 1e3-scaled rows; a single term anywhere is the exact regime's job.

GELU (erf form, fp32): y = 0.5 x (1 + erf(x / sqrt 2)); `gelu_delta` = 0.5 |x| (E_ERF + U (1 + erf)) + U |y|.  E_ERF, the absolute
error of the device erff: the ROCm device math library documents no error bound for it, so E_ERF = 16 U absolute is assumed
(five orders below the bf16 rounding it is compared with: it only widens the band in which either neighbour is accepted).
"""
import math

import torch

from loss_ref_util import LAMBDA, U

bf16 = torch.bfloat16
E_ERF = 16 * U
SENT = 12.5
EXACT_LIMIT = 2.0 ** 24


def bf(x):
    """float64 value of x rounded to bf16"""
    return x.to(bf16).double()


def bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def floor_g(*ops):
    """G = 2^-100 prod (1 + |operand|): the floor of results below fp32's normal range"""
    g = torch.full_like(ops[0].double(), 2.0 ** -100)
    for o in ops:
        g = g * (1 + o.double().abs())
    return g


def held(report, name, got, ref, model, delta, F=0.0, G=None):
    """assert the bound of the module docstring for every element; returns (and records in `report`) the worst error / bound"""
    got, ref, model = got.double(), ref.double(), model.double()
    assert bool(torch.isfinite(got).all()), (name, "non-finite results")
    bound = (model - ref).abs() + F * ref.abs() + 2 * delta + (0 if G is None else G)
    err = (got - ref).abs()
    bad = err > bound
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        raise AssertionError("%s: %d elements outside the bound, first %s, got %s want %s bound %s" % (
            name, int(bad.sum()), idx, got[bad][:4].tolist(), ref[bad][:4].tolist(), bound[bad][:4].tolist()))
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = float(r.max()) if r.numel() else 0.0
    if report is not None:
        report[name] = max(report.get(name, 0.0), worst)
    return worst


def exact(name, got, ref64, out_dtype=None):
    """the exact regime's comparison: fp32 results equal float64 bit for bit, bf16 results its nearest-even rounding"""
    assert bool(torch.isfinite(got.float()).all()), (name, "non-finite results")
    want = ref64.to(got.dtype if out_dtype is None else out_dtype)
    if got.dtype == torch.float32:
        assert bool((want.double() == ref64).all()), (name, "the reference is not an fp32 value: no headroom")
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        raise AssertionError("%s: %d elements differ from the exact result, first %s, got %s want %s" % (
            name, int(bad.sum()), idx, got[bad][:4].tolist(), want[bad][:4].tolist()))


# ---------------------------------------------------------------------------------------------------------------------------------
# bounds
def n_ops(K, splits=0):
    return K + 2 + splits


def delta_det(S, K, splits=0):
    return 2 * n_ops(K, splits) * U * S


def delta_prob(S, K, splits=0):
    return U * (LAMBDA * math.sqrt(n_ops(K, splits)) + 4) * S


def gelu64(x):
    x = x.double()
    return 0.5 * x * (1 + torch.erf(x * math.sqrt(0.5)))


def gelu_delta(x, y=None):
    x = x.double()
    y = gelu64(x) if y is None else y
    return 0.5 * x.abs() * (E_ERF + U * (1 + torch.erf(x * math.sqrt(0.5)))) + U * y.abs()


def assert_exact_headroom(S, prior=None, alpha=1.0):
    """S: float64 sum of magnitudes of all terms of every output element (bounds every partial sum).  In units of alpha, the scaled
    sum plus the prior C must stay below 2^24 for the last fp32 add to be exact."""
    m, e = math.frexp(alpha)
    assert m == 0.5 and alpha <= 1.0, "alpha must be a power of two <= 1"
    top = float(S.max()) + (0.0 if prior is None else float(prior.double().abs().max()) / alpha)
    assert top < EXACT_LIMIT, "exact regime: |terms| sum to %g >= 2^24" % top
    return top


# ---------------------------------------------------------------------------------------------------------------------------------
# inputs
def int_tensor(shape, gen, device, lo=-8, hi=8, dtype=bf16):
    """uniform integers in [lo, hi], stored in `dtype` (bf16 rounds integers above 256 to its own grid: still integers)"""
    x = torch.randint(lo, hi + 1, tuple(shape), generator=gen, device=device).to(torch.float32).to(dtype)
    assert bool((x.double() == x.double().round()).all()) and float(x.double().abs().max()) <= max(abs(lo), abs(hi))
    return x


def rand_tensor(rows, cols, gen, device, scale=1.0):
    """randn * scale in bf16; row r is scaled by 1e3 for r % 4 == 2, by 1e-3 for r % 4 == 3, and row 1 is all zero"""
    x = torch.randn(rows, cols, generator=gen, device=device) * scale
    r = torch.arange(rows, device=device)[:, None]
    x = torch.where(r % 4 == 2, x * 1e3, x)
    x = torch.where(r % 4 == 3, x * 1e-3, x)
    if rows > 1:
        x[1] = 0
    return x.to(bf16)


# ---------------------------------------------------------------------------------------------------------------------------------
# poison and sentinels
def poison(numel, dtype, device):
    """NaN, +Inf, -Inf, cycling"""
    return torch.tensor([float("nan"), float("inf"), float("-inf")], device=device).repeat(numel // 3 + 1)[:numel].to(dtype)


def embed(x, fill, ld=None, col0=0, rows_before=2, rows_after=2, align=True):
    """x [R, n] as the window [rows_before : rows_before + R, col0 : col0 + n] of a new [rows_before + R + rows_after, ld] buffer
    whose every other element holds `fill` ('nan': the cycling poison; a float: that sentinel).  The window starts on a 16-byte
    boundary unless align=False (for kernels that read element by element).  Returns (buffer, window view)."""
    R, n = x.shape
    ld = n if ld is None else ld
    assert col0 + n <= ld
    H = rows_before + R + rows_after
    if fill == "nan":
        buf = poison(H * ld, x.dtype, x.device).view(H, ld)
    else:
        buf = torch.full((H, ld), float(fill), dtype=x.dtype, device=x.device)
    win = buf[rows_before:rows_before + R, col0:col0 + n]
    win.copy_(x)
    assert not align or win.data_ptr() % 16 == 0, "window not 16-byte aligned"
    return buf, win


def guard_rows(ld, elems=2 * 128 + 64):
    """rows of width ld that cover at least `elems` elements and at least two full rows"""
    return max(2, -(-elems // ld))


def outside_unchanged(buf, before, rows_before, R, col0, n):
    """every byte of `buf` outside the window equals `before` (a clone taken ahead of the call)"""
    a, b = bits(buf).clone(), bits(before).clone()
    a[rows_before:rows_before + R, col0:col0 + n] = 0
    b[rows_before:rows_before + R, col0:col0 + n] = 0
    return torch.equal(a, b)
