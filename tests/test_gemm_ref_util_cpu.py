"""tests/gemm_ref_util.py proved on the CPU: the exact regime's premise holds at the largest weight-gradient case, both regimes
reject a reference with ONE wrong term, and the random regime accepts a correct fp32 product."""
import pytest
import torch

import gemm_ref_util as R

ROWS = 27424          # the packed bench row count of the weight gradients: the longest sum any kernel of gemm.hip forms
M, N = 48, 64         # (reduced: the premise and the bounds are per element)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mutants(A, B, ref, k):
    """float64 A^T B with one product of row k dropped / row k of the sum doubled / one pair of elements transposed; the product is
    the row's largest with i != j.  Returns (i, j, |product|, the three wrong references)."""
    a, b = A.double(), B.double()
    i = int(a[k].abs().argmax())
    bk = b[k, :M].abs().clone()
    bk[i] = -1
    j = int(bk.argmax())
    assert float(a[k, i] * b[k, j]) != 0 and float(ref[i, j]) != float(ref[j, i])
    dropped = ref.clone()
    dropped[i, j] -= a[k, i] * b[k, j]
    doubled = ref + torch.outer(a[k], b[k])
    transposed = ref.clone()
    transposed[i, j], transposed[j, i] = ref[j, i], ref[i, j]
    return i, j, abs(float(a[k, i] * b[k, j])), {"one product dropped": dropped, "one row doubled": doubled,
                                                   "one element transposed": transposed}


def test_exact_regime_is_exact_at_the_largest_case_and_rejects_one_wrong_term():
    g = _gen(1)
    A = R.int_tensor((ROWS, M), g, "cpu")
    B = R.int_tensor((ROWS, N), g, "cpu")
    C0 = R.int_tensor((M, N), g, "cpu", -1024, 1024, torch.float32)
    S = A.double().abs().t() @ B.double().abs()
    assert 64 * ROWS < 2 ** 21
    for alpha in (1.0, 0.5, 0.25):
        top = R.assert_exact_headroom(S, C0, alpha)
        assert top <= 64 * ROWS + 1024 / alpha
        ref = C0.double() + alpha * (A.double().t() @ B.double())
        got = C0 + alpha * (A.float().t() @ B.float())                 # fp32 throughout, the library's own blocking and order
        R.exact("fp32 matmul", got, ref)
        R.exact("bf16 of it", got.to(torch.bfloat16), ref, torch.bfloat16)
    ref = A.double().t() @ B.double()
    got = A.float().t() @ B.float()
    for k in (0, ROWS // 2, ROWS - 1):
        for name, wrong in _mutants(A, B, ref, k)[3].items():
            with pytest.raises(AssertionError):
                R.exact(name, got, wrong)
    with pytest.raises(AssertionError):                                  # the premise itself is checked
        R.assert_exact_headroom(S * 1024)
    with pytest.raises(AssertionError):
        R.assert_exact_headroom(S, C0, 0.3)


@pytest.mark.parametrize("rows", [72, 4608, ROWS])
def test_random_regime_accepts_fp32_arithmetic_and_rejects_one_wrong_term(rows):
    g = _gen(2)
    A = R.rand_tensor(rows, M, g, "cpu")
    B = R.rand_tensor(rows, N, g, "cpu")
    a, b = A.double(), B.double()
    ref = a.t() @ b
    S = a.abs().t() @ b.abs()
    got = A.float().t() @ B.float()
    report = {}
    assert R.held(report, "f32", got, ref, ref, R.delta_prob(S, rows)) < 1.0
    assert R.held(report, "bf16", got.to(torch.bfloat16), ref, R.bf(ref), R.delta_det(S, rows)) < 1.0
    assert set(report) == {"f32", "bf16"}
    # What the random regime can see is a wrong term above 2 delta (+ the output rounding): S is carried by the 1e3-scaled rows, so
    # the term is taken from one of them and the premise is asserted, not assumed.  bf16 outputs (the deterministic delta) exist in
    # the product up to K = 5120; the 27 424-row sums are fp32 only.
    k = 2 + 4 * (rows // 8)
    i, j, term, wrong = _mutants(A, B, ref, k)
    assert term > 2 * float(R.delta_prob(S, rows)[i, j]) * 2
    for name, w in wrong.items():
        with pytest.raises(AssertionError):
            R.held(None, name, got, w, w, R.delta_prob(S, rows))
    if rows <= 4608:
        assert term > 2 * (2 * float(R.delta_det(S, rows)[i, j]) + 2.0 ** -8 * abs(float(ref[i, j])))
        for name, w in wrong.items():
            with pytest.raises(AssertionError):
                R.held(None, name, got.to(torch.bfloat16), w, R.bf(w), R.delta_det(S, rows))


def test_embedding_helpers():
    x = torch.arange(24, dtype=torch.float32).view(3, 8).to(torch.bfloat16)
    buf, win = R.embed(x, "nan", ld=24, col0=8, rows_before=2, rows_after=3)
    assert buf.shape == (8, 24) and torch.equal(win, x) and win.data_ptr() % 16 == 0
    mask = torch.ones(8, 24, dtype=torch.bool)
    mask[2:5, 8:16] = False
    assert not bool(torch.isfinite(buf[mask].float()).any()) and bool(torch.isnan(buf.float()).any())
    before = buf.clone()
    win.fill_(1.0)
    assert R.outside_unchanged(buf, before, 2, 3, 8, 8)
    buf[5, 8] = 0.0
    assert not R.outside_unchanged(buf, before, 2, 3, 8, 8)
    sbuf, swin = R.embed(x.float(), R.SENT)
    assert bool((sbuf[:2] == R.SENT).all()) and bool((sbuf[-2:] == R.SENT).all()) and torch.equal(swin, x.float())


def test_gelu_reference_and_delta():
    x = torch.tensor([0.0, -0.0, 1.0, -1.0, 12.0, -12.0], dtype=torch.float64)
    y = R.gelu64(x)
    assert torch.allclose(y, torch.nn.functional.gelu(x), rtol=0, atol=1e-15)
    got = torch.nn.functional.gelu(x.float())
    assert R.held(None, "gelu", got, y, y, R.gelu_delta(x, y), G=R.floor_g(x)) <= 1.0
