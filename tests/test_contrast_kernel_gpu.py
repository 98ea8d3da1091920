"""halva_contrast_select (halva_amd/csrc/contrast.hip) row by row against the reference (tests/contrast_ref_util.py): x in float32 as the
kernel forms it, then the fp64 restatement of the sampling rule on x.

The acceptance is tests/test_sample_kernel_gpu.py's _check_row with x in place of the logits - the band DELTA = 1e-4 on cumulative mass that
file derives, nothing new: x itself is reproduced bit for bit on the host, so what the kernel kept is { x / temperature >= thr } on the very
values it held, and the number of plausible columns is exact.  The rows of contrast_ref_util.pair_rows keep the cut and the top of x clear of
the fp32 rounding of x (checked in tests/test_contrast_ref_cpu.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import contrast_ref_util as C  # noqa: E402
from sample_ref_util import DELTA, draw  # noqa: E402
from test_sample_kernel_gpu import _check_row, _rows, _u_for  # noqa: E402

VS = (1, 5, 4095, 4096, 4097, 32000, 32768)
CASES = ((0.5, 0.1), (1.0, 0.0), (0.0, 0.5), (2.0, 1.0))
GREEDY, WARPED = (1.0, 1, 1.0), (0.2, 50, 0.7)
PAD, PAD_CD = 13, 7                       # odd row strides V + 13 and V + 7, NaN in the padding of both


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _launch(l, lcd, u, alpha, beta, T, k, p, pad=PAD, pad_cd=PAD_CD):
    """l, lcd fp32 [B, V] numpy -> (token, thr, kept, plausible) numpy"""
    from halva_amd import kernels as K
    B, V = l.shape
    a = torch.full((B, V + pad), float("nan"), dtype=torch.float32, device="cuda")
    c = torch.full((B, V + pad_cd), float("nan"), dtype=torch.float32, device="cuda")
    a[:, :V], c[:, :V] = torch.as_tensor(l), torch.as_tensor(lcd)
    out = K.contrast_select(a[:, :V], c[:, :V], torch.as_tensor(u, dtype=torch.float32).cuda(), alpha, beta, T, k, p, want_diag=True)
    return tuple(t.cpu().numpy() for t in out)


def _same(a, b, rows=slice(None)):
    return all(x[rows].tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("V", VS)
def test_rows_against_the_reference(V):
    """B = 3 with odd, different strides and poisoned padding, every (alpha, beta), greedy and (T 0.2, k 50, p 0.7); each row again at B = 1
    and with other strides: the same bits."""
    _dev()
    l, lcd = C.pair_rows(V, 300 + V)
    rng = np.random.default_rng(V)
    n_exact = n_cases = 0
    for alpha, beta in CASES:
        for T, k, p in (GREEDY, WARPED):
            greedy = (T, k, p) == GREEDY
            u = np.zeros(3, np.float32) if greedy else rng.random(3).astype(np.float32)
            exact = [greedy] * 3
            if not greedy:
                for b in range(3):
                    ref, _, _ = C.contrast_ref(l[b], lcd[b], alpha, beta, T, k, p)
                    ub = _u_for(ref, float(u[b]), 0.25 + 0.5 * rng.random())
                    if ub is not None:
                        u[b], exact[b] = np.float32(ub), True
            out = _launch(l, lcd, u, alpha, beta, T, k, p)
            for b in range(3):
                x, plausible = C.contrast_x(l[b], lcd[b], alpha, beta)
                assert int(out[3][b]) == int(plausible.sum()), (V, alpha, beta, b)
                n_exact += _check_row(x, T, k, p, float(u[b]), int(out[0][b]), out[1][b], int(out[2][b]), exact=exact[b])
                n_cases += 1
                if greedy:
                    assert int(out[0][b]) == int(x.argmax()) == C.contrast_token(l[b], lcd[b], alpha, beta, T, k, p, 0.0)
                    assert int(out[2][b]) == int((x == x.max()).sum())
                assert _same(out, _launch(l[b:b + 1], lcd[b:b + 1], u[b:b + 1], alpha, beta, T, k, p, pad=0, pad_cd=3), slice(b, b + 1))
    print("V=%d: %d of %d row cases held to exact token equality" % (V, n_exact, n_cases))
    assert n_exact >= n_cases // 2


@pytest.mark.parametrize("V", (5, 4097, 32000))
def test_alpha_zero_beta_zero_is_the_plain_select_bitwise(V):
    """x = 1 * l - 0 * lcd = l: token, thr and kept are halva_sample_top_k_top_p's on `logits`, bit for bit, on all its row kinds (ties, -inf
    entries, one finite logit)."""
    _dev()
    from halva_amd import kernels as K
    rows = _rows(V, 100 + V)
    rng = np.random.default_rng(V)
    lcd = (4.0 * rng.standard_normal(rows.shape)).astype(np.float32)
    u = rng.random(16).astype(np.float32)
    for T, k, p in (GREEDY, WARPED, (1.0, 0, 1.0)):
        got = _launch(rows, lcd, u, 0.0, 0.0, T, k, p)
        want = K.sample_top_k_top_p(torch.as_tensor(rows).cuda(), torch.as_tensor(u).cuda(), T, k, p, want_diag=True)
        assert _same(got[:3], tuple(t.cpu().numpy() for t in want)), (V, T, k, p)
        assert (got[3] == V).all()                              # beta = 0: every column is plausible
        assert (got[0] >= 0).all()


def test_unservable_rows_give_minus_one_and_leave_the_others_alone():
    """NaN or +inf in either input, -inf - -inf in x, nothing above -inf in l: token -1, kept 0, thr NaN; the neighbours keep their bits.  A
    NaN, +inf or -inf in lcd under a MASKED column changes nothing (the column is masked before x is formed)."""
    _dev()
    V = 4097
    rng = np.random.default_rng(9)
    l, lcd = C.pair_rows(V, 9, B=8)
    u = rng.random(8).astype(np.float32)
    alpha, beta, (T, k, p) = 0.5, 0.1, WARPED
    clean = _launch(l, lcd, u, alpha, beta, T, k, p)
    assert (clean[0] >= 0).all()
    bl, bc = l.copy(), lcd.copy()
    top = l.argmax(1)
    plausible = [C.contrast_x(l[b], lcd[b], alpha, beta)[1] for b in range(8)]
    assert int((~plausible[2]).sum()) >= 3
    second = [int(np.flatnonzero(q)[-1]) for q in plausible]
    bl[0, 1234] = np.nan                                        # NaN in l (a masked or plausible column alike)
    bc[1, top[1]] = np.inf                                      # +inf in lcd, plausible column (x would be -inf, not NaN: still -1)
    bc[2, np.flatnonzero(~plausible[2])[:3]] = (np.nan, np.inf, -np.inf)      # masked columns: no effect
    bl[3, 7] = np.inf                                           # +inf in l
    bc[4, second[4]] = np.nan                                   # NaN in lcd, plausible column
    bl[5] = -np.inf                                             # nothing above -inf
    bc[6, top[6]] = -np.inf                                     # x = +inf
    out = _launch(bl, bc, u, alpha, beta, T, k, p)
    for b in (0, 1, 3, 4, 5, 6):
        assert not C.servable(bl[b], bc[b], alpha, beta)
        assert int(out[0][b]) == -1 and int(out[2][b]) == 0 and np.isnan(out[1][b]), b
    assert C.servable(bl[2], bc[2], alpha, beta)
    assert _same(clean, tuple(o[[2, 7]] for o in out), [2, 7])
    # -inf - -inf with everything plausible (beta = 0), alpha = 0 included (0 * -inf)
    bl2, bc2 = l.copy(), lcd.copy()
    bl2[0, 5] = bc2[0, 5] = -np.inf
    bc2[1, 5] = -np.inf
    for a in (0.5, 0.0):
        clean0 = _launch(l, lcd, u, a, 0.0, T, k, p)
        out = _launch(bl2, bc2, u, a, 0.0, T, k, p)
        assert out[0][:2].tolist() == [-1, -1] and _same(clean0, tuple(o[2:] for o in out), slice(2, 8))


def test_a_tie_among_the_maxima_of_x_gives_the_lower_index():
    _dev()
    for V in (5, 4097, 32768):
        l, lcd = C.pair_rows(V, 40 + V)
        x = [C.contrast_x(l[b], lcd[b], 0.5, 0.1)[0] for b in range(3)]
        top = [int(v.argmax()) for v in x]
        twins = []
        for b in range(3):                                      # a second column with the top column's l and lcd: the same x, bit for bit
            j = (top[b] + (1 + 2 * b) * max(V // 3, 1)) % V
            j = j if j != top[b] else (j + 1) % V
            l[b, j], lcd[b, j] = l[b, top[b]], lcd[b, top[b]]
            twins.append(j)
        tok, thr, kept, _ = _launch(l, lcd, np.zeros(3, np.float32), 0.5, 0.1, *GREEDY)
        assert tok.tolist() == [min(a, b) for a, b in zip(top, twins)] and kept.tolist() == [2, 2, 2]
        last, _, _, _ = _launch(l, lcd, np.full(3, np.nextafter(np.float32(1), np.float32(0))), 0.5, 0.1, *GREEDY)
        assert last.tolist() == [max(a, b) for a, b in zip(top, twins)]


def test_stratified_draws_follow_q():
    """One V = 64 row pair repeated 4096 times with u_j = (j + 0.5) / 4096: every token's count is within 1 + 4096 DELTA of 4096 q."""
    _dev()
    n = 4096
    l, lcd = C.pair_rows(64, 64, B=1)
    l, lcd = (l / 4).astype(np.float32), (lcd / 4).astype(np.float32)
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    rep = lambda a: np.broadcast_to(a, (n, 64)).copy()          # noqa: E731
    for alpha, beta, (T, k, p) in ((0.5, 0.1, (1.0, 0, 1.0)), (1.0, 0.0, (0.7, 50, 0.9))):
        tok, thr, kept, plaus = _launch(rep(l), rep(lcd), u, alpha, beta, T, k, p)
        ref, x, plausible = C.contrast_ref(l[0], lcd[0], alpha, beta, T, k, p)
        assert (kept == int(ref.K2.sum())).all() and (plaus == int(plausible.sum())).all() and (thr == thr[0]).all()
        q = np.diff(np.concatenate([[0.0], ref.cdf]))
        assert np.abs(np.bincount(tok, minlength=64) - n * q).max() <= 1 + n * DELTA
        assert int(tok[0]) == draw(ref.cdf, ref.K2, float(u[0]))
