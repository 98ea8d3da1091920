"""halva_sample_top_k_top_p (halva_amd/csrc/sample.hip) row by row against the fp64 restatement (tests/sample_ref_util.py).

The band DELTA = 1e-4 on cumulative mass.  The kernel's sums run per lane over its 32 values in index order, then over the wave's 64 lanes
as a 6-level tree, then over the 16 waves in order: at most (32 + 6 + 16) * 2^-24 = 3.3e-6 relative, plus a few fp32 ulps (<= 2^-21) on each
exp - under 1e-5 in all, far inside 1e-4 and below the bound of any order, V * 2^-24.

What the kernel kept is read from its two diagnostics: the set { x >= thr } on the fp32 quotients l / temperature (IEEE division, the
same bits on the host), whose size must be `kept`."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from sample_ref_util import DELTA, cdf_over, draw, sample_ref  # noqa: E402

VS = (1, 7, 64, 257, 4099, 32000, 32003)
PARAMS = ((1.0, 0, 1.0), (0.2, 0, 0.7), (1.0, 50, 1.0), (0.7, 50, 0.9), (1.0, 1, 1.0), (1.0, 0, 1e-6))
PEAKED = (0, 1, 2, 3, 4, 5, 6, 7, 14, 15)          # rows of _rows() that are 8 N(0,1) through bf16, nothing masked


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _bf16(a):
    return torch.as_tensor(a, dtype=torch.float32).bfloat16().float().numpy()


def _rows(V, seed):
    """16 fp32 rows: 0-7, 14, 15 peaked (8 N(0,1) rounded through bf16, so ties occur as behind the real head); 8 all equal; 9, 10 two
    levels (half / three entries high); 11, 12 peaked with -inf entries; 13 one finite logit."""
    rng = np.random.default_rng(seed)
    r = _bf16(8.0 * rng.standard_normal((16, V)))
    r[8] = 1.5
    r[9] = np.where(rng.random(V) < 0.5, 2.0, -1.0)
    r[9, rng.integers(V)] = 2.0
    r[10] = -3.0
    r[10, rng.integers(V, size=3)] = 4.0
    for b in (11, 12):
        r[b, rng.random(V) < 0.3] = -np.inf
        r[b, rng.integers(V)] = 1.0
    r[13] = -np.inf
    r[13, rng.integers(V)] = -2.5
    return r.astype(np.float32)


def _launch(rows, u, T, k, p, pad=0, B=None):
    """rows fp32 [B, V] numpy -> (token, thr, kept) numpy; pad > 0: row stride V + pad with NaN in the padding columns."""
    from halva_amd import kernels as K
    Bn, V = rows.shape
    buf = torch.full((Bn, V + pad), float("nan"), dtype=torch.float32, device="cuda")
    buf[:, :V] = torch.as_tensor(rows)
    tok, thr, kept = K.sample_top_k_top_p(buf[:, :V], torch.as_tensor(u, dtype=torch.float32).cuda(), T, k, p, want_diag=True)
    return tok.cpu().numpy(), thr.cpu().numpy(), kept.cpu().numpy()


def _u_for(ref, u0, frac):
    """A u inside a wide step of the fp64 CDF: the step u0 falls into if it is wider than 4 DELTA, else the next such step in ascending
    index (cyclically), at `frac` in [0.25, 0.75] of its width.  None when the row has no such step."""
    idx = np.flatnonzero(ref.K2)
    hi = ref.cdf[idx]
    lo = np.concatenate([[0.0], hi[:-1]])
    wide = np.flatnonzero(hi - lo > 4 * DELTA)
    if not len(wide):
        return None
    at = int(np.searchsorted(hi, u0, side="right"))
    j = wide[np.searchsorted(wide, at) % len(wide)]
    return float(lo[j] + frac * (hi[j] - lo[j]))


def _check_row(l, T, k, p, u, tok, thr, kept, exact):
    """The acceptance of one row; returns True when the token was also held to exact equality."""
    ref = sample_ref(l, T, k, p)
    x32 = (l.astype(np.float32) / np.float32(T)).astype(np.float32)
    mine = x32 >= thr
    assert int(mine.sum()) == int(kept) and kept >= 1, (int(mine.sum()), int(kept), float(thr))
    assert thr in x32                                                      # the threshold is a member
    # top-k is a count: exact.  top-p: a band on the mass above each entry
    p32 = float(np.float32(p))
    assert not (mine & ~ref.K1).any()
    if p32 >= 1.0:
        assert np.array_equal(mine, ref.K1)
    inner, outer = ref.K1 & (ref.S < p32 - DELTA), ref.K1 & (ref.S < p32 + DELTA)
    assert not (inner & ~mine).any() and not (mine & ~outer).any(), (int(inner.sum()), int(mine.sum()), int(outer.sum()))
    assert 0 <= tok < len(l) and mine[tok] and x32[tok] > -np.inf
    cdf = cdf_over(ref.x, mine)                                           # over the kernel's own threshold set
    before = np.flatnonzero(mine[:tok])
    lo = cdf[before[-1]] if len(before) else 0.0
    assert lo - DELTA <= u <= cdf[tok] + DELTA, (float(lo), float(u), float(cdf[tok]))
    if exact and np.array_equal(mine, ref.K2):
        assert tok == draw(ref.cdf, ref.K2, u)
        return True
    return False


@pytest.mark.parametrize("V", VS)
def test_rows_against_fp64(V):
    """Every row kind x parameter set x (ld = V, ld = V + 13 with NaN in the padding) at B = 16; rows run again at B = 1 and B = 3 give the
    same bits.  On the peaked rows u is seeded into a wide step of the fp64 CDF, more than DELTA from both ends (asserted), so the token
    there is held to exact equality."""
    _dev()
    rows = _rows(V, 100 + V)
    rng = np.random.default_rng(7 * V)
    n_exact = 0
    for T, k, p in PARAMS:
        u = rng.random(16).astype(np.float32)
        for b in PEAKED:
            ref = sample_ref(rows[b], T, k, p)
            ub = _u_for(ref, float(u[b]), 0.25 + 0.5 * rng.random())
            assert ub is not None, "a peaked row has a CDF step wider than 4 DELTA"
            u[b] = np.float32(ub)
            t = draw(ref.cdf, ref.K2, float(u[b]))
            prev = np.flatnonzero(ref.K2[:t])
            assert (ref.cdf[prev[-1]] if len(prev) else 0.0) + DELTA < float(u[b]) < ref.cdf[t] - DELTA
        u = np.minimum(u, np.nextafter(np.float32(1), np.float32(0)))
        out = _launch(rows, u, T, k, p)
        padded = _launch(rows, u, T, k, p, pad=13)
        for a, c in zip(out, padded):
            assert a.tobytes() == c.tobytes(), "row stride changes the result"
        for b in range(16):
            n_exact += _check_row(rows[b], T, k, p, float(u[b]), int(out[0][b]), out[1][b], int(out[2][b]), exact=b in PEAKED)
        # the same rows alone and in a batch of three, elsewhere in the batch: bitwise
        for sl in (slice(5, 6), slice(8, 11), slice(13, 14)):
            sub = _launch(rows[sl], u[sl], T, k, p, pad=13)
            for a, c in zip(out, sub):
                assert a[sl].tobytes() == c.tobytes(), (sl, a[sl], c)
        assert int(out[0][13]) == int(np.flatnonzero(rows[13] > -np.inf)[0])           # one finite logit: that index, any u
    print("V=%d: %d of %d peaked row cases held to exact equality" % (V, n_exact, len(PEAKED) * len(PARAMS)))
    assert n_exact >= len(PEAKED) * len(PARAMS) // 2


@pytest.mark.parametrize("V", (7, 257, 4099))
def test_u_at_both_ends_gives_the_first_and_last_kept_index(V):
    """All-equal and two-level rows (every kept entry carries at least 1 / V of the mass): u = 0 -> the first kept index,
    u = nextafter(1, 0) -> the last."""
    _dev()
    rows = _rows(V, 100 + V)[8:11]
    one = np.nextafter(np.float32(1), np.float32(0))
    for T, k, p in ((1.0, 0, 1.0), (1.0, 50, 1.0), (0.7, 50, 0.9)):
        first = _launch(rows, np.zeros(3, np.float32), T, k, p)
        last = _launch(rows, np.full(3, one, np.float32), T, k, p)
        for b in range(3):
            ref = sample_ref(rows[b], T, k, p)
            kept = np.flatnonzero(ref.K2)
            assert int(first[2][b]) == len(kept) == int(last[2][b])
            assert int(first[0][b]) == kept[0] and int(last[0][b]) == kept[-1], (b, T, k, p)


def test_bad_rows_give_minus_one_and_leave_the_others_alone():
    _dev()
    V = 4099
    rows = _rows(V, 5)
    u = np.random.default_rng(5).random(16).astype(np.float32)
    clean = _launch(rows, u, 0.7, 50, 0.9, pad=13)
    bad = rows.copy()
    bad[3, 1234] = np.nan
    bad[9] = -np.inf
    out = _launch(bad, u, 0.7, 50, 0.9, pad=13)
    for b in (3, 9):
        assert int(out[0][b]) == -1 and int(out[2][b]) == 0 and np.isnan(out[1][b])
    keep = [b for b in range(16) if b not in (3, 9)]
    for a, c in zip(clean, out):
        assert a[keep].tobytes() == c[keep].tobytes()
    assert (clean[0] >= 0).all()


@pytest.mark.parametrize("V", (7, 257, 32000))
def test_cuts_down_to_one_entry_return_argmax(V):
    _dev()
    rows = _rows(V, 100 + V)[:8]
    top = rows.argmax(1)
    rows[np.arange(8), top] += 1.0                                # unique maxima (8 N(0,1) through bf16 ties at the top now and then)
    assert all((rows[b] == rows[b].max()).sum() == 1 for b in range(8))
    u = np.random.default_rng(V).random(8).astype(np.float32)
    for T in (1.0, 0.2, 3.0):
        for k, p in ((1, 1.0), (0, 1e-6)):
            tok, thr, kept = _launch(rows, u, T, k, p)
            assert np.array_equal(tok, top) and (kept == 1).all(), (T, k, p)


def test_stratified_draws_follow_q():
    """One V = 64 row repeated 4096 times with u_j = (j + 0.5) / 4096: every token's count is within 1 + 4096 DELTA of 4096 q."""
    _dev()
    n = 4096
    row = _bf16(2.0 * np.random.default_rng(64).standard_normal(64)).astype(np.float32)
    u = ((np.arange(n) + 0.5) / n).astype(np.float32)
    for T, k, p in ((1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 5, 1.0)):
        tok, thr, kept = _launch(np.broadcast_to(row, (n, 64)).copy(), u, T, k, p)
        ref = sample_ref(row, T, k, p)
        assert (kept == int(ref.K2.sum())).all() and (thr == thr[0]).all()
        q = np.diff(np.concatenate([[0.0], ref.cdf]))
        counts = np.bincount(tok, minlength=64)
        assert np.abs(counts - n * q).max() <= 1 + n * DELTA, (counts, n * q)
        assert (np.diff(tok) >= 0).all()                          # ascending u walks the columns in ascending order
