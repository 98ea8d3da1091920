"""Row-wise checks of every launch path of the loss kernels (halva_amd/csrc/loss.hip) against float64, with poisoned padding.

test_hip_kernels.py holds token_logp / kl_rows to an atol, one Frobenius error per gradient and one comparison of the summed KL, on
contiguous rows at V = 32000.  Here every row of logp / lse / kl and every element of dlogits / dpol is held to the float64
reference of tests/loss_ref_util.py on the kernel's own inputs, with the bounds derived in that module's docstring (E_lse, E_logp,
E_kl, and (1 + F) delta + F |ref| per element, F = 2^-8 for bf16 and 2^-24 for fp32 outputs).  The worst ratio error / bound of
every quantity is printed.

Paths, selected by the launcher conditions in loss.hip (R rows, V columns, row stride ld, W = 8 bf16 / 4 fp32 elements per 16 bytes):
  token_logp fwd / bwd
    bf16 KCH=16     dt == BF16 and V / 8 <= 16 * 256           (V <= 32 775)
    bf16 KCH=0      dt == BF16 and V / 8 > 4096                (streaming: V = 32 784, 65 536)
    fp32            dt == F32                                 (the compat trainer's fp32 logits)
    inside each: vector only (row_vec_ok: base 16-byte aligned, ld * sizeof % 16 == 0, V % W == 0), vector + scalar tail (V % W != 0),
    whole-row scalar (ld * sizeof % 16 != 0, or a base pointer one element off: nvec = 0)
  kl_rows
    bf16 KEEP       dt == BF16 and dpol and HALVA_KL_KEEP != 0 and vec16 (pointers 16-byte aligned, ld % 8 == 0, V % 8 == 0) and
                    V / 8 <= 8 * 512: kl_rows_kernel<bf16, 512, true, 8>
    bf16 256        every other bf16 call: dpol == NULL, HALVA_KL_KEEP=0, V % 8 != 0, V > 32 768, misaligned
    fp32            dt == F32, with and without dpol
    with the same vector / tail / whole-row-scalar split inside the kernel (row_vec_ok of pol, ref and dpol)

Poisoning.  Every case runs clean, then with NaN / +-Inf in the logits columns [V, ld) and in the element before an offset base, in
whole rows with g == 0 (token bwd) or w == 0 (KL), and with NaN-prefilled logp / lse / kl / dlogits / dpol.  The valid results must
equal the clean run's bit for bit, rows with g == 0 / w == 0 come out as exact zeros, and the output columns [V, ld) keep their
sentinel.  The in-place forms (dlogits == logits as dpa.py's _LmHeadLogp runs it, dpol == pol as _LmHeadKL does) must equal the
out-of-place results bit for bit.  gscale = 0.5 scales dpol exactly (a power of two); gscale = -3 is held to the bound.

KL bias: test_kl_summed_error sums kl_r - kl_r^fp64 over R = 32 768 rows of V = 32 000 (the KEEP and the fp32 path) and holds the
signed sum to loss_ref_util.KL_SUM_TOL = 1.6e-3; test_mismatch_per_row_bias_is_caught_by_the_summed_check_only shows that this check
sees a bias of 2^-22 |lse| per row that every per-row check passes.  Entry points go through the C ABI (halva_amd.hip.call).
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import loss_ref_util as L  # noqa: E402
from halva_amd.hip import BF16, F32, call, ptr, stream_ptr  # noqa: E402

DEV = "cuda"
DT = {"bf16": torch.bfloat16, "f32": torch.float32}
CODE = {torch.bfloat16: BF16, torch.float32: F32}
SENT = {torch.bfloat16: 12.5, torch.float32: -3.25}
POISON = (float("nan"), float("inf"), float("-inf"))

# token cases: (dtype, V, ld, base offset in elements, R)
TOKEN_CASES = {
    "bf16_k16_vec": ("bf16", 32000, 32000, 0, 37),
    "bf16_k16_vec_R4099": ("bf16", 32000, 32000, 0, 4099),
    "bf16_k16_tail1": ("bf16", 32001, 32008, 0, 37),
    "bf16_k16_tail3": ("bf16", 32003, 32008, 0, 37),
    "bf16_k16_V32775": ("bf16", 32775, 32776, 0, 37),           # the largest KCH=16 row: 4096 chunks + a 7-element tail
    "bf16_k16_scalar_ld": ("bf16", 32001, 32001, 0, 37),
    "bf16_k16_scalar_off": ("bf16", 32000, 32008, 1, 37),
    "bf16_k16_V1": ("bf16", 1, 8, 0, 1),
    "bf16_k16_V7": ("bf16", 7, 8, 0, 37),
    "bf16_k16_V8": ("bf16", 8, 16, 0, 37),
    "bf16_k16_V255": ("bf16", 255, 264, 0, 37),
    "bf16_k0_V32784": ("bf16", 32784, 32784, 0, 37),
    "bf16_k0_V65536": ("bf16", 65536, 65544, 0, 37),
    "bf16_k0_tail": ("bf16", 32777, 32784, 0, 37),
    "bf16_k0_scalar_ld": ("bf16", 32785, 32785, 0, 37),
    "bf16_k0_scalar_off": ("bf16", 32784, 32792, 1, 37),
    "f32_vec": ("f32", 32000, 32000, 0, 37),
    "f32_vec_R4099": ("f32", 32000, 32004, 0, 4099),
    "f32_tail1": ("f32", 32001, 32004, 0, 37),
    "f32_tail3": ("f32", 32003, 32004, 0, 37),
    "f32_scalar_ld": ("f32", 32001, 32001, 0, 37),
    "f32_scalar_off": ("f32", 32000, 32004, 1, 37),
    "f32_V1": ("f32", 1, 4, 0, 1),
    "f32_V7": ("f32", 7, 8, 0, 37),
    "f32_V255": ("f32", 255, 256, 0, 37),
}

# KL cases: (dtype, V, ld, offset, R, with dpol, HALVA_KL_KEEP)
KL_CASES = {
    "bf16_keep": ("bf16", 32000, 32000, 0, 37, True, "1"),
    "bf16_keep_R4099": ("bf16", 32000, 32000, 0, 4099, True, "1"),
    "bf16_keep_V32768": ("bf16", 32768, 32768, 0, 37, True, "1"),
    "bf16_keep_V8": ("bf16", 8, 8, 0, 37, True, "1"),
    "bf16_256_nodpol": ("bf16", 32000, 32000, 0, 37, False, "1"),
    "bf16_256_keep0": ("bf16", 32000, 32000, 0, 37, True, "0"),
    "bf16_256_tail1": ("bf16", 32001, 32008, 0, 37, True, "1"),
    "bf16_256_tail3": ("bf16", 32003, 32008, 0, 37, True, "1"),
    "bf16_256_V32776": ("bf16", 32776, 32776, 0, 37, True, "1"),
    "bf16_256_V65536": ("bf16", 65536, 65536, 0, 37, True, "1"),
    "bf16_256_scalar_ld": ("bf16", 32001, 32001, 0, 37, True, "1"),
    "bf16_256_scalar_off": ("bf16", 32000, 32008, 1, 37, True, "1"),
    "bf16_256_V1": ("bf16", 1, 8, 0, 1, True, "1"),
    "bf16_256_V7": ("bf16", 7, 8, 0, 37, True, "1"),
    "bf16_256_V255": ("bf16", 255, 264, 0, 37, True, "1"),
    "f32_dpol": ("f32", 32000, 32000, 0, 37, True, "1"),
    "f32_dpol_R4099": ("f32", 32000, 32000, 0, 4099, True, "1"),
    "f32_nodpol": ("f32", 32000, 32000, 0, 37, False, "1"),
    "f32_tail1": ("f32", 32001, 32004, 0, 37, True, "1"),
    "f32_scalar_ld": ("f32", 32001, 32001, 0, 37, True, "1"),
    "f32_scalar_off": ("f32", 32000, 32004, 1, 37, True, "1"),
    "f32_V7": ("f32", 7, 8, 0, 37, True, "1"),
}
GSCALE_CASES = ["bf16_keep", "bf16_256_tail1", "bf16_256_scalar_off", "f32_dpol", "f32_scalar_ld"]


# ---------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def logit_rows(R, V, seed, kinds=6):
    """float32 [R, V]: row r of kind r % kinds - 0 N(0, 3); 1 LM-like: a N(0, 2) tail with one to three logits 15-25 nat above its
    max; 2 / 3 the N(0, 3) row shifted by +1000 / -1000; 4 all equal; 5 N(0, 0.5)"""
    g = _gen(seed)
    z = torch.randn(R, V, generator=g, device=DEV) * 3
    k = torch.arange(R, device=DEV) % kinds
    tail = torch.randn(R, V, generator=g, device=DEV) * 2
    npk = torch.randint(1, 4, (R,), generator=g, device=DEV)
    for j in range(3):
        idx = torch.randint(0, V, (R,), generator=g, device=DEV)
        up = tail.amax(-1) + 15 + 10 * torch.rand(R, generator=g, device=DEV)
        tail[torch.arange(R, device=DEV), idx] = torch.where(j < npk, up, tail[torch.arange(R, device=DEV), idx])
    z = torch.where((k == 1)[:, None], tail, z)
    z = torch.where((k == 2)[:, None], z + 1000, z)
    z = torch.where((k == 3)[:, None], z - 1000, z)
    z = torch.where((k == 4)[:, None], torch.full_like(z, 0.375) * (torch.arange(R, device=DEV)[:, None] % 5 - 2), z)
    z = torch.where((k == 5)[:, None], z / 6, z)
    return z


def kl_pair(R, V, seed, dtype):
    """(pol, ref) [R, V] in dtype: ref = pol + delta N(0, 1) with delta in {1e-3, 1e-2, 1e-1} by row, on the rows of logit_rows,
    and every 7th row a spread > 104 nat (+-60 logits on a N(0, 1) row), where fp32 softmax underflows"""
    pol = logit_rows(R, V, seed)
    g = _gen(seed + 1)
    r = torch.arange(R, device=DEV)
    spread = torch.randn(R, V, generator=g, device=DEV)
    if V >= 4:
        spread[:, 0] += 60
        spread[:, V // 2] -= 60
        spread[:, V - 1] -= 55
    pol = torch.where((r % 7 == 6)[:, None], spread, pol)
    delta = torch.tensor([1e-3, 1e-2, 1e-1], device=DEV)[r % 3][:, None]
    ref = pol + delta * torch.randn(R, V, generator=g, device=DEV)
    return pol.to(dtype), ref.to(dtype)


def _cycle(n, vals=POISON):
    return torch.tensor(vals, device=DEV).repeat(n // len(vals) + 1)[:n]


def rows_buffer(z, ld, off, pad_fill):
    """(flat, view): z [R, V] placed in a flat buffer at element offset `off` with row stride ld; columns [V, ld) and the `off`
    elements in front hold pad_fill ('poison' = NaN / +-Inf cycling, else a finite number)"""
    R, V = z.shape
    flat = torch.empty(off + R * ld + 8, dtype=z.dtype, device=DEV)
    if pad_fill == "poison":
        flat.copy_(_cycle(flat.numel()).to(z.dtype))
    else:
        flat.fill_(pad_fill)
    view = flat[off:off + R * ld].view(R, ld)
    view[:, :V] = z
    return flat, view


def _bits(x):
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


def same_bits(a, b):
    return torch.equal(_bits(a.contiguous()), _bits(b.contiguous()))


REPORT = {}


def _note(name, value):
    REPORT[name] = max(REPORT.get(name, 0.0), value)


def held(name, got, want, bound, rows=None):
    """got / want / bound: [R] or [R, V]; rows [R] bool (None = all).  Asserts |got - want| <= bound and returns the worst ratio"""
    got, want, bound = got.double(), want.double(), bound.double()
    if rows is not None:
        got, want, bound = got[rows], want[rows], bound[rows]
    assert bool(torch.isfinite(got).all()), (name, "non-finite results")
    err = (got - want).abs()
    bad = err > bound
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        raise AssertionError("%s: %d outside the bound, first %s, worst error / bound %.3g" % (name, int(bad.sum()), idx, L.ratio(err, bound)))
    r = L.ratio(err, bound)
    _note(name, r)
    return r


def targets(R, V, seed):
    """0, V - 1, inside the scalar tail (the last V % 8 columns; V - 1 where there is none) and random"""
    g = _gen(seed)
    t = torch.randint(0, V, (R,), generator=g, device=DEV)
    r = torch.arange(R, device=DEV)
    tail0 = V - (V % 8) if V % 8 else V - 1
    tail = tail0 + torch.randint(0, max(1, V - tail0), (R,), generator=g, device=DEV)
    t = torch.where(r % 4 == 0, torch.zeros_like(t), t)
    t = torch.where(r % 4 == 1, torch.full_like(t, V - 1), t)
    t = torch.where(r % 4 == 2, tail.clamp_max(V - 1), t)
    return t.int()


def _token_fwd(view, dt, ld, tgt, R, V, fill=None):
    logp = torch.full((R,), float("nan") if fill is None else fill, device=DEV)
    lse = torch.full((R,), float("nan") if fill is None else fill, device=DEV)
    call("halva_token_logp_fwd", view.data_ptr(), CODE[dt], ld, ptr(tgt), ptr(logp), ptr(lse), R, V, stream_ptr())
    return logp, lse


def _token_bwd(view, dt, ld, tgt, lse, g, dview, R, V):
    call("halva_token_logp_bwd", view.data_ptr(), CODE[dt], ld, ptr(tgt), ptr(lse), ptr(g), dview.data_ptr(), R, V, stream_ptr())


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", list(TOKEN_CASES))
def test_token_logp_rowwise_with_poison_and_in_place(case):
    dn, V, ld, off, R = TOKEN_CASES[case]
    dt = DT[dn]
    z = logit_rows(R, V, seed=V + R).to(dt)
    tgt = targets(R, V, seed=R + 1)
    g = torch.randn(R, generator=_gen(3), device=DEV)
    r = torch.arange(R, device=DEV)
    gzero = (r % 7 == 3) & (R > 1)
    g[gzero] = 0
    live = ~gzero
    # --- clean run: finite garbage in the padding
    _, x = rows_buffer(z, ld, off, 7.0)
    logp, lse = _token_fwd(x, dt, ld, tgt, R, V)
    want_lp, want_lse = L.logp_ref(z, tgt)
    a = held("token logp", logp, want_lp, L.logp_bound(z, want_lp))
    b = held("token lse", lse, want_lse, L.lse_bound(z))
    _, dl = rows_buffer(torch.full_like(z, SENT[dt]), ld, off, SENT[dt])
    _token_bwd(x, dt, ld, tgt, lse, g, dl, R, V)
    bound, want = L.dlogits_bound(z, tgt, g, dt)
    c = held("token dlogits", dl[:, :V], want, bound)
    assert bool((dl[gzero, :V] == 0).all()), "rows with g == 0 must be exact zeros"
    assert bool((dl[:, V:] == SENT[dt]).all()), "dlogits columns [V, ld) were written"
    print("[token %s] worst error / bound: logp %.3f, lse %.3f, dlogits %.3f" % (case, a, b, c))
    # --- poisoned run: padding, whole g == 0 rows, NaN-prefilled outputs
    zp = z.clone()
    zp[gzero] = _cycle(int(gzero.sum()) * V).view(-1, V).to(dt)
    _, xp = rows_buffer(zp, ld, off, "poison")
    logp_p, lse_p = _token_fwd(xp, dt, ld, tgt, R, V)
    assert same_bits(logp_p[live], logp[live]) and same_bits(lse_p[live], lse[live]), "poisoned padding changed logp / lse"
    _, dlp = rows_buffer(torch.full_like(z, float("nan")), ld, off, SENT[dt])
    _token_bwd(xp, dt, ld, tgt, lse_p, g, dlp, R, V)
    assert same_bits(dlp[:, :V], dl[:, :V]), "poisoned run's dlogits differ from the clean run's"
    assert bool((dlp[:, V:] == SENT[dt]).all())
    # --- in place (dlogits == logits), on the poisoned buffer: same bits, and the padding keeps its poison
    flat_i, xi = rows_buffer(zp, ld, off, "poison")
    pad_before = xi[:, V:].clone()
    _token_bwd(xi, dt, ld, tgt, lse_p, g, xi, R, V)
    assert same_bits(xi[:, :V], dl[:, :V]), "in-place dlogits differ from the out-of-place ones"
    assert same_bits(xi[:, V:], pad_before), "in-place run wrote the columns [V, ld)"


def _kl_call(pv, rv, dt, ld, w, dv, gscale, R, V):
    kl = torch.full((R,), float("nan"), device=DEV)
    call("halva_kl_rows", pv.data_ptr(), rv.data_ptr(), CODE[dt], ld, ptr(w), ptr(kl), None if dv is None else dv.data_ptr(),
         float(gscale), R, V, stream_ptr())
    return kl


def _kl_weights(R):
    r = torch.arange(R, device=DEV)
    w = torch.tensor([1.0, 0.5, 2.0], device=DEV)[r % 3]
    w[(r % 7 == 3) & (R > 1)] = 0
    return w


@pytest.mark.timeout(300)
@pytest.mark.parametrize("case", list(KL_CASES))
def test_kl_rows_rowwise_with_poison_and_in_place(case, monkeypatch):
    dn, V, ld, off, R, with_d, keep = KL_CASES[case]
    monkeypatch.setenv("HALVA_KL_KEEP", keep)
    dt = DT[dn]
    pol, ref = kl_pair(R, V, seed=V + 3 * R, dtype=dt)
    w = _kl_weights(R)
    wz, live = w == 0, w != 0
    _, pv = rows_buffer(pol, ld, off, 5.0)
    _, rv = rows_buffer(ref, ld, off, -5.0)
    dv = rows_buffer(torch.full_like(pol, SENT[dt]), ld, off, SENT[dt])[1] if with_d else None
    kl = _kl_call(pv, rv, dt, ld, w, dv, 1.0, R, V)
    a = held("kl", kl, L.kl_ref(pol, ref, w), L.kl_bound(pol, ref, w))
    assert bool((kl[wz] == 0).all())
    msg = "[kl %s] worst error / bound: kl %.3f" % (case, a)
    if with_d:
        bound, want = L.dpol_bound(pol, ref, dt, w, 1.0)
        c = held("kl dpol", dv[:, :V], want, bound)
        msg += ", dpol %.3f" % c
        assert bool((dv[wz, :V] == 0).all()), "rows with w == 0 must be exact zeros"
        assert bool((dv[:, V:] == SENT[dt]).all()), "dpol columns [V, ld) were written"
    print(msg)
    # --- poisoned: padding, whole w == 0 rows of both inputs, NaN-prefilled kl / dpol
    polp, refp = pol.clone(), ref.clone()
    polp[wz] = _cycle(int(wz.sum()) * V).view(-1, V).to(dt)
    refp[wz] = _cycle(int(wz.sum()) * V, POISON[::-1]).view(-1, V).to(dt)
    _, pvp = rows_buffer(polp, ld, off, "poison")
    _, rvp = rows_buffer(refp, ld, off, "poison")
    dvp = rows_buffer(torch.full_like(pol, float("nan")), ld, off, SENT[dt])[1] if with_d else None
    klp = _kl_call(pvp, rvp, dt, ld, w, dvp, 1.0, R, V)
    assert same_bits(klp, kl), "poisoned run's kl differ from the clean run's"
    if not with_d:
        return
    assert same_bits(dvp[:, :V], dv[:, :V]) and bool((dvp[:, V:] == SENT[dt]).all())
    # --- in place (dpol == pol)
    _, pvi = rows_buffer(polp, ld, off, "poison")
    pad_before = pvi[:, V:].clone()
    kli = _kl_call(pvi, rvp, dt, ld, w, pvi, 1.0, R, V)
    assert same_bits(kli, kl), "in-place kl differ"
    assert same_bits(pvi[:, :V], dv[:, :V]), "in-place dpol differ from the out-of-place one"
    assert same_bits(pvi[:, V:], pad_before)
    # --- gscale
    if case in GSCALE_CASES:
        d5 = rows_buffer(torch.zeros_like(pol), ld, off, SENT[dt])[1]
        _kl_call(pvp, rvp, dt, ld, w, d5, 0.5, R, V)
        assert same_bits(d5[:, :V], (dv[:, :V] * 0.5).to(dt)), "gscale = 0.5 must scale dpol exactly"
        d3 = rows_buffer(torch.zeros_like(pol), ld, off, SENT[dt])[1]
        _kl_call(pvp, rvp, dt, ld, w, d3, -3.0, R, V)
        bound, want = L.dpol_bound(pol, ref, dt, w, -3.0)
        held("kl dpol gscale=-3", d3[:, :V], want, bound, rows=live)
        assert bool((d3[wz, :V] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
def _kl_summed(dt, keep, monkeypatch, R=32768, V=32000, chunk=2048, kinds=6):
    """kernel kl (with dpol, in place) and float64 kl over R near-zero-KL rows: pol from logit_rows (all six kinds; kinds=2: only the
    N(0, 3) and the peaked LM-like rows), ref = pol + delta N(0, 1), delta in {1e-3, 1e-2, 1e-1} by row.  Returns (kl [R] fp32,
    kl64 [R], bound [R]).  Measured on the MI355X, |sum| over 32 768 rows: 8.4e-3 (bf16 KEEP) and 1.7e-3 (fp32) with the final
    combine Ar / Sr - lse_r + lse_p, 1.4e-4 and 2.1e-4 with (Mp - Mr) + log2(Sp / Sr) (loss.hip, kl_rows_kernel)."""
    monkeypatch.setenv("HALVA_KL_KEEP", keep)
    kls, refs, bounds = [], [], []
    for c0 in range(0, R, chunk):
        pol = logit_rows(chunk, V, seed=1000 + c0, kinds=kinds)
        d = torch.tensor([1e-3, 1e-2, 1e-1], device=DEV)[torch.arange(chunk, device=DEV) % 3][:, None]
        ref = (pol + d * torch.randn(chunk, V, generator=_gen(c0 + 1), device=DEV)).to(dt)
        pol = pol.to(dt)
        kl = torch.empty(chunk, device=DEV)
        dp = pol.clone()
        call("halva_kl_rows", ptr(dp), ptr(ref), CODE[dt], V, None, ptr(kl), ptr(dp), 1.0, chunk, V, stream_ptr())
        kls.append(kl)
        refs.append(L.kl_ref(pol, ref))
        bounds.append(L.kl_bound(pol, ref))
    return torch.cat(kls), torch.cat(refs), torch.cat(bounds)


@pytest.mark.timeout(600)
@pytest.mark.parametrize("dn,keep", [("bf16", "1"), ("f32", "1")], ids=["bf16_keep", "f32"])
def test_kl_summed_error(dn, keep, monkeypatch):
    kl, kl64, bound = _kl_summed(DT[dn], keep, monkeypatch)
    a = held("kl (summed-test rows)", kl, kl64, bound)
    err = kl.double() - kl64
    s, sa = float(err.sum()), float(err.abs().sum())
    print("[kl summed %s] R = %d: |sum(kl - kl64)| = %.3e, sum|kl - kl64| = %.3e, sum kl64 = %.4e, worst row error / bound %.3f"
          % (dn, kl.numel(), abs(s), sa, float(kl64.sum()), a))
    _note("kl summed error / KL_SUM_TOL", abs(s) / L.KL_SUM_TOL)
    assert abs(s) <= L.KL_SUM_TOL, ("summed KL error", s, sa)


# ---------------------------------------------------------------------------------------------------------------------------------
# phrase_sum
PHRASE = [(P, T1) for P in (0, 1, 40) for T1 in (1, 255, 256, 4095)]


def _phrase_inputs(B, T1, P, seed):
    g = _gen(seed)
    logp = -torch.rand(B, T1, generator=g, device=DEV) * 12
    labels = torch.randint(0, 32000, (B, T1), generator=g, device=DEV)
    labels[torch.rand(B, T1, generator=g, device=DEV) < 0.3] = -100
    slot_ids = torch.arange(1, P + 1, device=DEV) * 3                                    # sorted, unique, non-zero
    pool = torch.cat([slot_ids, torch.tensor([0, -100, 2, 1000], device=DEV)])              # 2 and 1000: ids no slot has
    signs = pool[torch.randint(0, pool.numel(), (B, T1), generator=g, device=DEV)]
    if P > 1:
        signs[0][signs[0] == slot_ids[P // 2]] = 0                                          # a slot id absent from row 0
    return logp, labels.long(), signs.long(), slot_ids.long()


@pytest.mark.parametrize("P,T1", PHRASE, ids=["P%d-T%d" % c for c in PHRASE])
def test_phrase_sum_rowwise_and_bitwise_scatter(P, T1):
    B = 5
    logp, labels, signs, slot_ids = _phrase_inputs(B, T1, P, seed=17 * T1 + P)
    st = stream_ptr()
    acc = torch.full((B, max(P, 1)), float("nan"), device=DEV)
    call("halva_phrase_sum_fwd", ptr(logp), ptr(labels), ptr(signs), ptr(slot_ids) if P else None, P, ptr(acc), B, T1, st)
    if P:
        acc = acc[:, :P]
        r = held("phrase_sum fwd", acc, L.phrase_sum_ref(logp, labels, signs, slot_ids), L.phrase_sum_bound(logp, labels, signs, slot_ids))
        # logp at masked positions is never read
        lpp = torch.where(labels == -100, _cycle(B * T1).view(B, T1), logp)
        acc_p = torch.full((B, P), float("nan"), device=DEV)
        call("halva_phrase_sum_fwd", ptr(lpp), ptr(labels), ptr(signs), ptr(slot_ids), P, ptr(acc_p), B, T1, st)
        assert same_bits(acc_p, acc)
        print("[phrase P=%d T1=%d] worst error / bound: acc %.3f" % (P, T1, r))
    else:
        assert bool(torch.isnan(acc).all()), "P = 0 must not write acc"
    dacc = torch.randn(B, max(P, 1), generator=_gen(5), device=DEV)[:, :P].contiguous()
    dl = torch.full((B, T1), float("nan"), device=DEV)
    call("halva_phrase_sum_bwd", ptr(dacc) if P else None, ptr(labels), ptr(signs), ptr(slot_ids) if P else None, P, ptr(dl), B, T1, st)
    assert same_bits(dl, L.phrase_sum_bwd_ref(dacc, labels, signs, slot_ids)), "phrase_sum bwd is a scatter: bit-exact"


# ---------------------------------------------------------------------------------------------------------------------------------
# sensitivity: the checks fail on one wrong row / element, and the summed check on a per-row bias the row checks pass
def test_mismatch_dropped_last_element_fails_the_row_check():
    R, V = 8, 32000
    z = logit_rows(R, V, seed=40, kinds=1)
    lse_rest = torch.logsumexp(z[:, :V - 1].double(), -1)
    z[:, V - 1] = (lse_rest - 12 * math.log(2)).float()           # p(V - 1) ~ 2^-12
    z = z.to(torch.bfloat16).contiguous()
    tgt = torch.zeros(R, dtype=torch.int32, device=DEV)
    logp, lse = _token_fwd(z, torch.bfloat16, V, tgt, R, V)
    held("token lse", lse, L.lse_ref(z), L.lse_bound(z))
    _, lse_drop = _token_fwd(z, torch.bfloat16, V, tgt, R, V - 1)    # the same rows without element V - 1
    bad = lse.clone()
    bad[5] = lse_drop[5]
    with pytest.raises(AssertionError, match=r"1 outside the bound, first \[\[5\]\]"):
        held("mismatch", bad, L.lse_ref(z), L.lse_bound(z))


def test_mismatch_target_off_by_one_in_one_of_32768_rows():
    R, V = 32768, 4096
    z = logit_rows(R, V, seed=41, kinds=2).to(torch.bfloat16)
    tgt = targets(R, V, seed=42)
    tgt[tgt == V - 1] = V - 2
    logp, _ = _token_fwd(z, torch.bfloat16, V, tgt, R, V)
    want, _ = L.logp_ref(z, tgt)
    held("token logp", logp, want, L.logp_bound(z, want))
    wrong = tgt.clone()
    wrong[12345] += 1
    logp_w, _ = _token_fwd(z, torch.bfloat16, V, wrong, R, V)
    with pytest.raises(AssertionError, match=r"1 outside the bound, first \[\[12345\]\]"):
        held("mismatch", logp_w, want, L.logp_bound(z, want))


def test_mismatch_per_row_bias_is_caught_by_the_summed_check_only():
    R, V = 32768, 4096
    pol, ref = kl_pair(R, V, seed=43, dtype=torch.bfloat16)
    kl = _kl_call(pol, ref, torch.bfloat16, V, None, pol.clone(), 1.0, R, V)
    want, bound = L.kl_ref(pol, ref), L.kl_bound(pol, ref)
    held("kl", kl, want, bound)
    biased = kl.double() + 2.0 ** -22 * L.lse_ref(ref).abs()
    r = held("mismatch (biased kl rows)", biased, want, bound)      # every row passes ...
    s = float((biased - want).sum())
    assert abs(s) > L.KL_SUM_TOL, s                                    # ... and the summed error does not
    print("[mismatch bias] worst row error / bound %.3f, summed error %.3e (tolerance %.1e)" % (r, s, L.KL_SUM_TOL))
    REPORT.pop("mismatch (biased kl rows)", None)


# ---------------------------------------------------------------------------------------------------------------------------------
# engine wrappers: dpa.lm_head_logp / lm_head_kl across two chunk boundaries
def test_engine_wrappers_across_chunks(monkeypatch):
    from halva_amd import dpa
    CH = dpa.LOGIT_CHUNK_ROWS
    R, Hd, V = 2 * CH + 37, 256, 32000
    g = _gen(50)
    h = (torch.randn(R, Hd, generator=g, device=DEV)).to(torch.bfloat16)
    hr = (h.float() + 0.05 * torch.randn(R, Hd, generator=g, device=DEV)).to(torch.bfloat16)
    Wt = (torch.randn(V, Hd, generator=g, device=DEV) / 6).to(torch.bfloat16)
    Wr = (Wt.float() + 0.002 * torch.randn(V, Hd, generator=g, device=DEV)).to(torch.bfloat16)
    tgt = targets(R, V, seed=51)
    gout = torch.randn(R, generator=g, device=DEV)
    monkeypatch.setattr(dpa, "LOGITS_F32", False)
    dh = {}
    for keep in (True, False):
        monkeypatch.setattr(dpa, "KEEP_LOGITS", keep)
        hh = h.clone().requires_grad_(True)
        lp = dpa.lm_head_logp(hh, Wt, tgt)
        lp.backward(gout)
        dh[keep] = hh.grad
        if keep:
            worst = 0.0
            for c0 in range(0, R, CH):                  # the reference on the logits of the same chunk boundaries
                c1 = min(R, c0 + CH)
                z = torch.mm(h[c0:c1], Wt.t())
                want, _ = L.logp_ref(z, tgt[c0:c1])
                worst = max(worst, held("lm_head_logp logp", lp[c0:c1].detach(), want, L.logp_bound(z, want)))
    assert torch.equal(dh[True], dh[False]), "dh with KEEP_LOGITS on and off must be bitwise equal"
    hp = h.clone().requires_grad_(True)
    kl = dpa.lm_head_kl(hp, hr, Wt, Wr)
    want = torch.zeros((), dtype=torch.float64, device=DEV)
    bsum = torch.zeros((), dtype=torch.float64, device=DEV)
    for c0 in range(0, R, CH):
        c1 = min(R, c0 + CH)
        zp, zr = torch.mm(h[c0:c1], Wt.t()), torch.mm(hr[c0:c1], Wr.t())
        want += L.kl_ref(zp, zr).sum()
        bsum += L.kl_bound(zp, zr).sum()
    r = held("lm_head_kl sum", kl.detach().reshape(1), want.reshape(1), bsum.reshape(1))
    kl.backward()
    assert bool(torch.isfinite(hp.grad).all())
    print("[engine] R = %d: worst error / bound logp %.3f, kl sum %.3f (|diff| %.2e)" % (R, worst, r, abs(float(kl) - float(want))))


def test_zz_report_worst_ratios():
    """(runs last in the file) the worst ratio error / bound of every quantity over the tests above"""
    print("worst error / bound per quantity: " + ", ".join("%s %.3g" % kv for kv in sorted(REPORT.items())))
    for k, v in REPORT.items():
        assert v <= 1.0, k
