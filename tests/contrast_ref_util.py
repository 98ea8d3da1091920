"""The semantics of halva_contrast_select (include/halva_hip.h) for the contrast tests: x in numpy float32 with the kernel's operation order
(each product and the difference rounded once, which is what numpy's float32 ufuncs do - they fuse nothing), then the fp64 restatement of
the sampling rule (tests/sample_ref_util.py) on that x.

Because x is reproduced bit for bit, the kernel is held to the reference exactly as halva_sample_top_k_top_p is: with the band DELTA on
cumulative mass and nothing else.  The row builders below also keep every decision that is taken on x or on the cut clear of the fp32
rounding of x (margins()), so that the exact rule - x in fp64 - decides the same way; tests/test_contrast_ref_cpu.py checks that."""
import numpy as np

from sample_ref_util import draw, sample_ref

NEG_INF = np.float32(-np.inf)


def log_beta32(beta):
    """log(beta) as the C entry receives it: the double logarithm rounded to float, -inf for beta = 0."""
    return np.float32(np.log(np.float64(beta))) if beta > 0 else NEG_INF


def contrast_x(l, lcd, alpha, beta):
    """-> (x float32 [V], plausible bool [V]): cut = max(l) + log(beta); x = -inf where l < cut, else (1 + alpha) * l - alpha * lcd as
    product, product, difference in float32, 1 + alpha formed once as a float32.  A masked column's lcd is never looked at."""
    l, lcd = np.asarray(l, dtype=np.float32), np.asarray(lcd, dtype=np.float32)
    a = np.float32(alpha)
    g1 = np.float32(np.float32(1.0) + a)
    cut = np.float32(l.max() + log_beta32(beta))
    plausible = ~(l < cut)
    with np.errstate(invalid="ignore", over="ignore"):
        x = (g1 * l).astype(np.float32) - (a * np.where(plausible, lcd, np.float32(0))).astype(np.float32)
    return np.where(plausible, x.astype(np.float32), NEG_INF).astype(np.float32), plausible


def servable(l, lcd, alpha, beta):
    """The -1 rule: False for a row where l holds a NaN or +inf or nothing above -inf, where lcd holds a NaN or +inf in a plausible
    column, or where x holds a NaN or +inf."""
    l, lcd = np.asarray(l, dtype=np.float32), np.asarray(lcd, dtype=np.float32)
    if np.isnan(l).any() or (l == np.inf).any() or not (l > -np.inf).any():
        return False
    x, plausible = contrast_x(l, lcd, alpha, beta)
    bad_cd = np.isnan(lcd) | (lcd == np.inf)
    return not ((bad_cd & plausible).any() or np.isnan(x).any() or (x == np.inf).any())


def contrast_ref(l, lcd, alpha, beta, temperature, top_k, top_p):
    """-> (SampleRef on x, x float32, plausible)"""
    x, plausible = contrast_x(l, lcd, alpha, beta)
    return sample_ref(x, temperature, top_k, top_p), x, plausible


def contrast_token(l, lcd, alpha, beta, temperature, top_k, top_p, u):
    ref, _, _ = contrast_ref(l, lcd, alpha, beta, temperature, top_k, top_p)
    return draw(ref.cdf, ref.K2, u)


def x_exact(l, lcd, alpha, beta):
    """The rule without fp32 rounding: x in fp64 from the fp32 inputs and the fp32 scalars, the cut in fp64."""
    l64, lcd64 = np.asarray(l, dtype=np.float32).astype(np.float64), np.asarray(lcd, dtype=np.float32).astype(np.float64)
    a = np.float64(np.float32(alpha))
    cut = l64.max() + (np.log(np.float64(beta)) if beta > 0 else -np.inf)
    plausible = ~(l64 < cut)
    return np.where(plausible, (1.0 + a) * l64 - a * np.where(plausible, lcd64, 0.0), -np.inf), plausible


def x_rounding(l, lcd, alpha):
    """A bound on |x float32 - x exact| per column: half an ulp on each product and on the difference, and half an ulp of 1 + alpha on the
    factor - at most 2^-24 (2 |g l| + |a lcd| + |x|), taken generously as 2^-22 (|g l| + |a lcd|)."""
    l64, lcd64 = np.abs(np.asarray(l, dtype=np.float64)), np.abs(np.asarray(lcd, dtype=np.float64))
    return 2.0 ** -22 * ((1.0 + float(alpha)) * l64 + float(alpha) * lcd64)


def margins(l, lcd, alpha, beta):
    """-> (cut margin, top margin): the smallest |l_i - cut| over columns off the cut, less the rounding of the fp32 cut; and the gap
    between the two largest distinct values of the exact x, less twice the largest rounding of x.  Both > 0: the exact rule masks the
    same columns and has the same maximum as the float32 one."""
    xe, plausible = x_exact(l, lcd, alpha, beta)
    l64 = np.asarray(l, dtype=np.float32).astype(np.float64)
    if beta > 0:
        cut = l64.max() + np.log(np.float64(beta))
        d = np.abs(l64 - cut)
        d = d[(d > 0) & np.isfinite(d)] if beta < 1 else d[d > 0]
        cut_margin = (d.min() if len(d) else np.inf) - 2.0 ** -22 * max(abs(cut), abs(l64.max()))
    else:
        cut_margin = np.inf
    vals = np.unique(xe[xe > -np.inf])
    top_margin = (vals[-1] - vals[-2] if len(vals) > 1 else np.inf) - 2 * float(x_rounding(l, lcd, alpha)[plausible].max())
    return float(cut_margin), float(top_margin)


def _bf16(a):
    import torch
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).bfloat16().float().numpy()


def pair_rows(V, seed, B=3):
    """B row pairs (l, lcd) fp32 [B, V]: l is 8 N(0,1) through bf16 (ties occur, as behind the real head), lcd = l + 2 N(0,1) through bf16 - a
    degraded view of the same scene - and the column that is largest in l is raised by 4 in l and lowered by 1 in lcd, so that the top of
    x is unique and clear of its rounding for every alpha >= 0."""
    rng = np.random.default_rng(seed)
    l = _bf16(8.0 * rng.standard_normal((B, V)))
    lcd = _bf16(l + 2.0 * rng.standard_normal((B, V)))
    top = l.argmax(1)
    l[np.arange(B), top] += 4.0
    lcd[np.arange(B), top] = l[np.arange(B), top] - 5.0
    # nothing else may overtake it in x: cap lcd from below on the other columns (x_i <= l_i + alpha (l_i - lcd_i) grows as lcd falls)
    lcd = np.maximum(lcd, l - 3.0).astype(np.float32)
    lcd[np.arange(B), top] = l[np.arange(B), top] - 5.0
    return l.astype(np.float32), lcd.astype(np.float32)
