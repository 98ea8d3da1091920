"""The semantics of halva_sample_top_k_top_p (include/halva_hip.h) in fp64 numpy, for the sampling tests.

With x_i = l_i / temperature:  K1 = { i : x_i > -inf, #{ j : x_j > x_i } < top_k }  (top_k = 0 or >= V: every x_i > -inf);  p = softmax of x
over K1;  S_i = sum_{j in K1, x_j > x_i} p_j;  K2 = { i in K1 : S_i < top_p }  (top_p = 1: K1).  Ties are kept together at both cuts, which
is what HF's TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper(min_tokens_to_keep=1) computes.  The scalars enter as the
fp32 values the C ABI receives."""
from collections import namedtuple

import numpy as np

DELTA = 1e-4        # band on cumulative mass (see tests/test_sample_kernel_gpu.py)

SampleRef = namedtuple("SampleRef", "x K1 K2 thr S cdf")
SampleRef.__doc__ = ("x: scaled logits fp64 [V]; K1, K2: bool [V]; thr: min of x over K2; S: fp64 [V], the K1-normalised mass strictly above "
                     "each entry (1 outside K1); cdf: fp64 [V], the inclusive CDF of q (p renormalised over K2) in ascending index")


def scaled(logits, temperature):
    return np.asarray(logits, dtype=np.float64) / np.float64(np.float32(temperature))


def mass_above(x, member):
    """For each i: the sum over { j in member : x_j > x_i } of exp(x_j - max), and the total over member (fp64, summed per distinct value
    from the top)."""
    m = x[member].max()
    vals, inv = np.unique(x, return_inverse=True)              # ascending
    w = np.where(member, np.exp(np.where(member, x - m, -np.inf)), 0.0)
    per_val = np.bincount(inv, weights=w, minlength=len(vals))
    incl_from_top = np.cumsum(per_val[::-1])[::-1]
    above = incl_from_top - per_val
    return above[inv], float(incl_from_top[0])


def cdf_over(x, member):
    """Inclusive CDF, in ascending index, of softmax(x) restricted to `member` (bool [V]); flat over non-members."""
    m = x[member].max()
    w = np.where(member, np.exp(np.where(member, x - m, -np.inf)), 0.0)
    c = np.cumsum(w)
    return c / c[-1]


def sample_ref(logits, temperature, top_k, top_p):
    x = scaled(logits, temperature)
    V = x.shape[0]
    finite = x > -np.inf
    assert not np.isnan(x).any() and finite.any()
    if top_k == 0 or top_k >= V:
        K1 = finite.copy()
    else:
        vals, inv, counts = np.unique(x, return_inverse=True, return_counts=True)
        greater = (V - np.cumsum(counts))[inv]                   # #{ j : x_j > x_i }
        K1 = finite & (greater < top_k)
    above, z1 = mass_above(x, K1)
    S = np.where(K1, above / z1, 1.0)
    p = np.float64(np.float32(top_p))
    K2 = K1.copy() if p >= 1.0 else (K1 & (S < p))
    assert K2.any()
    return SampleRef(x, K1, K2, float(x[K2].min()), S, cdf_over(x, K2))


def draw(cdf, member, u):
    """The first member k, in ascending index, with cdf[k] > u; the last member if none."""
    hit = np.flatnonzero(member & (cdf > u))
    return int(hit[0]) if len(hit) else int(np.flatnonzero(member)[-1])
