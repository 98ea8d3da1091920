"""Plain-torch float64 references and per-row / per-element error bounds for the loss kernels (halva_amd/csrc/loss.hip), for
row-wise checks.

The references work on the SAME bf16- or fp32-valued inputs the kernel reads (converted to float64 exactly) and compute, in float64:

  * lse[r] = logsumexp_v z[r, v];  logp[r] = z[r, t_r] - lse[r]                                  (halva_token_logp_fwd)
  * dlogits[r, v] = g[r] (1[v == t_r] - softmax(z)[r, v])                                           (halva_token_logp_bwd)
  * kl[r] = w[r] sum_v p_ref (log p_ref - log p_pol), with log-softmax algebra                     (halva_kl_rows)
  * dpol[r, v] = w[r] gscale (p_pol - p_ref)
  * acc[b, p] = sum_t logp[b, t] 1[labels != -100] 1[sign' == slot_ids[p]], sign' = 0 where sign == -100 (halva_phrase_sum_fwd)
    and its scatter back (halva_phrase_sum_bwd)

Error model (U = 2^-24, the fp32 unit roundoff).  The kernels work in the log2 domain: t = fl(z * kLog2e), a running max M and a
sum S = sum exp2f(t - M), merged per thread, then across a wave by shuffles, then across waves in LDS; lse = fl(fl(M + log2f(S)) * kLn2).

  * Magnitude terms, C_MAG = 4 ulps of (max|z| + ln V): the product z * kLog2e (1 rounding of |z| log2e), the constant kLog2e itself
    (2^-26 relative), the subtraction t - M (exact by Sterbenz near the max, at most 1 rounding of |t - M| elsewhere), and the final
    add and multiply by kLn2 (2 roundings of |lse| <= max|z| + ln V).  M cancels between the exponent and the final add, so the bound
    scales with the row's largest |z| and log V, never with a shift it shares: rows shifted by 1000 hold to 4 U 1010 ~ 2.4e-4.
  * Summation, LAMBDA sqrt(n) U relative with n = ceil(V / NT) + 8 terms along the longest path of a thread's sequential sum plus its
    6 wave-shuffle and 2 LDS merges (NT = 256 threads; the 512-thread KL form has shorter paths).  LAMBDA = 8 is the probabilistic
    rounding-error bound of Higham & Mary (SIAM J. Sci. Comput. 41(5), 2019): it holds with probability >= 1 - 2 exp(-LAMBDA^2 / 2)
    ~ 3e-14 per row.  All terms are positive, so a relative error of S is an absolute error of ln S of the same size.
  * Function terms, C_FN = 4 U: exp2f (v_exp_f32, 1 ulp, 2 U relative of every term and so of S) and log2f (v_log_f32, ~1 ulp).

    E_lse = U (C_MAG (max|z| + ln V) + LAMBDA sqrt(ceil(V / 256) + 8) + C_FN)                      (nat, per row)
    E_logp = E_lse + U |logp|                                                       (one more subtraction)

  * dlogits / dpol, per element, before the output rounding: p = exp2f(fl(z kLog2e) - fl(lse kLog2e)) has a relative error of
    rho = U C_MAG (|z| + |lse|) + E_lse + C_FN U  (the exponent's own roundings, the kernel's own lse, exp2f and the product with g);
    the target's 1 - p adds U |g|; a flush-to-zero floor of 2^-126 |g| covers terms below fp32's normal range.  With delta that
    pre-rounding error, the stored value holds |k - ref| <= (1 + F) delta + F |ref|, F = 2^-8 for a bf16 output (half a bf16 ulp
    <= 2^-8 of the value) and U for fp32.  dpol's delta is |w gscale| (p_pol rho_pol + p_ref rho_ref + U (p_pol + p_ref)): it scales
    with p_pol + p_ref, not their (cancelling) difference.
  * kl = A / S_ref + ((M_pol - M_ref) + log2 (S_pol / S_ref)) ln2, A = sum exp2f(t_ref - M_ref) (z_ref - z_pol): the weights carry
    lse's relative error, so E_kl = |w| ((1 + sum_v p_ref |z_ref - z_pol|) E_lse_ref + E_lse_pol + 2 U (|lse_ref| + |lse_pol|)).  The
    last term admits the combine A / S_ref - lse_ref + lse_pol, which rounds each |lse| once (the kernel's form until the summed
    check below exposed its bias): a per-row bound holds any correctly rounded fp32 combine, so it is set by |lse|, not by kl, and
    cannot see a bias of 2^-22 |lse| per row that sums to ~0.1 over 32 k rows.  KL_SUM_TOL = 1.6e-3 bounds |sum_r (kl_r - kl_r^fp64)|: at loss_alpha = 0.1 and B = 16 that is
    1e-5 of loss, 1 % of the 1e-3 target.
  * phrase_sum fwd: a per-thread fp32 sum of ceil(T1 / 256) terms and an 8-level block reduction: |err| <= (ceil(T1 / 256) + 8) U
    sum |terms| (Higham's gamma_n, first order).  The backward is a scatter: bit-exact.

Deviation from the reference trainer: it forms KL with softmax().log() in fp32, which is -inf (then nan) where a probability
underflows (logit spread > ~104 nat); the kernel (and kl_ref here) use log-softmax algebra and stay finite (include/halva_hip.h at
halva_kl_rows).  Nothing here calls a project kernel: the module imports without a GPU, and runs wherever its tensors live.
"""
import math

import torch

U = 2.0 ** -24
C_MAG = 4.0
LAMBDA = 8.0
C_FN = 4.0
F_BF16 = 2.0 ** -8
F_F32 = U
FTZ = 2.0 ** -126
KL_SUM_TOL = 1.6e-3
NT = 256


def _d(x):
    return x.double()


def lse_ref(z):
    """z [R, V] -> float64 [R]"""
    return torch.logsumexp(_d(z), -1)


def logp_ref(z, target):
    z = _d(z)
    lse = torch.logsumexp(z, -1)
    return z.gather(1, target.long()[:, None]).squeeze(1) - lse, lse


def dlogits_ref(z, target, g):
    """float64 [R, V]: g (onehot - softmax)"""
    z = _d(z)
    p = torch.softmax(z, -1)
    oh = torch.zeros_like(p)
    oh.scatter_(1, target.long()[:, None], 1.0)
    return _d(g)[:, None] * (oh - p)


def kl_ref(pol, ref, w=None):
    """float64 [R]: w sum p_ref (log p_ref - log p_pol) with log_softmax (finite where fp32 softmax underflows)"""
    r64, p64 = _d(ref), _d(pol)
    lr = torch.log_softmax(r64 - r64.amax(-1, keepdim=True), -1)     # (z - max z is exact: a per-row shift gives the same bits)
    lp = torch.log_softmax(p64 - p64.amax(-1, keepdim=True), -1)
    kl = (lr.exp() * (lr - lp)).sum(-1)
    return kl if w is None else _d(w) * kl


def dpol_ref(pol, ref, w=None, gscale=1.0):
    d = torch.softmax(_d(pol), -1) - torch.softmax(_d(ref), -1)
    s = gscale if w is None else _d(w)[:, None] * gscale
    return s * d


def phrase_sum_ref(logp, labels, signs, slot_ids):
    """float64 acc [B, P]"""
    sg = torch.where(signs == -100, torch.zeros_like(signs), signs)
    keep = labels != -100
    m = (sg[:, :, None] == slot_ids[None, None, :]) & keep[:, :, None]           # [B, T1, P]
    return (_d(logp)[:, :, None] * m.double()).sum(1)


def phrase_sum_bwd_ref(dacc, labels, signs, slot_ids):
    """fp32 dlogp [B, T1]: the scatter of dacc (exact)"""
    sg = torch.where(signs == -100, torch.zeros_like(signs), signs)
    out = torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)
    for p in range(slot_ids.numel()):
        m = (sg == slot_ids[p]) & (labels != -100)
        out = torch.where(m, dacc[:, p:p + 1].float().expand_as(out), out)
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# bounds
def n_terms(V, nt=NT):
    return math.ceil(V / nt) + 8


def lse_bound(z, lse64=None):
    """float64 [R]: E_lse of the module docstring"""
    V = z.shape[-1]
    zmax = _d(z).abs().amax(-1)
    return U * (C_MAG * (zmax + math.log(V)) + LAMBDA * math.sqrt(n_terms(V)) + C_FN)


def logp_bound(z, logp64):
    return lse_bound(z) + U * logp64.abs()


def _rho(z, lse64, e_lse):
    """relative error of one exp2f(z kLog2e - lse kLog2e) term, [R, V]"""
    return U * C_MAG * (_d(z).abs() + lse64.abs()[:, None]) + e_lse[:, None] + C_FN * U


def _stored(delta, ref, out_dtype):
    f = F_BF16 if out_dtype == torch.bfloat16 else F_F32
    return (1 + f) * delta + f * ref.abs()


def dlogits_bound(z, target, g, out_dtype):
    z64 = _d(z)
    lse64 = torch.logsumexp(z64, -1)
    p = torch.exp(z64 - lse64[:, None])
    ref = dlogits_ref(z, target, g)
    ga = _d(g).abs()[:, None]
    delta = ga * p * _rho(z, lse64, lse_bound(z)) + FTZ * ga
    delta.scatter_add_(1, target.long()[:, None], U * ga)
    return _stored(delta, ref, out_dtype), ref


def kl_bound(pol, ref, w=None):
    p64, r64 = _d(pol), _d(ref)
    lse_p, lse_r = torch.logsumexp(p64, -1), torch.logsumexp(r64, -1)
    pr = torch.exp(r64 - lse_r[:, None])
    mad = (pr * (r64 - p64).abs()).sum(-1)
    e = (1 + mad) * lse_bound(ref) + lse_bound(pol) + 2 * U * (lse_r.abs() + lse_p.abs())
    return e if w is None else _d(w).abs() * e


def dpol_bound(pol, ref, out_dtype, w=None, gscale=1.0):
    p64, r64 = _d(pol), _d(ref)
    lse_p, lse_r = torch.logsumexp(p64, -1), torch.logsumexp(r64, -1)
    pp, pr = torch.exp(p64 - lse_p[:, None]), torch.exp(r64 - lse_r[:, None])
    s = abs(gscale) * (torch.ones_like(lse_p) if w is None else _d(w).abs())[:, None]
    delta = s * (pp * _rho(pol, lse_p, lse_bound(pol)) + pr * _rho(ref, lse_r, lse_bound(ref)) + U * (pp + pr) + FTZ)
    want = dpol_ref(pol, ref, w, gscale)
    return _stored(delta, want, out_dtype), want


def phrase_sum_bound(logp, labels, signs, slot_ids):
    T1 = labels.shape[1]
    mag = phrase_sum_ref(_d(logp).abs(), labels, signs, slot_ids)
    return (math.ceil(T1 / 256) + 8) * U * mag


def ratio(err, bound):
    """largest err / bound (0 where both vanish)"""
    err, bound = _d(err), _d(bound)
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0
