"""Host-side references for the attention of halva_extend_attn and halva_decode_attn (include/halva_hip.h), torch only, any device.

One sequence at a time: q bf16 [H, >= n_new, D] (the rotated queries of the new rows), K, V bf16 [H, >= past + n_new, D] (the cache after the
append); key j is visible to new row i iff j <= past + i.  Everything is computed on the bf16 values actually stored.

  reference   float64 softmax(q K^T / sqrt(D)) V.
  model       the rounding model of tests/test_sdpa_rowwise_gpu.py's `out`: fp32 scores in the log2 domain, the TRUE row maximum, P rounded to
              bf16 before P V, the output rounded to bf16.
  emulate     the arithmetic csrc/extend_attn.h documents, restated plainly: 64-key tiles from key 0, per row an exponent reference m_ref that
              moves iff the row's tile maximum exceeds it by more than 64 log2 units (old sum and old O scaled by exp2(m_ref - m_next) at a
              move), P = exp2(s - m_ref) rounded to bf16 for P V, the fp32 sum over the unrounded P.  Never compared with the kernel bit for
              bit: it exists so that test inputs can be shown admissible (and the bound shown to discriminate) without a GPU.
  row_bound   |out_kernel[r] - out_ref[r]| <= C |out_model[r] - out_ref[r]| + F |out_ref[r]| + G rms_r' |out_ref[r']| with the constants of
              tests/test_sdpa_rowwise_gpu.py (C_X["out"], F_X["out"], G_X["out"]), restated here once for every extend test.
  layout_classes   a pure-integer restatement of the kernel's tiling: which paths a (past, n_new, n, Lcap) layout takes.
  wide_inputs      inputs whose scores follow a profile r(j) in nats, up to ~350 nats wide."""
import math

import torch

C_OUT, F_OUT, G_OUT = 2.0, 2.0 ** -8, 2.0 ** -14      # tests/test_sdpa_rowwise_gpu.py: C_X["out"], F_X["out"], G_X["out"]
BM, WAVE_ROWS, BN = 128, 32, 64                       # csrc/extend_attn.h: query rows per workgroup and per wave, keys per tile
RESCALE_AT = 64.0                                     # log2 units (kRescaleAt, sdpa_common.h)
LOG2E = 1.4426950408889634
WIDE_PROFILES = ("up", "down", "spike_late", "spike_first", "flat")
WIDE_SEEDS = (0, 1, 2, 3)


def _visible(past, m, L, device):
    return torch.arange(L, device=device)[None, :] <= (past + torch.arange(m, device=device))[:, None]


def _operands(q, K, V, past, n_new):
    L = past + n_new
    return q[:, :n_new], K[:, :L], V[:, :L], _visible(past, n_new, L, q.device)


def reference(q, K, V, past, n_new):
    """float64 [H, n_new, D]."""
    q, K, V, vis = _operands(q, K, V, past, n_new)
    s = torch.einsum("hid,hjd->hij", q.double(), K.double()) / math.sqrt(q.shape[-1])
    return torch.einsum("hij,hjd->hid", s.masked_fill(~vis, -math.inf).softmax(-1), V.double())


def model(q, K, V, past, n_new, bf16=True):
    """The rounding model, bf16 [H, n_new, D] (bf16=False: no rounding of P or of the output - the structure alone, fp32)."""
    q, K, V, vis = _operands(q, K, V, past, n_new)
    s = (torch.einsum("hid,hjd->hij", q.float(), K.float()) * (LOG2E / math.sqrt(q.shape[-1]))).masked_fill(~vis, -math.inf)
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    pv = torch.einsum("hij,hjd->hid", p.to(torch.bfloat16).float() if bf16 else p, V.float()) / p.sum(-1, keepdim=True)
    return pv.to(torch.bfloat16) if bf16 else pv


def emulate(q, K, V, past, n_new, rescale=True, bf16=True):
    """The kernel's documented per-tile arithmetic, bf16 [H, n_new, D].  rescale=False leaves the old sum and the old O unscaled when m_ref
    moves (the defect the wide-score tests must notice).  Returns (out, moves): moves = how often an m_ref moved after the first tile."""
    q, K, V, vis = _operands(q, K, V, past, n_new)
    H, m, D = q.shape
    L = K.shape[1]
    sc = LOG2E / math.sqrt(D)
    m_ref = torch.full((H, m), -math.inf, dtype=torch.float32, device=q.device)
    l_run = torch.zeros(H, m, dtype=torch.float32, device=q.device)
    o = torch.zeros(H, m, D, dtype=torch.float32, device=q.device)
    moves = 0
    for kv0 in range(0, L, BN):
        kt, vt = K[:, kv0:kv0 + BN].float(), V[:, kv0:kv0 + BN].float()
        s = (torch.einsum("hid,hjd->hij", q.float(), kt) * sc).masked_fill(~vis[:, kv0:kv0 + BN], -math.inf)
        tmax = s.amax(-1)
        move = tmax > m_ref + RESCALE_AT                  # -inf (no visible key in the tile) never moves; the first tile always does
        m_next = torch.where(move, tmax, m_ref)
        if kv0 > 0:
            moves += int(move.sum())
        if rescale:
            alpha = torch.where(move, torch.exp2(m_ref - m_next), torch.ones_like(m_ref))
            l_run, o = l_run * alpha, o * alpha[..., None]
        m_ref = m_next
        p = torch.exp2(s - m_ref[..., None])
        l_run = l_run + p.sum(-1)
        o = o + torch.einsum("hij,hjd->hid", p.to(torch.bfloat16).float() if bf16 else p, vt)
    out = o / l_run[..., None]
    return (out.to(torch.bfloat16) if bf16 else out), moves


def row_errors(got, ref, mdl):
    """Flat per-(head, row) norms: |got - ref|, |model - ref|, |ref|."""
    return ((got.double() - ref).norm(dim=-1).flatten(), (mdl.double() - ref).norm(dim=-1).flatten(), ref.norm(dim=-1).flatten())


def row_bound(err_model, ref_norm):
    """The row-wise bound over one test's rows (the RMS row norm is taken over the rows given)."""
    return C_OUT * err_model + F_OUT * ref_norm + G_OUT * float(ref_norm.pow(2).mean().sqrt())


# ------------------------------------------------------------------------------------------------
def ext_rows(past, n_new, n, Lcap):
    """csrc/extend_attn.h:ext_rows - n_new cut to [0, n] and to the free slots of the cache."""
    return max(min(min(n_new, n), Lcap - past), 0)


def layout_classes(past, n_new, n, Lcap):
    """The paths rows_attn_kernel takes for one sequence, as a set of tuples:
      ("blocks", k)            k live query blocks (0: the sequence returns early)
      ("last_waves", w)        live waves of the last live block
      ("dead_wave", later)     a live block with a dead trailing wave; later = the block is not the first
      ("past_mod64", r, multi) multi = at least two live blocks
      ("n_new_mod32", r), ("len_mod64", r), ("ntiles", parity), ("len_eq_Lcap",), ("clipped",)
      ("tile", cls, later)     per (block, wave, tile): cls in "skipped" (kv0 > wq_max), "diag" (ext_tile<true>, every key slot below len),
                               "len" (ext_tile<true>, the tile holds slots at or beyond len), "unmasked" (ext_tile<false>)
    For a live wave wq_min < len, so a tile that reaches beyond len also reaches beyond the wave's first row: "len" tiles are diagonal
    tiles too, and the len comparison only matters for the rows at or beyond n_new of the last live wave."""
    nn = ext_rows(past, n_new, n, Lcap)
    out = {("blocks", (nn + BM - 1) // BM)}
    if nn < min(n_new, n):
        out.add(("clipped",))
    if nn == 0:
        return out
    ln = past + nn
    nblk = (nn + BM - 1) // BM
    out |= {("past_mod64", past % BN, nblk >= 2), ("n_new_mod32", nn % WAVE_ROWS), ("len_mod64", ln % BN)}
    if ln == Lcap:
        out.add(("len_eq_Lcap",))
    for qb in range(nblk):
        i0 = qb * BM
        kv_end = min(ln, past + i0 + BM)
        ntiles = (kv_end + BN - 1) // BN
        out.add(("ntiles", ntiles % 2))
        live = sum(1 for w in range(BM // WAVE_ROWS) if i0 + WAVE_ROWS * w < nn)
        if qb == nblk - 1:
            out.add(("last_waves", live))
        if live < BM // WAVE_ROWS:
            out.add(("dead_wave", qb >= 1))
        for w in range(live):
            wq_min = past + i0 + WAVE_ROWS * w
            wq_max = wq_min + WAVE_ROWS - 1
            for it in range(ntiles):
                kv0 = it * BN
                if kv0 > wq_max:
                    cls = "skipped"
                elif kv0 + BN > ln:
                    cls = "len"
                elif kv0 + BN - 1 > wq_min:
                    cls = "diag"
                else:
                    cls = "unmasked"
                out.add(("tile", cls, qb >= 1))
    return out


# ------------------------------------------------------------------------------------------------
def wide_profile(name, L):
    """r(j) in nats, float64 [L]."""
    j = torch.arange(L, dtype=torch.float64)
    if name == "up":              # 46 log2 units per 64-key tile: a tile without a move and P up to 2^46, then a move, repeatedly
        return 0.5 * j
    if name == "down":            # never moves; later P underflows
        return 0.5 * (L - 1 - j)
    r = torch.zeros(L, dtype=torch.float64)
    if name == "spike_late":
        r[L - 70] = 150.0
    elif name == "spike_first":
        r[3] = 150.0
    elif name != "flat":
        raise ValueError(name)
    return r


def wide_inputs(name, L, m, D=128, seed=0):
    """q [1, m, D], K, V [1, L, D] in bf16 (CPU) such that row i's score on key j is about r(j) nats:
    k_j = randn + r(j) u, q_i = 0.25 randn + u, u = randn D^(-1/4) (|u|^2 ~ sqrt(D) cancels the 1/sqrt(D) of the scale).  The 0.25 keeps the
    coefficient of r(j) near 1 on every row; with q = randn + u it ranges from 0.1 to 2 and some rows are decided by two keys, where the
    "same kind of errors as the model" argument behind C = 2 has nothing to concentrate over."""
    g = torch.Generator().manual_seed(1000 * seed + WIDE_PROFILES.index(name))
    u = torch.randn(D, generator=g, dtype=torch.float64) * D ** -0.25
    K = torch.randn(L, D, generator=g, dtype=torch.float64) + wide_profile(name, L)[:, None] * u
    q = 0.25 * torch.randn(m, D, generator=g, dtype=torch.float64) + u
    V = torch.randn(L, D, generator=g, dtype=torch.float64)
    return q.to(torch.bfloat16)[None], K.to(torch.bfloat16)[None], V.to(torch.bfloat16)[None]


# ------------------------------------------------------------------------------------------------
# The boundary sweep of tests/test_extend_attn_gpu.py (n = 257, Lcap = 448).  past = 0 .. 63 under a cycle of n_new whose length, 11, is
# coprime to 64; where that cycle gives a residue of past mod 64 a single query block, the residue comes again (past + 64) under a cycle of
# long blocks; then n_new mod 32 = 31, a cache filled to the brim, an empty block and a block clipped by the capacity.  The conditions the
# layout must meet are asserted in tests/test_extend_ref_util_cpu.py.
SWEEP_N, SWEEP_LCAP = 257, 448
_SWEEP_CYCLE = [257, 129, 128, 161, 193, 225, 1, 33, 97, 256, 160]
_SWEEP_LONG = [257, 129, 161, 193, 225, 256, 160]      # >= 2 query blocks each
_SWEEP_BASE = [(b, _SWEEP_CYCLE[b % len(_SWEEP_CYCLE)]) for b in range(64)]
_SWEEP_AGAIN = [(b + 64, _SWEEP_LONG[k % len(_SWEEP_LONG)]) for k, b in enumerate(b for b, m in _SWEEP_BASE if m <= BM)]
_SWEEP_EXTRA = [(33, 191), (64, 63), (SWEEP_LCAP - 257, 257), (17, 0), (SWEEP_LCAP - 5, 9)]
SWEEP_PAST = [p for p, _ in _SWEEP_BASE + _SWEEP_AGAIN + _SWEEP_EXTRA]
SWEEP_N_NEW = [m for _, m in _SWEEP_BASE + _SWEEP_AGAIN + _SWEEP_EXTRA]
SWEEP_FULL, SWEEP_EMPTY, SWEEP_CLIP = len(SWEEP_PAST) - 3, len(SWEEP_PAST) - 2, len(SWEEP_PAST) - 1
