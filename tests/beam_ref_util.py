"""Host-side helpers for the beam-search tests (halva_amd/beam.py, halva_amd/csrc/beam.hip, the beam entries of csrc/kvcache.hip and csrc/fork.hip), torch only.

  select_reference   halva_beam_select in float64: per prompt the C best of beam_scores[k] + log_softmax(logits[k])[i], descending, ties
                     by the lower flat index k * V + i; also the C + 1-th score (for the gap condition) and each row's lse.
  select_inputs      logits [B * K, V] fp32 and beam scores whose float64 top C + 1 per prompt are at least `gap` apart (re-seeded until so).
  select_bound       the score bound of tests/test_beam_kernels_gpu.py.
  advance_reference  halva_beam_advance on the host.
  histories          ancestry tables drawn as real beam histories: random parent lists inside each group, advanced step by step.
  materialise        own caches gathered through a table: what an index_select per step would have left in every member's own rows."""
import math

import torch


def select_reference(logits, beam_scores, K, C):
    """-> dict(score [B, C] f64, token [B, C], beam [B, C], next [B] f64: the C + 1-th score or -inf, lse [B * K] f64)."""
    x = logits.double().cpu()
    M, V = x.shape
    B = M // K
    lse = torch.logsumexp(x, 1)
    flat = (beam_scores.double().cpu()[:, None] + (x - lse[:, None])).view(B, K * V)
    n = min(C + 1, K * V)
    # a stable descending sort = ties by the lower flat index
    order = torch.sort(flat, dim=1, descending=True, stable=True).indices[:, :n]
    top = flat.gather(1, order)
    nxt = top[:, C] if n > C else torch.full((B,), -math.inf, dtype=torch.float64)
    return dict(score=top[:, :C], token=(order[:, :C] % V), beam=(order[:, :C] // V), next=nxt, lse=lse)


def min_gap(ref):
    s = torch.cat([ref["score"], ref["next"][:, None]], 1)
    d = s[:, :-1] - s[:, 1:]
    return float(d[torch.isfinite(d)].min()) if bool(torch.isfinite(d).any()) else math.inf


def beam_scores_for(B, K, kind, g):
    """kind 'first': [0, -1e9, ...] (the first step: every candidate must come from beam 0); 'mixed': running scores of a search in
    progress, one beam per prompt as far down as -300."""
    if kind == "first":
        s = torch.full((B, K), -1.0e9)
        s[:, 0] = 0.0
        return s.view(-1)
    s = -(torch.rand(B, K, generator=g) * 3 + torch.arange(K)[None, :] * 0.25)
    if K > 1:
        s[:, K - 1] = -300.0
    return s.view(-1).float()


def select_inputs(B, K, C, V, kind="mixed", gap=1e-3, seed=0, tries=200):
    """-> (logits [B * K, V] fp32, beam_scores [B * K] fp32, reference) with every float64 gap among each prompt's top C + 1 above `gap`."""
    for t in range(tries):
        g = torch.Generator().manual_seed(1000 * seed + t)
        logits = torch.randn(B * K, V, generator=g) * 10.0          # wide rows: the top of a prompt's list is sparse enough to space out
        scores = beam_scores_for(B, K, kind, g)
        ref = select_reference(logits, scores, K, C)
        if min_gap(ref) > gap:
            return logits, scores, ref
    raise AssertionError("no inputs with a top-(C + 1) gap above %g for B=%d K=%d C=%d V=%d" % (gap, B, K, C, V))


def ulp32(v):
    """The fp32 unit in the last place at magnitude |v| (float64 tensor -> float64 tensor)."""
    v = v.abs().clamp_min(2.0 ** -126)
    return torch.pow(2.0, torch.floor(torch.log2(v)) - 23)


def select_bound(ref_score, beam_score, xmax, lse):
    """8 ulp_fp32(max(|beam score|, |x|max, |lse|, |ref|)) + 2^-19: three roundings of at most half an ulp of the largest operand each, with
    slack, plus the error of an fp32 sum of V <= 2^15 non-negative terms in a tree order carried into lse."""
    big = torch.stack([beam_score.abs(), xmax.abs(), lse.abs(), ref_score.abs()]).amax(0)
    return 8 * ulp32(big) + 2.0 ** -19


def advance_reference(src, parent, own_len, dst):
    """halva_beam_advance on host tensors: src, dst int [M, Lown]; parent [M]; own_len [M] -> dst (a copy, updated)."""
    M, Lown = src.shape
    out = dst.clone()
    for m in range(M):
        p, t = int(parent[m]), int(own_len[m])
        if p < 0 or p >= M or t < 0 or t >= Lown:
            continue
        out[m, :t] = src[p, :t]
        out[m, t] = m
    return out


def histories(sizes, own_len, Lown, g):
    """Ancestry tables [M, Lown] for groups of the given sizes after own_len lockstep steps of random parents drawn inside each group (step 0:
    every member continues the group's first, as a beam search starts).  Slots at or beyond own_len hold -7 (never read)."""
    M = sum(sizes)
    first = [sum(sizes[:i]) for i in range(len(sizes))]
    table = torch.full((M, Lown), -7, dtype=torch.int32)
    for t in range(own_len):
        parent = torch.empty(M, dtype=torch.long)
        for f, n in zip(first, sizes):
            parent[f:f + n] = f if t == 0 else f + torch.randint(0, n, (n,), generator=g)
        table = advance_reference(table, parent, torch.full((M,), t), torch.full((M, Lown), -7, dtype=torch.int32))
    return table


def materialise(kc, table, own_len):
    """kc [M, H, Lown, D] -> a cache whose slot (m, t), t < own_len[m], holds kc[table[m][t], :, t]; other slots NaN."""
    M, H, Lown, D = kc.shape
    out = torch.full_like(kc, float("nan"))
    for m in range(M):
        n = int(own_len[m])
        if n:
            src = table[m, :n].long().to(kc.device)
            out[m, :, :n] = kc[src, :, torch.arange(n, device=kc.device)].transpose(0, 1)
    return out
