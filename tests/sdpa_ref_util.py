"""Plain-torch references for the fused attention kernels (halva_amd/csrc/sdpa.hip and its sdpa_*.h), for row-wise checks.

Two restatements of one computation - causal varlen attention with the branch mask of halva_sdpa_branch_fwd (include/halva_hip.h),
the semantics of flash_attn_varlen_qkvpacked_func + unpad_input / pad_input (reference llama_flash_attn_monkey_patch.py:71-91):

  * reference(..., model=False): float64 throughout, on the same bf16-rounded inputs the kernel reads.  The "truth".
  * reference(..., model=True): the ROUNDING MODEL - the same computation in fp32, rounded to bf16 at the points the kernels
    document: P before P V and before dV = P^T dO, dS = P o (dP - delta) before dQ and dK, every output; delta is formed from the
    bf16 output as the forward stored it.  Its distance from the float64 result is the per-row noise scale of a correct bf16 kernel.

Only rows [start, start + len) of a sequence take part; every other row gets zero output and zero gradient by construction.  Rows of
a branched sequence [prefix | A | pad | B] at or past br_b do not see keys [br_a, br_b) (local indices; br_a = br_b >= len: no branch).
Nothing here calls a project kernel: the module imports without a GPU, and runs wherever its tensors live.
"""
import math

import torch

bf16 = torch.bfloat16


def _bf(x):
    return x.to(bf16).to(x.dtype)


def valid_rows(S, T, starts, lens):
    """[S, T] bool: rows inside [start, start + len)"""
    m = torch.zeros(S, T, dtype=torch.bool)
    for s in range(S):
        m[s, starts[s]:starts[s] + lens[s]] = True
    return m


def branch_pad_rows(S, T, br_a, br_b, a_len):
    """[S, T] bool: the in-sequence padding [br_a + len(A), br_b) of branched rows (contract: its output is unspecified)"""
    m = torch.zeros(S, T, dtype=torch.bool)
    if br_a is not None:
        for s in range(S):
            if br_a[s] < br_b[s]:
                m[s, br_a[s] + a_len[s]:br_b[s]] = True
    return m


def visible(L, br_a=None, br_b=None, causal=True, device="cpu"):
    """[L, L] bool, query x key, local indices"""
    i = torch.arange(L, device=device)
    ok = i[None, :] <= i[:, None] if causal else torch.ones(L, L, dtype=torch.bool, device=device)
    if br_a is not None:
        ok = ok & ~((i[:, None] >= br_b) & (i[None, :] >= br_a) & (i[None, :] < br_b))
    return ok


def reference(qkv, starts, lens, br_a=None, br_b=None, dout=None, scale=None, heads=None, model=False, causal=True, head_chunk=4,
              stored_out=None):
    """qkv [S, T, 3, H, D] bf16, dout [S, T, H, D] bf16 or None.  heads: the head indices to compute (None = all).
    stored_out [S, T, h, D] (model only): the output the forward stored, which the backward's delta = rowsum(dO o out) reads - so the
    model's delta carries the same rounding of out as the kernel's, and the comparison measures the backward alone (the stored output
    is held to the forward's own check).
    Returns a dict of out [S, T, h, D], lse [S, h, T] (natural log; 0 on padded rows) and, with dout, dq / dk / dv [S, T, h, D] - in
    float64 (model=False), or the rounding model's values (bf16-exact, held as float32).  Runs where qkv lives, head_chunk heads at a time."""
    S, T, _, H, D = qkv.shape
    dt = torch.float32 if model else torch.float64
    rnd = _bf if model else (lambda x: x)
    heads = list(range(H)) if heads is None else list(heads)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    dev = qkv.device
    h = len(heads)
    res = {"out": torch.zeros(S, T, h, D, dtype=dt, device=dev), "lse": torch.zeros(S, h, T, dtype=dt, device=dev)}
    if dout is not None:
        for n in ("dq", "dk", "dv"):
            res[n] = torch.zeros(S, T, h, D, dtype=dt, device=dev)
    hidx = torch.tensor(heads, device=dev)
    for s in range(S):
        st, L = starts[s], lens[s]
        if L == 0:
            continue
        ok = visible(L, None if br_a is None else br_a[s], None if br_b is None else br_b[s], causal, dev)
        for c0 in range(0, h, head_chunk):
            hc = hidx[c0:c0 + head_chunk]
            x = qkv[s, st:st + L].index_select(2, hc).to(dt)               # [L, 3, hc, D]
            q, k, v = (x[:, i].permute(1, 0, 2) for i in range(3))         # [hc, L, D]
            sc = torch.matmul(q, k.transpose(1, 2)) * scale
            sc = sc.masked_fill(~ok[None], float("-inf"))
            lse = torch.logsumexp(sc, -1)                                   # [hc, L]
            p = torch.exp(sc - lse[..., None])
            del sc
            pb = rnd(p)
            o = rnd(torch.matmul(pb, v))
            res["out"][s, st:st + L, c0:c0 + len(hc)] = o.permute(1, 0, 2)
            res["lse"][s, c0:c0 + len(hc), st:st + L] = lse
            if dout is None:
                continue
            do = dout[s, st:st + L].index_select(1, hc).to(dt).permute(1, 0, 2)     # [hc, L, D]
            dp = torch.matmul(do, v.transpose(1, 2))
            if stored_out is not None:
                o = stored_out[s, st:st + L, c0:c0 + len(hc)].to(dt).permute(1, 0, 2)
            delta = (do * o).sum(-1)
            ds = rnd(p * (dp - delta[..., None]))
            del dp, p
            res["dq"][s, st:st + L, c0:c0 + len(hc)] = rnd(torch.matmul(ds, k) * scale).permute(1, 0, 2)
            res["dk"][s, st:st + L, c0:c0 + len(hc)] = rnd(torch.matmul(ds.transpose(1, 2), q) * scale).permute(1, 0, 2)
            res["dv"][s, st:st + L, c0:c0 + len(hc)] = rnd(torch.matmul(pb.transpose(1, 2), do)).permute(1, 0, 2)
    return res


def branch_positions(T, br_a=None, br_b=None, S=1):
    """[S, T] int64 RoPE positions of halva_rope_qk_branch: row t at t, at br_a + (t - br_b) once t >= br_b (no branch points: t)"""
    t = torch.arange(T)[None].repeat(S, 1)
    if br_a is not None:
        for s in range(S):
            t[s, br_b[s]:] = br_a[s] + torch.arange(T - br_b[s])
    return t


def inverse_rope(g, cos, sin, pos):
    """The transpose of apply_rotary_pos_emb (modelling_llama.py:154-169) on g [S, T, h, D], in g's dtype, with the bf16 tables
    cos / sin [max_pos, D / 2] at positions pos [S, T]: g1 <- g1 c + g2 s, g2 <- g2 c - g1 s."""
    D = g.shape[-1]
    c = cos.to(g.device)[pos.to(g.device)].to(g.dtype)[:, :, None]         # [S, T, 1, D/2]
    s_ = sin.to(g.device)[pos.to(g.device)].to(g.dtype)[:, :, None]
    g1, g2 = g[..., :D // 2], g[..., D // 2:]
    return torch.cat([g1 * c + g2 * s_, g2 * c - g1 * s_], -1)


def row_norms(x):
    """per-row L2 norm over the last (head_dim) axis, in float64"""
    return x.double().norm(dim=-1)
