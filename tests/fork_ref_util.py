"""Host-side helpers for the fork tests (halva_amd/csrc/kvcache.hip, halva_amd/decode.py:ForkCache), torch only, any device.

A member's keys are the first plen rows of its prefix row followed by its own rows, so every reference here is extend_ref_util's on the
concatenated keys: nothing new is modelled.  tests/test_fork_cpu.py checks the float64 decode reference against extend_ref_util.reference.

  decode_reference   float64 softmax(q [Kp; Ko]^T / sqrt(D)) [Vp; Vo] for one query row per head.
  extend_operands    (K, V, past) of extend_ref_util.reference / model / emulate for a member: the concatenation, past = plen + own past.
  guarded            a tensor inside a larger buffer with sentinel elements on both sides.
  DECODE_TOL         tests/test_decode_kernels_gpu.py:_assert_fp64's element tolerance, restated: |err| <= 2^-8 |ref| + 1e-4."""
import math

import torch

import extend_ref_util as E

GUARD, SENTINEL = 4096, 7.5
KC, BLOCK = 256, 16          # csrc/kvcache.hip: keys per split-KV chunk, members served from one prefix load


def decode_tol(ref):
    return ref.abs() * 2 ** -8 + 1e-4


def decode_reference(q, Kp, Vp, Ko, Vo):
    """q [H, D], Kp / Vp [H, plen, D], Ko / Vo [H, olen, D] (the rows that count, nothing beyond) -> float64 [H, D]."""
    K, V = torch.cat([Kp, Ko], 1).double(), torch.cat([Vp, Vo], 1).double()
    s = torch.einsum("hd,hld->hl", q.double(), K) / math.sqrt(q.shape[-1])
    return torch.einsum("hl,hld->hd", s.softmax(-1), V)


def extend_operands(Kp, Vp, plen, Ko, Vo, past, n_new):
    """-> (K, V, past') for extend_ref_util: keys [prefix rows below plen; own rows below past + n_new], past' = plen + past."""
    L = past + n_new
    return torch.cat([Kp[:, :plen], Ko[:, :L]], 1), torch.cat([Vp[:, :plen], Vo[:, :L]], 1), plen + past


def guarded(shape, dev, fill=None):
    """-> (buffer, view): a contiguous bf16 tensor of `shape` with GUARD sentinel elements before its first and after its last element."""
    numel = math.prod(shape)
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.bfloat16, device=dev)
    view = buf[GUARD:GUARD + numel].view(shape)
    if fill is not None:
        view.fill_(fill)
    return buf, view


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def groups(sizes, skip=()):
    """prefix_of for groups of the given sizes on consecutive prefix rows; rows listed in `skip` get no member."""
    out, p = [], 0
    for n in sizes:
        while p in skip:
            p += 1
        out += [p] * n
        p += 1
    return out


def emulate_fork(q, Kp, Vp, plen, Ko, Vo, past, n_new, **kw):
    """extend_ref_util.emulate with the prefix tiles in front.  The kernel tiles the prefix from prefix key 0 and the own rows from own key 0,
    emulate tiles the concatenation from key 0: the two walks are the same when plen is a multiple of the tile (asserted)."""
    assert plen % E.BN == 0
    K, V, p = extend_operands(Kp, Vp, plen, Ko, Vo, past, n_new)
    return E.emulate(q, K, V, p, n_new, **kw)
