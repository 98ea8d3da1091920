"""GPU parity tests: every C-ABI kernel (through halva_amd.kernels -> libhalva_hip.so) against the oracle.

Floating-point tolerances are stated per test; the oracle is evaluated in fp32 on the SAME bf16-rounded inputs, so
the remaining error is the kernel's bf16 output rounding + accumulation order.  Integer/index results are exact.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from golden_util import load_npz, meta_of  # noqa: E402
from oracle import dpa, host, nets  # noqa: E402

DEV = "cuda"


def K():
    from halva_amd import kernels
    return kernels


def bf(t):
    return t.to(torch.bfloat16)


def rel_err(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-12))


def test_library_loads_and_probe_layouts():
    out = K().probe_layouts().numpy()
    tr = out[:256].reshape(64, 4)
    exp_tr = np.zeros((64, 4), dtype=np.int64)
    for l in range(64):
        for e in range(4):
            exp_tr[l, e] = 64 * (l >> 4) + 16 * e + (l & 15)
    assert (tr == exp_tr).all(), "ds_read_b64_tr_b16 map differs from the model:\n%s" % tr
    c = out[256:].reshape(64, 16)
    A = np.array([[((i * 7 + k * 3) % 5) - 2 for k in range(16)] for i in range(32)])
    B = np.array([[((k * 5 + j * 11) % 7) - 3 for j in range(32)] for k in range(16)])
    C = A @ B
    exp = np.zeros((64, 16), dtype=np.int64)
    for l in range(64):
        for r in range(16):
            exp[l, r] = C[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5), l & 31]
    assert (c == exp).all(), "MFMA 32x32x16 operand/accumulator map differs from the model"


@pytest.mark.parametrize("rows,d", [(7, 64), (1000, 4096), (33, 5120)])
def test_rmsnorm(rows, d):
    g = torch.Generator().manual_seed(0)
    x = bf(torch.randn(rows, d, generator=g) * 2)
    w = bf(1 + 0.1 * torch.randn(d, generator=g))
    dy = bf(torch.randn(rows, d, generator=g))
    xr = x.float().requires_grad_(True)
    # spec: y = bf16(w * x * rstd) - the fp32 value of the reference module (oracle fed fp32) rounded ONCE
    y_ref = nets.rmsnorm(x.float(), w.float(), 1e-5)
    xg = x.to(DEV).requires_grad_(True)
    y = K().rmsnorm(xg, w.to(DEV), 1e-5)
    assert float((y.cpu().float() - y_ref).abs().max()) <= 2 ** -8 * float(y_ref.abs().max())        # half a bf16 ulp of the largest value
    assert rel_err(y, y_ref) < 2e-3
    y.backward(dy.to(DEV))
    yf = nets.rmsnorm(xr, w.float(), 1e-5)
    yf.backward(dy.float())
    assert rel_err(xg.grad, xr.grad) < 6e-3          # bf16 output rounding of dx (2^-9 relative per element)


def test_rmsnorm_module_rounding_flag_reproduces_the_bf16_module_bit_for_bit():
    """HALVA_RMSNORM_MODULE_ROUNDING=1 (read once per process, hence the child process): y = w * bf16(x * rstd), the value
    LlamaRMSNorm.forward (modelling_llama.py:65-70) produces on a bf16 device, instead of the default single rounding."""
    import subprocess
    import sys
    code = r"""
import sys, torch
sys.path.insert(0, %r)
from halva_amd import kernels as K
g = torch.Generator().manual_seed(5)
x = (torch.randn(257, 4096, generator=g) * 3).to(torch.bfloat16)
w = (1 + 0.2 * torch.randn(4096, generator=g)).to(torch.bfloat16)
y = K.rmsnorm(x.cuda(), w.cuda(), 1e-5).cpu()
xf = x.float()
n = (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5)).to(torch.bfloat16)      # the module's cast back to the input dtype
spec = (w * n)                                                                            # bf16 x bf16 -> bf16
once = (w.float() * (xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + 1e-5))).to(torch.bfloat16)
print("RESULT", float((y != spec).float().mean()), float((y != once).float().mean()), float((y.float() - spec.float()).abs().max()))
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for flag in ("0", "1"):
        env = dict(os.environ, HALVA_RMSNORM_MODULE_ROUNDING=flag)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out[flag] = [float(v) for v in [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1].split()[1:]]
    # (rsqrt on the device and on the host may differ in the last bit of f32: a handful of elements sit on a bf16 rounding edge)
    assert out["1"][0] < 2e-4, out          # flag on: the module's two-rounding value, bit for bit
    assert out["0"][1] < 2e-4, out          # default: the single rounding
    assert out["0"][0] > 5e-3 and out["1"][1] > 5e-3, out      # ... and the two really differ on this input


@pytest.mark.parametrize("rows,d,width", [(37, 4096, 4480), (9, 5120, 5120)])
def test_rmsnorm_fork_sums_the_residual_gradient_in_the_kernel(rows, d, width):
    """(norm(x), x) as one autograd node: forward equals rmsnorm, backward is BIT-identical to autograd's accumulation of the norm's
    dx (a bf16 tensor) and the residual gradient - the decoder layer's use (DecoderLayer.forward)."""
    g = torch.Generator().manual_seed(3)
    x = bf(torch.randn(rows, d, generator=g) * 2).to(DEV)
    w = bf(1 + 0.1 * torch.randn(d, generator=g)).to(DEV)
    dy = bf(torch.randn(rows, width, generator=g)).to(DEV)
    dres = bf(torch.randn(rows, d, generator=g)).to(DEV)
    xa = x.clone().requires_grad_(True)
    y, xr = K().rmsnorm_fork(xa, w, 1e-5, width)
    (y * dy).sum().backward(retain_graph=True)
    only_norm = xa.grad.clone()
    xa.grad = None
    ((y * dy).sum() + (xr * dres).sum()).backward()
    xb = x.clone().requires_grad_(True)
    yb = K().rmsnorm(xb, w, 1e-5, width)
    assert torch.equal(y[:, :d], yb[:, :d]) and torch.equal(xr, x) and xr.data_ptr() != xa.data_ptr()      # a copy: the block accumulates onto it
    ((yb * dy).sum() + (xb * dres).sum()).backward()          # autograd: bf16(dx_norm) + dres, rounded to bf16
    assert torch.equal(xa.grad, xb.grad)
    xc = x.clone().requires_grad_(True)
    (K().rmsnorm(xc, w, 1e-5, width) * dy).sum().backward()
    assert torch.equal(only_norm, xc.grad)                     # no residual gradient: the plain kernel


def test_rope_forward_and_inverse():
    S, T, H, D = 2, 37, 3, 128
    g = torch.Generator().manual_seed(1)
    qkv = bf(torch.randn(S, T, 3, H, D, generator=g))
    cos, sin = K().rope_tables(D, 64, device=DEV)
    work = qkv.to(DEV).clone().view(S, T, 3 * H * D)
    from halva_amd.kernels import _rope_inplace
    _rope_inplace(work, cos, sin, T, H, D, False)
    got = work.view(S, T, 3, H, D).cpu()
    c32, s32 = nets.rope_tables(D, T, dtype=torch.bfloat16)
    pos = torch.arange(T)[None]
    for part in (0, 1):
        x = qkv[:, :, part].permute(0, 2, 1, 3).float()
        ref = nets.rope_apply(x, c32.float(), s32.float(), pos).permute(0, 2, 1, 3)
        assert rel_err(got[:, :, part], ref) < 4e-3
    assert torch.equal(got[:, :, 2], qkv[:, :, 2])          # v untouched
    _rope_inplace(work, cos, sin, T, H, D, True)             # inverse rotation restores q, k up to bf16 rounding
    assert rel_err(work.view(S, T, 3, H, D).cpu(), qkv) < 8e-3


@pytest.mark.parametrize("layout", ["plain_ragged", "left_padded", "packed", "packed_long"])
def test_dq2_fast_tile_equals_the_general_tile_bit_for_bit(layout, monkeypatch):
    """sdpa_bwd_dq2's fast tile (round 5: a tile's 40 operand reads issued ahead of its 16 products, a hidden strip's operand zeroed by a mask instead of its
    products branched over) against the general per-strip loop it replaced (HALVA_DQ2_FAST_TILE=0: sdpa_bwd_dq2_kernel<D, false, false>): the same products in
    the same order - the gradient of q, k and v must agree bit for bit, packed rows with wholly and partly hidden strips included."""
    from halva_amd import kernels as HK
    H, D = 2, 128
    if layout == "plain_ragged":
        S, T, lens, starts, br = 3, 700, [700, 411, 64], [0, 0, 0], None
    elif layout == "left_padded":
        S, T, lens, starts, br = 2, 600, [600, 531], [0, 69], None
    elif layout == "packed":
        S, T, lens, starts, br = 2, 1100, [1100, 1003], [0, 0], ([130, 100], [512, 420])
    else:
        S, T, lens, starts, br = 1, 3428, [3428], [0], ([668], [2048])
    g = torch.Generator().manual_seed(23)
    qkv = bf(torch.randn(S, T, 3 * H * D, generator=g)).to(DEV)
    dout = bf(torch.randn(S, T, H * D, generator=g)).to(DEV)
    mk = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    a_b = (None, None) if br is None else (mk(br[0]), mk(br[1]))

    def grads(fast):
        monkeypatch.setenv("HALVA_DQ2_FAST_TILE", "1" if fast else "0")
        qg = qkv.clone().requires_grad_(True)
        HK.sdpa_causal(qg, mk(starts), mk(lens), H, D, *a_b).backward(dout)
        torch.cuda.synchronize()
        return qg.grad.clone()

    a, b = grads(True), grads(False)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a.float() - b.float()).abs().max())


@pytest.mark.parametrize("layout", ["plain_ragged", "left_padded", "packed", "packed_long"])
def test_inverse_rope_in_the_backward_epilogues_equals_the_separate_launch(layout, monkeypatch):
    """halva_sdpa_branch_bwd_rope (round 5): the inverse rotation of dq / dk applied inside sdpa_bwd_dq2's and sdpa_bwd_dkv3's store epilogues must
    give the BITS of the separate halva_rope_qk launch it replaces (same roundings, same expression: common.h rope_pair) - positions of packed rows
    from the branch points, not from the table splice.pack_pairs writes (they agree on every row that carries a token), and
    halva_rope_qk_branch (the fall-back launch of kernel combinations without the rotating epilogue) agrees with both."""
    from halva_amd import kernels as HK
    from halva_amd.hip import call, ptr, stream_ptr
    H, D = 2, 128
    if layout == "plain_ragged":
        S, T, lens, starts, br = 3, 300, [300, 211, 64], [0, 0, 0], None
    elif layout == "left_padded":
        S, T, lens, starts, br = 2, 200, [200, 131], [0, 69], None
    elif layout == "packed":
        S, T, lens, starts, br = 2, 520, [520, 470], [0, 0], ([130, 100], [256, 192])
    else:
        S, T, lens, starts, br = 1, 1500, [1500], [0], ([628], [832])
    g = torch.Generator().manual_seed(17)
    qkv = bf(torch.randn(S, T, 3, H, D, generator=g))
    dout = bf(torch.randn(S, T, H, D, generator=g))
    for s_ in range(S):
        dout[s_, :starts[s_]] = 0
        dout[s_, starts[s_] + lens[s_]:] = 0
    cos, sin = K().rope_tables(D, 2048, device=DEV)
    mk = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    branch = None
    if br is not None:      # the position table pack_pairs would write: rows of B continue from the prefix (padding rows: 0)
        pos = torch.zeros(S, T, dtype=torch.int32)
        for s_ in range(S):
            a, b = br[0][s_], br[1][s_]
            pos[s_, :b] = torch.arange(b)
            pos[s_, b:] = a + torch.arange(T - b)
        branch = (mk(br[0]), mk(br[1]), pos.view(-1).to(DEV))

    def grads(fused):
        monkeypatch.setenv("HALVA_ROPE_FUSED_BWD", "1" if fused else "0")
        qg = qkv.to(DEV).view(S, T, 3 * H * D).clone().requires_grad_(True)
        out = HK.attention(qg * 1, cos, sin, mk(starts), mk(lens), H, D, None, branch)
        out.backward(dout.to(DEV).view(S, T, H * D))
        torch.cuda.synchronize()
        return qg.grad.clone()

    a, b = grads(True), grads(False)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b), float((a.float() - b.float()).abs().max())
    # the fall-back launch against the table-driven one on a random buffer (this test's table gives the padding rows below br_b their index as well)
    x = bf(torch.randn(S, T, 3 * H * D, generator=g)).to(DEV)
    y1, y2 = x.clone(), x.clone()
    call("halva_rope_qk", ptr(y1), ptr(cos), ptr(sin), ptr(branch[2]) if branch else None, S * T, T, H, D, cos.shape[0], 1, stream_ptr())
    call("halva_rope_qk_branch", ptr(y2), ptr(cos), ptr(sin), ptr(branch[0]) if branch else None, ptr(branch[1]) if branch else None, S * T, T, H, D,
         cos.shape[0], 1, stream_ptr())
    assert torch.equal(y1, y2)


def test_forward_rope_positions_come_from_the_branch_points_like_the_backwards():
    """kernels.attention() rotated q / k with the caller's position table in the forward and with the positions implied by the branch
    points in the backward - a table that disagreed gave silently wrong dq / dk.  One source of truth now (halva_rope_qk_branch in both
    directions): a scrambled table changes nothing, and the result is the table-driven rotation (halva_rope_qk) with the table
    halva_amd/splice.py:pack_pairs writes (reference llava/model/language_model/modelling_llama.py:154-169 at those positions)."""
    from halva_amd import kernels as HK
    from halva_amd.hip import call, ptr, stream_ptr
    S, T, H, D = 2, 520, 2, 128
    lens, br = [520, 470], ([130, 100], [256, 192])
    g = torch.Generator().manual_seed(23)
    qkv = bf(torch.randn(S, T, 3 * H * D, generator=g)).to(DEV)
    dout = bf(torch.randn(S, T, H * D, generator=g)).to(DEV)
    cos, sin = K().rope_tables(D, 2048, device=DEV)
    mk = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    pos = torch.zeros(S, T, dtype=torch.int32)
    for s_ in range(S):
        a, b = br[0][s_], br[1][s_]
        pos[s_, :b] = torch.arange(b)
        pos[s_, b:] = a + torch.arange(T - b)

    def run(table):
        qg = qkv.clone().requires_grad_(True)
        out = HK.attention(qg * 1, cos, sin, mk([0, 0]), mk(lens), H, D, None, (mk(br[0]), mk(br[1]), table))
        out.backward(dout)
        torch.cuda.synchronize()
        return out.detach().clone(), qg.grad.clone()
    good = run(pos.view(-1).to(DEV))
    scrambled = run(torch.randint(0, 2048, (S * T,), dtype=torch.int32, generator=g).to(DEV))
    assert torch.equal(good[0], scrambled[0]) and torch.equal(good[1], scrambled[1])
    # against the table-driven rotation + the attention kernel on its own
    rot = qkv.clone()
    call("halva_rope_qk", ptr(rot), ptr(cos), ptr(sin), ptr(pos.view(-1).to(DEV)), S * T, T, H, D, cos.shape[0], 0, stream_ptr())
    want = HK.sdpa_causal(rot, mk([0, 0]), mk(lens), H, D, mk(br[0]), mk(br[1]))
    valid = torch.zeros(S, T, dtype=torch.bool)
    for s_ in range(S):
        valid[s_, :lens[s_]] = True
    assert torch.equal(good[0][valid.to(DEV)], want[valid.to(DEV)])


def test_swiglu():
    rows, Fd = 50, 11008
    g = torch.Generator().manual_seed(2)
    gu = bf(torch.randn(rows, 2 * Fd, generator=g) * 1.5)
    dout = bf(torch.randn(rows, Fd, generator=g))
    gug = gu.to(DEV).requires_grad_(True)
    out = K().swiglu(gug)
    out.backward(dout.to(DEV))
    r = gu.float().requires_grad_(True)
    ref = F.silu(r[:, :Fd]) * r[:, Fd:]
    ref.backward(dout.float())
    assert rel_err(out, ref) < 6e-3
    assert rel_err(gug.grad, r.grad) < 6e-3


def _attn_ref(qkv, starts, lens, causal=True):
    """fp32 reference on bf16-rounded inputs: un-padded causal softmax attention, zeros on padded rows
    (oracle.nets.attention_varlen semantics; reference llama_flash_attn_monkey_patch.py:71-91)."""
    S, T, _, H, D = qkv.shape
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).float() for i in range(3))
    keep = torch.zeros(S, T, dtype=torch.bool)
    for s in range(S):
        keep[s, starts[s]:starts[s] + lens[s]] = True
    if causal:
        return nets.attention_varlen(q, k, v, keep).permute(0, 2, 1, 3)
    att = torch.softmax(q @ k.transpose(2, 3) / math.sqrt(D), -1)
    return (att @ v).permute(0, 2, 1, 3)


@pytest.mark.parametrize("slow_tr", ["0", "1"])
@pytest.mark.parametrize("T,lens,starts,H,D", [
    (20, [20, 13], [0, 0], 2, 128),            # tiny, right padded
    (200, [200, 77, 1], [0, 0, 0], 2, 128),    # ragged, len 1
    (333, [333, 300], [0, 33], 1, 128),        # left padded second row (tokenizer_padding_side == "left")
    (512, [512, 129], [0, 0], 2, 128),         # multiple q blocks, tile-aligned
    (96, [96, 50], [0, 0], 4, 64),             # head_dim 64 instantiation
])
def test_sdpa_causal_fwd_bwd(T, lens, starts, H, D, slow_tr):
    os.environ["HALVA_SDPA_SLOW_TR"] = slow_tr
    try:
        S = len(lens)
        g = torch.Generator().manual_seed(3)
        qkv = bf(torch.randn(S, T, 3, H, D, generator=g))
        dout = bf(torch.randn(S, T, H, D, generator=g))
        for s in range(S):                                   # gradient only flows from valid rows
            dout[s, :starts[s]] = 0
            dout[s, starts[s] + lens[s]:] = 0
        ident_cos = torch.ones(T, D // 2, dtype=torch.bfloat16, device=DEV)     # RoPE == identity: isolate attention
        ident_sin = torch.zeros(T, D // 2, dtype=torch.bfloat16, device=DEV)
        qg = qkv.to(DEV).view(S, T, 3 * H * D).clone().requires_grad_(True)
        ss = torch.tensor(starts, dtype=torch.int32, device=DEV)
        sl = torch.tensor(lens, dtype=torch.int32, device=DEV)
        out = K().attention(qg * 1, ident_cos, ident_sin, ss, sl, H, D)
        out.backward(dout.to(DEV).view(S, T, H * D))
        r = qkv.float().requires_grad_(True)
        ref = _attn_ref(r, starts, lens)
        ref.backward(dout.float())
        o = out.view(S, T, H, D).cpu().float()
        # padded rows are exactly zero (pad_input)
        for s in range(S):
            assert float(o[s, :starts[s]].abs().sum()) == 0 and float(o[s, starts[s] + lens[s]:].abs().sum()) == 0
        assert rel_err(o, ref) < 1e-2, "fwd"
        assert float((o - ref.detach()).abs().max()) < 3e-2
        dq = qg.grad.view(S, T, 3, H, D).cpu().float()
        names = "dq dk dv".split()
        for i in range(3):
            assert rel_err(dq[:, :, i], r.grad[:, :, i]) < 2e-2, names[i]
    finally:
        os.environ["HALVA_SDPA_SLOW_TR"] = "0"


@pytest.mark.gpu
@pytest.mark.parametrize("D", [128, 64])
def test_sdpa_exponent_reference_moves_when_later_keys_dominate(D):
    """The forward keeps ONE exponent reference per row (the maximum over its first 32 visible keys) and only moves it when the row's
    sums show that P = exp2(score - reference) overflowed or is about to (a partial row sum not below 2^100) - a path ordinary
    activations never take: the row block is then repeated with the reference of those rows raised by 120 log2 units, as often
    as it takes.  Keys whose scores grow by ~56 then ~136 nats from one 64-key tile to the next force one repeat for the rows of the
    third tile and two for the rows of the fourth; the result must still match the fp32 softmax (and the backward, which recomputes
    P from the saved log-sum-exp, must agree as well)."""
    T, H, S = 256, 2, 1
    g = torch.Generator().manual_seed(11)
    u = torch.randn(H, D, generator=g)
    u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(D)                       # |u|^2 = D: score(q=u, k=c*u) = c * sqrt(D)
    c = torch.tensor([0.1, 3.0, 8.0, 20.0]).repeat_interleave(64) * (11.3 / math.sqrt(D))      # ~1, 34, 90, 226 nats
    qkv = torch.zeros(S, T, 3, H, D)
    w = torch.randn(T, H, D, generator=g)                                     # per key: a direction orthogonal to u, as long as u
    w = w - (w * u[None]).sum(-1, keepdim=True) / D * u[None]                 # (keys that are all parallel would make dq a
    w = w / w.norm(dim=-1, keepdim=True) * math.sqrt(D)                       #  difference of large equal terms: ill-conditioned in bf16)
    qkv[0, :, 0] = u[None] + 0.05 * torch.randn(T, H, D, generator=g)
    qkv[0, :, 1] = c[:, None, None] * (u[None] + w)
    qkv[0, :, 2] = torch.randn(T, H, D, generator=g)
    qkv = bf(qkv)
    dout = bf(torch.randn(S, T, H, D, generator=g))
    ident_cos = torch.ones(T, D // 2, dtype=torch.bfloat16, device=DEV)
    ident_sin = torch.zeros(T, D // 2, dtype=torch.bfloat16, device=DEV)
    qg = qkv.to(DEV).view(S, T, 3 * H * D).clone().requires_grad_(True)
    ss = torch.zeros(S, dtype=torch.int32, device=DEV)
    sl = torch.full((S,), T, dtype=torch.int32, device=DEV)
    out = K().attention(qg * 1, ident_cos, ident_sin, ss, sl, H, D)
    out.backward(dout.to(DEV).view(S, T, H * D))
    r = qkv.float().requires_grad_(True)
    ref = _attn_ref(r, [0], [T])
    ref.backward(dout.float())
    o = out.view(S, T, H, D).cpu().float()
    assert torch.isfinite(o).all()
    scores = (r[0, :, 0].detach().permute(1, 0, 2) @ r[0, :, 1].detach().permute(1, 2, 0)) / math.sqrt(D)
    assert float(scores[:, 200, 128:201].max() - scores[:, 200, :32].max()) > 220 * math.log(2)     # row 200 needs two repeats (2 x 120 log2 units)
    assert float(scores[:, 150, 128:151].max() - scores[:, 150, :32].max()) > 100 * math.log(2)     # row 150 one
    assert rel_err(o, ref) < 1e-2, "fwd"
    assert float((o - ref.detach()).abs().max()) < 3e-2
    dq = qg.grad.view(S, T, 3, H, D).cpu().float()
    assert torch.isfinite(dq).all()
    for i, name in enumerate("dq dk dv".split()):
        assert rel_err(dq[:, :, i], r.grad[:, :, i]) < 2e-2, name


@pytest.mark.gpu
@pytest.mark.parametrize("scale_last", [200.0, 2000.0])
def test_sdpa_forward_far_beyond_the_repeat_budget_is_repaired(scale_last, monkeypatch):
    """Round-4 advice: sdpa_fwd3 repeated a row block at most 8 times (+120 log2 units each: 660 nats); now 64 times (5 300 nats).  A FINITE row whose
    maximum lies further out than that - here ~22 000 nats above its first 32 keys - comes back as NaN (loud), and with HALVA_FWD3_REPAIR=1 the launch
    is followed by the running-maximum kernel in repair mode (sdpa_common.h: SdpaParams::repair, sdpa_fwd.h), which redoes exactly the row blocks that hold a
    non-finite lse.  Rows ~2 200 nats out (the old failure) are handled by the kernel itself."""
    T, H, S, D = 256, 2, 1, 128
    g = torch.Generator().manual_seed(12)
    u = torch.randn(H, D, generator=g)
    u = u / u.norm(dim=-1, keepdim=True) * math.sqrt(D)
    c = torch.tensor([0.1, 3.0, 8.0, scale_last]).repeat_interleave(64)             # ~1, 34, 90, 11.3 x scale_last nats
    qkv = torch.zeros(S, T, 3, H, D)
    w = torch.randn(T, H, D, generator=g)
    w = w - (w * u[None]).sum(-1, keepdim=True) / D * u[None]
    w = w / w.norm(dim=-1, keepdim=True) * math.sqrt(D)
    qkv[0, :, 0] = u[None] + 0.05 * torch.randn(T, H, D, generator=g)
    qkv[0, :, 1] = c[:, None, None] * (u[None] + w)
    qkv[0, :, 2] = torch.randn(T, H, D, generator=g)
    qkv = bf(qkv)
    ss = torch.zeros(S, dtype=torch.int32, device=DEV)
    sl = torch.full((S,), T, dtype=torch.int32, device=DEV)
    ref = _attn_ref(qkv.float(), [0], [T])

    def run():
        with torch.no_grad():
            return K().sdpa_causal(qkv.to(DEV).view(S, T, 3 * H * D), ss, sl, H, D).view(S, T, H, D).cpu().float()

    monkeypatch.setenv("HALVA_FWD3_REPAIR", "1")
    o = run()
    assert torch.isfinite(o).all()
    assert rel_err(o, ref) < 1e-2 and float((o - ref).abs().max()) < 4e-2
    monkeypatch.setenv("HALVA_FWD3_REPAIR", "0")
    alone = run()
    if scale_last <= 200.0:      # ~2 260 nats: inside the kernel's own repeat budget
        assert torch.isfinite(alone).all() and rel_err(alone, ref) < 1e-2
    else:                        # ~22 600 nats: the rows of the last tile come back as NaN (l = inf), never as finite wrong numbers
        assert torch.isnan(alone[0, 192:]).any() and rel_err(alone[0, :192], ref[0, :192]) < 1e-2


def _branch_ref(qkv, starts, lens, br_a, br_b):
    """fp32 dense-mask reference of the branched attention: causal inside [start, start+len), rows >= br_b do not see rows in
    [br_a, br_b) (local indices); padded rows produce zeros."""
    S, T, _, H, D = qkv.shape
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3).float() for i in range(3))
    out = torch.zeros(S, H, T, D)
    for s in range(S):
        L, st = lens[s], starts[s]
        idx = torch.arange(L)
        ok = idx[None, :] <= idx[:, None]
        ok &= ~((idx[:, None] >= br_b[s]) & (idx[None, :] >= br_a[s]) & (idx[None, :] < br_b[s]))
        att = (q[s, :, st:st + L] @ k[s, :, st:st + L].transpose(1, 2)) / math.sqrt(D)
        att = att.masked_fill(~ok[None], float("-inf")).softmax(-1)
        out[s, :, st:st + L] = att @ v[s, :, st:st + L]
    return out.permute(0, 2, 1, 3)


@pytest.mark.parametrize("T,lens,starts,br_a,br_b,H,D", [
    (700, [700, 650, 300], [0, 0, 0], [100, 257, 512], [384, 448, 512], 2, 128),   # br_a unaligned; row 2 has no branch
    (1100, [1100, 1000], [0, 0], [628, 0], [832, 512], 1, 128),                     # 256-row blocks wholly in B; empty prefix
    (200, [200, 150], [0, 0], [64, 10], [128, 64], 2, 64),                          # tile-aligned br_a; D = 64
    (520, [520, 513], [0, 0], [130, 511], [512, 512], 1, 128),                      # short B; one-row A
    (2048, [2048], [0], [628], [1344], 1, 128),                                     # the bench geometry: prefix 628, A 716 rows
])
def test_sdpa_branch_fwd_bwd(T, lens, starts, br_a, br_b, H, D):
    """[prefix | A | B] packed rows: B must not attend to A (halva_sdpa_branch_fwd / _bwd), against a dense-mask fp32 reference."""
    S = len(lens)
    g = torch.Generator().manual_seed(5)
    qkv = bf(torch.randn(S, T, 3, H, D, generator=g))
    dout = bf(torch.randn(S, T, H, D, generator=g))
    for s in range(S):
        dout[s, :starts[s]] = 0
        dout[s, starts[s] + lens[s]:] = 0
    qg = qkv.to(DEV).view(S, T, 3 * H * D).clone().requires_grad_(True)
    mk = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    out = K().sdpa_causal(qg, mk(starts), mk(lens), H, D, mk(br_a), mk(br_b))
    out.backward(dout.to(DEV).view(S, T, H * D))
    r = qkv.float().requires_grad_(True)
    ref = _branch_ref(r, starts, lens, br_a, br_b)
    ref.backward(dout.float())
    o = out.view(S, T, H, D).cpu().float()
    for s in range(S):
        assert float(o[s, :starts[s]].abs().sum()) == 0 and float(o[s, starts[s] + lens[s]:].abs().sum()) == 0
    assert rel_err(o, ref) < 1e-2, "fwd"
    assert float((o - ref.detach()).abs().max()) < 3e-2
    dq = qg.grad.view(S, T, 3, H, D).cpu().float()
    for i, n in enumerate("dq dk dv".split()):
        assert rel_err(dq[:, :, i], r.grad[:, :, i]) < 2e-2, n
    # a branch-free call on the same data must differ (the mask is really applied) ...
    plain = K().sdpa_causal(qg.detach(), mk(starts), mk(lens), H, D).view(S, T, H, D).cpu().float()
    assert rel_err(plain, ref) > 5e-2
    # ... and rows before br_b equal plain causal attention (not bit for bit: a wave that also holds B rows may move its
    # exponent reference at another tile)
    for s in range(S):
        e = starts[s] + min(br_b[s], lens[s])
        if e > starts[s]:
            assert rel_err(o[s, starts[s]:e].detach(), plain[s, starts[s]:e]) < 3e-3


@pytest.mark.parametrize("seed", list(range(8)))
def test_sdpa_branch_random_layouts(seed):
    """Random packed layouts as halva_amd/splice.py:pack_pairs produces them (prefix, rest of the correct row, pad to 64, rest of
    the hallucinated row; empty parts included), two rows per launch, against the dense-mask reference."""
    rng = np.random.RandomState(100 + seed)
    H, D = 2, 128
    lens, br_a, br_b = [], [], []
    for _ in range(2):
        L = int(rng.choice([0, 1, 17, 64, 130, 333]))           # common prefix
        la = int(rng.choice([0, 1, 40, 64, 200]))               # rest of the correct row
        nb = int(rng.choice([0, 1, 33, 64, 257]))               # rest of the hallucinated row
        if L + la == 0:
            la = 5
        b = (L + la + 63) // 64 * 64
        lens.append(b + nb), br_a.append(L), br_b.append(b)
    T = max(lens) + int(rng.randint(0, 40))
    starts = [0, 0]
    g = torch.Generator().manual_seed(seed)
    qkv = bf(torch.randn(2, T, 3, H, D, generator=g))
    dout = bf(torch.randn(2, T, H, D, generator=g))
    for s in range(2):
        dout[s, lens[s]:] = 0
    qg = qkv.to(DEV).view(2, T, 3 * H * D).clone().requires_grad_(True)
    mk = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    out = K().sdpa_causal(qg, mk(starts), mk(lens), H, D, mk(br_a), mk(br_b))
    out.backward(dout.to(DEV).view(2, T, H * D))
    r = qkv.float().requires_grad_(True)
    ref = _branch_ref(r, starts, lens, br_a, br_b)
    ref.backward(dout.float())
    o = out.view(2, T, H, D).cpu().float()
    assert torch.isfinite(o).all() and torch.isfinite(qg.grad).all()
    assert rel_err(o, ref) < 1e-2, (lens, br_a, br_b)
    dq = qg.grad.view(2, T, 3, H, D).cpu().float()
    for i, n in enumerate("dq dk dv".split()):
        assert rel_err(dq[:, :, i], r.grad[:, :, i]) < 2e-2, (n, lens, br_a, br_b)


def test_sdpa_full_clip_shape():
    N, S, H, D = 2, 577, 16, 64
    g = torch.Generator().manual_seed(4)
    qkv = bf(torch.randn(N, S, 3, H, D, generator=g))
    out = K().sdpa_full(qkv.to(DEV).view(N, S, 3 * H * D), H, D).view(N, S, H, D).cpu()
    ref = _attn_ref(qkv, [0] * N, [S] * N, causal=False)
    assert rel_err(out, ref) < 1e-2


@pytest.mark.parametrize("M,N,Kd", [(100, 64, 32), (576, 4096, 1024), (300, 200, 72)])
def test_gemm_forms(M, N, Kd):
    g = torch.Generator().manual_seed(5)
    A = bf(torch.randn(M, Kd, generator=g))
    B = bf(torch.randn(N, Kd, generator=g))
    bias = bf(torch.randn(N, generator=g))
    k = K()
    ref = A.float() @ B.float().T + bias.float()
    out = k.gemm(A.to(DEV), B.to(DEV), bias.to(DEV))
    assert rel_err(out, ref) < 6e-3
    pre = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    out = k.gemm(A.to(DEV), B.to(DEV), bias.to(DEV), epilogue=1, pre_act=pre)
    assert rel_err(pre, ref) < 6e-3
    assert rel_err(out, F.gelu(ref.bfloat16().float())) < 8e-3
    if N % 8 == 0 and M % 8 == 0:
        Bt = B.T.contiguous()                                   # [K, N]
        out = k.gemm(A.to(DEV), Bt.to(DEV), trans_b=True)
        assert rel_err(out, A.float() @ B.float().T) < 6e-3
        At = A.T.contiguous()                                   # [K, M]
        out = k.gemm(At.to(DEV), Bt.to(DEV), trans_a=True, trans_b=True, out_dtype=torch.float32)
        assert rel_err(out, A.float() @ B.float().T) < 1e-3
        acc = torch.ones(M, N, dtype=torch.float32, device=DEV)
        k.gemm(At.to(DEV), Bt.to(DEV), trans_a=True, trans_b=True, out=acc, accumulate=True)
        assert rel_err(acc, A.float() @ B.float().T + 1) < 1e-3


def test_projector_fwd_bwd():
    M, dv, d = 576 * 2, 1024, 512
    g = torch.Generator().manual_seed(6)
    x = bf(torch.randn(2, 576, dv, generator=g))
    W = {"model.mm_projector.0.weight": bf(torch.randn(d, dv, generator=g) * 0.03),
         "model.mm_projector.0.bias": bf(torch.randn(d, generator=g) * 0.1),
         "model.mm_projector.2.weight": bf(torch.randn(d, d, generator=g) * 0.05),
         "model.mm_projector.2.bias": bf(torch.randn(d, generator=g) * 0.1)}
    dy = bf(torch.randn(2, 576, d, generator=g))
    dev = {k: v.to(DEV).requires_grad_(True) for k, v in W.items()}
    y = K().projector_mlp(x.to(DEV), dev["model.mm_projector.0.weight"], dev["model.mm_projector.0.bias"],
                          dev["model.mm_projector.2.weight"], dev["model.mm_projector.2.bias"])
    y.backward(dy.to(DEV))
    Wf = {k: v.float().requires_grad_(True) for k, v in W.items()}
    ref = nets.projector(x.float(), Wf)
    ref.backward(dy.float())
    assert rel_err(y, ref) < 8e-3
    for k_ in W:
        assert rel_err(dev[k_].grad, Wf[k_].grad) < 1.5e-2, k_


def _projector_against_float_torch(proj, reference, x, sink, tol_y, tol_g):
    """Output and every parameter gradient of `proj` on x against `reference(x, {name: float parameter})`, the same bf16 values run in
    float torch; sink=True: the fp32 sums land in `.main_grad` and autograd returns None."""
    g = torch.Generator().manual_seed(61)
    W = {n: bf(torch.randn(p.shape, generator=g) * 0.1 + (1.0 if "layers.1.weight" in n else 0.0)) for n, p in proj.named_parameters()}
    proj.load_state_dict(W)
    for p in proj.parameters():
        p.requires_grad_(True)
        if sink:
            p.main_grad, p.grad_sink = torch.zeros(p.shape, dtype=torch.float32, device=DEV), True
    y = proj(x.to(DEV))
    dy = bf(torch.randn(y.shape, generator=g))
    y.backward(dy.to(DEV))
    Wf = {n: v.float().requires_grad_(True) for n, v in W.items()}
    ref = reference(x.float(), Wf)
    ref.backward(dy.float())
    print("output rel_err %.3e" % rel_err(y, ref))
    assert y.shape == ref.shape and rel_err(y, ref) < tol_y
    for n, p in proj.named_parameters():
        assert (p.grad is None) == sink, n
        got = p.main_grad if sink else p.grad
        print("%s rel_err %.3e" % (n, rel_err(got, Wf[n].grad)))
        assert rel_err(got, Wf[n].grad) < tol_g, n


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "main_grad"])
@pytest.mark.parametrize("kind", ["linear", "mlp3x_gelu"])
def test_projector_types_beside_the_shipped_one(kind, sink):
    """`linear` and `mlp3x_gelu` through build_vision_projector, [2, 9, 64] -> 128: 18 rows, no multiple of 8 (as 196 rows per image
    is none; halva_gemm_bf16 asks a multiple of 8 of the contiguous dimensions only, which 64 and 128 are).  Bounds of
    test_projector_fwd_bwd."""
    from types import SimpleNamespace
    from halva_amd.clip import build_vision_projector
    proj = build_vision_projector(SimpleNamespace(mm_projector_type=kind, mm_hidden_size=64, hidden_size=128), device=DEV)
    x = bf(torch.randn(2, 9, 64, generator=torch.Generator().manual_seed(60)))

    def reference(h, W):
        if kind == "linear":
            return F.linear(h, W["weight"], W["bias"])
        for i in (0, 2, 4):
            h = F.linear(h, W["%d.weight" % i], W["%d.bias" % i])
            h = F.gelu(h) if i < 4 else h
        return h
    _projector_against_float_torch(proj, reference, x, sink, 8e-3, 1.5e-2)


@pytest.mark.parametrize("sink", [False, True], ids=["autograd", "main_grad"])
def test_mlp_downsample_on_an_odd_grid(sink):
    """[2, 9, 32]: g = 3, zero padded to a 2 x 2 grid of 4c = 128 channels (out[n, b*G + a, (f*2 + e)*c + ch] = x[n, (2a + f)*g + 2b + e, ch],
    halva_amd/csrc/vision.hip) -> LayerNorm -> Linear -> GELU -> Linear.  Tolerances of tests/test_vila_gpu.py for the same Function."""
    from types import SimpleNamespace
    from halva_amd.vila_model import MultimodalProjector
    proj = MultimodalProjector("mlp_downsample", SimpleNamespace(mm_hidden_size=32, hidden_size=128), device=DEV)
    x = bf(torch.randn(2, 9, 32, generator=torch.Generator().manual_seed(62)))

    def reference(h, W):
        n, c = h.shape[0], h.shape[2]
        hp = h.new_zeros(n, 4, 4, c)
        hp[:, :3, :3] = h.view(n, 3, 3, c)
        h = hp.view(n, 2, 2, 2, 2, c).permute(0, 3, 1, 2, 4, 5).reshape(n, 4, 4 * c)            # [n, a, f, b, e, c] -> [n, b, a, f, e, c]
        h = F.layer_norm(h, (4 * c,), W["layers.1.weight"], W["layers.1.bias"], proj.layers[1].eps)
        h = F.gelu(F.linear(h, W["layers.2.weight"], W["layers.2.bias"]))
        return F.linear(h, W["layers.4.weight"], W["layers.4.bias"])
    _projector_against_float_torch(proj, reference, x, sink, 2e-2, 3e-2)


def test_clip_patch_embed():
    n, hw, p, d = 3, 336, 14, 256
    g = torch.Generator().manual_seed(7)
    img = bf(torch.randn(n, 3, hw, hw, generator=g))
    w = bf(torch.randn(d, 3, p, p, generator=g) * 0.05)
    Kp = (3 * p * p + 7) // 8 * 8
    wkp = torch.zeros(d, Kp, dtype=torch.bfloat16)
    wkp[:, :3 * p * p] = w.reshape(d, -1)
    out = K().clip_patch_embed(img.to(DEV), wkp.to(DEV), p, d)
    ref = F.conv2d(img.float(), w.float(), stride=p).flatten(2).transpose(1, 2)
    assert rel_err(out, ref) < 6e-3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_token_logp_and_golden(dtype):
    z = load_npz("loss_small.npz")
    logits = torch.from_numpy(z["logits"])
    labels = torch.from_numpy(z["labels"])
    S, T, V = logits.shape
    tgt = labels[:, 1:].clone()
    tgt[tgt == -100] = 0
    lg = logits[:, :-1].reshape(-1, V).to(dtype).contiguous()
    got = K().token_logp(lg.to(DEV), tgt.reshape(-1).int().to(DEV)).view(S, T - 1).cpu()
    tol = 1e-5 if dtype == torch.float32 else 5e-2
    np.testing.assert_allclose(got.numpy(), z["logps"], atol=tol)
    # big row + backward against the oracle on identical (rounded) inputs
    g = torch.Generator().manual_seed(8)
    R, V = 37, 32000
    big = (torch.randn(R, V, generator=g) * 4).to(dtype)
    t = torch.randint(0, V, (R,), generator=g)
    gout = torch.randn(R, generator=g)
    gout[5] = 0.0
    bg = big.to(DEV).requires_grad_(True)
    lp = K().token_logp(bg, t.int().to(DEV))
    lp.backward(gout.to(DEV))
    br = big.float().requires_grad_(True)
    ref = torch.gather(br.log_softmax(-1), 1, t[:, None]).squeeze(1)
    ref.backward(gout)
    np.testing.assert_allclose(lp.detach().cpu().numpy(), ref.detach().numpy(), atol=2e-5)
    assert rel_err(bg.grad, br.grad) < (1e-5 if dtype == torch.float32 else 4e-3)
    assert float(bg.grad[5].abs().sum()) == 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kl_rows(dtype):
    g = torch.Generator().manual_seed(9)
    R, V = 29, 32000
    pol = (torch.randn(R, V, generator=g) * 3).to(dtype)
    ref = (pol.float() + 0.3 * torch.randn(R, V, generator=g)).to(dtype)
    w = torch.ones(R)
    w[3] = 0
    w[17] = 0
    pg = pol.to(DEV).requires_grad_(True)
    kl = K().kl_rows(pg, ref.to(DEV), w.to(DEV))
    kl.sum().backward()
    pr = pol.float().requires_grad_(True)
    labels = torch.where(w > 0, torch.ones(R, dtype=torch.long), torch.full((R,), -100))
    kl_ref = dpa.kl_to_reference(pr[None], ref.float()[None], labels[None])       # sum / 1
    kl_ref.backward()
    assert abs(float(kl.sum()) - float(kl_ref)) < 2e-4 * max(1.0, abs(float(kl_ref)))
    assert rel_err(pg.grad, pr.grad) < (1e-5 if dtype == torch.float32 else 6e-3)
    same = K().kl_rows(pol.to(DEV), pol.to(DEV).clone(), None)
    assert float(same.abs().max()) < 1e-5                    # identical models -> exactly ~0


def test_kl_rows_register_resident_rows_match_the_two_read_form(monkeypatch):
    """halva_kl_rows keeps both bf16 rows in registers between its statistics pass and its gradient pass (one HBM read per logit);
    HALVA_KL_KEEP=0 is the form that reads them twice.  Same values up to the summation order of 512 instead of 256 partial sums per row."""
    g = torch.Generator().manual_seed(10)
    R, V = 37, 32000
    pol = (torch.randn(R, V, generator=g) * 3).to(torch.bfloat16)
    ref = (pol.float() + 0.3 * torch.randn(R, V, generator=g)).to(torch.bfloat16)
    w = torch.ones(R)
    w[5] = 0
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HALVA_KL_KEEP", mode)
        pg = pol.to(DEV).requires_grad_(True)
        kl = K().kl_rows(pg, ref.to(DEV), w.to(DEV))
        kl.sum().backward()
        torch.cuda.synchronize()
        out[mode] = (kl.detach().cpu(), pg.grad.cpu().float())
    assert float((out["1"][0] - out["0"][0]).abs().max()) < 1e-5 * max(1.0, float(out["0"][0].abs().max()))
    assert float(out["1"][0][5]) == 0.0 and float(out["1"][1][5].abs().sum()) == 0.0
    d = (out["1"][1] - out["0"][1]).abs()
    assert float(d.max()) <= 2.0 ** -7 * float(out["0"][1].abs().max())          # at most one bf16 rounding apart, and almost nowhere
    assert float((d > 0).float().mean()) < 1e-3


def test_phrase_sum_golden_and_grad():
    z = load_npz("loss_small.npz")
    logps = torch.from_numpy(z["logps"])
    signs = torch.from_numpy(z["signs"])
    labels = torch.zeros_like(signs)                          # all valid: the golden was made without the mask multiply
    slots = torch.unique(signs)[1:]
    lp = logps.to(DEV).requires_grad_(True)
    acc = K().phrase_sum(lp, labels.to(DEV), signs.to(DEV), slots.to(DEV))
    np.testing.assert_allclose(acc.detach().cpu().numpy(), z["acc"], atol=1e-5)
    gacc = torch.randn(acc.shape)
    acc.backward(gacc.to(DEV))
    lr = logps.clone().requires_grad_(True)
    dpa.accumulate_logps(lr, signs).backward(gacc)
    np.testing.assert_allclose(lp.grad.cpu().numpy(), lr.grad.numpy(), atol=1e-6)
    # mask multiply + IGNORE_INDEX signs (halva_trainer.py:556-560)
    labels2 = labels.clone()
    labels2[0, 4] = -100
    signs2 = signs.clone()
    signs2[1, 0] = -100
    acc2 = K().phrase_sum(logps.to(DEV), labels2.to(DEV), signs2.to(DEV), slots.to(DEV)).cpu()
    ref2 = dpa.accumulate_logps(logps * (labels2 != -100).float(), signs2.masked_fill(signs2 == -100, 0))
    np.testing.assert_allclose(acc2.numpy(), ref2.numpy(), atol=1e-5)


def test_splice_rows_against_golden():
    from halva_amd import splice as sp
    z = load_npz("splice.npz")
    for ci, m in enumerate(meta_of(z)):
        p = "s%d_" % ci
        plan = sp.plan_splice(torch.from_numpy(z[p + "ids"]), torch.from_numpy(z[p + "mask"]), torch.from_numpy(z[p + "labels"]),
                              torch.from_numpy(z[p + "signs"]), n_patch=z[p + "features"].shape[1], max_len=m["max_len"],
                              padding_side=m["padding_side"])
        np.testing.assert_array_equal(plan.labels.numpy(), z[p + "out_labels"])
        np.testing.assert_array_equal(plan.signs.numpy(), z[p + "out_signs"])
        np.testing.assert_array_equal(plan.mask.numpy(), z[p + "out_mask"])
        emb = bf(torch.from_numpy(z[p + "embed_tokens"]))
        feats = bf(torch.from_numpy(z[p + "features"]))
        out = K().splice_rows(emb.to(DEV), feats.to(DEV), plan.src.to(DEV), plan.S, plan.T).cpu()
        ref, _, _, _ = host.splice(z[p + "ids"], z[p + "mask"], z[p + "labels"], z[p + "signs"], feats.float().numpy(),
                                   emb.float().numpy(), m["max_len"], m["padding_side"])
        assert torch.equal(out.float(), torch.from_numpy(ref))          # pure row copies: bit exact


@pytest.mark.parametrize("rows,M,N,lda,ldb", [(1000, 128, 256, 640, 384), (3428, 512, 128, 1536, 4224), (77, 8, 8, 8, 8),
                                                (27424, 384, 4096, 4480, 4480), (3000, 256, 4096, 4352, 4352), (1500, 320, 1032, 512, 1104),      # short M: one workgroup takes all of M
                                                (2000, 128, 13824, 13952, 13952), (2000, 5120, 128, 15360, 5248)])      # 13B factor shapes
def test_wgrad_accumulate_matches_fp32_reference(rows, M, N, lda, ldb):
    """C += alpha * A^T B over column windows of wider buffers (the LoRA weight gradients), accumulated into an f32 sink; two runs agree bitwise."""
    g = torch.Generator().manual_seed(5)
    abuf = bf(torch.randn(rows, lda, generator=g)).to(DEV)
    bbuf = bf(torch.randn(rows, ldb, generator=g)).to(DEV)
    a0, b0 = (lda - M) // 16 * 8, (ldb - N) // 16 * 8                 # 16-byte aligned windows inside the buffers
    A, B = abuf[:, a0:a0 + M], bbuf[:, b0:b0 + N]
    C0 = torch.randn(M, N, generator=g).to(DEV)
    ref = C0.double() + 0.5 * (A.double().t() @ B.double())
    out = []
    for _ in range(2):
        C = C0.clone()
        K().wgrad_accumulate(C, A, B, 0.5)
        out.append(C)
    assert torch.equal(out[0], out[1])
    assert float((out[0].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())) * max(1, rows // 2000)


@pytest.mark.parametrize("rows,M,N,lda,ldb", [(27424, 384, 4096, 4480, 4480), (3001, 128, 11008, 11136, 11136), (2000, 4096, 128, 12288, 4480)])
def test_wgrad_lds_dma_kernel_gives_the_register_staged_kernels_bits(rows, M, N, lda, ldb, monkeypatch):
    """halva_wgrad_accumulate's operand tiles arrive by LDS-DMA (wgrad_dma_kernel, M and N multiples of 128); HALVA_WGRAD_DMA=0 is the
    register-staged gemm_kernel<true, true> of rounds 2-3.  Same slabs, same MFMA order inside a slab: the same bits - including a k-slab
    that ends inside a 64-row tile (rows past it arrive as zeros through the bounds-checked descriptor)."""
    g = torch.Generator().manual_seed(6)
    abuf = bf(torch.randn(rows, lda, generator=g)).to(DEV)
    bbuf = bf(torch.randn(rows, ldb, generator=g)).to(DEV)
    A, B = abuf[:, lda - M:], bbuf[:, :N]
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("HALVA_WGRAD_DMA", mode)
        C = torch.zeros(M, N, device=DEV)
        K().wgrad_accumulate(C, A, B, 1.0)
        torch.cuda.synchronize()
        out[mode] = C
    assert torch.equal(out["1"], out["0"])


@pytest.mark.parametrize("group", ["qkv_7b", "gate_up_7b", "o_7b", "down_7b", "odd_shapes"])
def test_wgrad_batch_gives_the_bits_of_one_call_per_factor(group):
    """halva_wgrad_accumulate_batch (round 6): the A factor and the B factors of ONE LoRA group as one launch of the tile
    kernel + one of the reduction - with the slab counts of the single-problem call, so the partials, their order and the results are the bits of
    halva_wgrad_accumulate called once per factor (peft's LoRA linear backward as used by llava/train/train_halva.py:1085-1101).  The shapes of the
    7B step's four groups at the packed bench rows; "odd_shapes": items the LDS-DMA table kernel does not take get one register-staged
    tile launch each, into their own regions of the workspace, and share the one reduction."""
    rows, d, F, r = 27424, 4096, 11008, 128
    shapes = {"qkv_7b": [(3 * r, d)] + [(d, r)] * 3, "gate_up_7b": [(2 * r, d)] + [(F, r)] * 2, "o_7b": [(r, d), (d, r)], "down_7b": [(r, F), (d, r)],
              "odd_shapes": [(320, 1032), (8, 8)]}[group]
    if group == "odd_shapes":
        rows = 1500
    g = torch.Generator().manual_seed(11)
    items = []
    for i, (M, N) in enumerate(shapes):
        lda, ldb = M + 8 * (i + 1), N + 16 * (i + 2)
        A = bf(torch.randn(rows, lda, generator=g)).to(DEV)[:, 8 * (i + 1):]
        B = bf(torch.randn(rows, ldb, generator=g)).to(DEV)[:, :N]
        items.append((torch.randn(M, N, generator=g).to(DEV), A, B, 0.25 * (i + 1)))
    one_by_one = [C.clone() for C, _, _, _ in items]
    for C, (_, A, B, alpha) in zip(one_by_one, items):
        K().wgrad_accumulate(C, A, B, alpha)
    batched = [C.clone() for C, _, _, _ in items]
    K().wgrad_accumulate_batch([(C, A, B, alpha) for C, (_, A, B, alpha) in zip(batched, items)])
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(batched, one_by_one)):
        assert torch.equal(a, b), (group, i, float((a - b).abs().max()))
    ref = items[0][0].double() + items[0][3] * (items[0][1].double().t() @ items[0][2].double())
    assert float((batched[0].double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())) * max(1, rows // 2000)


def test_clip_tower_features_match_reference():
    """CLIPVisionTower.forward of the reference (clip_encoder.py:37-56 around HF CLIPVisionModel: patch conv, class token +
    position embeddings, pre-LN, pre-norm blocks with quick_gelu, hidden_states[-2], CLS row dropped) and encode_images
    (llava_arch.py:80-83: + mlp2x_gelu projector), run by the product tower (HIP patch-embed / LayerNorm / attention / projector
    GEMMs) against the reference's own fp32 outputs on bf16-exact weights and images."""
    from golden_util import load_npz, meta_of, tensors
    from halva_amd.clip import CLIPVisionConfig, CLIPVisionTower, build_vision_projector
    from types import SimpleNamespace
    z = load_npz("clip_tower_d64.npz")
    cfg = meta_of(z, "cfg")
    for feature, want in (("patch", z["features"]), ("cls_patch", z["hidden_m2"])):
        vt = CLIPVisionTower("fixture", args=SimpleNamespace(mm_vision_select_layer=-2, mm_vision_select_feature=feature),
                             delay_load=True, config=CLIPVisionConfig(**cfg), device="cuda")
        vt._alloc()
        vt.load_hf_state_dict(tensors(z, "clip."))
        vt.is_loaded = True
        images = torch.from_numpy(z["images"]).cuda().bfloat16()
        f = vt(images)
        assert f.shape == tuple(want.shape) and f.dtype == torch.bfloat16
        w = torch.from_numpy(want)
        err = float((f.float().cpu() - w).norm() / w.norm())
        assert err < 1e-2, (feature, err)                       # bf16 activations through 2 blocks + LNs: ~4e-3 observed
        assert float((f.float().cpu() - w).abs().max()) < 0.05 * float(w.abs().max())
    # projector on the tower's features = encode_images
    pcfg = SimpleNamespace(mm_projector_type="mlp2x_gelu", mm_hidden_size=cfg["hidden_size"], hidden_size=z["proj.0.weight"].shape[0])
    proj = build_vision_projector(pcfg, device="cuda")
    proj.load_state_dict({k: v.bfloat16() for k, v in tensors(z, "proj.").items()})
    vt.select_feature = "patch"
    y = proj(vt(images))
    w = torch.from_numpy(z["projected"])
    assert y.shape == tuple(w.shape)
    assert float((y.float().cpu() - w).norm() / w.norm()) < 1e-2


@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(64, 64, 64, 64), (72, 200, 328, 80), (4096, 12288, 12288 + 384, 4096), (8, 8, 8, 8)])
def test_transpose_bf16_matches_torch(rows, cols, ld_src, ld_dst):
    """halva_transpose_bf16 (the refresh of the transposed, LoRA-merged weight copy: llama.py LoraGroup.refresh_tail): exact, for strided
    sources / destinations and partial tiles; what lies outside the [cols x rows] destination window is not touched."""
    g = torch.Generator().manual_seed(rows + cols)
    src = bf(torch.randn(rows, ld_src, generator=g)).to(DEV)
    dst = torch.full((cols, ld_dst), 7.0, dtype=torch.bfloat16, device=DEV)
    K().transpose_into(dst[:, :rows], src[:, :cols])
    torch.cuda.synchronize()
    assert torch.equal(dst[:, :rows], src[:, :cols].t())
    assert bool((dst[:, rows:] == 7.0).all())


def test_quick_gelu_matches_the_three_bf16_tensor_ops():
    """halva_quick_gelu = `x * torch.sigmoid(1.702 * x)` in bf16 (transformers QuickGELUActivation of the CLIP tower) with the same three
    roundings: equal to torch's result up to one bf16 ulp (the fast exponential), and within 1e-2 of the fp32 function."""
    g = torch.Generator().manual_seed(4)
    x = bf(4.0 * torch.randn(577 * 4096 // 8 * 8, generator=g)).to(DEV)
    ref = x * torch.sigmoid(1.702 * x)
    y = K().quick_gelu_(x.clone())
    torch.cuda.synchronize()
    d = (y.float() - ref.float()).abs()
    assert float((d / ref.float().abs().clamp_min(1e-3)).max()) < 1.6e-2      # <= 2 bf16 ulp
    assert float((d > 0).float().mean()) < 0.05
    xf = x.float()
    assert rel_err(y.float().cpu(), (xf * torch.sigmoid(1.702 * xf)).cpu()) < 1e-2
