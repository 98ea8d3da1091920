"""Row-wise checks of every dispatch path of the fused causal attention (halva_amd/csrc/sdpa.hip) against float64, with poisoned padding.

The tests in test_hip_kernels.py / test_sdpa_bench_shapes_gpu.py take one Frobenius error per tensor (or per head): one query row that
sees a wrong key at T = 2048 moves the total by far less than their 1e-2 / 2e-2.  Here every (sequence, row, head) row r of out / dq /
dk / dv is held to

    |X_kernel[r] - X_ref[r]|  <=  C_X |X_model[r] - X_ref[r]|  +  F_X |X_ref[r]|  +  G_X rms_r' |X_ref[r']|

X_ref: float64 on the same bf16 inputs (tests/sdpa_ref_util.reference).  X_model: the rounding model - the same computation in fp32,
rounded to bf16 where the kernels round (P before P V and dV, dS before dQ / dK, outputs; delta from the stored output).

  * C_X = 2 (every X): the kernel and the model make the same kind of errors - bf16 roundings of P / dS / the output, independent in
    detail - so the row norm of the kernel's error is a draw from the distribution the model's is: over D = 64 or 128 components it
    concentrates within ~10 % of its mean.  A factor of 2 leaves room for the kernels' own exponent references and partial sums.
  * F_X = 2^-8 (every X): rows whose model error is (nearly) zero - a row of length 1 is v itself, a key seen by one query gets one
    term.  A kernel may stack two bf16 roundings (an intermediate and the output), each at most 2^-9 of the row: 2^-8 in all.
  * G_X = 2^-14 of the tensor's RMS row norm (every X): rows whose REFERENCE is zero - dq of a sequence's first row is
    P (dP - delta) k with dP = delta exactly; in fp32 the two differ by ~2^-24 |dP|, ~2^-18 of a typical dq row.
  * lse: |lse_kernel - lse_ref| <= LSE_TOL (1 + |lse_ref|), LSE_TOL = 2^-20, elementwise on valid rows: fp32 scores (exact bf16 products,
    fp32 sums), exp2 / log2 and the row sums carry a few fp32 ulps (2^-24) of the row's magnitude; 2^-20 is 16 ulps, and ~1000x below
    the shift one key with P ~ 1e-3 causes.

The constants are written once, here, and hold for every path and layout.  Rows outside [start, start + len) must be exact zeros
(equal as values: -0 counts) in out and in all three thirds of dqkv.  The padding [br_a + len(A), br_b) inside a branched sequence is
unspecified by the contract and excluded.

Poisoning.  Every case runs twice: clean, and with NaN / +-Inf in the qkv rows outside [start, start + len), NaN / +-Inf and non-zero
finite garbage in the dout rows outside it (and in dout's columns beyond H*D), and the outputs (out including the columns of a wider
ld_out, lse, dqkv, delta_ws and the dS workspace) pre-filled with NaN.  The poisoned run must give the clean run's valid rows bit for bit,
zeros on the padded rows, and leave out's columns beyond H*D untouched.  The branch padding gets finite garbage in that run: its rows
are real query rows of the packed computation (what splice.pack_pairs writes there is zero embeddings), a NaN among them makes their P
NaN, and P o (dP - delta) carries it into the prefix keys' dK even with dO = 0 on those rows.  Non-finite values there are a forward
question only (its valid rows never see them): test_forward_with_nonfinite_branch_padding, a strict xfail that states the gap.

Paths are selected per call (environment switches read on every launch, sdpa.hip read_switches / choose_fwd / choose_bwd); entry points go through
the C ABI (halva_amd.hip.call) directly.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from sdpa_ref_util import branch_pad_rows, branch_positions, inverse_rope, reference, row_norms, valid_rows  # noqa: E402

DEV = "cuda"

C_X = {"out": 2.0, "dq": 2.0, "dk": 2.0, "dv": 2.0}
F_X = {"out": 2.0 ** -8, "dq": 2.0 ** -8, "dk": 2.0 ** -8, "dv": 2.0 ** -8}
G_X = {"out": 2.0 ** -14, "dq": 2.0 ** -14, "dk": 2.0 ** -14, "dv": 2.0 ** -14}
LSE_TOL = 2.0 ** -20

# ---------------------------------------------------------------------------------------------------------------------------------
# layouts.  a_len: len(A) of branched rows (the branch padding is [br_a + a_len, br_b)); heads: the heads held against float64
# (None = all; the kernel always runs all of them, and the padding / poisoning checks cover all of them)
CASES = {
    # T not a multiple of 32; T - len = 1, 63, 64, 65; S = 4 ragged
    "tail_T333": dict(S=4, T=333, H=2, D=128, starts=[0, 0, 0, 0], lens=[332, 270, 269, 268]),
    # len 1; left padding with start 1, 33, 64, 500
    "leftpad_len1": dict(S=5, T=600, H=2, D=128, starts=[0, 1, 33, 64, 500], lens=[1, 599, 300, 536, 100]),
    # branched rows: br_a = 63 / 129 / 65 / 127 (64-boundary +-1), empty A (s1), empty B (s2), no branch (s3: br_a = br_b >= len)
    "branch_edges": dict(S=5, T=700, H=2, D=128, starts=[0] * 5, lens=[392, 492, 256, 650, 700],
                         br_a=[63, 129, 65, 700, 127], br_b=[192, 192, 256, 700, 128], a_len=[100, 0, 130, 0, 1]),
    # H = 40 and S * H * ceil(T / 128) = 1080 dkv3 items, ~4x the CU count
    "h40_many_items": dict(S=3, T=1100, H=40, D=128, starts=[0, 0, 0], lens=[1100, 1037, 700], heads=[0, 1, 19, 38, 39]),
    # 3 dkv3 items: far below the CU count
    "few_items": dict(S=1, T=384, H=1, D=128, starts=[0], lens=[384]),
    # the bench's packed row [668 | 1380 | 1380], T = 3428, H = 32
    "bench_packed": dict(S=1, T=3428, H=32, D=128, starts=[0], lens=[3428], br_a=[668], br_b=[2048], a_len=[1380],
                         heads=[0, 11, 20, 31]),
    # head_dim 64 (no dS workspace: the split backward)
    "d64_leftpad": dict(S=3, T=333, H=2, D=64, starts=[0, 1, 64], lens=[333, 268, 1]),
    "d64_branch": dict(S=2, T=200, H=2, D=64, starts=[0, 0], lens=[200, 150], br_a=[63, 10], br_b=[128, 64], a_len=[30, 20]),
}

# dispatch paths: environment switches (sdpa.hip, read on every call).  Forward-only switches run the default backward on their
# forward's lse and output, and backward-only switches the default forward.
PATHS = {
    "default": {},
    "fwd3_twin": {"HALVA_FWD3_ASM": "0"},
    "fwd_legacy": {"HALVA_SDPA_FWD3": "0"},
    "slow_tr": {"HALVA_SDPA_SLOW_TR": "1"},
    "dkv3_hip": {"HALVA_DKV3_ASM": "0"},
    "dq2_general_tile": {"HALVA_DQ2_FAST_TILE": "0"},
    "dkv2": {"HALVA_SDPA_DKV3": "0"},
    "order0": {"HALVA_DKV3_ORDER": "0"},
    "order1": {"HALVA_DKV3_ORDER": "1"},
    "order2": {"HALVA_DKV3_ORDER": "2"},
    "rope_unfused": {"HALVA_ROPE_FUSED_BWD": "0"},
}

# entry points: forward + backward
#   causal      halva_sdpa_causal_fwd / _bwd (ld = H*D; the split backward: no workspace)
#   causal_ld   halva_sdpa_causal_fwd_ld / _bwd_ld with ld_out, ld_dout > H*D (split backward)
#   split       halva_sdpa_branch_fwd / halva_sdpa_branch_bwd: no dS workspace, the split backward (kernels.SDPA_DS_WS = False)
#   ws          halva_sdpa_branch_fwd / halva_sdpa_branch_bwd_ws with the dS workspace (the shipped backward), wide ld
#   rope        halva_sdpa_branch_fwd / halva_sdpa_branch_bwd_rope (workspace + inverse RoPE of dq / dk), wide ld
D128 = ["tail_T333", "leftpad_len1", "branch_edges", "h40_many_items", "few_items", "bench_packed"]
ALT = ["tail_T333", "leftpad_len1", "branch_edges"]
MATRIX = (
    [("default", "ws", c) for c in D128]
    + [("default", "rope", c) for c in D128]
    + [("default", "causal", c) for c in ["tail_T333", "leftpad_len1", "few_items"]]
    + [("default", "causal_ld", c) for c in ["tail_T333", "leftpad_len1", "h40_many_items"]]
    + [("default", "split", c) for c in ["branch_edges", "leftpad_len1", "bench_packed"]]
    + [(p, "ws", c) for p in ["fwd3_twin", "fwd_legacy", "slow_tr", "dq2_general_tile", "dkv2"] for c in ALT]
    + [("dkv3_hip", "ws", c) for c in ALT + ["h40_many_items"]]
    + [(p, "ws", c) for p in ["order0", "order1", "order2"] for c in ["leftpad_len1", "branch_edges", "h40_many_items", "few_items"]]
    + [("rope_unfused", "rope", c) for c in ["leftpad_len1", "branch_edges"]]
    + [("default", e, c) for e in ["ws", "rope"] for c in ["d64_leftpad", "d64_branch"]]
    + [("default", "causal", "d64_leftpad"), ("slow_tr", "ws", "d64_branch"), ("slow_tr", "ws", "d64_leftpad")]
)


def _case(name):
    c = dict(CASES[name])
    c.setdefault("br_a", None), c.setdefault("br_b", None), c.setdefault("a_len", None), c.setdefault("heads", None)
    c["branched"] = c["br_a"] is not None
    return c


def _i32(v):
    return None if v is None else torch.tensor(v, dtype=torch.int32, device=DEV)


def _row_masks(c):
    """(valid [S, T]: rows held to the reference; outside [S, T]: rows outside [start, start + len); branch padding [S, T])"""
    inside = valid_rows(c["S"], c["T"], c["starts"], c["lens"])
    pad = branch_pad_rows(c["S"], c["T"], c["br_a"], c["br_b"], c["a_len"])
    return (inside & ~pad).to(DEV), (~inside).to(DEV), pad.to(DEV)


_inputs_cache, _ref_cache = {}, {}


def _inputs(name):
    """clean bf16 qkv [S, T, 3, H, D] and dout [S, T, H, D] on the device; dout is zero outside the valid rows (the loss never reads
    them).  The rows outside [start, start + len) hold ordinary numbers in the clean run."""
    if name not in _inputs_cache:
        c = _case(name)
        g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
        qkv = torch.randn(c["S"], c["T"], 3, c["H"], c["D"], generator=g).to(torch.bfloat16)
        dout = torch.randn(c["S"], c["T"], c["H"], c["D"], generator=g).to(torch.bfloat16)
        valid, _, _ = _row_masks(c)
        dout[~valid.cpu()] = 0
        _inputs_cache[name] = (qkv.to(DEV), dout.to(DEV))
    return _inputs_cache[name]


def _ref(name):
    """the float64 reference of a case, computed once per session"""
    if name not in _ref_cache:
        c = _case(name)
        qkv, dout = _inputs(name)
        _ref_cache[name] = reference(qkv, c["starts"], c["lens"], c["br_a"], c["br_b"], dout, heads=c["heads"])
    return _ref_cache[name]


def _model(c, qkv, dout, stored_out):
    """the rounding model of a case; its backward forms delta from the output the kernel's forward stored"""
    return reference(qkv, c["starts"], c["lens"], c["br_a"], c["br_b"], dout, heads=c["heads"], model=True, stored_out=stored_out)


def _cycle(shape, values, gen_garbage=None):
    """a tensor of `shape` whose elements cycle through `values` (float); with gen_garbage the last slot of the cycle is finite garbage"""
    n = math.prod(shape)
    idx = torch.arange(n, device=DEV) % (len(values) + (1 if gen_garbage is not None else 0))
    vals = torch.tensor(values + ([0.0] if gen_garbage is not None else []), dtype=torch.float32, device=DEV)
    x = vals[idx]
    if gen_garbage is not None:
        x = torch.where(idx == len(values), gen_garbage(n), x)
    return x.view(shape).to(torch.bfloat16)


NONFINITE = [float("nan"), float("inf"), float("-inf")]


def _poisoned_inputs(c, qkv, dout, nonfinite_branch_pad=False):
    _, outside, pad = _row_masks(c)
    g = torch.Generator(device=DEV).manual_seed(7)
    garbage = lambda n, a=50.0: a * torch.randn(n, generator=g, device=DEV)
    qkv_p, dout_p = qkv.clone(), dout.clone()
    qkv_p[outside] = _cycle(qkv_p[outside].shape, NONFINITE)
    dout_p[outside] = _cycle(dout_p[outside].shape, NONFINITE, garbage)
    if bool(pad.any()):
        qkv_p[pad] = _cycle(qkv_p[pad].shape, NONFINITE) if nonfinite_branch_pad else \
            (4.0 * torch.randn(qkv_p[pad].shape, generator=g, device=DEV)).to(torch.bfloat16)
    return qkv_p, dout_p


def _lib():
    from halva_amd import hip
    return hip


def _forward(c, entry, qkv, poison):
    """(out buffer [S, T, ld_out], lse [S, H, T]) of one forward call; outputs pre-filled with NaN (poison) or 0 / a 1.5 sentinel
    beyond H*D (clean)"""
    hip = _lib()
    S, T, H, D = c["S"], c["T"], c["H"], c["D"]
    hd = H * D
    ld_out = hd if entry == "causal" else hd + 64
    fill = float("nan") if poison else 0.0
    out = torch.full((S, T, ld_out), fill, dtype=torch.bfloat16, device=DEV)
    if not poison:
        out[..., hd:] = 1.5
    lse = torch.full((S, H, T), fill, dtype=torch.float32, device=DEV)
    st, ln, ba, bb = _i32(c["starts"]), _i32(c["lens"]), _i32(c["br_a"]), _i32(c["br_b"])
    x = qkv.view(S, T, 3 * hd)
    sp = hip.stream_ptr()
    if entry == "causal":
        assert not c["branched"]
        hip.call("halva_sdpa_causal_fwd", hip.ptr(x), hip.ptr(out), hip.ptr(lse), hip.ptr(st), hip.ptr(ln), S, T, H, D, 0.0, sp)
    elif entry == "causal_ld":
        assert not c["branched"]
        hip.call("halva_sdpa_causal_fwd_ld", hip.ptr(x), hip.ptr(out), ld_out, hip.ptr(lse), hip.ptr(st), hip.ptr(ln), S, T, H, D, 0.0, sp)
    else:
        hip.call("halva_sdpa_branch_fwd", hip.ptr(x), hip.ptr(out), ld_out, hip.ptr(lse), hip.ptr(st), hip.ptr(ln), hip.ptr(ba), hip.ptr(bb),
                 S, T, H, D, 0.0, sp)
    torch.cuda.synchronize()
    return out, lse


def _rope_tables(D):
    from halva_amd import kernels
    return kernels.rope_tables(D, 4096, device=DEV)


def _backward(c, entry, qkv, out, lse, dout, poison):
    """dqkv [S, T, 3, H, D] of one backward call on the forward's own out / lse; dout sits in a buffer of row stride ld_dout whose
    columns beyond H*D hold NaN / garbage (poison) or zeros; dqkv, delta_ws and the dS workspace pre-filled with NaN (poison) or 0"""
    hip = _lib()
    S, T, H, D = c["S"], c["T"], c["H"], c["D"]
    hd = H * D
    ld_out = out.shape[-1]
    ld_do = hd if entry == "causal" else hd + 48
    fill = float("nan") if poison else 0.0
    dbuf = torch.zeros(S, T, ld_do, dtype=torch.bfloat16, device=DEV)
    if poison and ld_do > hd:
        dbuf[..., hd:] = _cycle((S, T, ld_do - hd), NONFINITE, lambda n: 50.0 * torch.randn(n, device=DEV))
    dbuf[..., :hd] = dout.view(S, T, hd)
    dqkv = torch.full((S, T, 3, H, D), fill, dtype=torch.bfloat16, device=DEV)
    delta = torch.full((S, H, T), fill, dtype=torch.float32, device=DEV)
    ws, ws_bytes = None, 0
    if entry in ("ws", "rope"):
        ws_bytes = int(hip.load().halva_sdpa_bwd_ws_bytes(S, T, H, D))
        if ws_bytes:
            ws = torch.full((ws_bytes,), 0xFF if poison else 0, dtype=torch.uint8, device=DEV)      # 0xFF..: NaN as bf16 and as f32
    st, ln, ba, bb = _i32(c["starts"]), _i32(c["lens"]), _i32(c["br_a"]), _i32(c["br_b"])
    x = qkv.view(S, T, 3 * hd)
    P = hip.ptr
    sp = hip.stream_ptr()
    if entry == "causal":
        hip.call("halva_sdpa_causal_bwd", P(x), P(out), P(dbuf), P(lse), P(dqkv), P(delta), None, P(st), P(ln), S, T, H, D, 0.0, sp)
    elif entry == "causal_ld":
        hip.call("halva_sdpa_causal_bwd_ld", P(x), P(out), ld_out, P(dbuf), ld_do, P(lse), P(dqkv), P(delta), None, P(st), P(ln),
                 S, T, H, D, 0.0, sp)
    elif entry == "split":
        hip.call("halva_sdpa_branch_bwd", P(x), P(out), ld_out, P(dbuf), ld_do, P(lse), P(dqkv), P(delta), P(st), P(ln), P(ba), P(bb),
                 S, T, H, D, 0.0, sp)
    elif entry == "ws":
        hip.call("halva_sdpa_branch_bwd_ws", P(x), P(out), ld_out, P(dbuf), ld_do, P(lse), P(dqkv), P(delta), P(ws), ws_bytes, P(st), P(ln),
                 P(ba), P(bb), S, T, H, D, 0.0, sp)
    else:
        cos, sin = _rope_tables(D)
        hip.call("halva_sdpa_branch_bwd_rope", P(x), P(out), ld_out, P(dbuf), ld_do, P(lse), P(dqkv), P(delta), P(ws), ws_bytes, P(st),
                 P(ln), P(ba), P(bb), P(cos), P(sin), cos.shape[0], S, T, H, D, 0.0, sp)
    torch.cuda.synchronize()
    return dqkv


def rowwise_violations(name, xk, xref, xmodel, rows):
    """[S, T, h] bool: rows (of the [S, T] mask `rows`) where the kernel's error exceeds the bound of the module docstring; and the
    largest ratio error / bound over those rows"""
    xref = xref.double()
    ek = row_norms(xk.double() - xref)
    em = row_norms(xmodel.double() - xref)
    nr = row_norms(xref)
    m = rows[..., None].expand_as(nr)
    rms = float(nr[m].pow(2).mean().sqrt()) if bool(m.any()) else 0.0
    bound = C_X[name] * em + F_X[name] * nr + G_X[name] * rms
    viol = (ek > bound) & m
    ratio = float((ek / bound.clamp_min(1e-300))[m].max()) if bool(m.any()) else 0.0
    return viol, ratio


def frobenius_rel(xk, xref):
    """the old criterion (test_hip_kernels.rel_err): one relative Frobenius error over the whole tensor"""
    xref = xref.double()
    return float((xk.double() - xref).norm() / (xref.norm() + 1e-12))


def _describe(viol, limit=6):
    idx = viol.nonzero().tolist()
    return "%d rows, first (s, t, h): %s" % (len(idx), idx[:limit])


def _zero_rows(x, rows):
    """x [S, T, ...]: every element of the rows in `rows` equals 0 (as a value: -0 counts)"""
    return bool((x[rows] == 0).all())


def _same(a, b):
    """equal as values (so the same bits wherever a value is not zero), and finite"""
    return bool(torch.isfinite(a).all()) and torch.equal(a, b)


def _differ(a, b, rows):
    """a, b [S, T, ...] and rows [S, T]: where the two differ on those rows (for a failure message)"""
    bad = ((a != b) | ~torch.isfinite(a)).flatten(2).any(-1) & rows
    idx = bad.nonzero().tolist()
    d = (a.float() - b.float())[bad]
    return "%d rows differ, first (s, t): %s, non-finite %d, max |diff| %s" % (
        len(idx), idx[:6], int((~torch.isfinite(d)).sum()), float(d[torch.isfinite(d)].abs().max()) if bool(torch.isfinite(d).any()) else None)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("path,entry,case", MATRIX, ids=["%s-%s-%s" % m for m in MATRIX])
def test_rowwise_against_float64_with_poisoned_padding(path, entry, case, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = _case(case)
    S, T, H, D = c["S"], c["T"], c["H"], c["D"]
    hd = H * D
    heads = c["heads"] if c["heads"] is not None else list(range(H))
    valid, outside, _ = _row_masks(c)
    qkv, dout = _inputs(case)
    ref = _ref(case)

    out_c, lse_c = _forward(c, entry, qkv, poison=False)
    dqkv_c = _backward(c, entry, qkv, out_c, lse_c, dout, poison=False)
    qkv_p, dout_p = _poisoned_inputs(c, qkv, dout)
    out_p, lse_p = _forward(c, entry, qkv_p, poison=True)
    extra_p = out_p[..., hd:].clone()
    dqkv_p = _backward(c, entry, qkv_p, out_p, lse_p, dout_p, poison=True)

    o_c = out_c[..., :hd].view(S, T, H, D)
    o_p = out_p[..., :hd].view(S, T, H, D)
    # --- row-wise against float64 (clean run; the heads of the case)
    hsel = torch.tensor(heads, device=DEV)
    got = {"out": o_c.index_select(2, hsel)}
    for i, n in enumerate(("dq", "dk", "dv")):
        got[n] = dqkv_c[:, :, i].index_select(2, hsel)
    model = _model(c, qkv, dout, got["out"])
    want, mod = dict(ref), dict(model)
    if entry == "rope":
        cos, sin = _rope_tables(D)
        pos = branch_positions(T, c["br_a"], c["br_b"], S)
        for n in ("dq", "dk"):
            want[n] = inverse_rope(ref[n], cos, sin, pos)
            mod[n] = inverse_rope(model[n].double(), cos, sin, pos)
    report = []
    for n in ("out", "dq", "dk", "dv"):
        assert bool(torch.isfinite(got[n][valid]).all()), (n, "non-finite values on valid rows")
        viol, ratio = rowwise_violations(n, got[n], want[n], mod[n], valid)
        report.append("%s %.3f" % (n, ratio))
        assert not bool(viol.any()), (n, "row-wise bound exceeded", _describe(viol), "worst error / bound %.3f" % ratio)
    lk = lse_c.index_select(1, hsel).double()
    lr = ref["lse"]
    vl = valid[:, None, :].expand_as(lr)
    lse_err = ((lk - lr).abs() / (1 + lr.abs()))[vl]
    report.append("lse %.2e" % float(lse_err.max()))
    print("[%s-%s-%s] worst error / bound: %s" % (path, entry, case, ", ".join(report)))
    assert float(lse_err.max()) <= LSE_TOL, ("lse", float(lse_err.max()))
    # --- padded rows: exact zeros, both runs
    for o, dq, tag in ((o_c, dqkv_c, "clean"), (o_p, dqkv_p, "poisoned")):
        assert _zero_rows(o, outside), ("out padded rows", tag)
        for i, n in enumerate(("dq", "dk", "dv")):
            assert _zero_rows(dq[:, :, i], outside), (n + " padded rows", tag)
    # --- the poisoned run: the clean run's valid rows bit for bit, out's columns beyond H*D untouched
    assert _same(o_p[valid], o_c[valid]), ("poisoned out", _differ(o_p, o_c, valid))
    assert _same(lse_p.transpose(1, 2)[valid], lse_c.transpose(1, 2)[valid]), ("poisoned lse", _differ(lse_p.transpose(1, 2), lse_c.transpose(1, 2), valid))
    for i, n in enumerate(("dq", "dk", "dv")):
        assert _same(dqkv_p[:, :, i][valid], dqkv_c[:, :, i][valid]), ("poisoned " + n, _differ(dqkv_p[:, :, i], dqkv_c[:, :, i], valid))
    if out_p.shape[-1] > hd:
        assert torch.equal(out_p[..., hd:].view(torch.int16), extra_p.view(torch.int16)), "out columns beyond H*D were written (bwd)"
        assert bool((out_p[..., hd:].view(torch.int16) == torch.tensor(float("nan"), dtype=torch.bfloat16).view(torch.int16)).all()), \
            "out columns beyond H*D were written (fwd)"
        assert bool((out_c[..., hd:] == 1.5).all()), "out columns beyond H*D were written (clean)"


# Known gap, kept visible: NaN / Inf INSIDE the branch padding [br_a + len(A), br_b) reach valid rows of the same sequence on every
# forward kernel.  Observed: sdpa_fwd3 (generated asm and its plain-HIP twin) returns NaN on every row of such a sequence, row 0 included;
# sdpa_fwd_kernel (HALVA_SDPA_FWD3=0, HALVA_SDPA_SLOW_TR=1, head_dim 64) on the rows that share a row block with the padding and on the
# branch-B rows behind an empty A, whose hidden keys share a key tile with it.  The contract leaves only the OUTPUT of those rows
# unspecified, and what the product writes there is finite (zero embeddings, splice.pack_pairs) - the finite-garbage run above holds
# every path to the clean bits.  Strict: the day a forward discards these keys' scores before its row statistics, this turns green.
@pytest.mark.timeout(120)
@pytest.mark.xfail(strict=True, reason="non-finite values in the in-sequence branch padding reach valid rows of every forward kernel")
@pytest.mark.parametrize("path,case", [("default", "branch_edges"), ("fwd3_twin", "branch_edges"), ("fwd_legacy", "branch_edges"),
                                       ("slow_tr", "branch_edges"), ("default", "d64_branch")])
def test_forward_with_nonfinite_branch_padding(path, case, monkeypatch):
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)
    c = _case(case)
    S, T, H, D = c["S"], c["T"], c["H"], c["D"]
    hd = H * D
    valid, outside, _ = _row_masks(c)
    qkv, dout = _inputs(case)
    out_c, lse_c = _forward(c, "ws", qkv, poison=False)
    qkv_n, _ = _poisoned_inputs(c, qkv, dout, nonfinite_branch_pad=True)
    out_n, lse_n = _forward(c, "ws", qkv_n, poison=True)
    o_c, o_n = out_c[..., :hd].view(S, T, H, D), out_n[..., :hd].view(S, T, H, D)
    assert _zero_rows(o_n, outside)
    assert _same(o_n[valid], o_c[valid]), ("out with non-finite branch padding", _differ(o_n, o_c, valid))
    assert _same(lse_n.transpose(1, 2)[valid], lse_c.transpose(1, 2)[valid]), \
        ("lse with non-finite branch padding", _differ(lse_n.transpose(1, 2), lse_c.transpose(1, 2), valid))


# ---------------------------------------------------------------------------------------------------------------------------------
# the non-causal tower attention (halva_sdpa_full_fwd): CLIP ViT-L/14-336 (577 rows, head_dim 64) and SigLIP so400m (729 rows,
# head_dim 72 zero-padded to 128, scale 72**-0.5 - halva_amd/siglip.py's call)
@pytest.mark.parametrize("tower", ["clip_S577_D64", "siglip_S729_D72pad128"])
def test_full_attention_rowwise(tower):
    from halva_amd import hip, kernels
    N, H = 2, 16
    if tower.startswith("clip"):
        S, D, Dh, scale = 577, 64, 64, 0.0
        ref_scale = 64 ** -0.5
    else:
        S, D, Dh = 729, 128, 72
        scale = ref_scale = float(Dh) ** -0.5
    g = torch.Generator().manual_seed(77)
    qkv = torch.zeros(N, S, 3, H, D)
    qkv[..., :Dh] = torch.randn(N, S, 3, H, Dh, generator=g)
    qkv = qkv.to(torch.bfloat16).to(DEV)
    out = kernels.sdpa_full(qkv.view(N, S, 3 * H * D), H, D, scale).view(N, S, H, D)
    buf = torch.full((N, S, H * D), float("nan"), dtype=torch.bfloat16, device=DEV)       # every element written
    hip.call("halva_sdpa_full_fwd", hip.ptr(qkv), hip.ptr(buf), N, S, H, D, float(scale), hip.stream_ptr())
    torch.cuda.synchronize()
    assert _same(buf.view(N, S, H, D), out)
    assert bool((out[..., Dh:] == 0).all())                                                   # the zero lanes stay zero
    starts, lens = [0] * N, [S] * N
    ref = reference(qkv, starts, lens, scale=ref_scale, causal=False)["out"]
    mod = reference(qkv, starts, lens, scale=ref_scale, causal=False, model=True)["out"]
    rows = torch.ones(N, S, dtype=torch.bool, device=DEV)
    viol, ratio = rowwise_violations("out", out, ref, mod, rows)
    print("[%s] worst error / bound: out %.3f" % (tower, ratio))
    assert not bool(viol.any()), (_describe(viol), ratio)


# ---------------------------------------------------------------------------------------------------------------------------------
# proof that the row-wise check can fail where the Frobenius criterion cannot: the unmodified kernels on deliberately mismatched
# inputs.  Each mismatch changes a handful of rows; the Frobenius error of the whole tensor stays below 1e-2 / 2e-2.
def _plain_case(T, H, lens, br=None):
    c = dict(S=len(lens), T=T, H=H, D=128, starts=[0] * len(lens), lens=lens, br_a=None, br_b=None, a_len=None, heads=None, branched=False)
    if br is not None:
        c.update(br_a=br[0], br_b=br[1], a_len=br[2], branched=True)
    return c


def _random_inputs(c, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(c["S"], c["T"], 3, c["H"], c["D"], generator=g).to(torch.bfloat16).to(DEV)
    dout = torch.randn(c["S"], c["T"], c["H"], c["D"], generator=g).to(torch.bfloat16).to(DEV)
    return qkv, dout


def test_mismatch_swapped_key_rows_is_caught_rowwise_only():
    """keys (k and v) t and t + 1 swapped for the kernel only, at a 256-row tile edge inside a 2048-row sequence: only row t's visible
    set changes (rows past t + 1 see the same set in another order)"""
    t = 255
    c = _plain_case(2048, 4, [2048])
    qkv, _ = _random_inputs(c, 51)
    ref = reference(qkv, c["starts"], c["lens"])
    mod = reference(qkv, c["starts"], c["lens"], model=True)
    bad = qkv.clone()
    bad[:, [t, t + 1], 1:] = qkv[:, [t + 1, t], 1:]
    out, _ = _forward(c, "ws", bad, poison=False)
    o = out[..., :c["H"] * 128].view(1, 2048, c["H"], 128)
    rows = torch.ones(1, 2048, dtype=torch.bool, device=DEV)
    viol, _ = rowwise_violations("out", o, ref["out"], mod["out"], rows)
    assert bool(viol.any()), "the row-wise check missed the swapped keys"
    assert set(viol.nonzero()[:, 1].tolist()) == {t}, _describe(viol)
    assert frobenius_rel(o, ref["out"]) < 1e-2


def test_mismatch_shifted_branch_point_is_caught_rowwise_only():
    """br_a one row later for the kernel than for the reference: key br_a becomes visible to the 64 rows of branch B"""
    br_a, br_b = 1000, 1984
    c = _plain_case(2048, 4, [2048], br=([br_a], [br_b], [br_b - br_a]))
    qkv, _ = _random_inputs(c, 52)
    ref = reference(qkv, c["starts"], c["lens"], c["br_a"], c["br_b"])
    mod = reference(qkv, c["starts"], c["lens"], c["br_a"], c["br_b"], model=True)
    shifted = dict(c, br_a=[br_a + 1])
    out, _ = _forward(shifted, "ws", qkv, poison=False)
    o = out[..., :c["H"] * 128].view(1, 2048, c["H"], 128)
    rows = torch.ones(1, 2048, dtype=torch.bool, device=DEV)
    viol, _ = rowwise_violations("out", o, ref["out"], mod["out"], rows)
    assert bool(viol.any()), "the row-wise check missed the shifted branch point"
    assert min(viol.nonzero()[:, 1].tolist()) >= br_b, _describe(viol)
    assert frobenius_rel(o, ref["out"]) < 1e-2


def test_mismatch_scaled_dout_row_is_caught_rowwise_only():
    """one dout row scaled by 1.05 for the kernel only: its dq row is 5 % off"""
    r = 1000
    c = _plain_case(2048, 2, [2048])
    qkv, dout = _random_inputs(c, 53)
    ref = reference(qkv, c["starts"], c["lens"], dout=dout)
    bad = dout.clone()
    bad[:, r] = (bad[:, r].float() * 1.05).to(torch.bfloat16)
    out, lse = _forward(c, "ws", qkv, poison=False)
    dqkv = _backward(c, "ws", qkv, out, lse, bad, poison=False)
    o = out[..., :c["H"] * 128].view(1, 2048, c["H"], 128)
    mod = reference(qkv, c["starts"], c["lens"], dout=dout, model=True, stored_out=o)
    rows = torch.ones(1, 2048, dtype=torch.bool, device=DEV)
    viol, _ = rowwise_violations("dq", dqkv[:, :, 0], ref["dq"], mod["dq"], rows)
    assert bool(viol[0, r].any()), "the row-wise check missed dq of the scaled row: " + _describe(viol)
    assert frobenius_rel(o, ref["out"]) < 1e-2
    for i, n in enumerate(("dq", "dk", "dv")):
        assert frobenius_rel(dqkv[:, :, i], ref[n]) < 2e-2, n
