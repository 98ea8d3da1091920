"""Elementwise checks of halva_amd/csrc/gemm.hip (gemm_tile.h, wgrad.h) against float64, with poisoned surroundings: halva_gemm_bf16 in its three forms
and every argument combination, halva_wgrad_accumulate(_batch), halva_transpose_bf16, halva_colsum, halva_gelu_bwd.

test_hip_kernels.py takes one relative Frobenius error (or one maximum error scaled by the row count) per tensor.  Here every element
is held, in the two regimes of tests/gemm_ref_util.py: EXACT (integer inputs: bit equality with float64, no tolerance) and RANDOM

    |X_kernel - X_ref|  <=  |X_model - X_ref|  +  2 delta  +  G

  * GEMM, bf16 output: delta = 2 n U S (deterministic), n = K + 2, S = |A| |B|^T + |bias| + |prior C|.
  * GEMM and weight gradients, fp32 output: delta = U (8 sqrt(n) + 4) S (probabilistic), n = K + 2 + splits, S = alpha |A|^T |B| + |prior C|.
  * epilogue = 1: `pre` is held as above; C is held to gelu64(pre AS THE KERNEL STORED IT) (+ prior C), so that one rounding is
    modelled: delta = 0.5 |x| (E_ERF + U (1 + erf)) + U |y| (+ U |C| for the accumulating add), E_ERF = 16 U assumed (gemm_ref_util).
    The run without `pre_act` must give the bits of the run with it.
  * colsum: delta = U (8 sqrt(n) + 4) S, n = rows of a slab + splits.
  * gelu_bwd, dh = bf16(dy (cdf + x pdf)): e_cdf = 0.5 (E_ERF + U (1 + erf)) + U |x| phi + U cdf (erff, the rounding of x / sqrt 2, the
    product with 0.5); e_pdf = phi U (2 |arg| + 8), arg = -x^2 / 2 (the rounding of x x, __expf: U (|arg| + 6) relative as in
    test_rowops_rowwise_gpu.py, the constant's product); delta = |dy| (e_cdf + |x| e_pdf + U |x| phi + U |cdf + x phi|) + U |dh|.

Poison: every operand is a window of a larger allocation whose other elements - the columns beside it, two or more rows before it and
64 or more rows after it for the weight gradients - cycle NaN / +Inf / -Inf: a read past a tail that reaches the MFMA gives a
non-finite result.  Every output (C, `pre`, the split-k workspace, the transpose's destination, colsum's sums) is a window of a
sentinel-filled allocation whose every other byte must survive the call.  So every address a predicate or descriptor off by up to
one tile could reach lies inside the test's own allocations.  What no result can show: a non-transposed operand read ONE row past
its M (or N) tail - that row feeds only the accumulator row M (column N), which the epilogue never stores.

Entry points go through the C ABI (halva_amd.hip.call).
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref_util as R  # noqa: E402
from gemm_ref_util import U, bf, embed, exact, held, outside_unchanged, same_bits  # noqa: E402
from halva_amd import hip  # noqa: E402
from halva_amd.hip import BF16, F32, HalvaHipError, call, ptr, stream_ptr  # noqa: E402

DEV = "cuda"
bf16 = torch.bfloat16
REPORT = {}
SENT = R.SENT


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _gemm(A, B, bias, C, pre, M, N, K, ta, tb, epi, acc):
    call("halva_gemm_bf16", ptr(A), ptr(B), ptr(bias), ptr(C), ptr(pre), M, N, K, ta, tb, epi, F32 if C.dtype == torch.float32 else BF16, acc,
         stream_ptr())


def _wgrad(A, B, C, rows, alpha, ws, ws_floats):
    M, N = C.shape
    call("halva_wgrad_accumulate", ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), M, N, rows, float(alpha), ptr(ws), ws_floats, stream_ptr())


def _wgrad_items(items):
    arr = (hip.WgradItem * len(items))()
    for it, (C, A, B, alpha) in zip(arr, items):
        it.A, it.lda, it.B, it.ldb, it.C, it.M, it.N, it.rows, it.alpha = ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), C.shape[0], C.shape[1], \
            A.shape[0], float(alpha)
    return arr


def _wgrad_batch(items, ws, ws_floats):
    arr = items if isinstance(items, ctypes.Array) else _wgrad_items(items)
    call("halva_wgrad_accumulate_batch", len(arr), ctypes.cast(arr, ctypes.c_void_p), ptr(ws), ws_floats, stream_ptr())


def _transpose(src, dst, rows, cols):
    call("halva_transpose_bf16", ptr(src), src.stride(0), ptr(dst), dst.stride(0), rows, cols, stream_ptr())


def _colsum(x, out, M, N):
    call("halva_colsum", ptr(x), ptr(out), M, N, stream_ptr())


def _gelu_bwd(dy, h, dh, M, N):
    call("halva_gelu_bwd", ptr(dy), ptr(h), ptr(dh), M, N, stream_ptr())


def _guard(ld):
    return R.guard_rows(ld, 2 * ld + 64)


def _poisoned(x, align=True):
    """x [R, n] contiguous inside a poisoned allocation: more than two rows of NaN / Inf before and after it"""
    g = _guard(x.shape[1])
    return embed(x, "nan", rows_before=g, rows_after=g, align=align)[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# halva_gemm_bf16
FORMS = {"NN": (0, 0), "NT": (0, 1), "TN": (1, 1)}
VILA_C4, VILA_H = 4 * 1152, 5120        # mlp_downsample (halva_amd/vila_model.py: LayerNorm(4 c) -> Linear(4 c, h) -> GELU -> Linear(h, h)), SigLIP c, 13B h
GEMM_CASES = [("min", f, 8, 8, 8) for f in FORMS] + [("chunk-over", f, 136, 264, 72) for f in FORMS] + \
             [("k-below-tile", f, 264, 136, 40) for f in FORMS] + [("odd-k", "TN", 136, 264, 71), ("k7", "TN", 8, 8, 7)]
for _n in (1, 3):
    _m = 576 * _n                       # LLaVA mlp2x_gelu: 1024 -> 4096 -> 4096 (kernels.py _ProjectorMLP)
    GEMM_CASES += [("llava%d-fc1" % _n, "NN", _m, 4096, 1024), ("llava%d-fc2" % _n, "NN", _m, 4096, 4096),
                   ("llava%d-dw2" % _n, "TN", 4096, 4096, _m), ("llava%d-dg" % _n, "NT", _m, 4096, 4096),
                   ("llava%d-dw1" % _n, "TN", 4096, 1024, _m)]
    _m = 196 * _n                       # VILA mlp_downsample (kernels.py _DownsampleMLP)
    GEMM_CASES += [("vila%d-fc1" % _n, "NN", _m, VILA_H, VILA_C4), ("vila%d-fc2" % _n, "NN", _m, VILA_H, VILA_H),
                   ("vila%d-dw2" % _n, "TN", VILA_H, VILA_H, _m), ("vila%d-dg" % _n, "NT", _m, VILA_H, VILA_H),
                   ("vila%d-dw1" % _n, "TN", VILA_H, VILA_C4, _m), ("vila%d-dxn" % _n, "NT", _m, VILA_C4, VILA_H)]


def _gemm_inputs(form, M, N, K, regime, g):
    ta, tb = FORMS[form]
    sa, sb = ((K, M) if ta else (M, K)), ((K, N) if tb else (N, K))
    if regime == "exact":
        A, B = R.int_tensor(sa, g, DEV), R.int_tensor(sb, g, DEV)
        bias = R.int_tensor((N,), g, DEV)
        C0 = R.int_tensor((M, N), g, DEV, -1024, 1024, torch.float32)
    else:
        A, B = R.rand_tensor(sa[0], sa[1], g, DEV), R.rand_tensor(sb[0], sb[1], g, DEV)
        bias = torch.randn(N, generator=g, device=DEV).to(bf16)
        C0 = torch.randn(M, N, generator=g, device=DEV) * math.sqrt(K)
    a64 = A.double().t() if ta else A.double()              # logical [M, K]
    b64 = B.double() if tb else B.double().t()              # logical [K, N]
    return A, B, bias, C0, a64 @ b64, a64.abs() @ b64.abs()


@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("name,form,M,N,K", GEMM_CASES, ids=["%s-%s-%dx%dx%d" % c for c in GEMM_CASES])
def test_gemm_elementwise(name, form, M, N, K, regime):
    """Every combination of bias, output type, accumulate, pre_act and epilogue, on poisoned operands and sentinel-framed outputs."""
    ta, tb = FORMS[form]
    g = _gen(M + 3 * N + 7 * K + ta + tb)
    A, B, bias, C0, P, S = _gemm_inputs(form, M, N, K, regime, g)
    if regime == "exact":
        R.assert_exact_headroom(S + 8, C0)
    Ap, Bp = _poisoned(A), _poisoned(B)
    bias_p = embed(bias[None], "nan", rows_before=0, rows_after=0, ld=N + 16, col0=8, align=False)[1][0]
    worst = {}
    for use_bias in (0, 1):
        v = P + (bias.double() if use_bias else 0)
        Sv = S + (bias.double().abs() if use_bias else 0)
        for dt in (bf16, torch.float32):
            delta = R.delta_det if dt == bf16 else R.delta_prob
            rnd = bf if dt == bf16 else (lambda t: t)
            tag = "bf16" if dt == bf16 else "f32"
            for acc in (0, 1):
                c0 = C0.to(dt)
                for epi in (0, 1):
                    with_pre = None
                    for use_pre in (1, 0):
                        start = c0 if acc else torch.full((M, N), float("nan"), dtype=dt, device=DEV)
                        cbuf, C = embed(start, SENT, rows_before=_guard(N), rows_after=_guard(N))
                        pbuf, pre = embed(torch.full((M, N), float("nan"), dtype=dt, device=DEV), SENT, rows_before=_guard(N), rows_after=_guard(N))
                        cb, pb = cbuf.clone(), pbuf.clone()
                        _gemm(Ap, Bp, bias_p if use_bias else None, C, pre if use_pre else None, M, N, K, ta, tb, epi, acc)
                        what = "%s %s bias%d acc%d epi%d pre%d" % (form, tag, use_bias, acc, epi, use_pre)
                        assert outside_unchanged(cbuf, cb, _guard(N), M, 0, N), (what, "bytes around C were written")
                        if use_pre:
                            assert outside_unchanged(pbuf, pb, _guard(N), M, 0, N), (what, "bytes around pre were written")
                            if regime == "exact":
                                exact(what + ": pre", pre, v)
                            else:
                                r = held(REPORT, "gemm %s pre %s" % (form, tag), pre, v, rnd(v), delta(Sv, K), G=R.floor_g(Sv))
                                worst["pre " + tag] = max(worst.get("pre " + tag, 0.0), r)
                        else:
                            assert same_bits(pbuf, pb), (what, "pre was written without pre_act")
                        if epi == 1 and not use_pre:
                            assert same_bits(C, with_pre), (what, "the run without pre_act differs from the run with it")
                            continue
                        if use_pre:
                            with_pre = C.clone()
                        if epi == 0:
                            ref = v + (c0.double() if acc else 0)
                            if regime == "exact":
                                exact(what + ": C", C, ref)
                            else:
                                Sc = Sv + (c0.double().abs() if acc else 0)
                                r = held(REPORT, "gemm %s C %s" % (form, tag), C, ref, rnd(ref), delta(Sc, K), G=R.floor_g(Sc))
                                worst["C " + tag] = max(worst.get("C " + tag, 0.0), r)
                        else:
                            x = pre.double()                                     # the kernel's own pre-activation, as stored
                            y = R.gelu64(x)
                            ref = y + (c0.double() if acc else 0)
                            d = R.gelu_delta(x, y) + (U * ref.abs() if acc else 0)
                            r = held(REPORT, "gemm %s gelu %s" % (form, tag), C, ref, rnd(ref), d, G=R.floor_g(x))
                            worst["gelu " + tag] = max(worst.get("gelu " + tag, 0.0), r)
    if worst:
        print("[gemm %s %s %dx%dx%d %s] worst error / bound: %s" % (name, form, M, N, K, regime, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


def test_gemm_tn_without_trans_b_is_an_argument_error():
    A = torch.zeros(8, 8, dtype=bf16, device=DEV)
    C = torch.full((8, 8), SENT, dtype=bf16, device=DEV)
    with pytest.raises(HalvaHipError, match="trans_a"):
        _gemm(A, A, None, C, None, 8, 8, 8, 1, 0, 0, 0)
    torch.cuda.synchronize()
    assert bool((C == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# halva_wgrad_accumulate
def wgrad_slabs(M, N, rows, ws_floats):
    """the split of wgrad.h's wgrad_slabs, restated (only the bound's operation count uses it)"""
    tiles = -(-M // 128) * -(-N // 128)
    splits = max(1, min(64, 512 // tiles, ws_floats // (M * N)))
    ksplit = (-(-rows // splits) + 63) // 64 * 64
    return -(-rows // ksplit), ksplit


WGRAD_SHAPES = [(1000, 128, 256, 640, 384), (3428, 512, 128, 1536, 4224), (77, 8, 8, 8, 8), (27424, 384, 4096, 4480, 4480),
                (3000, 256, 4096, 4352, 4352), (1500, 320, 1032, 512, 1104), (2000, 128, 13824, 13952, 13952), (2000, 5120, 128, 15360, 5248),
                # the last k-slab ends one row into a 64-row tile / one row short of one (64 slabs of one tile; 43 slabs of three tiles / 64 of two)
                (4033, 128, 256, 640, 384), (4095, 128, 256, 640, 384), (8193, 128, 256, 640, 384), (8191, 128, 256, 640, 384),
                (65, 128, 128, 136, 128), (63, 128, 128, 136, 128)]


def _windows(rows, M, N, lda, ldb, regime, g, i=0):
    """A [rows, M] and B [rows, N] as column windows of poisoned buffers with 2 rows of poison before and 64 + after them"""
    a0, b0 = (lda - M) // 16 * 8, (ldb - N) // 16 * 8
    if regime == "exact":
        A, B = R.int_tensor((rows, M), g, DEV), R.int_tensor((rows, N), g, DEV)
        C0 = R.int_tensor((M, N), g, DEV, -1024, 1024, torch.float32)
    else:
        A, B = R.rand_tensor(rows, M, g, DEV), R.rand_tensor(rows, N, g, DEV)
        C0 = torch.randn(M, N, generator=g, device=DEV) * math.sqrt(rows)
    Aw = embed(A, "nan", ld=lda, col0=a0, rows_before=2, rows_after=64 + 8 * i)[1]
    Bw = embed(B, "nan", ld=ldb, col0=b0, rows_before=2, rows_after=72 + 8 * i)[1]
    return Aw, Bw, C0


def _framed_ws(ws_floats):
    G = 4096
    full = torch.full((ws_floats + 2 * G,), SENT, device=DEV)
    return full, full[G:G + ws_floats]


def _ws_intact(full, ws_floats):
    G = 4096
    return bool((full[:G] == SENT).all()) and bool((full[G + ws_floats:] == SENT).all())


def _check_wgrad(what, C, C0, Aw, Bw, alpha, regime, splits, P=None, S=None):
    rows = Aw.shape[0]
    P = Aw.double().t() @ Bw.double() if P is None else P
    S = Aw.double().abs().t() @ Bw.double().abs() if S is None else S
    ref = C0.double() + alpha * P
    if regime == "exact":
        R.assert_exact_headroom(S, C0, alpha)
        exact(what, C, ref)
        return 0.0
    St = alpha * S + C0.double().abs()
    return held(REPORT, "wgrad C", C, ref, ref, R.delta_prob(St, rows, splits), G=R.floor_g(St))


@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("rows,M,N,lda,ldb", WGRAD_SHAPES, ids=["r%d-%dx%d-ld%d-%d" % c for c in WGRAD_SHAPES])
def test_wgrad_elementwise(rows, M, N, lda, ldb, regime, monkeypatch):
    """C += alpha A^T B over poisoned column windows, for the default split, a workspace that allows three slabs and one that allows
    one; the LDS-DMA kernel, the register-staged one (HALVA_WGRAD_DMA=0) and the four-stage one (HALVA_WGRAD_KT=32) where the shape
    is eligible - all with the same bits, two runs agreeing bitwise, and nothing written around the workspace."""
    case = WGRAD_SHAPES.index((rows, M, N, lda, ldb))
    alpha = (1.0, 0.5, 0.25)[case % 3]
    g = _gen(rows + M + N)
    Aw, Bw, C0 = _windows(rows, M, N, lda, ldb, regime, g)
    P = Aw.double().t() @ Bw.double()
    S = Aw.double().abs().t() @ Bw.double().abs()
    mn = M * N
    dma = M % 128 == 0 and N % 128 == 0
    default_splits = wgrad_slabs(M, N, rows, 64 * mn)[0]
    worst = 0.0
    for ws_floats in (max(default_splits, 1) * mn, 3 * mn, mn):
        splits = wgrad_slabs(M, N, rows, ws_floats)[0]
        assert splits * mn <= ws_floats
        got = {}
        for mode in (("default", "dma0", "kt32") if dma else ("default",)):
            monkeypatch.delenv("HALVA_WGRAD_DMA", raising=False)
            monkeypatch.delenv("HALVA_WGRAD_KT", raising=False)
            if mode == "dma0":
                monkeypatch.setenv("HALVA_WGRAD_DMA", "0")
            if mode == "kt32":
                monkeypatch.setenv("HALVA_WGRAD_KT", "32")
            runs = []
            for _ in range(2):
                full, ws = _framed_ws(ws_floats)
                cbuf, C = embed(C0, SENT, rows_before=_guard(N), rows_after=_guard(N))
                cb = cbuf.clone()
                _wgrad(Aw, Bw, C, rows, alpha, ws, ws_floats)
                torch.cuda.synchronize()
                what = "wgrad %s ws=%d slabs (%d) alpha=%g" % (mode, ws_floats // mn, splits, alpha)
                assert _ws_intact(full, ws_floats), (what, "floats around the workspace were written")
                assert outside_unchanged(cbuf, cb, _guard(N), M, 0, N), (what, "bytes around C were written")
                runs.append(C.clone())
            assert torch.equal(runs[0], runs[1]), (what, "two runs differ")
            worst = max(worst, _check_wgrad(what, runs[0], C0, Aw, Bw, alpha, regime, splits, P, S))
            got[mode] = runs[0]
        for mode in got:
            assert torch.equal(got[mode], got["default"]), ("wgrad %s differs from the LDS-DMA kernel's bits" % mode, ws_floats // mn)
    if regime == "random":
        print("[wgrad rows=%d %dx%d] worst error / bound %.3f" % (rows, M, N, worst))


@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("group", ["qkv_7b", "down_7b", "gate_up_7b", "odd_shapes"])
def test_wgrad_batch_elementwise(group, regime):
    """One launch pair for a LoRA group's products: the bits of one call per factor, and EVERY item held to float64."""
    rows, d, F, r = 27424, 4096, 11008, 128
    shapes = {"qkv_7b": [(3 * r, d)] + [(d, r)] * 3, "gate_up_7b": [(2 * r, d)] + [(F, r)] * 2, "down_7b": [(r, F), (d, r)],
              "odd_shapes": [(320, 1032), (8, 8)]}[group]
    if group == "odd_shapes":
        rows = 1500
    g = _gen(len(group))
    ws_floats = 48 * 2 ** 20
    items = []
    for i, (M, N) in enumerate(shapes):
        Aw, Bw, C0 = _windows(rows, M, N, M + 16 * (i + 1), N + 32 * (i + 2), regime, g, i)
        items.append((C0, Aw, Bw, (1.0, 0.5, 0.25, 0.5)[i]))
    one = []
    for C0, Aw, Bw, alpha in items:
        C = C0.clone()
        full, ws = _framed_ws(ws_floats)
        _wgrad(Aw, Bw, C, rows, alpha, ws, ws_floats)
        torch.cuda.synchronize()
        assert _ws_intact(full, ws_floats)
        one.append(C)
        del full, ws
    full, ws = _framed_ws(ws_floats)
    framed = [embed(C0, SENT, rows_before=_guard(C0.shape[1]), rows_after=_guard(C0.shape[1])) for C0, _, _, _ in items]
    before = [f[0].clone() for f in framed]
    _wgrad_batch([(f[1], Aw, Bw, alpha) for f, (_, Aw, Bw, alpha) in zip(framed, items)], ws, ws_floats)
    torch.cuda.synchronize()
    assert _ws_intact(full, ws_floats), "floats around the workspace were written"
    worst = 0.0
    for i, ((cbuf, C), cb, (C0, Aw, Bw, alpha)) in enumerate(zip(framed, before, items)):
        M, N = C0.shape
        assert outside_unchanged(cbuf, cb, _guard(N), M, 0, N), (group, i, "bytes around C were written")
        assert torch.equal(C, one[i]), (group, i, "the batch differs from one call per factor")
        worst = max(worst, _check_wgrad("wgrad batch %s item %d" % (group, i), C, C0, Aw, Bw, alpha, regime, wgrad_slabs(M, N, rows, ws_floats)[0]))
    if regime == "random":
        print("[wgrad batch %s] worst error / bound %.3f" % (group, worst))


# One planned path: both entry points run wgrad.h's wgrad_run, which cuts a call's items in order into chunks of at most four whose
# partials fit the workspace side by side.  "Batch equals one call per item" therefore compares two routes through the same kernels; what
# holds the result independently is the float64 bound on every item here and the register-staged kernel's bits (HALVA_WGRAD_DMA=0).
CHUNK_ROWS = 200                        # ends 8 rows into a 64-row tile
T128 = 128 * 128
CHUNK_CASES = {"six": ([(128, 128), (128, 256), (256, 128), (8, 8), (128, 128), (128, 128)], 48 * 2 ** 20),      # more than four items
               "mixed": ([(128, 256), (8, 8), (256, 128)], 48 * 2 ** 20),                                      # LDS-DMA and register-staged items in one chunk
               "ws9": ([(128, 128)] * 3, 9 * T128),     # 4 slabs each (200 rows / 64): two items side by side, the third opens a chunk
               "ws5": ([(128, 128)] * 3, 5 * T128),     # every item its own chunk
               "three": ([(128, 128)] * 3, 48 * 2 ** 20)}


def _batch_against_single_calls(case, regime):
    """the case's items through ONE batch call: nothing written around any C or the workspace, every item the bits of a call of its own
    with the same workspace size and held to float64 -> the batch call's results"""
    shapes, ws_floats = CHUNK_CASES[case]
    rows, g = CHUNK_ROWS, _gen(len(case))
    items = []
    for i, (M, N) in enumerate(shapes):
        Aw, Bw, C0 = _windows(rows, M, N, M + 16, N + 32, regime, g, i)
        items.append((C0, Aw, Bw, (1.0, 0.5, 0.25)[i % 3]))
    full, ws = _framed_ws(ws_floats)
    one = []
    for C0, Aw, Bw, alpha in items:
        one.append(C0.clone())
        _wgrad(Aw, Bw, one[-1], rows, alpha, ws, ws_floats)
        torch.cuda.synchronize()
        assert _ws_intact(full, ws_floats), (case, "floats around the workspace were written")
    framed = [embed(C0, SENT, rows_before=_guard(C0.shape[1]), rows_after=_guard(C0.shape[1])) for C0, _, _, _ in items]
    before = [f[0].clone() for f in framed]
    _wgrad_batch([(f[1], Aw, Bw, alpha) for f, (_, Aw, Bw, alpha) in zip(framed, items)], ws, ws_floats)
    torch.cuda.synchronize()
    assert _ws_intact(full, ws_floats), (case, "floats around the workspace were written")
    for i, ((cbuf, C), cb, (C0, Aw, Bw, alpha)) in enumerate(zip(framed, before, items)):
        M, N = C0.shape
        splits = wgrad_slabs(M, N, rows, ws_floats)[0]
        assert splits * M * N <= ws_floats
        assert outside_unchanged(cbuf, cb, _guard(N), M, 0, N), (case, i, "bytes around C were written")
        assert torch.equal(C, one[i]), (case, i, "the batch differs from one call per item")
        _check_wgrad("wgrad chunks %s item %d" % (case, i), C, C0, Aw, Bw, alpha, regime, splits)
    return [C.clone() for _, C in framed]


@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("case", ["six", "mixed", "ws9", "ws5"])
def test_wgrad_batch_chunks(case, regime):
    """More items than one table holds, a chunk boundary forced by the workspace, and a chunk whose items take different tile kernels."""
    if case in ("ws9", "ws5"):
        assert wgrad_slabs(128, 128, CHUNK_ROWS, CHUNK_CASES[case][1])[0] == 4
    _batch_against_single_calls(case, regime)


@pytest.mark.parametrize("regime", ["exact", "random"])
def test_wgrad_batch_ab_kernels(regime, monkeypatch):
    """The register-staged kernel and the four-stage LDS-DMA kernel through the batch entry: the bits of the default run."""
    monkeypatch.delenv("HALVA_WGRAD_DMA", raising=False)
    monkeypatch.delenv("HALVA_WGRAD_KT", raising=False)
    default = _batch_against_single_calls("three", regime)
    for name, value in (("HALVA_WGRAD_DMA", "0"), ("HALVA_WGRAD_KT", "32")):
        with monkeypatch.context() as m:
            m.setenv(name, value)
            got = _batch_against_single_calls("three", regime)
        for i, (a, b) in enumerate(zip(got, default)):
            assert torch.equal(a, b), ("%s=%s differs from the default run's bits" % (name, value), i)


@pytest.mark.parametrize("bad_lda", [128 - 8, 128 + 4], ids=["lda-below-M", "lda-not-8"])
def test_wgrad_batch_validates_every_item_before_any_launch(bad_lda):
    """An invalid item 2 (its row stride does not cover M / is no multiple of 8): the error names it, and items 0 and 1 - valid, and
    ahead of it - have NOT been added into their C.  (Every pointer is a live allocation; nothing here reaches a kernel.)"""
    rows, ws_floats, g = CHUNK_ROWS, 48 * T128, _gen(7)
    items = []
    for i in range(3):
        Aw, Bw, C0 = _windows(rows, 128, 128, 144, 160, "random", g, i)
        items.append((C0.clone(), Aw, Bw, 1.0))
    arr = _wgrad_items(items)
    arr[2].lda = bad_lda
    full, ws = _framed_ws(ws_floats)
    before = [C.clone() for C, _, _, _ in items]
    with pytest.raises(HalvaHipError, match="item 2"):
        _wgrad_batch(arr, ws, ws_floats)
    torch.cuda.synchronize()
    for i, ((C, _, _, _), b) in enumerate(zip(items, before)):
        assert same_bits(C, b), ("item %d's C was touched by a call that failed" % i)
    assert bool((full == SENT).all()), "the workspace was written by a call that failed"


# ---------------------------------------------------------------------------------------------------------------------------------
# halva_transpose_bf16
@pytest.mark.parametrize("rows,cols,ld_src,ld_dst", [(64, 64, 72, 72), (72, 200, 328, 80), (8, 8, 16, 16), (1000, 136, 264, 1024), (4096, 1152, 1536, 4096)])
def test_transpose_poisoned_source(rows, cols, ld_src, ld_dst):
    g = _gen(rows + cols)
    x = torch.randn(rows, cols, generator=g, device=DEV).to(bf16)
    src = embed(x, "nan", ld=ld_src, col0=0, rows_before=2, rows_after=66)[1]
    dbuf, dst = embed(torch.full((cols, rows), float("nan"), dtype=bf16, device=DEV), SENT, ld=ld_dst, col0=0, rows_before=2, rows_after=66)
    db = dbuf.clone()
    _transpose(src, dst, rows, cols)
    torch.cuda.synchronize()
    assert same_bits(dst.contiguous(), x.t().contiguous())
    assert outside_unchanged(dbuf, db, 2, cols, 0, rows), "the destination outside the window was written"


# ---------------------------------------------------------------------------------------------------------------------------------
# halva_colsum, halva_gelu_bwd
@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("N", [8, 257, 1000])
@pytest.mark.parametrize("M", [1, 5, 127, 129, 8193])
def test_colsum_elementwise(M, N, regime):
    g = _gen(M + N)
    if regime == "exact":
        x = R.int_tensor((M, N), g, DEV)
        out0 = R.int_tensor((1, N), g, DEV, -1024, 1024, torch.float32)
    else:
        x = R.rand_tensor(M, N, g, DEV)
        out0 = torch.randn(1, N, generator=g, device=DEV) * math.sqrt(M)
    xp = _poisoned(x, align=False)
    obuf, out = embed(out0, SENT, ld=N + 16, col0=8, rows_before=1, rows_after=1, align=False)
    ob = obuf.clone()
    _colsum(xp, out, M, N)
    torch.cuda.synchronize()
    assert outside_unchanged(obuf, ob, 1, 1, 8, N), "floats around the sums were written"
    ref = out0.double() + x.double().sum(0, keepdim=True)
    S = out0.double().abs() + x.double().abs().sum(0, keepdim=True)
    if regime == "exact":
        R.assert_exact_headroom(S)
        exact("colsum", out.contiguous(), ref)
    else:
        splits = min(64, -(-M // 128))
        r = held(REPORT, "colsum", out, ref, ref, R.delta_prob(S, -(-M // splits), splits), G=R.floor_g(S))
        print("[colsum %dx%d] worst error / bound %.3f" % (M, N, r))


def test_gelu_bwd_elementwise():
    """every bf16 value in [-12, 12], +-0, +-88, +-1e4, against float64 dy (Phi(x) + x phi(x)); the total is not a multiple of 256 and
    exceeds the 8192 x 256 elements of one pass of the grid-stride loop"""
    allb = torch.arange(-32768, 32768, device=DEV).to(torch.int16).view(bf16)
    grid = allb[torch.isfinite(allb.float()) & (allb.float().abs() <= 12)]
    grid = torch.cat([grid, torch.tensor([0.0, -0.0, 88.0, -88.0, 1e4, -1e4], device=DEV).to(bf16)])
    total = 8192 * 256 + 3 * 256 + 77
    g = _gen(3)
    x = grid[torch.arange(total, device=DEV) % grid.numel()].view(1, total)
    assert int((x.view(torch.int16) == -32768).sum()) > 0                                  # -0 is in
    dy = R.rand_tensor(4, total, g, DEV)[torch.arange(total, device=DEV) % 4, torch.arange(total, device=DEV)].view(1, total)
    dy[0, :grid.numel()] = 1.0
    xp, dyp = _poisoned(x, align=False), _poisoned(dy, align=False)
    hbuf, dh = embed(torch.full((1, total), float("nan"), dtype=bf16, device=DEV), SENT, ld=total + 64, col0=32, rows_before=1, rows_after=1,
                     align=False)
    hb = hbuf.clone()
    _gelu_bwd(dyp, xp, dh, 1, total)
    torch.cuda.synchronize()
    assert outside_unchanged(hbuf, hb, 1, 1, 32, total), "bytes around dh were written"
    x64, d64 = x.double(), dy.double()
    z = x64 * math.sqrt(0.5)
    cdf = 0.5 * torch.erfc(-z)
    phi = torch.exp(-0.5 * x64 * x64) / math.sqrt(2 * math.pi)
    t = cdf + x64 * phi
    ref = d64 * t
    arg = 0.5 * x64 * x64
    e_cdf = 0.5 * (R.E_ERF + U * (1 + torch.erf(z))) + U * x64.abs() * phi + U * cdf
    e_pdf = phi * U * (2 * arg + 8)
    delta = d64.abs() * (e_cdf + x64.abs() * e_pdf + U * x64.abs() * phi + U * t.abs()) + U * ref.abs()
    r = held(REPORT, "gelu_bwd dh", dh, ref, bf(ref), delta, G=R.floor_g(dy, x))
    print("[gelu_bwd total=%d, %d distinct x] worst error / bound %.3f" % (total, grid.numel(), r))


def test_zz_report_gemm_worst_ratios():
    """(runs last in the file) the worst ratio error / bound of every quantity over the random-regime tests above; the exact regime
    has no ratio: it is equality"""
    print("worst error / bound per quantity: " + ", ".join("%s %.3g" % kv for kv in sorted(REPORT.items())))
    for k, v in REPORT.items():
        assert v <= 1.0, k
