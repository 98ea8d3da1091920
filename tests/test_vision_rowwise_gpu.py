"""Row- and elementwise checks of the vision side against float64, with poisoned surroundings: halva_layernorm_fwd,
halva_layernorm_bwd_params, halva_downsample2x2 (halva_amd/csrc/vision.hip) and halva_vit_patch_embed / halva_clip_patch_embed
(im2col + the MFMA GEMM of gemm.hip).  Regimes, `held`, `exact` and the embedding helpers: tests/gemm_ref_util.py.  U = 2^-24.

LayerNorm forward (one wave per row; a lane sums 8 ceil(d / 512) elements, then 6 shuffles: n = 8 ceil(d / 512) + 6 terms on the
longest path; LAMBDA = 8, C_FN = 4 as in test_rowops_rowwise_gpu.py).  With mu, sigma^2 the float64 statistics of the bf16 row and
A1 = mean |x|:
  * mean      e_mu = U (LAMBDA sqrt(n) + 2) A1 absolute: the sum, the rounding of 1 / d and the product with it.
  * rstd      E_r = U (LAMBDA / 2 sqrt(n) + 1.5 + C_FN) + e_mu^2 / (2 (sigma^2 + eps)) relative.  Each term (x - mean)^2 carries 3 U (the
              subtraction's rounding twice, the square's once), the sum LAMBDA sqrt(n) U, both halved by the square root; C_FN: the
              product with 1 / d, + eps, rsqrtf.  The error of the mean enters only in second order (sum (x - mu) = 0): it adds e_mu^2 to
              the variance - which is what limits a row with mean >> spread.
  * y         delta = e_mu r |w| + (E_r + 4 U) |(x - mu) r w| + U |b|: the mean's error through the subtraction, rstd's, and one
              rounding each for x - mean, the products with r and w and the final sum (U |y| <= U |term| + U |b|).
  A row of zeros has mean 0 and variance 0 exactly: y = b bit for bit.  stats = NULL gives the same y bits; rows past `rows` of y and
  stats keep their sentinel; d = 8200 is refused.

LayerNorm parameter gradients (one thread per column, min(128, ceil(rows / 64)) slabs of rows, one atomic pair per slab): exact with
integer dy and x, mean = 0 and rstd = 1, and a non-zero prior dw / db.  Random: delta = U (LAMBDA sqrt(n) + 4 + 3) S for dw (three
roundings per term: x - mean, the product with rstd, the product with dy) and U (LAMBDA sqrt(n) + 4) S for db, n = rows of a slab +
slabs, S = the sum of the magnitudes of the terms + |prior|, on the fp32 statistics the kernel is given.

Patch embedding: exact with an integer image, weights and bias against conv2d in float64, and random with the deterministic
delta = 2 (Kp + 2) U S for its bf16 output.  The im2col workspace's padding columns [3 p^2, Kp) are filled with NaN before the
call - the kernel must write zeros there or the NaN reaches the output - and the pixels a valid convolution drops (384 = 27 x 14 + 6)
hold NaN too.  downsample2x2 is a gather: bit exact against its index formula, zeros (+0) where an odd grid is padded.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import gemm_ref_util as R  # noqa: E402
from gemm_ref_util import U, bf, embed, exact, held, outside_unchanged, same_bits  # noqa: E402
from halva_amd.hip import HalvaHipError, call, ptr, stream_ptr  # noqa: E402
from loss_ref_util import C_FN, LAMBDA  # noqa: E402

DEV = "cuda"
bf16 = torch.bfloat16
REPORT = {}
SENT = R.SENT


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _ln_fwd(x, w, b, y, stats, rows, d, eps):
    call("halva_layernorm_fwd", ptr(x), ptr(w), ptr(b), ptr(y), ptr(stats), rows, d, float(eps), stream_ptr())


def _ln_bwd_params(dy, x, stats, dw, db, rows, d):
    call("halva_layernorm_bwd_params", ptr(dy), ptr(x), ptr(stats), ptr(dw), ptr(db), rows, d, stream_ptr())


def _patch_embed(kind, img, wkp, bias, col, out, n, hw, p, d, Kp):
    if kind == "vit":
        call("halva_vit_patch_embed", ptr(img), ptr(wkp), ptr(bias), ptr(col), ptr(out), n, hw, p, d, Kp, stream_ptr())
    else:
        call("halva_clip_patch_embed", ptr(img), ptr(wkp), ptr(col), ptr(out), n, hw, p, d, Kp, stream_ptr())


def _downsample(x, out, n, g, c):
    call("halva_downsample2x2", ptr(x), ptr(out), n, g, c, stream_ptr())


def _poisoned(x, align=True):
    g = R.guard_rows(x.shape[1], 2 * x.shape[1] + 64)
    return embed(x, "nan", rows_before=g, rows_after=g, align=align)[1]


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm forward
LN = [(d, rows) for d in (8, 64, 1024, 1152, 4608, 8192) for rows in (1, 3, 5, 4099)]


def _ln_inputs(rows, d, g):
    """rows of rand_tensor (row 1 all zero, 1e3- and 1e-3-scaled rows), row 4 with mean >> spread, row 5 a non-zero constant"""
    x = R.rand_tensor(rows, d, g, DEV).float()
    if rows > 4:
        x[4] = 1000 + torch.randn(d, generator=g, device=DEV)
    if rows > 5:
        x[5] = 3.0
    w = (1 + 0.1 * torch.randn(d, generator=g, device=DEV)).to(bf16)
    b = (0.1 * torch.randn(d, generator=g, device=DEV)).to(bf16)
    return x.to(bf16), w, b


@pytest.mark.parametrize("d,rows", LN, ids=["d%d-r%d" % c for c in LN])
def test_layernorm_fwd_rowwise(d, rows):
    eps = 1e-6 if d in (1152, 4608) else 1e-5                 # SigLIP's / nn.LayerNorm's
    x, w, b = _ln_inputs(rows, d, _gen(d + rows))
    xp, wp, bp = _poisoned(x), _poisoned(w[None])[0], _poisoned(b[None])[0]
    nan_y = torch.full((rows, d), float("nan"), dtype=bf16, device=DEV)
    ybuf, y = embed(nan_y, SENT, rows_before=2, rows_after=4)
    sbuf, stats = embed(torch.full((rows, 2), float("nan"), device=DEV), SENT, rows_before=8, rows_after=4)
    yb, sb = ybuf.clone(), sbuf.clone()
    _ln_fwd(xp, wp, bp, y, stats, rows, d, eps)
    torch.cuda.synchronize()
    assert outside_unchanged(ybuf, yb, 2, rows, 0, d), "rows around y were written"
    assert outside_unchanged(sbuf, sb, 8, rows, 0, 2), "rows around stats were written"
    y2buf, y2 = embed(nan_y, SENT, rows_before=2, rows_after=4)
    _ln_fwd(xp, wp, bp, y2, None, rows, d, eps)
    torch.cuda.synchronize()
    assert same_bits(y2buf, ybuf), "stats = NULL changed y"
    x64, w64, b64 = x.double(), w.double(), b.double()
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    mu = x64.mean(-1, keepdim=True)
    var = ((x64 - mu) ** 2).mean(-1, keepdim=True)
    r64 = 1.0 / torch.sqrt(var + eps32)
    n = 8 * math.ceil(d / 512) + 6
    e_mu = U * (LAMBDA * math.sqrt(n) + 2) * x64.abs().mean(-1, keepdim=True)
    E_r = U * (LAMBDA / 2 * math.sqrt(n) + 1.5 + C_FN) + e_mu ** 2 / (2 * (var + eps32))
    a = held(REPORT, "layernorm mean", stats[:, :1], mu, mu, e_mu / 2)            # (held's 2 delta = e_mu)
    c = held(REPORT, "layernorm rstd", stats[:, 1:], r64, r64, E_r * r64 / 2)
    term = (x64 - mu) * r64 * w64
    yref = term + b64
    delta = e_mu * r64 * w64.abs() + (E_r + 4 * U) * term.abs() + U * b64.abs()
    e = held(REPORT, "layernorm y", y, yref, bf(yref), delta, G=R.floor_g(x, w, b))
    if rows > 1:
        assert same_bits(y[1], b), "an all-zero row must give y = b exactly"
        assert float(stats[1, 0]) == 0.0
    print("[layernorm d=%d rows=%d] worst error / bound: mean %.3f, rstd %.3f, y %.3f" % (d, rows, a, c, e))


def test_layernorm_fwd_refuses_rows_that_do_not_fit_the_registers():
    d = 8200
    x = torch.zeros(1, d, dtype=bf16, device=DEV)
    y = torch.full((1, d), SENT, dtype=bf16, device=DEV)
    with pytest.raises(HalvaHipError, match="layernorm_fwd"):
        _ln_fwd(x, x[0], x[0], y, None, 1, d, 1e-5)
    torch.cuda.synchronize()
    assert bool((y == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# LayerNorm parameter gradients
LNB = [(rows, d) for rows in (1, 63, 65, 8193) for d in (40, 1000, 4608 + 8)]


@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("rows,d", LNB, ids=["r%d-d%d" % c for c in LNB])
def test_layernorm_bwd_params_elementwise(rows, d, regime):
    g = _gen(rows + d)
    if regime == "exact":
        dy, x = R.int_tensor((rows, d), g, DEV), R.int_tensor((rows, d), g, DEV)
        stats = torch.tensor([0.0, 1.0], device=DEV).repeat(rows, 1)
        dw0 = R.int_tensor((1, d), g, DEV, -1024, 1024, torch.float32)
        db0 = R.int_tensor((1, d), g, DEV, -1024, 1024, torch.float32)
    else:
        dy, x = R.rand_tensor(rows, d, g, DEV), R.rand_tensor(rows, d, g, DEV)
        mu = x.double().mean(-1, keepdim=True)
        r = 1.0 / torch.sqrt(((x.double() - mu) ** 2).mean(-1, keepdim=True) + 1e-5)
        stats = torch.cat([mu, r], 1).float()
        dw0 = torch.randn(1, d, generator=g, device=DEV) * math.sqrt(rows)
        db0 = torch.randn(1, d, generator=g, device=DEV) * math.sqrt(rows)
    dyp, xp = _poisoned(dy, align=False), _poisoned(x, align=False)
    stp = embed(stats, "nan", rows_before=8, rows_after=8)[1]
    wbuf, dw = embed(dw0, SENT, ld=d + 16, col0=8, rows_before=1, rows_after=1, align=False)
    bbuf, db = embed(db0, SENT, ld=d + 16, col0=8, rows_before=1, rows_after=1, align=False)
    wb, bb = wbuf.clone(), bbuf.clone()
    _ln_bwd_params(dyp, xp, stp, dw, db, rows, d)
    torch.cuda.synchronize()
    assert outside_unchanged(wbuf, wb, 1, 1, 8, d) and outside_unchanged(bbuf, bb, 1, 1, 8, d), "floats around dw / db were written"
    m64, r64 = stats[:, :1].double(), stats[:, 1:].double()
    tw = dy.double() * (x.double() - m64) * r64
    refw = dw0.double() + tw.sum(0, keepdim=True)
    refb = db0.double() + dy.double().sum(0, keepdim=True)
    Sw = dw0.double().abs() + tw.abs().sum(0, keepdim=True)
    Sb = db0.double().abs() + dy.double().abs().sum(0, keepdim=True)
    if regime == "exact":
        R.assert_exact_headroom(Sw)
        exact("dw", dw.contiguous(), refw)
        exact("db", db.contiguous(), refb)
    else:
        splits = min(128, -(-rows // 64))
        per = -(-rows // splits)
        a = held(REPORT, "layernorm dw", dw, refw, refw, R.delta_prob(Sw, per, splits) + 3 * U * Sw, G=R.floor_g(Sw))
        c = held(REPORT, "layernorm db", db, refb, refb, R.delta_prob(Sb, per, splits), G=R.floor_g(Sb))
        print("[layernorm_bwd_params rows=%d d=%d] worst error / bound: dw %.3f, db %.3f" % (rows, d, a, c))


# ---------------------------------------------------------------------------------------------------------------------------------
# patch embedding
PE = [("vit", 28, 3, 136, 592), ("vit", 48, 3, 136, 640), ("vit", 336, 2, 136, 592), ("vit", 384, 1, 1160, 592),
      ("clip", 28, 3, 136, 640), ("clip", 336, 2, 264, 592)]


@pytest.mark.parametrize("regime", ["exact", "random"])
@pytest.mark.parametrize("kind,hw,n,d,Kp", PE, ids=["%s-hw%d-n%d-d%d-Kp%d" % c for c in PE])
def test_patch_embed_elementwise(kind, hw, n, d, Kp, regime):
    p = 14
    K = 3 * p * p
    np1 = hw // p
    used = np1 * p
    g = _gen(hw + n + d + Kp)
    if regime == "exact":
        img = R.int_tensor((n * 3 * hw, hw), g, DEV)
        w = R.int_tensor((d, K), g, DEV)
        bias = R.int_tensor((1, d), g, DEV)
    else:
        img = R.rand_tensor(n * 3 * hw, hw, g, DEV)
        w = (0.05 * torch.randn(d, K, generator=g, device=DEV)).to(bf16)
        bias = torch.randn(1, d, generator=g, device=DEV).to(bf16)
    img = img.view(n, 3, hw, hw).clone()
    clean = img[:, :, :used, :used].contiguous()
    img[:, :, used:, :] = float("nan")                      # what a valid convolution drops is never read
    img[:, :, :, used:] = float("nan")
    imgp = _poisoned(img.view(n * 3 * hw, hw), align=False)
    wkp = torch.zeros(d, Kp, dtype=bf16, device=DEV)
    wkp[:, :K] = w
    wkp = _poisoned(wkp)
    rows = n * np1 * np1
    col0 = torch.zeros(rows, Kp, dtype=bf16, device=DEV)
    col0[:, K:] = float("nan")                              # the kernel must write zeros here
    cbuf, col = embed(col0, SENT, rows_before=2, rows_after=2)
    obuf, out = embed(torch.full((rows, d), float("nan"), dtype=bf16, device=DEV), SENT, rows_before=2, rows_after=2)
    cb, ob = cbuf.clone(), obuf.clone()
    use_bias = kind == "vit"
    _patch_embed(kind, imgp, wkp, _poisoned(bias, align=False) if use_bias else None, col, out, n, hw, p, d, Kp)
    torch.cuda.synchronize()
    assert outside_unchanged(cbuf, cb, 2, rows, 0, Kp) and outside_unchanged(obuf, ob, 2, rows, 0, d), "bytes around the workspace / output were written"
    assert bool((col[:, K:] == 0).all()), "the workspace's padding columns are not zero"
    w4 = w.double().cpu().view(d, 3, p, p)
    ref = F.conv2d(clean.double().cpu(), w4, bias[0].double().cpu() if use_bias else None, stride=p).flatten(2).transpose(1, 2)
    ref = ref.reshape(rows, d).to(DEV)
    if regime == "exact":
        assert 64 * K + 8 < R.EXACT_LIMIT
        exact("patch embed", out.contiguous(), ref)
    else:
        S = F.conv2d(clean.double().abs().cpu(), w4.abs(), bias[0].double().abs().cpu() if use_bias else None, stride=p).flatten(2).transpose(1, 2)
        S = S.reshape(rows, d).to(DEV)
        r = held(REPORT, "%s_patch_embed" % kind, out, ref, bf(ref), R.delta_det(S, Kp), G=R.floor_g(S))
        print("[%s_patch_embed hw=%d n=%d d=%d Kp=%d] worst error / bound %.3f" % (kind, hw, n, d, Kp, r))


def test_clip_patch_embed_refuses_a_trailing_partial_patch():
    x = torch.zeros(3 * 48 * 48 + 64, dtype=bf16, device=DEV)
    w = torch.zeros(8, 592, dtype=bf16, device=DEV)
    col = torch.zeros(9, 592, dtype=bf16, device=DEV)
    out = torch.full((9, 8), SENT, dtype=bf16, device=DEV)
    with pytest.raises(HalvaHipError, match="clip_patch_embed"):
        _patch_embed("clip", x, w, None, col, out, 1, 48, 14, 8, 592)
    torch.cuda.synchronize()
    assert bool((out == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# downsample2x2
DS = [(g, n, c) for g in (1, 2, 27, 24) for n in (1, 3) for c in (8, 1152)]


@pytest.mark.parametrize("g,n,c", DS, ids=["g%d-n%d-c%d" % t for t in DS])
def test_downsample2x2_is_its_index_formula(g, n, c):
    G = (g + 1) // 2
    x = torch.randn(n * g * g, c, generator=_gen(g + n + c), device=DEV).to(bf16)
    x[x == 0] = 1.0                                         # (so that a zero in the output is a padded position)
    xp = _poisoned(x)
    obuf, out = embed(torch.full((n * G * G, 4 * c), float("nan"), dtype=bf16, device=DEV), SENT, rows_before=2, rows_after=4)
    ob = obuf.clone()
    _downsample(xp, out, n, g, c)
    torch.cuda.synchronize()
    assert outside_unchanged(obuf, ob, 2, n * G * G, 0, 4 * c), "rows around the output were written"
    # out[n, b2 G + a2, (2 f + e) c + ch] = x[n, (2 a2 + f) g + (2 b2 + e), ch], zero where 2 a2 + f or 2 b2 + e reaches g
    pad = torch.zeros(n, 2 * G, 2 * G, c, dtype=bf16, device=DEV)
    pad[:, :g, :g] = x.view(n, g, g, c)
    ref = pad.view(n, G, 2, G, 2, c).permute(0, 3, 1, 2, 4, 5).reshape(n * G * G, 4 * c)      # (n, b2, a2, f, e, ch)
    assert same_bits(out.contiguous(), ref.contiguous())
    assert int((R.bits(out) == 0).sum()) == n * ((2 * G) ** 2 - g * g) * c, "exact +0 at the padded row and column of an odd grid, nowhere else"


def test_zz_report_vision_worst_ratios():
    """(runs last in the file) the worst ratio error / bound of every quantity over the random-regime tests above"""
    print("worst error / bound per quantity: " + ", ".join("%s %.3g" % kv for kv in sorted(REPORT.items())))
    for k, v in REPORT.items():
        assert v <= 1.0, k
