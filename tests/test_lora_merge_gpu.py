"""halva_lora_merge (halva_amd/csrc/gemm.hip): w[n, k] <- bf16(w[n, k] + scale * sum_j B[n, j] A[j, k]) in place on a strided window.

Every element is held to float64 on the kernel's own inputs.  With e the float64 value,

    |out - e|  <=  ulp_bf16(e) / 2  +  (r + 2) 2^-24 (|w| + |scale| sum_j |B[n, j]| |A[j, k]|)

the first term is the one rounding to bf16, the second the fp32 arithmetic in front of it: r - 1 additions inside the accumulator, the
multiplication by scale and the addition of w are r + 1 roundings of at most 2^-24 relative each, on partial sums that the sum of the
magnitudes bounds; r + 2 covers the second-order terms (gamma_{r+1} <= (r + 2) 2^-24 for r <= 128).  Nothing measured enters the bound.

The window sits inside a buffer whose other elements - the columns [K, ldw) of its own rows and guard rows before and after - hold
NaN / +Inf / -Inf; they must come back bit for bit.  The shapes: the three small ones (r = 1, 8, 4: a k-fragment zero-filled up to 16;
N and K no multiples of the 32 x 256 tile), the production layout (256 rows of a [.., 4096 + 64] fused weight, r = 128, scale 2), tile
edges in both dimensions at r = 128, and one window that is not 16-byte aligned with odd strides (the element-wise path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gemm_ref_util import bits, embed, guard_rows, outside_unchanged, same_bits  # noqa: E402

U = 2.0 ** -24
#        N     K    ldw         r   scale
SHAPES = [(33, 17, 24, 1, 0.75),
          (70, 100, 104, 8, 2.0),
          (96, 160, 160, 4, 4.0),
          (256, 4096, 4096 + 64, 128, 2.0),          # production layout
          (130, 1000, 1128, 128, 0.5),               # tile edges in both dimensions
          (5, 9, 11, 3, 1.5)]                        # odd strides, window not 16-byte aligned
IDS = ["%dx%d_ld%d_r%d" % s[:4] for s in SHAPES]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _inputs(N, K, ldw, r, seed):
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(seed)
    w = (torch.randn(N, K, device=dev, generator=g) * 0.05).to(torch.bfloat16)
    w[0, 0] = -0.0
    w[N - 1, K - 1] = 0.0
    B = (torch.randn(N, r, device=dev, generator=g) * 0.1).to(torch.bfloat16)
    A = ((torch.rand(r, K, device=dev, generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
    return w, B, A


def _window(w, ldw):
    """(buffer, window view, rows before): w inside a poisoned [guard + N + guard, ldw] buffer"""
    gr = guard_rows(ldw)
    buf, win = embed(w, "nan", ld=ldw, rows_before=gr, rows_after=gr, align=ldw % 8 == 0)
    return buf, win, gr


def _ulp_bf16(e):
    """one unit in the last place of bf16 at the float64 value e (normal range; the smallest normal's below it)"""
    _, ex = torch.frexp(e.abs())                       # |e| = m 2^ex, m in [0.5, 1): floor(log2 |e|) = ex - 1
    ex = torch.where(e == 0, torch.full_like(ex, -125), ex).clamp_min(-125)
    return torch.ldexp(torch.ones_like(e), ex - 1 - 7)


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def case(request):
    from halva_amd import kernels as K_
    N, K, ldw, r, scale = request.param
    w, B, A = _inputs(N, K, ldw, r, 11 + N)
    buf, win, gr = _window(w, ldw)
    before = buf.clone()
    K_.lora_merge(win, B, A, scale)
    torch.cuda.synchronize()
    return dict(id=IDS[SHAPES.index(request.param)], N=N, K=K, ldw=ldw, r=r, scale=scale, w=w, B=B, A=A, buf=buf, win=win, gr=gr, before=before)


def test_every_element_within_the_derived_bound(case):
    c = case
    w, B, A, s = c["w"].double(), c["B"].double(), c["A"].double(), c["scale"]
    e = w + s * (B @ A)
    S = w.abs() + abs(s) * (B.abs() @ A.abs())
    bound = 0.5 * _ulp_bf16(e) + (c["r"] + 2) * U * S
    got = c["win"].double()
    assert bool(torch.isfinite(got).all())
    err = (got - e).abs()
    print("%s: worst |out - e| / bound = %.3f" % (c["id"], float((err / bound).max())))
    bad = err > bound
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:6].tolist(), got[bad][:4].tolist(), e[bad][:4].tolist())
    # the update is there at all: the merged weight is not the old one
    assert not same_bits(c["win"].contiguous(), c["w"])


def test_memory_outside_the_window_is_untouched(case):
    c = case
    assert outside_unchanged(c["buf"], c["before"], c["gr"], c["N"], 0, c["K"])


def test_two_runs_give_the_same_bits(case):
    from halva_amd import kernels as K_
    c = case
    buf, win, _ = _window(c["w"], c["ldw"])
    K_.lora_merge(win, c["B"], c["A"], c["scale"])
    assert same_bits(buf, c["buf"])


def test_zero_scale_and_zero_B_leave_the_weight_as_it_is(case):
    """scale = 0, and B = 0 - the state right after LoRA init - change no bit of w (a -0.0 included)"""
    from halva_amd import kernels as K_
    c = case
    for B, scale in ((c["B"], 0.0), (torch.zeros_like(c["B"]), c["scale"])):
        buf, win, _ = _window(c["w"], c["ldw"])
        K_.lora_merge(win, B, c["A"], scale)
        assert same_bits(buf, c["before"])


def test_two_targets_of_one_group_do_not_see_each_other():
    """Two row ranges of one fused weight, each merged with its own block of A_cat and its own B (LoraGroup.merge_): the rows of a
    target depend on that target alone - changing the other target's B changes none of their bits.  The second range starts inside a
    32-row tile."""
    from halva_amd import kernels as K_
    N1, N2, K, ldw, r, scale = 40, 33, 100, 104, 8, 2.0
    w, B, A_cat = _inputs(N1 + N2, K, ldw, 2 * r, 5)
    B1, B2 = B[:N1, :r].contiguous(), B[N1:, r:].contiguous()

    def run(Ba, Bb):
        buf, win, gr = _window(w, ldw)
        K_.lora_merge(win[:N1], Ba, A_cat[:r], scale)
        K_.lora_merge(win[N1:], Bb, A_cat[r:], scale)
        return buf, win
    buf0, win0 = run(B1, B2)
    e = w.double()
    e[:N1] += scale * (B1.double() @ A_cat[:r].double())
    e[N1:] += scale * (B2.double() @ A_cat[r:].double())
    S = w.double().abs()
    S[:N1] += scale * (B1.double().abs() @ A_cat[:r].double().abs())
    S[N1:] += scale * (B2.double().abs() @ A_cat[r:].double().abs())
    assert bool(((win0.double() - e).abs() <= 0.5 * _ulp_bf16(e) + (r + 2) * U * S).all())
    _, win1 = run(B1, (B2.float() * -3 + 0.25).to(torch.bfloat16))
    assert same_bits(win1[:N1].contiguous(), win0[:N1].contiguous()) and not same_bits(win1[N1:].contiguous(), win0[N1:].contiguous())
    _, win2 = run((B1.float() * -3 + 0.25).to(torch.bfloat16), B2)
    assert same_bits(win2[N1:].contiguous(), win0[N1:].contiguous()) and not same_bits(win2[:N1].contiguous(), win0[:N1].contiguous())


def test_bad_arguments_are_refused_with_a_message():
    from halva_amd import hip
    dev = _dev()
    lib = hip.load()
    w = torch.zeros(4, 16, dtype=torch.bfloat16, device=dev)
    B = torch.zeros(4, 8, dtype=torch.bfloat16, device=dev)
    A = torch.zeros(8, 16, dtype=torch.bfloat16, device=dev)
    keep = bits(w).clone()
    st = hip.stream_ptr()
    pw, pB, pA = w.data_ptr(), B.data_ptr(), A.data_ptr()
    for args, word in (((None, 16, pB, 8, pA, 16, 4, 16, 8), b"null pointer"),
                       ((pw, 16, None, 8, pA, 16, 4, 16, 8), b"null pointer"),
                       ((pw, 16, pB, 8, None, 16, 4, 16, 8), b"null pointer"),
                       ((pw, 15, pB, 8, pA, 16, 4, 16, 8), b"row strides"),
                       ((pw, 16, pB, 8, pA, 16, 4, 16, 0), b"rank"),
                       ((pw, 16, pB, 8, pA, 16, 0, 16, 8), b"bad sizes")):
        rc = lib.halva_lora_merge(*args, 1.0, st)
        assert rc != 0 and word in lib.halva_last_error(), (args, rc, lib.halva_last_error())
    with pytest.raises(hip.HalvaHipError, match="lora_merge"):
        hip.call("halva_lora_merge", pw, 8, pB, 8, pA, 16, 4, 16, 8, 1.0, st)
    torch.cuda.synchronize()
    assert torch.equal(bits(w), keep)
