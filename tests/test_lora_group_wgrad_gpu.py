"""The weight-gradient routes of _LoraGroupFn.backward (halva_amd/llama.py) on one LoRA group: the group's products as one native
call (the default), one native call per factor (WGRAD_BATCH off), the library GEMM added into main_grad (WGRAD_KERNEL off) and the
library GEMM returned through autograd (sink off).  The references dA = da^T x, dB_g = scale * dy_g^T xa_g are formed in float64 from
the bf16 operands the backward itself used: xa as the forward left it, da as the backward returned it in dxa's LoRA columns."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref_util as R  # noqa: E402
from halva_amd import dpa, llama  # noqa: E402
from lora_group_ref_util import wgrad_operands  # noqa: E402
from test_gemm_elementwise_gpu import wgrad_slabs  # noqa: E402

DEV = "cuda"
bf16 = torch.bfloat16
ROWS, K_IN, OUTS = 200, 256, (256, 256, 256)


def _backward(grp, flat, src, dy, sink):
    """one forward + backward of the group -> (dxa, xa as the forward filled it, {parameter: gradient})"""
    flat.zero_grad()
    params = [grp.A_cat] + grp._Bs()
    for p in params:
        p.grad = None
    grp.grad_sink = sink
    x0 = src.clone().requires_grad_(True)
    xa = x0.clone()
    grp(xa).backward(dy)
    torch.cuda.synchronize()
    if sink:
        assert all(p.grad is None for p in params)
        return x0.grad, xa.detach(), [p.main_grad.clone() for p in params]
    assert not bool(flat.grad.any()), "the sink is off, yet main_grad was written"
    for p in params:
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype
    return x0.grad, xa.detach(), [p.grad.clone() for p in params]


@pytest.mark.parametrize("r", [128, 16], ids=["r128-lds-dma", "r16-register-staged"])
def test_lora_group_weight_gradient_routes_agree(r, monkeypatch):
    g = torch.Generator(device=DEV).manual_seed(r)
    grp = llama.LoraGroup(("q_proj", "k_proj", "v_proj"), K_IN, OUTS, bf16, DEV)
    grp.weight_cat.data[:, :K_IN].copy_(torch.randn(sum(OUTS), K_IN, generator=g, device=DEV) * K_IN ** -0.5)
    grp.attach_lora(r, 2 * r, bf16, DEV, generator=g)
    for B in grp._Bs():
        B.data.copy_(torch.randn(B.shape, generator=g, device=DEV) * 0.05)
    grp.build_dgrad_copy()
    flat = dpa.FlatTrainables([("A_cat", grp.A_cat)] + [("B%d" % i, B) for i, B in enumerate(grp._Bs())])
    src = torch.randn(ROWS, grp.in_width, generator=g, device=DEV).to(bf16)
    dy = torch.randn(ROWS, sum(OUTS), generator=g, device=DEV).to(bf16)
    scale = grp.scale
    assert scale == 2.0

    got = {}
    for name, kernel, batch, sink in (("batched", True, True, True), ("per-factor", True, False, True), ("library", False, True, True),
                                      ("autograd", False, True, False)):
        monkeypatch.setattr(llama, "WGRAD_KERNEL", kernel)
        monkeypatch.setattr(llama, "WGRAD_BATCH", batch)
        got[name] = _backward(grp, flat, src, dy, sink)
    dxa, xa, _ = got["batched"]
    for name, (d, x, _) in got.items():
        assert R.same_bits(d, dxa) and R.same_bits(x, xa), "%s: the weight-gradient route changed dxa" % name

    # (left, right, factor) of every product, in the order of the parameters: the A factors' rows, then each B
    prods = wgrad_operands(dy, xa, dxa, K_IN, OUTS, r, scale)
    assert len(prods) == 4 and prods[0][0].shape == (ROWS, 3 * r) and [p[2] for p in prods] == [1.0, scale, scale, scale]
    for q, (L, Rt, f) in enumerate(prods):
        ref = f * (L.double().t() @ Rt.double())
        S = f * (L.double().abs().t() @ Rt.double().abs())
        M, N = ref.shape
        assert (M % 128 == 0 and N % 128 == 0) == (r == 128)      # r = 128: every product takes the LDS-DMA kernel; r = 16: none does
        a, b = got["batched"][2][q], got["per-factor"][2][q]
        assert R.same_bits(a, b), ("product %d: one call for the group and one call per factor differ" % q)
        splits = wgrad_slabs(M, N, ROWS, 48 * 2 ** 20)[0]
        worst = R.held(None, "native product %d" % q, a, ref, ref, R.delta_prob(S, ROWS, splits), G=R.floor_g(S))
        # library GEMM: the bf16 rounding of torch.mm's output + fp32 accumulation over ROWS terms; the factor is a power of two
        bound = 2.0 ** -8 * ref.abs() + ROWS * 2.0 ** -23 * S
        for name in ("library", "autograd"):
            err = (got[name][2][q].double() - ref).abs()
            assert bool((err <= bound).all()), ("%s product %d" % (name, q), float((err - bound).max()))
        print("[lora group r=%d product %d %dx%d] native worst error / bound %.3f" % (r, q, M, N, worst))
