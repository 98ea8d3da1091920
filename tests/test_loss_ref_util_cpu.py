"""CPU checks of the float64 loss references (tests/loss_ref_util.py) that the GPU row-wise tests hold the kernels to."""
import torch

import loss_ref_util as L


def _rows(seed, R=6, V=97):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(R, V, generator=g, dtype=torch.float64) * 3).to(torch.bfloat16), g


def test_references_agree_with_float64_log_softmax():
    z, g = _rows(1)
    t = torch.randint(0, z.shape[1], (z.shape[0],), generator=g)
    gout = torch.randn(z.shape[0], generator=g, dtype=torch.float64)
    zz = z.double().requires_grad_(True)
    ls = torch.log_softmax(zz, -1)
    want = ls.gather(1, t[:, None]).squeeze(1)
    (want * gout).sum().backward()
    lp, lse = L.logp_ref(z, t)
    assert torch.allclose(lp, want.detach(), rtol=0, atol=1e-13)
    assert torch.allclose(lse, torch.logsumexp(z.double(), -1), rtol=0, atol=1e-13)
    assert torch.allclose(L.dlogits_ref(z, t, gout), zz.grad, rtol=0, atol=1e-15)
    pol, _ = _rows(2)
    w = torch.tensor([1.0, 0.0, 2.0, 0.5, 1.0, 3.0])
    pp = pol.double().requires_grad_(True)
    lr, lpl = torch.log_softmax(z.double(), -1), torch.log_softmax(pp, -1)
    kl = (lr.exp() * (lr - lpl)).sum(-1) * w.double()
    (kl.sum() * -3.0).backward()
    assert torch.allclose(L.kl_ref(pol, z, w), kl.detach(), rtol=0, atol=1e-13)
    assert torch.allclose(L.dpol_ref(pol, z, w, -3.0), pp.grad, rtol=0, atol=1e-14)


def test_kl_reference_is_exactly_zero_for_equal_and_shifted_rows():
    pol, _ = _rows(3)
    pol = (pol.double() * 4).round().div(4).to(torch.bfloat16)      # quarter grid: exact in bf16 after a shift below
    assert bool((L.kl_ref(pol, pol.clone()) == 0).all())
    c = torch.tensor([0.0, 1.0, -4.0, 8.0, 16.0, -24.0], dtype=torch.float64)[:, None]
    shifted = (pol.double() + c).to(torch.bfloat16)
    assert torch.equal(shifted.double(), pol.double() + c)          # the shift is exact in bf16 at these magnitudes
    assert float(L.kl_ref(pol, shifted).abs().max()) == 0.0
    assert float(L.dpol_ref(pol, shifted).abs().max()) < 1e-16


def test_kl_reference_is_finite_where_fp32_softmax_underflows():
    g = torch.Generator().manual_seed(4)
    pol = torch.randn(4, 300, generator=g, dtype=torch.float64)
    pol[:, 0] += 60
    pol[:, 1] -= 60                                                 # spread > 104 nat
    ref = (pol + 0.01 * torch.randn(4, 300, generator=g, dtype=torch.float64)).to(torch.bfloat16)
    pol = pol.to(torch.bfloat16)
    naive = (ref.float().softmax(-1) * (ref.float().softmax(-1).log() - pol.float().softmax(-1).log())).sum(-1)
    assert not bool(torch.isfinite(naive).all())                    # the reference trainer's fp32 softmax().log() form
    kl = L.kl_ref(pol, ref)
    assert bool(torch.isfinite(kl).all()) and bool((kl >= -1e-15).all())
    assert bool(torch.isfinite(L.kl_bound(pol, ref)).all())


def test_phrase_references_and_lse_bound_scale():
    logp = -torch.rand(2, 5, dtype=torch.float64)
    labels = torch.tensor([[1, -100, 3, 4, 5], [1, 2, 3, 4, -100]])
    signs = torch.tensor([[2, 2, -100, 7, 0], [7, 7, 2, -100, 2]])
    slots = torch.tensor([2, 7])
    acc = L.phrase_sum_ref(logp, labels, signs, slots)
    assert torch.allclose(acc, torch.stack([torch.stack([logp[0, 0], logp[0, 3]]), torch.stack([logp[1, 2], logp[1, 0] + logp[1, 1]])]))
    d = L.phrase_sum_bwd_ref(torch.tensor([[1.0, 2.0], [3.0, 4.0]]), labels, signs, slots)
    assert torch.equal(d, torch.tensor([[1.0, 0, 0, 2, 0], [4, 4, 3, 0, 0]]))
    z, _ = _rows(5)
    shifted = (z.double() + 1024).to(torch.bfloat16)
    b0, b1 = L.lse_bound(z), L.lse_bound(shifted)
    assert bool((b1 < 4.5 * L.U * 1100).all()) and bool((b1 > b0).all())   # scales with max|z| + ln V, not with |lse| alone
