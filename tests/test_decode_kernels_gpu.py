"""The two decode kernels (include/halva_hip.h: halva_decode_rope_append, halva_decode_attn) against torch restatements."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda:0")


def _rope_ref(x, cos, sin, pos):
    """rope_qk_kernel's arithmetic on bf16 rows x [B, H, D] at positions pos [B]: fp32 products, one rounding."""
    h = D // 2
    c = cos[pos.long()].float()[:, None, :]
    s = sin[pos.long()].float()[:, None, :]
    x1, x2 = x[..., :h].float(), x[..., h:].float()
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(torch.bfloat16)


def test_rope_append_matches_torch():
    from halva_amd import kernels as K
    dev = _dev()
    B, H, Lcap = 5, 4, 40
    cos, sin = K.rope_tables(D, 64, device=dev)
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(B, 3 * H * D, generator=g, device=dev).to(torch.bfloat16)
    kc = torch.full((B, H, Lcap, D), float("nan"), dtype=torch.bfloat16, device=dev)
    vc = torch.full_like(kc, float("nan"))
    lens = torch.tensor([0, 1, 7, 38, 39], dtype=torch.int32, device=dev)
    before = qkv.clone().view(B, 3, H, D)
    K.decode_rope_append(qkv, cos, sin, kc, vc, lens, H, D)
    torch.cuda.synchronize()
    pos = torch.tensor([0, 1, 7, 38, 39], device=dev)
    q_ref = _rope_ref(before[:, 0], cos, sin, pos)
    k_ref = _rope_ref(before[:, 1], cos, sin, pos)
    q = qkv.view(B, 3, H, D)[:, 0]
    # within 1 ulp of bf16 (fma contraction may differ from torch's separate products)
    assert torch.allclose(q.float(), q_ref.float(), rtol=2 ** -7, atol=1e-6)
    assert torch.equal(qkv.view(B, 3, H, D)[:, 1:], before[:, 1:])           # k and v of the input rows untouched
    assert lens.tolist() == [1, 2, 8, 39, 40]
    for b in range(B):
        p = int(pos[b])
        assert torch.allclose(kc[b, :, p].float(), k_ref[b].float(), rtol=2 ** -7, atol=1e-6)
        assert torch.equal(vc[b, :, p], before[b, 2])
        other = [i for i in range(Lcap) if i != p]
        assert torch.isnan(kc[b, :, other].float()).all() and torch.isnan(vc[b, :, other].float()).all()
    # a full cache is left as it is
    lens_full = torch.full((B,), Lcap, dtype=torch.int32, device=dev)
    k1 = kc.clone()
    K.decode_rope_append(qkv, cos, sin, kc, vc, lens_full, H, D)
    torch.cuda.synchronize()
    assert lens_full.tolist() == [Lcap] * B and torch.equal(kc.view(-1).view(torch.int16), k1.view(-1).view(torch.int16))


def _attn_ref(q, kc, vc, lens):
    """fp64 softmax(q K^T / sqrt(D)) V per (b, h) over the first lens[b] slots."""
    B, H = q.shape[0], kc.shape[1]
    out = torch.zeros(B, H, D, dtype=torch.float64)
    for b in range(B):
        L = int(lens[b])
        k = kc[b, :, :L].double().cpu()
        v = vc[b, :, :L].double().cpu()
        s = torch.einsum("hd,hld->hl", q[b].view(H, D).double().cpu(), k) / math.sqrt(D)
        out[b] = torch.einsum("hl,hld->hd", torch.softmax(s, -1), v)
    return out


def _run_attn(q, kc, vc, lens, H, width=None, ws_fill=None):
    from halva_amd import kernels as K
    B, Lcap = q.shape[0], kc.shape[2]
    ws = torch.empty(K.decode_ws_bytes(B, H, Lcap), dtype=torch.uint8, device=q.device)
    if ws_fill is not None:
        ws.view(torch.float32).fill_(ws_fill)
    return K.decode_attention(q, kc, vc, lens, ws, H, D, width)


def _case(dev, B, H, lens_list, seed, poison=True):
    g = torch.Generator(device=dev).manual_seed(seed)
    Lcap = max(lens_list) + 3
    kc = torch.randn(B, H, Lcap, D, generator=g, device=dev).to(torch.bfloat16)
    vc = torch.randn(B, H, Lcap, D, generator=g, device=dev).to(torch.bfloat16)
    if poison:         # slots at or beyond lens[b] hold NaN / Inf: never read
        for b, L in enumerate(lens_list):
            kc[b, :, L:] = float("nan")
            vc[b, :, L:] = float("inf")
    q = (torch.randn(B, 3 * H * D, generator=g, device=dev) * 2).to(torch.bfloat16)
    lens = torch.tensor(lens_list, dtype=torch.int32, device=dev)
    return q, kc, vc, lens


@pytest.mark.parametrize("B,H", [(1, 2), (5, 2), (5, 32), (16, 32)])
def test_decode_attention_matches_fp64(B, H):
    from halva_amd import kernels as K
    dev = _dev()
    kc_ = K.decode_kc()
    pool = [1, kc_ - 1, kc_, kc_ + 1, 577, 2048, 4097]
    lens_list = [pool[(b * 3 + H) % len(pool)] for b in range(B)]
    if B == 1:
        lens_list = [4097]
    q, kc, vc, lens = _case(dev, B, H, lens_list, seed=B * 100 + H)
    out = _run_attn(q, kc, vc, lens, H, width=H * D + 64, ws_fill=float("nan"))
    torch.cuda.synchronize()
    ref = _attn_ref(q[:, :H * D], kc, vc, lens.cpu())
    got = out[:, :H * D].view(B, H, D).double().cpu()
    assert torch.isfinite(got).all()
    # bf16 output: |err| <= half an ulp of the rounded value + fp32 accumulation noise
    tol = ref.abs() * 2 ** -8 + 1e-4
    err = (got - ref).abs()
    assert (err <= tol).all(), "max err %.3e (worst excess %.3e)" % (float(err.max()), float((err - tol).max()))


def test_decode_attention_poison_and_determinism():
    """NaN / Inf beyond lens[b] and in the unused workspace change nothing; two calls are bitwise equal; row b is bitwise the same
    computed in a batch of 16 and alone."""
    dev = _dev()
    from halva_amd import kernels as K
    kc_ = K.decode_kc()
    H = 32
    lens_list = [1, kc_ - 1, kc_, kc_ + 1, 577, 2048, 4097, 3, 100, 1000, 1500, 2500, 3000, 333, 64, 4000]
    q, kc, vc, lens = _case(dev, 16, H, lens_list, seed=7, poison=False)
    clean = _run_attn(q, kc, vc, lens, H, ws_fill=0.0)
    for b, L in enumerate(lens_list):
        kc[b, :, L:] = float("nan")
        vc[b, :, L:] = float("-inf")
    a = _run_attn(q, kc, vc, lens, H, ws_fill=float("nan"))
    b2 = _run_attn(q, kc, vc, lens, H, ws_fill=float("inf"))
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a, clean) and torch.equal(a, b2)
    for b in (0, 5, 6, 15):
        L = lens_list[b]
        Lc = L + 5          # a cache of another capacity, holding row b alone
        k1 = torch.full((1, H, Lc, D), float("nan"), dtype=torch.bfloat16, device=dev)
        v1 = torch.full_like(k1, float("nan"))
        k1[:, :, :L] = kc[b:b + 1, :, :L]
        v1[:, :, :L] = vc[b:b + 1, :, :L]
        one = _run_attn(q[b:b + 1].contiguous(), k1, v1, lens[b:b + 1].contiguous(), H)
        torch.cuda.synchronize()
        assert torch.equal(one[0], a[b]), "row %d differs alone vs in the batch" % b

