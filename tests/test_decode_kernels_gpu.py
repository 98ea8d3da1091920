"""The two decode kernels (include/halva_hip.h: halva_decode_rope_append, halva_decode_attn) against torch restatements; the attention
also at the chunk sizes of halva_decode_attn_chunked (64 and 128 keys: two more instantiations of both kernels), on scores hundreds of nats
wide (tests/extend_ref_util.py:wide_inputs - the chunk maxima the combine pass sees lie far apart) and with an empty row in the batch."""
import math

import pytest
import torch

import extend_ref_util as E

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


def _run_attn(q, kc, vc, lens, H, width=None, ws_fill=None, chunk=None):
    """chunk: None = halva_decode_attn, 64 / 128 = halva_decode_attn_chunked; the workspace is the header's formula for that chunk, to the byte."""
    from halva_amd import kernels as K
    B, Lcap = q.shape[0], kc.shape[2]
    nbytes = K.decode_ws_bytes(B, H, Lcap, chunk)
    assert nbytes == B * H * ((Lcap + (chunk or K.decode_kc()) - 1) // (chunk or K.decode_kc())) * (D + 2) * 4
    ws = torch.empty(nbytes, dtype=torch.uint8, device=q.device)
    if ws_fill is not None:
        ws.view(torch.float32).fill_(ws_fill)
    return K.decode_attention(q, kc, vc, lens, ws, H, D, width, kc=chunk)


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


def _assert_fp64(got, ref, what):
    assert torch.isfinite(got).all()
    # bf16 output: |err| <= half an ulp of the rounded value + fp32 accumulation noise
    tol = ref.abs() * 2 ** -8 + 1e-4
    err = (got - ref).abs()
    print("%s: worst error / tolerance %.3f (max err %.3e)" % (what, float((err / tol).max()), float(err.max())))
    assert (err <= tol).all(), "max err %.3e (worst excess %.3e)" % (float(err.max()), float((err - tol).max()))


def _fp64_case(B, H, chunk):
    from halva_amd import kernels as K
    dev = _dev()
    kc_ = chunk or K.decode_kc()
    pool = [1, kc_ - 1, kc_, kc_ + 1, 577, 2048, 4097]
    lens_list = [pool[(b * 3 + H) % len(pool)] for b in range(B)]
    if B == 1:
        lens_list = [4097]
    if B == 8:         # both sides of one, two and three chunks
        lens_list = [kc_ - 1, kc_, kc_ + 1, 2 * kc_ + 1, 2 * kc_, 3 * kc_ - 1, 1, 577]
    q, kc, vc, lens = _case(dev, B, H, lens_list, seed=B * 100 + H)
    out = _run_attn(q, kc, vc, lens, H, width=H * D + 64, ws_fill=float("nan"), chunk=chunk)
    torch.cuda.synchronize()
    ref = _attn_ref(q[:, :H * D], kc, vc, lens.cpu())
    got = out[:, :H * D].view(B, H, D).double().cpu()
    _assert_fp64(got, ref, "decode attention B=%d H=%d chunk=%s" % (B, H, chunk))


@pytest.mark.parametrize("B,H", [(1, 2), (5, 2), (5, 32), (16, 32)])
def test_decode_attention_matches_fp64(B, H):
    _fp64_case(B, H, None)


@pytest.mark.parametrize("chunk", [64, 128, None])
def test_decode_attention_straddling_the_chunk_matches_fp64(chunk):
    _fp64_case(8, 2, chunk)


@pytest.mark.parametrize("B,H", [(1, 2), (5, 2), (5, 32), (16, 32)])
@pytest.mark.parametrize("chunk", [64, 128])
def test_decode_attention_chunked_matches_fp64(chunk, B, H):
    _fp64_case(B, H, chunk)


@pytest.mark.parametrize("chunk", [64, 128, None])
def test_decode_attention_wide_scores_match_fp64(chunk):
    """One query row over 700 keys per profile of extend_ref_util (scores up to ~450 nats): the chunk maxima lie hundreds of log2 units
    apart, so the combine pass's exp2(m_c - M) runs from 1 down to 0."""
    dev = _dev()
    L = 700
    ins = [E.wide_inputs(name, L, 1, seed=E.WIDE_SEEDS[0]) for name in E.WIDE_PROFILES]
    B = len(ins)
    kc = torch.full((B, 1, L + 3, D), float("nan"), dtype=torch.bfloat16, device=dev)
    vc = torch.full((B, 1, L + 3, D), float("inf"), dtype=torch.bfloat16, device=dev)
    for b, (_, Kb, Vb) in enumerate(ins):
        kc[b, :, :L] = Kb.to(dev)
        vc[b, :, :L] = Vb.to(dev)
    q = torch.cat([i[0][0] for i in ins]).to(dev).contiguous()      # [B, D]
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    out = _run_attn(q, kc, vc, lens, 1, ws_fill=float("nan"), chunk=chunk)
    torch.cuda.synchronize()
    ref = torch.stack([E.reference(qb, Kb, Vb, L - 1, 1)[:, 0] for qb, Kb, Vb in ins])      # [B, 1, D]: the last row sees every key
    assert torch.allclose(ref, _attn_ref(q, kc, vc, lens.cpu()), rtol=0, atol=1e-12)
    _assert_fp64(out.view(B, 1, D).double().cpu(), ref, "decode attention, wide scores, chunk=%s" % chunk)


@pytest.mark.parametrize("chunk", [64, 128, None])
def test_decode_attention_empty_row_in_a_batch(chunk):
    """lens[b] = 0 inside a batch: a zero, finite output row; the other rows keep their bits."""
    dev = _dev()
    H = 2
    lens_list = [130, 577, 65, 1]
    q, kc, vc, lens = _case(dev, 4, H, lens_list, seed=17)
    full = _run_attn(q, kc, vc, lens, H, ws_fill=float("nan"), chunk=chunk)
    lens0 = lens.clone()
    lens0[2] = 0
    kc[2], vc[2] = float("nan"), float("nan")          # nothing of an empty row's cache is read
    got = _run_attn(q, kc, vc, lens0, H, ws_fill=float("nan"), chunk=chunk)
    torch.cuda.synchronize()
    assert torch.isfinite(got.float()).all() and not got[2].any()
    assert full[2].any()
    for b in (0, 1, 3):
        assert torch.equal(got[b], full[b]), b


def test_decode_attention_poison_and_determinism():
    """NaN / Inf beyond lens[b] and in the unused workspace change nothing; two calls are bitwise equal; row b is bitwise the same
    computed in a batch of 16 and alone."""
    _poison_case(None)


@pytest.mark.parametrize("chunk", [64, 128])
def test_decode_attention_chunked_poison_and_determinism(chunk):
    _poison_case(chunk)


def _poison_case(chunk):
    dev = _dev()
    from halva_amd import kernels as K
    kc_ = chunk or K.decode_kc()
    H = 32
    lens_list = [1, kc_ - 1, kc_, kc_ + 1, 577, 2048, 4097, 3, 100, 1000, 1500, 2500, 3000, 333, 64, 4000]
    if chunk is not None:
        lens_list[8] = 2 * kc_ + 1

    def _run(*a, **kw):
        return _run_attn(*a, chunk=chunk, **kw)
    q, kc, vc, lens = _case(dev, 16, H, lens_list, seed=7, poison=False)
    clean = _run(q, kc, vc, lens, H, ws_fill=0.0)
    for b, L in enumerate(lens_list):
        kc[b, :, L:] = float("nan")
        vc[b, :, L:] = float("-inf")
    a = _run(q, kc, vc, lens, H, ws_fill=float("nan"))
    b2 = _run(q, kc, vc, lens, H, ws_fill=float("inf"))
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
        one = _run(q[b:b + 1].contiguous(), k1, v1, lens[b:b + 1].contiguous(), H)
        torch.cuda.synchronize()
        assert torch.equal(one[0], a[b]), "row %d differs alone vs in the batch" % b

