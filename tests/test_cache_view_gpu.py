"""A plain cache is the fork without a prefix (halva_amd/csrc/kvcache.hip: one kernel set over a CacheView): the fork entries over an
EMPTY prefix - prefix_lens all zero - give, bit for bit, what the plain entries give on the same own rows.  H = 2, D = 128, 3 rows, for the
four operations: step append, step attention, rows append, rows attention.  Slots no call may read hold NaN; the one prefix row is NaN
throughout.  Outputs, caches and lens are compared as bits (the poison is NaN, which equals nothing as a number)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

H, D, ROWS = 2, 128, 3
L = 300                          # own capacity: a full 256-key chunk and 44 keys of a second
LPRE = 8                         # the fork entries take no empty parent cache; none of its slots is read
MAX_POS = 512
STEP_LENS = [1, 256, 257]        # one key, an exactly full chunk, one key into the second chunk
PAST = [0, 70, 63]
N, N_NEW = 130, [130, 1, 65]     # across the 128-row query block and the 64-key tile


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda"


def _bits(t):
    return t.contiguous().view(torch.int16)


def _t(v, dev):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _caches(dev, g, lens):
    """K, V [ROWS, H, L, D] filled up to lens[m], NaN behind."""
    k = torch.randn(ROWS, H, L, D, device=dev, generator=g).to(torch.bfloat16)
    v = torch.randn(ROWS, H, L, D, device=dev, generator=g).to(torch.bfloat16)
    for m, n in enumerate(lens):
        k[m, :, n:], v[m, :, n:] = float("nan"), float("nan")
    return k, v


def _prefix(dev):
    """One prefix row of length 0 behind every member: (pk, pv, prefix_lens, prefix_of)."""
    pk = torch.full((1, H, LPRE, D), float("nan"), dtype=torch.bfloat16, device=dev)
    return pk, pk.clone(), _t([0], dev), _t([0] * ROWS, dev)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def test_step_append():
    from halva_amd import kernels as K
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(11)
    cos, sin = K.rope_tables(D, MAX_POS, device=dev)
    lens0 = [0, 255, L]                                        # an empty row, a chunk's last slot, a full row (left untouched)
    k, v = _caches(dev, g, lens0)
    qkv = torch.randn(ROWS, 3 * H * D, device=dev, generator=g).to(torch.bfloat16)
    pk, pv, plens, pof = _prefix(dev)
    ka, va, la, qa = k.clone(), v.clone(), _t(lens0, dev), qkv.clone()
    kb, vb, lb, qb = k.clone(), v.clone(), _t(lens0, dev), qkv.clone()
    K.decode_rope_append(qa, cos, sin, ka, va, la, H, D)
    K.fork_rope_append(qb, cos, sin, plens, pof, kb, vb, lb, H, D)
    torch.cuda.synchronize()
    assert la.tolist() == [1, 256, L] and not _same(qa, qkv)
    assert _same(qa, qb) and _same(ka, kb) and _same(va, vb) and torch.equal(la, lb)


def test_step_attention():
    from halva_amd import kernels as K
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(12)
    k, v = _caches(dev, g, STEP_LENS)
    q = (torch.randn(ROWS, 3 * H * D, device=dev, generator=g) * 2).to(torch.bfloat16)
    pk, pv, plens, pof = _prefix(dev)
    lens = _t(STEP_LENS, dev)
    ws_a = torch.empty(K.decode_ws_bytes(ROWS, H, L), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(K.fork_ws_bytes(ROWS, H, LPRE, L), dtype=torch.uint8, device=dev)
    ws_a.view(torch.float32).fill_(float("nan")), ws_b.view(torch.float32).fill_(float("nan"))
    a = K.decode_attention(q, k, v, lens, ws_a, H, D)
    b = K.fork_decode_attention(q, pk, pv, plens, pof, k, v, lens, ws_b, H, D)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all() and bool(a.float().abs().sum() > 0)
    assert _same(a, b)


@pytest.fixture(scope="module")
def rows():
    """Both sides after the rows append: qkv rotated in place, caches written, lens as they were."""
    from halva_amd import kernels as K
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(13)
    cos, sin = K.rope_tables(D, MAX_POS, device=dev)
    k, v = _caches(dev, g, PAST)
    qkv = torch.randn(ROWS, N, 3 * H * D, device=dev, generator=g).to(torch.bfloat16)
    for m, n in enumerate(N_NEW):
        qkv[m, n:] = float("nan")                              # rows at or beyond n_new are neither read nor written
    pre = _prefix(dev)
    n_new = _t(N_NEW, dev)
    a = dict(k=k.clone(), v=v.clone(), lens=_t(PAST, dev), qkv=qkv.clone())
    b = dict(k=k.clone(), v=v.clone(), lens=_t(PAST, dev), qkv=qkv.clone())
    K.extend_rope_append(a["qkv"], cos, sin, a["k"], a["v"], a["lens"], n_new, H, D)
    K.fork_extend_rope_append(b["qkv"], cos, sin, pre[2], pre[3], b["k"], b["v"], b["lens"], n_new, H, D)
    torch.cuda.synchronize()
    return dict(a=a, b=b, pre=pre, n_new=n_new, qkv0=qkv, k0=k)


def test_rows_append(rows):
    a, b = rows["a"], rows["b"]
    assert not _same(a["qkv"], rows["qkv0"]) and not _same(a["k"], rows["k0"])
    assert a["lens"].tolist() == PAST
    assert _same(a["qkv"], b["qkv"]) and _same(a["k"], b["k"]) and _same(a["v"], b["v"]) and torch.equal(a["lens"], b["lens"])


def test_rows_attention(rows):
    from halva_amd import kernels as K
    a, b, (pk, pv, plens, pof), n_new = rows["a"], rows["b"], rows["pre"], rows["n_new"]
    oa = K.extend_attention(a["qkv"], a["k"], a["v"], a["lens"], n_new, None, H, D)
    ob = K.fork_extend_attention(b["qkv"], pk, pv, plens, pof, b["k"], b["v"], b["lens"], n_new, H, D)
    torch.cuda.synchronize()
    assert torch.isfinite(oa.float()).all()
    for m, n in enumerate(N_NEW):
        assert bool((oa[m, :n].float().abs().sum(-1) > 0).all()) and not bool(oa[m, n:].any())
    assert _same(oa, ob)
    la, lb = K.extend_advance(a["lens"].clone(), n_new, L), K.extend_advance(b["lens"].clone(), n_new, L)
    torch.cuda.synchronize()
    assert la.tolist() == [p + n for p, n in zip(PAST, N_NEW)] and torch.equal(la, lb)
