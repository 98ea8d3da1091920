"""The surface the three KV caches share (halva_amd/decode.py: KVCache, ForkCache, BeamCache - attend_step, attend_rows, rows, room), without a
GPU: the kernel wrappers are replaced by recorders, and each cache must make exactly the calls, in the order and with the tensors, that
DecoderLayer's decode / fork_decode / beam_decode / extend / fork_extend closures made before the caches took them over."""
from types import SimpleNamespace

import pytest
import torch

H, D, W, LAYERS = 2, 128, 320, 2
WRAPPERS = ("decode_rope_append", "decode_attention", "extend_rope_append", "extend_attention", "extend_advance", "fork_rope_append",
            "fork_decode_attention", "beam_decode_attention", "fork_extend_rope_append", "fork_extend_attention", "beam_advance")


def _stack():
    from halva_amd import decode as DEC
    cfg = SimpleNamespace(num_attention_heads=H, hidden_size=H * D, num_hidden_layers=LAYERS)
    lm = SimpleNamespace(config=cfg, embed_tokens=torch.nn.Embedding(8, 4), layers=[], _rope={},
                         rope=lambda n, dev: (torch.zeros(max(n, 16), 2), torch.zeros(max(n, 16), 2)))
    return DEC.DecodeStack(lm, torch.zeros(8, 4), False)


def _caches():
    """A KVCache of 2 rows over 12 slots holding 5 and 7 rows, a ForkCache of 3 members and a BeamCache of 2 x 2 beams over it."""
    from halva_amd import decode as DEC
    kv = DEC.KVCache(_stack(), 2, 12, "cpu")
    kv.lens += torch.tensor([5, 7], dtype=torch.int32)
    kv.filled = 7
    return kv, DEC.ForkCache(kv, [0, 0, 1], 4, [5, 7]), DEC.BeamCache(kv, 2, 2, 4, [5, 7])


@pytest.fixture
def calls(monkeypatch):
    """Every wrapper a cache may call records (name, args) and hands back a value of its own."""
    from halva_amd import kernels as K
    rec = []

    def recorder(name):
        def fn(*args):
            rec.append((name, args))
            return (name, len(rec))
        return fn
    for name in WRAPPERS:
        monkeypatch.setattr(K, name, recorder(name))
    monkeypatch.setattr(K, "call", lambda *a: pytest.fail("a native call behind the recorders"))
    return rec


def _same(got, want):
    if isinstance(want, torch.Tensor):
        return isinstance(got, torch.Tensor) and got.data_ptr() == want.data_ptr() and got.shape == want.shape and got.stride() == want.stride()
    return got is want if want is None else got == want


def _check(rec, want):
    assert [name for name, _ in rec] == [name for name, _ in want]
    for (name, got), (_, args) in zip(rec, want):
        assert len(got) == len(args), name
        for j, (g, w) in enumerate(zip(got, args)):
            assert _same(g, w), (name, j)


@pytest.mark.parametrize("layer", range(LAYERS))
def test_kv_cache_attends_as_decode_and_extend_did(calls, layer):
    c, _, _ = _caches()
    qkv, n_new = torch.zeros(2, 3 * H * D), torch.ones(2, dtype=torch.int32)
    kc, vc, lens = c.k[layer], c.v[layer], c.lens[layer]
    assert c.attend_step(layer, qkv, H, D, W) == ("decode_attention", 2)
    _check(calls, [("decode_rope_append", (qkv, c.cos, c.sin, kc, vc, lens, H, D)),
                   ("decode_attention", (qkv, kc, vc, lens, c.ws, H, D, W))])
    del calls[:]
    assert c.attend_rows(layer, qkv, n_new, H, D, W) == ("extend_attention", 2)
    _check(calls, [("extend_rope_append", (qkv, c.cos, c.sin, kc, vc, lens, n_new, H, D)),
                   ("extend_attention", (qkv, kc, vc, lens, n_new, None, H, D, W)),
                   ("extend_advance", (lens, n_new, 12))])
    assert (c.rows, c.room) == (2, 12)


@pytest.mark.parametrize("layer", range(LAYERS))
def test_fork_cache_attends_as_fork_decode_and_fork_extend_did(calls, layer):
    par, f, _ = _caches()
    qkv, n_new = torch.zeros(3, 3 * H * D), torch.ones(3, dtype=torch.int32)
    pk, pv, kc, vc, lens = par.k[layer], par.v[layer], f.k[layer], f.v[layer], f.own_lens[layer]
    assert f.attend_step(layer, qkv, H, D, W) == ("fork_decode_attention", 2)
    _check(calls, [("fork_rope_append", (qkv, f.cos, f.sin, f.prefix_lens, f.prefix_of, kc, vc, lens, H, D)),
                   ("fork_decode_attention", (qkv, pk, pv, f.prefix_lens, f.prefix_of, kc, vc, lens, f.ws, H, D, W))])
    del calls[:]
    assert f.attend_rows(layer, qkv, n_new, H, D, W) == ("fork_extend_attention", 2)
    _check(calls, [("fork_extend_rope_append", (qkv, f.cos, f.sin, f.prefix_lens, f.prefix_of, kc, vc, lens, n_new, H, D)),
                   ("fork_extend_attention", (qkv, pk, pv, f.prefix_lens, f.prefix_of, kc, vc, lens, n_new, H, D, W)),
                   ("extend_advance", (lens, n_new, 4))])
    assert (f.rows, f.room, f.Lcap) == (3, 4, 4) and f.lens is f.own_lens


@pytest.mark.parametrize("cur", (0, 1))
def test_beam_cache_attends_through_its_table_and_takes_no_rows(calls, cur):
    par, _, b = _caches()
    b.cur = cur
    qkv = torch.zeros(4, 3 * H * D)
    pk, pv, kc, vc, lens = par.k[1], par.v[1], b.k[1], b.v[1], b.own_lens[1]
    assert b.attend_step(1, qkv, H, D, W) == ("beam_decode_attention", 2)
    _check(calls, [("fork_rope_append", (qkv, b.cos, b.sin, b.prefix_lens, b.prefix_of, kc, vc, lens, H, D)),
                   ("beam_decode_attention", (qkv, pk, pv, b.prefix_lens, b.prefix_of, kc, vc, lens, b.anc[cur], b.ws, H, D, W))])
    del calls[:]
    with pytest.raises(NotImplementedError):
        b.attend_rows(1, qkv, torch.ones(4, dtype=torch.int32), H, D, W)
    assert calls == [] and (b.rows, b.room) == (4, 4)


def test_decoder_layer_hands_the_projection_to_the_cache():
    from halva_amd.llama import DecoderLayer
    seen = []
    layer = SimpleNamespace(H=H, D=D, o=SimpleNamespace(in_width=W), _block=lambda x, attend, use_lora, own_x, rows: (attend(x), use_lora, own_x, rows))
    cache = SimpleNamespace(attend_step=lambda *a: seen.append(("step", a)) or "s", attend_rows=lambda *a: seen.append(("rows", a)) or "r")
    assert DecoderLayer.decode(layer, "qkv", cache, 3, False) == ("s", False, True, None)
    assert DecoderLayer.extend(layer, "qkv", cache, 3, "n_new_d", True, "top") == ("r", True, True, "top")
    assert seen == [("step", (3, "qkv", H, D, W)), ("rows", (3, "qkv", "n_new_d", H, D, W))]


def test_extend_on_a_beam_cache_is_refused_before_any_launch(calls):
    from halva_amd import decode as DEC
    _, _, b = _caches()
    b.filled = 1
    with pytest.raises(NotImplementedError):
        DEC.extend(_stack(), b, torch.zeros(4, 2, 4), [1, 1, 1, 1])
    assert calls == [] and b.filled == 1


def test_beam_decode_step_on_a_full_cache_leaves_the_table_alone(calls):
    from halva_amd import decode as DEC
    _, _, b = _caches()
    b.anc.copy_(torch.arange(b.anc.numel(), dtype=torch.int32).view_as(b.anc))
    before = b.anc.clone()
    b.filled, b.cur = 4, 1
    with pytest.raises(RuntimeError, match="KV cache full"):
        DEC.beam_decode_step(_stack(), b, torch.zeros(4, dtype=torch.long), torch.zeros(4, dtype=torch.int32))
    assert calls == [] and (b.filled, b.cur) == (4, 1) and torch.equal(b.anc, before)
