"""Forks without a GPU (halva_amd/decode.py: ForkCache, DecodeSession.fork, ForkedSession; the halva_fork_* entry points): the host rules,
the pending-token bookkeeping against a scripted stand-in for the model (the style of tests/test_session_cpu.py), the C ABI's argument
errors, and tests/fork_ref_util.py's references against tests/extend_ref_util.py's on the concatenated keys."""
import os
import re
from types import SimpleNamespace

import pytest
import torch

import extend_ref_util as E
import fork_ref_util as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 32


# ------------------------------------------------------------------------------------------------
def test_decode_reference_is_extend_ref_utils_on_the_concatenated_keys():
    g = torch.Generator().manual_seed(1)
    mk = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16)      # noqa: E731
    for plen, olen in ((1, 0), (5, 1), (300, 257), (64, 64)):
        q, Kp, Vp, Ko, Vo = mk(2, 128), mk(2, plen, 128), mk(2, plen, 128), mk(2, olen, 128), mk(2, olen, 128)
        got = F.decode_reference(q, Kp, Vp, Ko, Vo)
        L = plen + olen
        want = E.reference(q[:, None], torch.cat([Kp, Ko], 1), torch.cat([Vp, Vo], 1), L - 1, 1)[:, 0]      # the last row sees every key
        assert torch.allclose(got, want, rtol=0, atol=1e-12), (plen, olen)


def test_extend_operands_put_the_prefix_in_front():
    Kp, Ko = torch.arange(10.)[None, :, None].expand(1, 10, 2), 100 + torch.arange(8.)[None, :, None].expand(1, 8, 2)
    K, V, past = F.extend_operands(Kp, Kp, 7, Ko, Ko, 3, 4)
    assert past == 10 and K[0, :, 0].tolist() == [0, 1, 2, 3, 4, 5, 6, 100, 101, 102, 103, 104, 105, 106]


@pytest.mark.parametrize("name", E.WIDE_PROFILES)
def test_wide_inputs_are_admissible_with_the_prefix_tiles_in_front(name):
    """The inputs of test_fork_kernels_gpu.py:test_extend_wide_scores_against_float64 (prefix 128, own past 37, 300 new rows) through
    extend_ref_util.emulate: the documented per-tile arithmetic meets the row bound on them, and a walk that drops the rescale does not on the
    profiles that move the exponent reference."""
    plen, past, m = 128, 37, 300
    q, K, V = E.wide_inputs(name, plen + past + m, m, seed=E.WIDE_SEEDS[0])
    Kp, Vp, Ko, Vo = K[:, :plen], V[:, :plen], K[:, plen:], V[:, plen:]
    Kc, Vc, p = F.extend_operands(Kp, Vp, plen, Ko, Vo, past, m)
    assert torch.equal(Kc, K) and p == plen + past
    ref, mdl = E.reference(q, K, V, p, m), E.model(q, K, V, p, m)
    out, moves = F.emulate_fork(q, Kp, Vp, plen, Ko, Vo, past, m)
    ek, em, nr = E.row_errors(out, ref, mdl)
    assert float((ek / E.row_bound(em, nr)).max()) <= 1.0
    if name in ("up", "spike_late"):
        assert moves > 0
        bad, _ = F.emulate_fork(q, Kp, Vp, plen, Ko, Vo, past, m, rescale=False)
        ek, em, nr = E.row_errors(bad, ref, mdl)
        assert float((ek / E.row_bound(em, nr)).max()) > 10.0


def test_groups_helper():
    assert F.groups([1, 2, 3], skip=(1,)) == [0, 2, 2, 3, 3, 3]


# ------------------------------------------------------------------------------------------------
# host rules
def _parent(lens, Lcap=64, layers=2, cos_rows=None):
    B = len(lens)
    kv = [torch.zeros(B, 2, Lcap, 128, dtype=torch.bfloat16) for _ in range(layers)]
    made = []

    def rope(n, dev):
        made.append(n)
        return torch.zeros(n, 2), torch.zeros(n, 2)
    par = SimpleNamespace(B=B, H=2, D=128, Lcap=Lcap, k=kv, v=kv, lens=torch.tensor([list(lens)] * layers, dtype=torch.int32), filled=max(lens),
                          cos=torch.zeros(cos_rows or Lcap, 2), sin=torch.zeros(cos_rows or Lcap, 2), rope=rope)
    return par, made


def test_fork_cache_rules():
    from halva_amd import decode as DEC
    par, made = _parent([5, 9, 3])
    for bad in ([1, 0], [0, 3], [-1, 0], []):
        with pytest.raises(ValueError):
            DEC.ForkCache(par, bad, 4)
    with pytest.raises(ValueError):
        DEC.ForkCache(par, [0], 0)
    with pytest.raises(ValueError):
        DEC.ForkCache(par, [0, 1], 4, [5, 0, 3])          # a forked row without rows
    with pytest.raises(ValueError):
        DEC.ForkCache(par, [0], 4, [5, 9])
    f = DEC.ForkCache(par, [0, 0, 2], 4, [5, 9, 3])
    assert (f.M, f.P, f.Lown) == (3, 3, 4) and f.prefix_of.tolist() == [0, 0, 2] and f.prefix_lens.tolist() == [5, 9, 3]
    assert f.prefix_of.dtype == torch.int32 and f.prefix_lens.dtype == torch.int32
    assert [tuple(t.shape) for t in f.k] == [(3, 2, 4, 128)] * 2 and tuple(f.own_lens.shape) == (2, 3) and not f.own_lens.any()
    assert f.cos is par.cos and made == []                # 5 + 4 rows fit the parent's tables
    assert f.ws.numel() >= DEC.K.fork_ws_bytes(3, 2, 64, 4) > 0
    assert DEC.ForkCache(par, [1], 4).prefix_lens.tolist() == [5, 9, 3]          # None: read from the parent
    # the tables are re-sized when max(prefix_lens) + Lown outgrows them - over the rows that have a member
    par2, made2 = _parent([60, 9], cos_rows=64)
    assert DEC.ForkCache(par2, [1], 50).cos is par2.cos and made2 == []
    assert DEC.ForkCache(par2, [0, 1], 50).cos.shape[0] == 110 and made2 == [110]


def test_fork_cache_refuses_tables_that_stay_short():
    from halva_amd import decode as DEC
    par, _ = _parent([60, 9], cos_rows=64)
    par.rope = lambda n, dev: (par.cos, par.sin)          # a stack that hands back its short cached tables
    with pytest.raises(RuntimeError, match="RoPE tables"):
        DEC.ForkCache(par, [0], 50)


class _Script:
    def __init__(self, scripts):
        self.scripts = scripts
        self.extends, self.fork_extends, self.steps = [], [], []

    def logits(self, scripts, held):
        out = torch.zeros(len(held), V)
        for b, n in enumerate(held):
            out[b, scripts[b].get(n, 1)] = 1.0
        return out


def _session(monkeypatch, lens, parent_scripts, member_scripts, max_len=64):
    """A parent session over a stub stack.  A member's next token is read from member_scripts[m], indexed by its OWN rows."""
    from halva_amd import decode as DEC
    rec = _Script(parent_scripts)
    lm = SimpleNamespace(embed_tokens=torch.nn.Embedding(V, 4), layers=[None, None])
    model = DEC.DecodeStack(lm, torch.zeros(V, 4), False)
    cache, _ = _parent(lens, Lcap=max_len)
    emb = lm.embed_tokens.weight

    def ids_of(embeds, n_new):
        return [[int((emb == embeds[b, i]).all(-1).nonzero()[0, 0]) for i in range(n_new[b])] for b in range(embeds.shape[0])]

    def fake_extend(m, c, embeds, n_new):
        if isinstance(c, DEC.ForkCache):
            return fake_fork_extend(m, c, embeds, n_new)
        assert c is cache
        rec.extends.append(ids_of(embeds, n_new))
        c.lens += torch.tensor(n_new, dtype=torch.int32)
        c.filled += max(n_new)
        return rec.logits(parent_scripts, c.lens[0].tolist())

    def fake_fork_extend(m, f, embeds, n_new):
        assert isinstance(f, DEC.ForkCache)
        rec.fork_extends.append(ids_of(embeds, n_new))
        f.own_lens += torch.tensor(n_new, dtype=torch.int32)
        f.filled += max(n_new)
        out = rec.logits(member_scripts, f.own_lens[0].tolist())
        out[torch.tensor(n_new) == 0] = float("nan")
        return out

    def fake_step(m, f, tok):
        if not isinstance(f, DEC.ForkCache):
            pytest.fail("a fork must not run a step on the parent's cache")
        rec.steps.append(tok.tolist())
        f.own_lens += 1
        f.filled += 1
        return rec.logits(member_scripts, f.own_lens[0].tolist())
    monkeypatch.setattr(DEC, "extend", fake_extend)
    monkeypatch.setattr(DEC, "decode_step", fake_step)
    cfg = SimpleNamespace(eos_token_id=None, pad_token_id=None)
    ses = DEC.DecodeSession(model, cache, rec.logits(parent_scripts, list(lens)), list(lens), cfg)
    return ses, rec, cache


def test_fork_pushes_pending_tokens_and_starts_from_the_parents_logits(monkeypatch):
    from halva_amd import decode as DEC
    ses, rec, cache = _session(monkeypatch, [5, 3], [{6: 21}, {4: 22}], [{}, {}, {}, {}])
    ses.pending = [[7], [8]]
    fk = ses.fork(n=2, max_new=6)
    assert rec.extends == [[[7], [8]]] and ses.lens == [6, 4] and ses.pending == [[], []]
    assert isinstance(fk, DEC.ForkedSession) and fk.prefix_of == [0, 0, 1, 1] and fk.prefix_lens == [6, 6, 4, 4]
    assert fk.cache.prefix_lens.tolist() == [6, 4] and fk.lens == [0, 0, 0, 0] and fk.max_len == 6
    assert fk.logits.argmax(-1).tolist() == [21, 21, 22, 22]
    assert ses.fork(prefix_of=[1, 1, 1], max_new=2).prefix_of == [1, 1, 1]
    for kw in (dict(), dict(n=2, prefix_of=[0]), dict(n=0), dict(prefix_of=[1, 0]), dict(prefix_of=[2]), dict(n=1, max_new=0)):
        with pytest.raises(ValueError):
            ses.fork(**kw)
    with pytest.raises(NotImplementedError):
        fk.fork(n=2)


def test_forked_session_bookkeeping(monkeypatch):
    # member 0 emits 7, 9 (EOS) ...; member 1 emits 11, 12, 13, 14 ...; member 2 (of parent row 1) emits 3, 4, 5, 6
    s0 = {0: 7, 1: 9, 2: 1, 3: 1}
    s1 = {0: 11, 1: 12, 2: 13, 3: 14, 4: 15, 8: 16, 9: 17}
    s2 = {0: 3, 1: 4, 2: 5, 3: 6, 4: 2, 7: 18, 8: 19}
    ses, rec, cache = _session(monkeypatch, [5, 3], [{}, {}], [s0, s1, s2])
    fk = ses.fork(prefix_of=[0, 0, 1], max_new=12)
    fk.logits = rec.logits([s0, s1, s2], [0, 0, 0])
    out = fk.generate(4, eos_token_id=9, pad_token_id=0)
    assert out.tolist() == [[7, 9, 0, 0], [11, 12, 13, 14], [3, 4, 5, 6]]
    assert rec.steps == [[7, 11, 3], [9, 12, 4], [0, 13, 5]] and rec.fork_extends == []
    # own_lens is set back behind the stopped member's last real row; the parent's cache is not touched
    assert fk.lens == [2, 3, 3] and fk.pending == [[], [14], [6]]
    assert fk.cache.own_lens.tolist() == [[2, 3, 3]] * 2 and fk.cache.filled == 3
    assert cache.lens.tolist() == [[5, 3]] * 2 and ses.lens == [5, 3]
    fk.append(torch.tensor([[21, 22, 0, 0], [23, 24, 25, 26], [27, 0, 0, 0]]), torch.tensor([[1, 1, 0, 0], [1, 1, 1, 1], [1, 0, 0, 0]]))
    assert rec.fork_extends == [[[21, 22], [14, 23, 24, 25, 26], [6, 27]]]
    assert fk.lens == [4, 8, 5] and fk.pending == [[], [], []]
    assert fk.generate(2, eos_token_id=[], pad_token_id=0).tolist() == [[1, 1], [16, 17], [1, 1]]
    assert fk.lens == [5, 9, 6] and [len(p) for p in fk.pending] == [1, 1, 1]


def test_forked_session_limits_come_before_any_launch(monkeypatch):
    ses, rec, _ = _session(monkeypatch, [5, 3], [{}, {}], [{}, {}])
    fk = ses.fork(n=1, max_new=4)
    with pytest.raises(RuntimeError):
        fk.append(torch.zeros(2, 5, dtype=torch.long))
    with pytest.raises(RuntimeError):
        fk.generate(6, eos_token_id=[])
    assert rec.steps == [] and rec.fork_extends == [] and fk.lens == [0, 0] and fk.cache.filled == 0
    with pytest.raises(NotImplementedError):
        fk.append(torch.zeros(2, 1, dtype=torch.long), images=torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        fk.append(torch.tensor([[0, 3], [3, 3]]), torch.tensor([[0, 1], [1, 1]]))      # left padded
    with pytest.raises(NotImplementedError):
        fk.append(torch.tensor([[-200, 3], [3, 3]]))                                   # an image token
    with pytest.raises(NotImplementedError):
        fk.generate(2, do_sample=True)                                                  # no temperature
    fk.append(torch.zeros(2, 4, dtype=torch.long))
    assert fk.lens == [4, 4]


def test_fork_step_and_extend_checks_come_before_any_launch():
    from halva_amd import decode as DEC
    lm = SimpleNamespace(embed_tokens=torch.nn.Embedding(V, 4), layers=[])
    model = DEC.DecodeStack(lm, torch.zeros(V, 4), False)
    par, _ = _parent([5, 3])
    f = DEC.ForkCache(par, [0, 1], 4, [5, 3])
    for bad in ([0, 0], [5, 1], [-1, 2], [1]):
        with pytest.raises(ValueError):
            DEC.extend(model, f, torch.zeros(2, 4, 4), bad)
    with pytest.raises(RuntimeError, match="KV cache full"):
        DEC.extend(model, f, torch.zeros(2, 5, 4), [5, 1])
    f.filled = 4
    with pytest.raises(RuntimeError, match="KV cache full"):
        DEC.decode_step(model, f, torch.zeros(2, dtype=torch.long))
    assert f.filled == 4


def test_generate_refuses_several_greedy_sequences_and_beams():
    """multimodal._generate's argument rules run before the prompt is embedded."""
    from halva_amd.multimodal import MultimodalMixin

    class Stub:
        _generate = MultimodalMixin._generate

        def _embed_prompt(self, *a):
            pytest.fail("the arguments are checked first")
    kw = dict(input_ids=None, images=None, attention_mask=None, num_beams=1, max_new_tokens=4, eos_token_id=None, pad_token_id=None,
              stopping_criteria=None)
    with pytest.raises(ValueError, match="num_return_sequences"):
        Stub()._generate(do_sample=False, num_return_sequences=3, **kw)
    with pytest.raises(ValueError, match="num_return_sequences"):
        Stub()._generate(do_sample=True, temperature=1.0, num_return_sequences=0, **kw)
    with pytest.raises(NotImplementedError):
        Stub()._generate(do_sample=True, temperature=1.0, num_return_sequences=2, **dict(kw, num_beams=2))


# ------------------------------------------------------------------------------------------------
# the C ABI
def test_names_declared_exported_and_argument_errors():
    from halva_amd import hip
    header = open(os.path.join(ROOT, "include", "halva_hip.h")).read()
    lib = hip.load()
    for name in ("halva_fork_rope_append", "halva_fork_decode_attn", "halva_fork_decode_attn_ws_bytes", "halva_fork_extend_rope_append",
                 "halva_fork_extend_attn"):
        assert re.search(r"\b%s\s*\(" % name, header) and hasattr(lib, name), name
    ws = lib.halva_fork_decode_attn_ws_bytes
    assert ws(16, 40, 2048, 32) == 16 * 40 * (8 + 1) * 130 * 4 and ws(3, 2, 257, 256) == 3 * 2 * (2 + 1) * 130 * 4
    assert ws(0, 2, 8, 8) == 0 and ws(1, 0, 8, 8) == 0 and ws(1, 2, 0, 8) == 0 and ws(1, 2, 8, -1) == 0
    err = lib.halva_last_error
    # argument checks run before any launch, so they answer without a GPU (16 stands for an aligned non-null pointer)
    attn = lambda **k: lib.halva_fork_decode_attn(k.get("q", 16), k.get("ldq", 768), 16, 16, 16, 16, 16, 16, 16, 16, 256, k.get("ws", 16),      # noqa: E731
                                                  k.get("ws_bytes", 1 << 20), k.get("M", 2), 1, 2, k.get("D", 128), 8, k.get("Lown", 8), 0.0, None)
    assert attn(D=64) == -1 and b"head_dim" in err()
    assert attn(q=None) == -1 and b"null pointer" in err()
    assert attn(q=18) == -1 and b"aligned" in err()
    assert attn(ldq=250) == -1 and b"stride" in err()
    assert attn(M=0) == -1 and attn(Lown=0) == -1 and attn(M=70000) == -1
    assert attn(ws_bytes=2 * 2 * 2 * 130 * 4 - 1) == -1 and b"workspace" in err()
    app = lambda **k: lib.halva_fork_rope_append(k.get("q", 16), k.get("ld", 768), 16, 16, k.get("max_pos", 8), 16, 16, 16, 16, 16, 2, k.get("P", 1), 2,      # noqa: E731
                                                 k.get("D", 128), 8, None)
    assert app(D=64) == -1 and b"head_dim" in err()
    assert app(q=None) == -1 and app(ld=760) == -1 and app(max_pos=0) == -1 and app(P=0) == -1 and app(q=24) == -1
    xapp = lambda **k: lib.halva_fork_extend_rope_append(16, 768, k.get("ldseq", 768 * 4), 16, 16, 8, 16, 16, 16, 16, 16, k.get("n_new", 16), 2,      # noqa: E731
                                                         k.get("n", 4), 1, 2, k.get("D", 128), 8, None)
    assert xapp(D=64) == -1 and xapp(n=0) == -1 and xapp(n_new=None) == -1
    assert xapp(ldseq=768 * 4 - 8) == -1 and b"sequence stride" in err()
    xattn = lambda **k: lib.halva_fork_extend_attn(16, 256, k.get("ldseq", 1024), 16, 16, 16, 16, 16, 16, 16, 16, k.get("out", 16), k.get("ldo", 256),      # noqa: E731
                                                   1024, 2, k.get("n", 4), 1, 2, k.get("D", 128), k.get("Lpre", 8), 8, 0.0, None)
    assert xattn(D=64) == -1 and b"head_dim" in err()
    assert xattn(n=0) == -1 and xattn(Lpre=0) == -1 and xattn(out=None) == -1 and xattn(ldo=250) == -1
    assert xattn(ldseq=1016) == -1 and b"sequence stride" in err()


# ------------------------------------------------------------------------------------------------
# tools/bench_decode.py --fork: argument handling and the byte counts, without a GPU
def test_bench_decode_fork_mode_is_declared_and_counts_bytes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_decode_tool", os.path.join(ROOT, "tools", "bench_decode.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    row = 2 * 32 * 128 * 2                                   # K and V of one key row over 32 heads, bf16
    assert tool.fork_attn_bytes(2048, 32, 16, 32) == ((2048 + 16 * 32) * row, 16 * (2048 + 32) * row)
    assert tool.fork_attn_bytes(639, 32, 17, 32) == ((2 * 639 + 17 * 32) * row, 17 * (639 + 32) * row)      # 17 members: two blocks
    assert (tool.FORK_N, tool.FORK_OWN) == (16, 32)
    src = open(os.path.join(ROOT, "tools", "bench_decode.py")).read()
    assert '"--fork"' in src and "fork_kernel_numbers" in src and "fork_loop_numbers" in src and "fork_question_numbers" in src
