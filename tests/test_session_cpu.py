"""Host logic of sessions and chunked prefill (halva_amd/decode.py) without a GPU: DecodeSession's pending-token bookkeeping against a
stub stack that records what extend() and decode_step() were handed, prefill_chunked's n_new schedule, and the new C ABI names."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 32


class _Script:
    """Stands in for the model: the next token of a row is read from a per-row script, indexed by how many rows that sequence holds."""

    def __init__(self, scripts):
        self.scripts = scripts
        self.extends, self.steps = [], []

    def logits(self, held):
        out = torch.zeros(len(held), V)
        for b, n in enumerate(held):
            out[b, self.scripts[b].get(n, 1)] = 1.0
        return out


def _session(monkeypatch, scripts, lens, max_len=64):
    from halva_amd import decode as DEC
    rec = _Script(scripts)
    lm = SimpleNamespace(embed_tokens=torch.nn.Embedding(V, 4), layers=[None, None])
    model = DEC.DecodeStack(lm, torch.zeros(V, 4), False)
    cache = SimpleNamespace(B=len(lens), Lcap=max_len, filled=max(lens), lens=torch.tensor([list(lens)] * 2, dtype=torch.int32),
                            cos=torch.zeros(max_len, 2))
    emb = lm.embed_tokens.weight

    def fake_extend(m, c, embeds, n_new):
        ids = [[int((emb == embeds[b, i]).all(-1).nonzero()[0, 0]) for i in range(n_new[b])] for b in range(embeds.shape[0])]
        rec.extends.append(ids)
        c.lens += torch.tensor(n_new, dtype=torch.int32)
        c.filled += max(n_new)
        out = rec.logits(c.lens[0].tolist())
        out[torch.tensor(n_new) == 0] = float("nan")
        return out

    def fake_step(m, c, tok):
        rec.steps.append(tok.tolist())
        c.lens += 1
        c.filled += 1
        return rec.logits(c.lens[0].tolist())
    monkeypatch.setattr(DEC, "extend", fake_extend)
    monkeypatch.setattr(DEC, "decode_step", fake_step)
    cfg = SimpleNamespace(eos_token_id=None, pad_token_id=None)
    return DEC.DecodeSession(model, cache, rec.logits(list(lens)), list(lens), cfg), rec, cache


def test_pending_tokens_eos_rows_and_the_last_token(monkeypatch):
    # row 0 holds 5 rows and will emit 7, 9 (EOS) ...; row 1 holds 3 rows and emits 11, 12, 13, 14 ...
    s0 = {5: 7, 6: 9, 7: 1, 8: 1, 9: 1, 10: 2, 11: 3, 12: 4, 13: 5}
    s1 = {3: 11, 4: 12, 5: 13, 6: 14, 7: 15, 8: 16, 9: 17, 10: 18, 11: 19, 12: 20, 13: 21}
    ses, rec, cache = _session(monkeypatch, [s0, s1], [5, 3])
    out = ses.generate(4, eos_token_id=9, pad_token_id=0)
    assert out.tolist() == [[7, 9, 0, 0], [11, 12, 13, 14]]
    # the loop pushed three columns; row 0's pads were among them but belong to no history: lens counts 7, 9 only and is set back
    assert rec.steps == [[7, 11], [9, 12], [0, 13]] and rec.extends == []
    assert ses.lens == [7, 6] and ses.pending == [[], [14]]
    assert cache.lens.tolist() == [[7, 6], [7, 6]] and cache.filled == 7
    # next turn: the EOS row pushes its new ids only, the live row its pending token first - once
    ses.append(torch.tensor([[21, 22, 0], [23, 24, 25]]), torch.tensor([[1, 1, 0], [1, 1, 1]]))
    assert rec.extends == [[[21, 22], [14, 23, 24, 25]]]
    assert ses.lens == [9, 10] and ses.pending == [[], []]
    out2 = ses.generate(2, eos_token_id=[], pad_token_id=0)
    assert out2.tolist() == [[s0[9], s0[10]], [s1[10], s1[11]]]
    assert len(rec.extends) == 1 and rec.steps[-1] == [s0[9], s1[10]]
    assert ses.lens == [10, 11] and ses.pending == [[s0[10]], [s1[11]]]
    # generate() again without a turn in between: the pending tokens go through extend first, exactly once
    ses.generate(1, eos_token_id=[], pad_token_id=0)
    assert rec.extends[-1] == [[s0[10]], [s1[11]]] and len(rec.extends) == 2
    assert ses.lens == [11, 12] and [len(p) for p in ses.pending] == [1, 1]


def test_a_row_that_stops_on_the_last_column_keeps_its_eos_pending(monkeypatch):
    s0 = {2: 5, 3: 9, 4: 1}
    ses, rec, _ = _session(monkeypatch, [s0], [2])
    assert ses.generate(2, eos_token_id=9, pad_token_id=0).tolist() == [[5, 9]]
    assert ses.lens == [3] and ses.pending == [[9]]
    ses.append(torch.tensor([[6]]))
    assert rec.extends == [[[9, 6]]] and ses.lens == [5]


def test_limits_are_checked_before_anything_is_pushed(monkeypatch):
    ses, rec, cache = _session(monkeypatch, [{4: 1, 5: 2}, {2: 1, 3: 2}], [4, 2], max_len=8)
    with pytest.raises(RuntimeError):
        ses.append(torch.zeros(2, 5, dtype=torch.long))
    assert ses.lens == [4, 2] and rec.extends == [] and cache.filled == 4
    with pytest.raises(RuntimeError):
        ses.generate(6, eos_token_id=[])
    assert rec.steps == []
    with pytest.raises(NotImplementedError):
        ses.append(torch.zeros(2, 1, dtype=torch.long), images=torch.zeros(2, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        ses.append(torch.tensor([[0, 3], [3, 3]]), torch.tensor([[0, 1], [1, 1]]))      # left padded
    with pytest.raises(NotImplementedError):
        ses.generate(2, do_sample=True)                                                  # no temperature
    ses.append(torch.zeros(2, 4, dtype=torch.long))
    assert ses.lens == [8, 6]


def test_chunk_schedule_for_ragged_prompts():
    from halva_amd.decode import chunk_schedule
    assert chunk_schedule([5, 9, 1], 9, 4) == [(0, 4, [4, 4, 1]), (4, 4, [1, 4, 0]), (8, 1, [0, 1, 0])]
    assert chunk_schedule([5, 9, 1], 12, 4) == [(0, 4, [4, 4, 1]), (4, 4, [1, 4, 0]), (8, 4, [0, 1, 0])]      # all-padding columns dropped
    assert chunk_schedule([3, 2], 7, 16) == [(0, 7, [3, 2])]
    assert chunk_schedule([3], 3, 1) == [(0, 1, [1]), (1, 1, [1]), (2, 1, [1])]
    for seq, T, c in (([7, 20, 13], 20, 3), ([1], 1, 5), ([64, 65], 70, 64)):
        sched = chunk_schedule(seq, T, c)
        assert [sum(col) for col in zip(*[s[2] for s in sched])] == seq
        assert all(n <= c and max(nn) >= 1 and max(nn) <= n for _, n, nn in sched)
        assert [s[0] for s in sched] == [sum(x[1] for x in sched[:i]) for i in range(len(sched))]
    with pytest.raises(ValueError):
        chunk_schedule([3], 3, 0)


def test_extend_checks_come_before_any_launch():
    from halva_amd import decode as DEC
    lm = SimpleNamespace(embed_tokens=torch.nn.Embedding(V, 4), layers=[])
    model = DEC.DecodeStack(lm, torch.zeros(V, 4), False)
    cache = SimpleNamespace(rows=2, room=10, Lcap=10, filled=6, rows_refusal=None)
    x = torch.zeros(2, 4, 4)
    for bad in ([0, 0], [5, 1], [-1, 2], [1]):
        with pytest.raises(ValueError):
            DEC.extend(model, cache, x, bad)
    with pytest.raises(RuntimeError, match="KV cache full"):
        DEC.extend(model, cache, torch.zeros(2, 5, 4), [5, 1])
    assert cache.filled == 6


def test_new_names_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "halva_hip.h")).read()
    lib = os.path.join(ROOT, "halva_amd", "libhalva_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as g
        g.build()
    dll = ctypes.CDLL(lib)
    for name in ("halva_extend_rope_append", "halva_extend_attn", "halva_extend_attn_ws_bytes", "halva_extend_advance"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(dll, name), name
    from halva_amd import hip
    lib = hip.load()
    assert lib.halva_extend_attn_ws_bytes(16, 639, 32, 1024) >= 0
    # argument checks run before any launch, so they answer without a GPU
    assert lib.halva_extend_attn(16, 1024, 1024, 16, 16, 16, 16, 16, 1024, 1024, None, 0, 1, 1, 2, 64, 8, 0.0, None) == -1
    assert b"head_dim" in lib.halva_last_error()
    assert lib.halva_extend_attn(16, 1024, 0, 16, 16, 16, 16, 16, 1024, 0, None, 0, 1, 0, 2, 128, 8, 0.0, None) == -1      # n = 0
    assert lib.halva_extend_rope_append(16, 768, 768, 16, 16, 8, 16, 16, 16, 16, 1, 1, 2, 64, 8, None) == -1
    assert lib.halva_extend_advance(None, None, 1, 8, None) == -1
