"""Sessions, chunked prefill and block teacher forcing (halva_amd/decode.py: extend, prefill_chunked, DecodeSession; start_session and
generate(prefill_chunk=) of both wrappers) on the small d128 models of tests/generate_models_util.py and their goldens
(tests/golden/generate_d128.npz, generate_vila.npz: 24 greedy steps of the reference's own forward).

Bounds are the existing generation tests', restated:
  * against the golden (tests/test_generate_gpu.py:test_against_the_reference_golden): per prompt, GOLD = 1.5 x the largest distance of the
    product's own cache-free forward from the golden logits over the 24 steps; tokens must equal the golden's up to the first step whose
    golden top-2 gap is below 4 x GOLD.
  * one cached path against another (test_cached_decode_matches_full_forward / test_batched_ragged_equals_one_at_a_time): ROW = what two
    cache-free forwards that differ only in row grouping disagree by on the last-row logits, floored at one bf16 ulp of the largest logit;
    logits within 3 x ROW, tokens equal up to the first step whose top-2 gap is below 4 x ROW."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from generate_models_util import build_llava, build_vila, pad_batch  # noqa: E402
from golden_util import load_npz  # noqa: E402

N_GOLD = 24


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@torch.no_grad()
def _full_last_logits(model, rows, images):
    ids, mask = pad_batch(rows)
    out = model.forward(input_ids=ids.cuda(), attention_mask=mask.cuda(), images=images).logits
    n = model._last_plan.seq_len.long()
    return out[torch.arange(len(rows)), n - 1].float()


class _Env:
    def __init__(self, build, golden):
        self.model, self.prompts, self.images = build()
        self.g = load_npz(golden)
        self.toks = [torch.as_tensor(self.g["tokens.%d" % i]) for i in range(3)]
        self.glog = [torch.as_tensor(self.g["logits.%d" % i]).double() for i in range(3)]
        self.gap = [torch.as_tensor(self.g["gap.%d" % i]) for i in range(3)]
        self._gold = {}
        self._row = None

    def gold(self, i):
        """GOLD of prompt i (module docstring)."""
        if i not in self._gold:
            p, im = self.prompts[i], self.images[i:i + 1]
            full = torch.stack([_full_last_logits(self.model, [torch.cat([p, self.toks[i][:s]])], im)[0] for s in range(N_GOLD)]).double().cpu()
            self._gold[i] = 1.5 * float((full - self.glog[i]).abs().amax(-1).max())
        return self._gold[i]

    def row(self):
        """ROW (module docstring), on the first two prompts: together in one batch against each alone."""
        if self._row is None:
            together = _full_last_logits(self.model, self.prompts[:2], self.images[:2])
            alone = torch.cat([_full_last_logits(self.model, [p], self.images[i:i + 1]) for i, p in enumerate(self.prompts[:2])])
            floor = 2.0 ** (math.floor(math.log2(float(together.abs().max()))) - 7)
            self._row = max(float((together - alone).abs().max()), floor)
        return self._row

    def spliced(self, rows, images):
        ids, mask = pad_batch(rows)
        return self.model._splice(ids.cuda(), mask.cuda(), None, None, images)


@pytest.fixture(scope="module")
def llava():
    _dev()
    return _Env(build_llava, "generate_d128.npz")


@pytest.fixture(scope="module")
def vila():
    _dev()
    return _Env(build_vila, "generate_vila.npz")


def _golden_tokens_hold(env, i, got, where):
    for s in range(min(len(got), N_GOLD)):
        if float(env.gap[i][s]) < 4 * env.gold(i):
            break
        assert int(got[s]) == int(env.toks[i][s]), (where, i, s, list(map(int, got)), env.toks[i].tolist())


# ------------------------------------------------------------------------------------------------
def test_chunked_prefill_matches_the_golden(llava):
    from halva_amd import decode as DEC
    env, model = llava, llava.model
    none = torch.zeros(0, dtype=torch.long, device="cuda")
    for i, p in enumerate(env.prompts):
        embeds, plan = env.spliced([p], env.images[i:i + 1])
        T = embeds.shape[1]
        for chunk in (1, 16, T - 1):
            cache = DEC.KVCache(model, 1, T + N_GOLD)
            logits = DEC.prefill_chunked(model, embeds, plan.seq_len, cache, chunk)
            d = float((logits[0].double().cpu() - env.glog[i][0]).abs().max())
            print("prompt %d chunk %d: |chunked prefill - golden| %.3e (bound %.3e)" % (i, chunk, d, env.gold(i)))
            assert d <= env.gold(i), (i, chunk)
            assert cache.lens.tolist() == [[T]] * len(cache.k) and cache.filled == T
            toks = DEC.greedy(model, embeds, plan.seq_len, N_GOLD, none, 0, prefill_chunk=chunk)[0].tolist()
            assert len(toks) == N_GOLD
            _golden_tokens_hold(env, i, toks, "chunk %d" % chunk)


def test_generate_with_prefill_chunk_and_without(llava):
    env, model = llava, llava.model
    ids, mask = pad_batch(env.prompts)
    kw = dict(images=env.images, attention_mask=mask, max_new_tokens=N_GOLD, eos_token_id=[])
    chunked = model.generate(ids, prefill_chunk=16, **kw)
    assert chunked.shape == (3, ids.shape[1] + N_GOLD)
    for i in range(3):
        single = model.generate(env.prompts[i][None], images=env.images[i:i + 1], max_new_tokens=N_GOLD, eos_token_id=[], prefill_chunk=16)
        _golden_tokens_hold(env, i, single[0, len(env.prompts[i]):].tolist(), "generate(prefill_chunk=16)")
    plain = model.generate(ids, **kw)
    assert torch.equal(plain, model.generate(ids, **kw))                        # the default path: the same bits call after call
    assert torch.equal(plain, model.generate(ids, prefill_chunk=None, **kw))
    with pytest.raises(ValueError):
        model.generate(ids, prefill_chunk=0, **kw)


def test_block_teacher_forcing(llava):
    from halva_amd import decode as DEC
    env, model = llava, llava.model
    emb = model.get_model().embed_tokens
    for i, p in enumerate(env.prompts):
        embeds, plan = env.spliced([p], env.images[i:i + 1])
        cache = DEC.KVCache(model, 1, embeds.shape[1] + 10)
        DEC.prefill(model, embeds, plan.seq_len, cache)
        lg = DEC.extend(model, cache, emb(env.toks[i][:8].cuda())[None], [8])
        d8 = float((lg[0].double().cpu() - env.glog[i][8]).abs().max())
        lg = DEC.decode_step(model, cache, env.toks[i][8:9].cuda())
        d9 = float((lg[0].double().cpu() - env.glog[i][9]).abs().max())
        print("prompt %d: block of 8 -> |logits - golden[8]| %.3e, next step %.3e (bound %.3e)" % (i, d8, d9, env.gold(i)))
        assert d8 <= env.gold(i) and d9 <= env.gold(i), i
        assert cache.lens.tolist() == [[embeds.shape[1] + 9]] * len(cache.k)
    # ragged: three prompts in one batch, blocks of 8, 3 and 0 rows
    embeds, plan = env.spliced(env.prompts, env.images)
    cache = DEC.KVCache(model, 3, embeds.shape[1] + 10)
    DEC.prefill(model, embeds, plan.seq_len, cache)
    before = [(cache.k[l][2].clone(), cache.v[l][2].clone()) for l in range(len(cache.k))]
    block = torch.zeros(3, 8, dtype=torch.long)
    block[0], block[1, :3] = env.toks[0][:8], env.toks[1][:3]
    lg = DEC.extend(model, cache, emb(block.cuda()), [8, 3, 0])
    for i, m in ((0, 8), (1, 3)):
        d = float((lg[i].double().cpu() - env.glog[i][m]).abs().max())
        print("ragged row %d: block of %d -> |logits - golden[%d]| %.3e (bound %.3e)" % (i, m, m, d, env.gold(i)))
        assert d <= env.gold(i), i
    assert torch.isnan(lg[2]).all()
    want = [int(n) + m for n, m in zip(plan.seq_len.tolist(), (8, 3, 0))]
    assert cache.lens.tolist() == [want] * len(cache.k)
    for l, (k, v) in enumerate(before):
        assert torch.equal(cache.k[l][2].view(torch.int16), k.view(torch.int16)) and torch.equal(cache.v[l][2].view(torch.int16), v.view(torch.int16))


# ------------------------------------------------------------------------------------------------
def _real(row, eos):
    """a row's tokens up to and including its first EOS"""
    row = list(map(int, row))
    return row[:row.index(eos) + 1] if eos in row else row


def _two_turns(env, strip_prompt):
    from halva_amd import decode as DEC
    model = env.model
    prompts, images = env.prompts[:2], env.images[:2]
    ids, mask = pad_batch(prompts)
    T = env.spliced(prompts, images)[0].shape[1]
    max_len = T + 6 + 9 + 4
    free = model.start_session(ids, images=images, attention_mask=mask, max_len=max_len).generate(6, eos_token_id=[])
    assert free.shape == (2, 6) and free.dtype == torch.long
    if strip_prompt is not None:              # the session's first turn is generate()'s own continuation
        gen = model.generate(ids, images=images, attention_mask=mask, max_new_tokens=6, eos_token_id=[])
        assert torch.equal(strip_prompt(gen, ids.shape[1]), free)
    eos = int(free[0, 2])                     # row 0 stops at step 2 (earlier if the id came before)
    ses = model.start_session(ids, images=images, attention_mask=mask, max_len=max_len)
    assert ses.lens == env.spliced(prompts, images)[1].seq_len.tolist()
    out1 = ses.generate(6, eos_token_id=eos, pad_token_id=0)
    real = [_real(out1[b], eos) for b in range(2)]
    assert len(real[0]) <= 3 and (out1[0, len(real[0]):] == 0).all()
    extra = [torch.tensor([5, 17, 44, 9, 131]), torch.tensor([12, 150, 7, 7, 63, 21, 90, 3, 110])]
    eids, emask = pad_batch(extra)
    ses.append(eids, emask)
    kept = ses.logits.clone()
    held = [int(n) + len(r) + len(e) for n, r, e in zip(env.spliced(prompts, images)[1].seq_len.tolist(), real, extra)]
    assert ses.lens == held and ses.cache.lens.tolist() == [held] * len(ses.cache.k)
    out2 = ses.generate(4, eos_token_id=[])
    assert out2.shape == (2, 4)
    row = env.row()
    for b in range(2):
        hist = torch.cat([prompts[b], torch.tensor(real[b], dtype=torch.long), extra[b]])
        fresh = model.start_session(hist[None], images=images[b:b + 1], max_len=max_len)
        assert fresh.lens == [held[b]]
        lg, got = fresh.logits, []
        for s in range(4):
            top2 = lg[0].topk(2)
            if s == 0:
                d = float((lg[0] - kept[b]).abs().max())
                print("row %d: |kept logits - fresh prefill| %.3e (3 x ROW = %.3e)" % (b, d, 3 * row))
                assert d <= 3 * row, b
            if float(top2.values[0] - top2.values[1]) < 4 * row:
                break
            assert int(out2[b, s]) == int(top2.indices[0]), (b, s, out2[b].tolist(), got)
            got.append(int(top2.indices[0]))
            lg = DEC.decode_step(model, fresh.cache, top2.indices[:1])
    return ses


def test_two_turns_llava(llava):
    _two_turns(llava, lambda gen, T0: gen[:, T0:])


def test_two_turns_vila_past_max_position_embeddings(vila):
    ses = _two_turns(vila, lambda gen, T0: gen)
    assert max(ses.lens) > int(vila.g["max_position_embeddings"])


def test_session_limits(llava):
    env, model = llava, llava.model
    p = env.prompts[0]
    T = env.spliced([p], env.images[:1])[0].shape[1]
    ses = model.start_session(p[None], images=env.images[:1], max_len=T + 4)
    assert ses.lens == [T]
    lens_d = ses.cache.lens.clone()
    with pytest.raises(RuntimeError):
        ses.append(torch.full((1, 5), 7))
    assert ses.lens == [T] and torch.equal(ses.cache.lens, lens_d) and ses.cache.filled == T
    with pytest.raises(NotImplementedError):
        ses.append(torch.full((1, 2), 7), images=env.images[:1])
    with pytest.raises(RuntimeError):
        ses.generate(6, eos_token_id=[])
    ses.append(torch.full((1, 4), 7))
    assert ses.lens == [T + 4] and ses.cache.lens.tolist() == [[T + 4]] * len(ses.cache.k)
    with pytest.raises(ValueError):
        model.start_session(p[None], images=env.images[:1], max_len=T - 1)
    chunked = model.start_session(p[None], images=env.images[:1], max_len=T + 4, prefill_chunk=16)
    d = float((chunked.logits[0].double().cpu() - env.glog[0][0]).abs().max())
    assert d <= env.gold(0) and chunked.lens == [T]
