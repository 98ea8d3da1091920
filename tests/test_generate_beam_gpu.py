"""Beam search end to end (halva_amd/decode.py: BeamCache, beam_loop, DecodeSession.beam_search; MultimodalMixin.beam_search) on the small d128
models of tests/generate_models_util.py, LLaVA and VILA.

Nothing here needs a tolerance but the num_beams = 1 score: the zero-copy loop is compared bit for bit with a loop assembled from public pieces
that moves every layer's own K / V rows by index_select after every step (what the ancestry table replaces), and halva_beam_decode_attn is
bitwise halva_fork_decode_attn on such rows (tests/test_beam_kernels_gpu.py), so the logits are the same bits too."""
import pytest
import torch

import beam_ref_util as R
from generate_models_util import build_llava, build_vila, pad_batch
from test_generate_session_gpu import _Env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["llava", "vila"])
def env(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    e = _Env(build_llava, "generate_d128.npz") if request.param == "llava" else _Env(build_vila, "generate_vila.npz")
    e.name = request.param
    return e


def _start(env, extra=64, first=0, count=2, **kw):
    rows, images = env.prompts[first:first + count], env.images[first:first + count]
    ids, mask = pad_batch(rows)
    T = env.spliced(rows, images)[0].shape[1]
    return env.model.start_session(ids, images=images, attention_mask=mask, max_len=T + extra, **kw)


def _eos_for(env, n=1):
    """Frequent tokens as EOS ids, so that hypotheses finish: the golden greedy tokens of the first prompt, from the third on."""
    return [int(t) for t in env.toks[0][2:2 + n]]


def _materialised(env, ses, Kb, steps, **kw):
    """session.beam_search assembled from public pieces, with the K / V rows moved: ForkCache, decode_step, an index_select of every
    layer's own rows by the parents before each step, kernels.beam_select, BeamState."""
    from halva_amd import decode as DEC, kernels as KR
    from halva_amd.beam import BeamState
    ses._push([[] for _ in ses.lens])
    B = len(ses.lens)
    eos_ids, pad = DEC.eos_and_pad(ses.config, kw.get("eos_token_id"), kw.get("pad_token_id"), "cuda")
    st = BeamState(B, Kb, steps, eos_ids.tolist(), pad, kw.get("length_penalty", 1.0), kw.get("early_stopping", False),
                   kw.get("num_return_sequences", 1))
    fork = DEC.ForkCache(ses.cache, [b for b in range(B) for _ in range(Kb)], max(steps - 1, 1), ses.lens)
    logits = ses.logits[torch.arange(B, device="cuda").repeat_interleave(Kb)]
    while True:
        s, t, b = KR.beam_select(logits, st.run_scores.view(-1).cuda(), Kb, st.C)
        nxt, parents, finished = st.step(s.cpu(), t.cpu(), b.cpu())
        if finished:
            break
        idx = parents.cuda()
        for i in range(len(fork.k)):
            fork.k[i], fork.v[i] = fork.k[i].index_select(0, idx), fork.v[i].index_select(0, idx)
        logits = DEC.decode_step(env.model, fork, nxt.cuda())
    return st.finalize(), st


def test_zero_copy_equals_materialised(env):
    kw = dict(eos_token_id=_eos_for(env, 2), num_return_sequences=3, length_penalty=1.0)
    got = _start(env).beam_search(3, 12, **kw)
    want, st = _materialised(env, _start(env), 3, 12, **kw)
    assert got.sequences.shape[0] == 6 and got.sequences.is_cuda and got.sequences.dtype == torch.long
    assert torch.equal(got.sequences.cpu(), want.sequences)
    assert torch.equal(got.sequences_scores.cpu().view(torch.int32), want.sequences_scores.view(torch.int32))
    assert any(bool((p != torch.arange(st.M)).any()) for p in st.parents[1:]), "no beam ever continued another beam: the table was not exercised"


@pytest.mark.parametrize("early", [True, False, "never"])
def test_one_beam_is_greedy(env, early):
    """num_beams = 1 against greedy decoding.  One beam is greedy until its best candidate is an EOS id; that hypothesis takes the one finished
    slot.  early_stopping=True stops there; the other two rules may go on with the runner-up and may only replace the hypothesis by one that
    scores higher.

    Tokens: against session.generate, the public greedy path, up to and including the first EOS.  The session's decode attention and the
    beams' prefix / own attention reduce in different orders, so their logits agree within ROW (tests/test_generate_session_gpu.py), not bit
    for bit: the tokens are held from the first step up to the first one whose top-2 gap is below 4 x ROW, and the fixture must decide at
    least the first step.  Score: against a greedy run through a 1-way fork, whose attention is the beams' own bit for bit, so the sum of the
    fp64 log_softmax of that run's logits at its tokens over len ** length_penalty is held within the select bound summed over the steps."""
    from halva_amd import decode as DEC
    steps, lp = 10, 1.0
    eos = _eos_for(env, 1)
    out = _start(env).beam_search(1, steps, length_penalty=lp, early_stopping=early, eos_token_id=eos)
    public = _start(env).generate(steps, eos_token_id=eos).tolist()
    twin = _start(env).fork(1, max_new=steps)
    lg = twin.logits
    B = lg.shape[0]
    toks, lps, done = [[] for _ in range(B)], [0.0] * B, [False] * B
    bound, decided = [0.0] * B, [None] * B
    row = env.row()
    f64 = lambda v: torch.tensor(v, dtype=torch.float64)      # noqa: E731
    for s in range(steps):
        l64 = lg.double().cpu()
        nxt = lg.argmax(-1)
        for b in range(B):
            if done[b]:
                continue
            t = int(nxt[b])
            top2 = l64[b].topk(2).values
            if decided[b] is None and float(top2[0] - top2[1]) < 4 * row:
                decided[b] = s
            lse = float(torch.logsumexp(l64[b], 0))
            lps[b] += float(l64[b, t]) - lse
            bound[b] += float(R.select_bound(f64(lps[b]), f64(lps[b]), l64[b].abs().max(), f64(lse)))
            toks[b].append(t)
            done[b] = t in eos
        if all(done) or s + 1 == steps:
            break
        lg = DEC.decode_step(env.model, twin.cache, nxt)
    for b in range(B):
        n = len(toks[b])
        want = lps[b] / (n ** lp)
        same = out.sequences[b, :n].tolist() == toks[b]
        err = abs(float(out.sequences_scores[b]) - want)
        held = n if decided[b] is None else min(decided[b], n)
        print("%s prompt %d, early_stopping=%r: %d greedy tokens (%d held to session.generate), score %.6f, |err| %.3e, bound %.3e, same=%s"
              % (env.name, b, early, n, held, want, err, bound[b], same))
        assert held >= 1, (b, decided[b])
        if early is True or same:
            assert same, (b, out.sequences[b], toks[b])
            assert err <= bound[b], (b, err, bound[b])
            assert out.sequences[b, :held].tolist() == public[b][:held], (b, out.sequences[b], public[b])
        else:
            assert float(out.sequences_scores[b]) > want, (b, float(out.sequences_scores[b]), want)


def test_left_padding_is_refused(env):
    ids = torch.tensor([[0, 0, 5, 6, 7], [0, 9, 8, 7, 6]])          # text only, the padding in front
    with pytest.raises(NotImplementedError, match="beam_search: left-padded"):
        env.model.beam_search(ids, attention_mask=ids != 0, num_beams=2, max_new_tokens=4)


def test_session_is_left_as_it_was(env):
    eos = _eos_for(env, 1)
    ses = _start(env)
    ses.generate(3, eos_token_id=[])                      # leaves one token pending: beam_search pushes it first, as fork() does
    twin = _start(env)
    twin.generate(3, eos_token_id=[])
    a = ses.beam_search(3, 8, eos_token_id=eos)
    lens, filled = list(ses.lens), ses.cache.filled
    assert ses.pending == [[], []] and ses.cache.lens.tolist() == [lens] * len(ses.cache.k)
    b = ses.beam_search(3, 8, eos_token_id=eos)
    assert torch.equal(a.sequences, b.sequences) and torch.equal(a.sequences_scores.view(torch.int32), b.sequences_scores.view(torch.int32))
    assert ses.lens == lens and ses.cache.filled == filled and ses.pending == [[], []]
    assert torch.equal(ses.generate(8, eos_token_id=[]), twin.generate(8, eos_token_id=[]))
    assert torch.equal(ses.logits.view(torch.int32), twin.logits.view(torch.int32))


@pytest.mark.parametrize("chunk", [None, 7])
def test_model_beam_search_is_the_sessions(env, chunk):
    rows, images = env.prompts[:2], env.images[:2]
    ids, mask = pad_batch(rows)
    kw = dict(num_beams=3, max_new_tokens=8, eos_token_id=_eos_for(env, 1), num_return_sequences=2)
    a = env.model.beam_search(ids, images=images, attention_mask=mask, prefill_chunk=chunk, **kw)
    b = _start(env, prefill_chunk=chunk).beam_search(**kw)
    assert a.sequences.shape[0] == 4 and torch.equal(a.sequences, b.sequences)
    assert torch.equal(a.sequences_scores.view(torch.int32), b.sequences_scores.view(torch.int32))
    with pytest.raises(NotImplementedError):
        env.model.generate(ids, images=images, attention_mask=mask, num_beams=2, max_new_tokens=4)


def test_returned_rows_are_distinct_and_descending(env):
    Kb = 4
    out = _start(env).beam_search(Kb, 8, num_return_sequences=Kb, eos_token_id=_eos_for(env, 1))
    assert out.sequences.shape[0] == 2 * Kb
    for b in range(2):
        rows = [tuple(r.tolist()) for r in out.sequences[b * Kb:(b + 1) * Kb]]
        sc = out.sequences_scores[b * Kb:(b + 1) * Kb].tolist()
        assert len(set(rows)) == Kb and sc == sorted(sc, reverse=True) and all(v > -1e8 for v in sc), (rows, sc)
