"""Beam search without a GPU (halva_amd/beam.py: BeamState, check_beam_args; the host rules of DecodeSession.beam_search).

BeamState against transformers itself: a tiny random LlamaForCausalLM on the CPU runs `generate(num_beams=K, do_sample=False)`, and BeamState
is driven from the same model's fp32 logits (a full forward on every beam's sequence per step; the candidates come from
tests/beam_ref_util.py's float64 select reference, rounded to fp32 as HF holds them).  `sequences` are held equal exactly, `sequences_scores`
to 1e-5 relative.  The fixtures are chosen so that the grid is not vacuous (asserted below): hypotheses that finish early, loops that end
early under early_stopping False and True, prompts that finish at different steps, a finished best below a running beam's raw score, and
every step's top C + 1 candidates more than 1e-4 apart in float64.

The ancestry table on the host: beam_ref_util.advance_reference over the parents BeamState produced, with a fake own cache that stores token
ids as rows - after every step the gather through the table is the beam's token history."""
from types import SimpleNamespace

import pytest
import torch
import transformers

import beam_ref_util as R

VOCAB, PROMPT, MAX_NEW = 100, 5, 10
PAD = 1          # (not 0: transformers fills with `pad_token_id or eos_token_id[0]`, so a pad id of 0 would come back as the EOS id)
GAP = 1e-4
MODEL_SEED, PROMPT_SEED, HEAD_SCALE = 0, 23, 25.0          # chosen on the CPU so that transformers alone meets the conditions below


@pytest.fixture(scope="module")
def hf():
    torch.manual_seed(MODEL_SEED)
    cfg = transformers.LlamaConfig(vocab_size=VOCAB, hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2,
                                   num_key_value_heads=2, max_position_embeddings=64, pad_token_id=PAD, bos_token_id=1, eos_token_id=2)
    model = transformers.LlamaForCausalLM(cfg).eval().float()
    with torch.no_grad():
        model.lm_head.weight.mul_(HEAD_SCALE)          # peaked rows: beams differ, EOS ids finish hypotheses
    g = torch.Generator().manual_seed(PROMPT_SEED)
    prompts = torch.randint(3, VOCAB, (2, PROMPT), generator=g)
    with torch.no_grad():
        first = model(prompts).logits[:, -1].float()
    # frequent tokens as EOS ids: the two most likely second-step tokens of greedy decoding finish hypotheses soon
    greedy = model.generate(prompts, max_new_tokens=MAX_NEW, do_sample=False, num_beams=1, eos_token_id=None, pad_token_id=PAD)[:, PROMPT:]
    counts = torch.bincount(greedy.flatten(), minlength=VOCAB)
    counts[:3] = 0
    eos = counts.topk(2).indices.tolist()
    return SimpleNamespace(model=model, prompts=prompts, eos=eos, first=first)


def _logits(model, seqs):
    with torch.no_grad():
        return model(seqs).logits[:, -1].float()


def _drive(hf, K, early, lp, n_ret, eos):
    """BeamState from the model's own fp32 logits -> (BeamOutput, BeamState, facts about the run)."""
    from halva_amd.beam import BeamState
    B = hf.prompts.shape[0]
    st = BeamState(B, K, MAX_NEW, eos, PAD, lp, early, n_ret)
    seqs = hf.prompts.repeat_interleave(K, 0)
    facts = dict(steps=0, gap=float("inf"), first_closed=[None] * B)
    while True:
        lg = _logits(hf.model, seqs)
        ref = R.select_reference(lg, st.run_scores.view(-1), K, st.C)
        live = ~st.closed()
        gaps = torch.cat([ref["score"], ref["next"][:, None]], 1)
        d = (gaps[:, :-1] - gaps[:, 1:])[live]
        d = d[torch.isfinite(d) & (gaps[:, :-1][live] > -1e8)]          # (candidates of the K - 1 silent copies at step 0 sit at -1e9)
        if d.numel():
            facts["gap"] = min(facts["gap"], float(d.min()))
        # HF's candidates: fp32 log_softmax + fp32 running score, topk
        acc = (torch.log_softmax(lg, -1) + st.run_scores.view(-1)[:, None]).view(B, K * VOCAB)
        top = acc.topk(st.C, 1)
        assert torch.equal(top.indices[live], (ref["beam"] * VOCAB + ref["token"])[live])
        nxt, parent, finished = st.step(top.values, top.indices % VOCAB, top.indices // VOCAB)
        facts["steps"] += 1
        for b in range(B):
            if facts["first_closed"][b] is None and bool(st.closed()[b]):
                facts["first_closed"][b] = facts["steps"]
        if finished:
            break
        seqs = torch.cat([seqs[parent], nxt[:, None]], 1)
    return st.finalize(), st, facts


GRID = [(K, early, lp, n_ret, n_eos) for K in (1, 2, 3, 4) for early in (False, True, "never") for lp in (0.0, 1.0, 2.0)
        for n_ret in sorted({1, K}) for n_eos in (1, 2)]


@pytest.fixture(scope="module")
def runs(hf):
    out = {}
    for K, early, lp, n_ret, n_eos in GRID:
        eos = hf.eos[:n_eos]
        want = hf.model.generate(hf.prompts, num_beams=K, do_sample=False, max_new_tokens=MAX_NEW, early_stopping=early, length_penalty=lp,
                                 num_return_sequences=n_ret, eos_token_id=eos, pad_token_id=PAD, return_dict_in_generate=True,
                                 output_scores=True)
        got, st, facts = _drive(hf, K, early, lp, n_ret, eos)
        out[(K, early, lp, n_ret, n_eos)] = (want, got, st, facts)
    return out


def _greedy_hypothesis(want, eos, lp):
    """HF's greedy run (what generate(num_beams=1) is) as beam hypotheses: per prompt the tokens up to and including the first EOS id and the
    fp32 sum of their log-probabilities over length ** lp."""
    out = []
    new = want.sequences[:, PROMPT:]
    for b in range(new.shape[0]):
        hit = torch.isin(new[b], torch.tensor(eos)).nonzero().flatten()
        n = int(hit[0]) + 1 if hit.numel() else new.shape[1]
        lp_sum = sum(float(torch.log_softmax(want.scores[t][b].float(), -1)[new[b, t]]) for t in range(n))
        out.append((new[b, :n].tolist(), lp_sum / (n ** lp)))
    return out


@pytest.mark.parametrize("case", GRID, ids=lambda c: "K%d-%s-lp%g-ret%d-eos%d" % c)
def test_beam_state_equals_transformers(runs, case, hf):
    K, early, lp, n_ret, n_eos = case
    want, got, st, facts = runs[case]
    assert st.C == max(2, 1 + n_eos) * K
    assert got.sequences_scores.dtype == torch.float32 and got.sequences_scores.shape == (2 * n_ret,)
    if K == 1:
        # transformers routes num_beams=1 to greedy decoding, so there is no beam output to compare with.  One beam is greedy until its best
        # candidate is an EOS id; that hypothesis takes the one finished slot.  early_stopping=True stops there: greedy's tokens up to and
        # including the EOS id, scored as a beam hypothesis.  The other two rules may go on with the runner-up and may only replace the
        # hypothesis by one that scores higher.
        for b, (toks, score) in enumerate(_greedy_hypothesis(want, hf.eos[:n_eos], lp)):
            same = got.sequences[b].tolist() == toks + [PAD] * (got.sequences.shape[1] - len(toks))
            if early is True or same:
                assert same, (b, got.sequences[b], toks)
                assert abs(float(got.sequences_scores[b]) - score) <= 1e-5 * abs(score), (b, float(got.sequences_scores[b]), score)
            else:
                assert float(got.sequences_scores[b]) > score, (b, float(got.sequences_scores[b]), score)
        return
    new = want.sequences[:, PROMPT:]
    assert got.sequences.shape == new.shape and torch.equal(got.sequences, new), (got.sequences, new)
    assert torch.allclose(got.sequences_scores, want.sequences_scores, rtol=1e-5, atol=0), (got.sequences_scores, want.sequences_scores)


def test_the_fixtures_are_not_vacuous(runs, hf):
    ended_early = {False: 0, True: 0}
    finished_early, staggered, finished_beats_running, gap = 0, 0, 0, float("inf")
    for (K, early, lp, n_ret, n_eos), (want, got, st, facts) in runs.items():
        eos = torch.tensor(hf.eos[:n_eos])
        lens = [int((row != PAD).sum()) for row in got.sequences]
        finished_early += any(n < MAX_NEW and bool(torch.isin(row[n - 1], eos)) for row, n in zip(got.sequences, lens))
        if facts["steps"] < MAX_NEW and early in (False, True):
            ended_early[early] += 1
        fc = facts["first_closed"]
        staggered += fc[0] != fc[1]
        gap = min(gap, facts["gap"])
        # the returned best is a finished hypothesis although a running beam held the higher raw score (sum of log-probabilities)
        for b in range(2):
            n = lens[b * n_ret]
            raw_best = float(got.sequences_scores[b * n_ret]) * (n ** lp)
            if n < MAX_NEW and float(st.run_scores[b, 0]) > raw_best and float(st.run_scores[b, 0]) > -1e8:
                finished_beats_running += 1
    print("grid of %d: hypotheses finished early in %d, loop ended early %s, prompts closed at different steps in %d, finished best under a "
          "running raw score in %d, smallest candidate gap %.3e" % (len(runs), finished_early, ended_early, staggered, finished_beats_running, gap))
    assert finished_early >= 1 and ended_early[False] >= 1 and ended_early[True] >= 1 and staggered >= 1 and finished_beats_running >= 1
    assert gap > GAP, gap


def test_ancestry_table_on_the_host(runs):
    """A fake own cache stores token ids as rows: member m writes its pushed token at own slot t; the gather through the table built by
    advance_reference from the parents BeamState recorded is every beam's pushed history, at every step.  Every case of the grid with more
    than one beam (with one beam every member is its own parent)."""
    seen = 0
    for (K, early, lp, n_ret, n_eos), (want, got, st, facts) in runs.items():
        if K == 1:
            continue
        M, Lown = st.M, MAX_NEW
        tables = [torch.full((M, Lown), -1, dtype=torch.int32), torch.full((M, Lown), -1, dtype=torch.int32)]
        cur = 0
        cache = torch.full((M, Lown), -1, dtype=torch.long)
        hist = [[] for _ in range(M)]
        for t, (parent, tok) in enumerate(zip(st.parents, st.pushed)):
            tables[1 - cur] = R.advance_reference(tables[cur], parent, torch.full((M,), t), tables[1 - cur])
            cur = 1 - cur
            cache[:, t] = tok                                   # the append: member m's own slot t
            hist = [hist[int(parent[m])] + [int(tok[m])] for m in range(M)]
            for m in range(M):
                via = cache[tables[cur][m, :t + 1].long(), torch.arange(t + 1)]
                assert via.tolist() == hist[m], (m, t)
            seen += bool((parent != torch.arange(M)).any()) and t > 0
    assert seen > 0          # some beam did continue another beam's history


# ------------------------------------------------------------------------------------------------
def test_argument_rules():
    from halva_amd.beam import MAX_BEAMS, MAX_CANDIDATES, BeamState, check_beam_args
    assert check_beam_args(1, 4) == (1, 1, 2) and check_beam_args(3, 4, n_eos=2, num_return_sequences=3) == (3, 3, 9)
    for bad in (0, -1, None, 1.5):
        with pytest.raises(ValueError):
            check_beam_args(bad, 4)
    for n_ret in (0, 4):
        with pytest.raises(ValueError):
            check_beam_args(3, 4, num_return_sequences=n_ret)
    for early in ("always", 1, None, "True"):
        with pytest.raises(ValueError):
            check_beam_args(3, 4, early_stopping=early)
    for early in (False, True, "never"):
        check_beam_args(3, 4, early_stopping=early)
    with pytest.raises(ValueError):
        check_beam_args(2, 0)
    with pytest.raises(ValueError, match="%d beams" % MAX_BEAMS):
        check_beam_args(MAX_BEAMS + 1, 4)
    with pytest.raises(ValueError, match="limit is %d" % MAX_CANDIDATES):
        check_beam_args(16, 4, n_eos=4)          # 5 * 16 candidates
    with pytest.raises(ValueError, match="at most 32768"):
        check_beam_args(2, 4, vocab=32769, max_vocab=32768)
    with pytest.raises(NotImplementedError, match="do_sample"):
        check_beam_args(2, 4, do_sample=True)
    with pytest.raises(NotImplementedError, match="stopping_criteria"):
        check_beam_args(2, 4, stopping_criteria=[lambda *a: False])
    with pytest.raises(ValueError):
        BeamState(1, 2, 4, num_return_sequences=3)


def _stub_session(lens=(5, 7), V=32):
    """A DecodeSession on host tensors, as tests/test_fork_cpu.py builds its parents: enough for every rule that fires before a launch."""
    from halva_amd import decode as DEC
    B = len(lens)
    kv = [torch.zeros(B, 2, 64, 128, dtype=torch.bfloat16) for _ in range(2)]
    cache = SimpleNamespace(B=B, H=2, D=128, Lcap=64, k=kv, v=kv, lens=torch.tensor([list(lens)] * 2, dtype=torch.int32), filled=max(lens),
                            cos=torch.zeros(64, 2), sin=torch.zeros(64, 2), rope=lambda n, dev: (torch.zeros(n, 2), torch.zeros(n, 2)))
    cfg = SimpleNamespace(eos_token_id=2, pad_token_id=0)
    return DEC.DecodeSession(None, cache, torch.zeros(B, V), list(lens), cfg), DEC


def test_session_rules_fire_before_any_launch():
    ses, DEC = _stub_session()
    with pytest.raises(ValueError):
        ses.beam_search(0, 4)
    with pytest.raises(ValueError):
        ses.beam_search(2, 4, num_return_sequences=3)
    with pytest.raises(ValueError):
        ses.beam_search(2, 4, early_stopping="sometimes")
    with pytest.raises(ValueError, match="16 beams"):
        ses.beam_search(17, 4)
    with pytest.raises(ValueError, match="limit is 64"):
        ses.beam_search(16, 4, eos_token_id=[2, 3, 4, 5])
    with pytest.raises(NotImplementedError, match="stopping_criteria"):
        ses.beam_search(2, 4, stopping_criteria=lambda *a: False)
    with pytest.raises(NotImplementedError, match="do_sample"):
        ses.beam_search(2, 4, do_sample=True)
    with pytest.raises(NotImplementedError, match="images"):
        ses.beam_search(2, 4, images=torch.zeros(1, 3, 8, 8))
    assert ses.lens == [5, 7] and ses.pending == [[], []]
    fk = DEC.ForkedSession(None, DEC.ForkCache(ses.cache, [0, 0, 1], 4, [5, 7]), torch.zeros(3, 32), ses.config)
    with pytest.raises(NotImplementedError, match="forked session"):
        fk.beam_search(2, 4)


def test_num_beams_through_generate_still_raises():
    from halva_amd import decode as DEC
    with pytest.raises(NotImplementedError):
        DEC.check_generate_args(2, False, 8)
    from halva_amd.multimodal import MultimodalMixin

    class Stub(MultimodalMixin):
        def _embed_prompt(self, *a):
            raise AssertionError("generate(num_beams=2) must be refused before the prompt is embedded")
    with pytest.raises(NotImplementedError, match="beam search"):
        Stub()._generate(torch.zeros(1, 3, dtype=torch.long), None, None, False, 2, 8, None, None, None)


def test_beam_cache_rules():
    ses, DEC = _stub_session()
    with pytest.raises(ValueError):
        DEC.BeamCache(ses.cache, 3, 2, 4, [5, 7])
    with pytest.raises(ValueError):
        DEC.BeamCache(ses.cache, 2, 0, 4, [5, 7])
    bc = DEC.BeamCache(ses.cache, 2, 3, 4, [5, 7])
    assert bc.host_prefix_of == [0, 0, 0, 1, 1, 1] and (bc.M, bc.Lown, bc.cur) == (6, 4, 0)
    assert bc.anc.dtype == torch.int32 and tuple(bc.anc.shape) == (2, 6, 4) and bc.table.data_ptr() == bc.anc[0].data_ptr()
