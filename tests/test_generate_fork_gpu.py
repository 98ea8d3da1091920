"""Forked sessions and generate(num_return_sequences=) end to end (halva_amd/decode.py: ForkCache, ForkedSession, sample_fork) on the small
d128 models of tests/generate_models_util.py and their goldens (tests/golden/generate_d128.npz, generate_vila.npz).

Bounds are tests/test_generate_session_gpu.py's (its module docstring), taken from its _Env: GOLD against the golden, ROW between two
cached paths."""
import numpy as np
import pytest
import torch

import sample_ref_util as S
from generate_models_util import build_llava, build_vila, pad_batch
from test_generate_session_gpu import N_GOLD, _Env

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["llava", "vila"])
def env(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    e = _Env(build_llava, "generate_d128.npz") if request.param == "llava" else _Env(build_vila, "generate_vila.npz")
    e.name = request.param
    e.new_only = (lambda out, T0: out[:, T0:]) if request.param == "llava" else (lambda out, T0: out)      # LLaVA returns the prompt too
    return e


def _start(env, extra=64, first=0, count=3):
    rows, images = env.prompts[first:first + count], env.images[first:first + count]
    ids, mask = pad_batch(rows)
    T = env.spliced(rows, images)[0].shape[1]
    return env.model.start_session(ids, images=images, attention_mask=mask, max_len=T + extra)


# What the goldens allow.  A step whose stored top-2 gap is below 4 x GOLD is too close to call between two correct implementations
# (tests/test_generate_gpu.py), and a free-running row that picks the other token there leaves the golden's history for good.  The stored
# gaps (host data): generate_d128 prompt 2 has every gap >= 0.14 - the only prompt of either file that meets "every gap exceeds the
# tolerance", so it is held to all 24 tokens.  The others dip to 4.4e-3 (d128 prompt 0, step 14), 3.4e-3 (d128 prompt 1, step 12), 2.0e-3,
# 7.0e-4 and 4.5e-3 (vila prompts 0, 1, 2; steps 2, 15, 14) against 4 x GOLD of 2.4e-2 .. 4.2e-2.  FREE[i]: the steps a free-running row is
# held to the golden for at least.  Every stored gap in front of them is at least 1.7 times the tolerance measured (d128: 0.067 at prompt 0
# step 0, 0.086 and more at prompt 1 steps 0 - 1; vila: 0.070 and more at prompt 0 steps 0 - 1, 0.043 and more at prompts 1 and 2 steps
# 0 - 9), and the step behind them is below it or close to it.  Under teacher forcing no row ever leaves the golden's history, so every
# step whose gap reaches 4 x GOLD is held to the golden's token: at least FORCED of the 24 per prompt (the files hold 11 to 24 steps per
# prompt with a gap of 0.05 or more).
FREE = {"llava": (1, 2, 24), "vila": (2, 10, 10)}
FORCED = 11


def test_greedy_fork_gives_the_golden_tokens_for_every_member(env):
    from halva_amd import decode as DEC
    decided = []
    for i in range(3):
        close = (env.gap[i][:N_GOLD] < 4 * env.gold(i)).nonzero().flatten().tolist()
        decided.append(close[0] if close else N_GOLD)
        print("%s prompt %d: smallest top-2 gap %.3e, 4 x GOLD %.3e, steps decided %d" % (env.name, i, float(env.gap[i][:N_GOLD].min()),
                                                                                          4 * env.gold(i), decided[i]))
        assert decided[i] >= FREE[env.name][i], (i, decided[i])
    if env.name == "llava":          # the fixture condition, where it holds: every stored gap of prompt 2 exceeds the tolerance
        assert float(env.gap[2][:N_GOLD].min()) > 4 * env.gold(2) and decided[2] == N_GOLD
    fk = _start(env).fork(3, max_new=N_GOLD)
    assert fk.prefix_of == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    out = fk.generate(N_GOLD, eos_token_id=[])
    assert out.shape == (9, N_GOLD)
    for m in range(9):
        i = m // 3
        assert out[m, :decided[i]].tolist() == env.toks[i][:decided[i]].tolist(), m
        assert torch.equal(out[m], out[3 * i]), m          # behind the first close step, still one answer per prompt, bit for bit
    # teacher forced: the members' logits against the golden's at all 24 steps, and the golden's token wherever its gap decides
    ses = _start(env)
    fk = ses.fork(prefix_of=[0, 1, 1, 2], max_new=N_GOLD)
    lg, of = fk.logits, [0, 1, 1, 2]
    held = [0, 0, 0]
    for s in range(N_GOLD):
        for m, i in enumerate(of):
            d = float((lg[m].double().cpu() - env.glog[i][s]).abs().max())
            assert d <= env.gold(i), (m, s, d, env.gold(i))
            if float(env.gap[i][s]) >= 4 * env.gold(i):
                assert int(lg[m].argmax()) == int(env.toks[i][s]), (m, s)
                held[i] += m != 2
        if s + 1 < N_GOLD:
            lg = DEC.decode_step(env.model, fk.cache, torch.stack([env.toks[i][s] for i in of]).cuda())
    print("%s: steps held to the golden's token under teacher forcing %s of %d" % (env.name, held, N_GOLD))
    assert min(held) >= FORCED, held
    assert torch.equal(lg[1], lg[2])                      # two members with one history: the same bits


def test_sampling_with_num_return_sequences(env):
    model = env.model
    ids, mask = pad_batch(env.prompts)
    n, steps, temp, top_k, top_p = 4, 6, 0.9, 20, 0.95
    kw = dict(images=env.images, attention_mask=mask, max_new_tokens=steps, eos_token_id=[], do_sample=True, temperature=temp, top_k=top_k, top_p=top_p)
    gen = lambda seed: torch.Generator(device="cuda").manual_seed(seed)      # noqa: E731
    a = model.generate(ids, num_return_sequences=n, generator=gen(7), **kw)
    b = model.generate(ids, num_return_sequences=n, generator=gen(7), **kw)
    assert torch.equal(a, b)
    new = env.new_only(a, ids.shape[1])
    assert new.shape == (3 * n, steps)
    if env.name == "llava":
        assert torch.equal(a[:, :ids.shape[1]], ids.cuda().repeat_interleave(n, 0))
    one = model.generate(ids, num_return_sequences=1, generator=gen(7), **kw)
    assert torch.equal(one, model.generate(ids, generator=gen(7), **kw))
    with pytest.raises(ValueError):
        model.generate(ids, num_return_sequences=n, **dict(kw, do_sample=False))
    # row b * n + i depends on its own u stream alone: replay each step's u through the fp64 semantics on the member's own logits
    from halva_amd import decode as DEC
    g = gen(7)
    fk = _start(env).fork(n, max_new=steps)
    lg = fk.logits
    for s in range(steps):
        u = torch.rand(3 * n, device="cuda", generator=g).cpu().numpy()
        l64 = lg.double().cpu().numpy()
        for m in range(3 * n):
            ref = S.sample_ref(l64[m], temp, top_k, top_p)
            tok = int(new[m, s])
            # the drawn token must be one the reference admits within the band DELTA on cumulative mass (tests/test_sample_kernel_gpu.py)
            lo = ref.cdf[tok - 1] if tok > 0 else 0.0
            assert ref.K2[tok] and lo - S.DELTA <= u[m] < ref.cdf[tok] + S.DELTA, (m, s, tok, float(u[m]), S.draw(ref.cdf, ref.K2, u[m]))
        if s + 1 < steps:
            lg = DEC.decode_step(model, fk.cache, new[:, s].cuda())
    assert np.isfinite(l64).all()


def test_questions_forked_from_one_prompt(env):
    from halva_amd import decode as DEC
    model, row = env.model, env.row()
    i = 1
    ses = _start(env, extra=80, first=i, count=1)
    g = torch.Generator().manual_seed(9)
    vocab = model.get_model().embed_tokens.weight.shape[0]
    suffix = [torch.randint(1, vocab, (k,), generator=g) for k in (1, 31, 33)]
    fk = ses.fork(3, max_new=33 + 6)
    sids, smask = pad_batch(suffix)
    fk.append(sids, smask)
    assert fk.lens == [1, 31, 33] and fk.cache.own_lens.tolist() == [[1, 31, 33]] * len(fk.cache.k)
    kept = fk.logits.clone()
    out = fk.generate(4, eos_token_id=[])
    for m, sfx in enumerate(suffix):
        fresh = model.start_session(torch.cat([env.prompts[i], sfx])[None], images=env.images[i:i + 1], max_len=ses.cache.Lcap + 40)
        assert fresh.lens == [ses.lens[0] + len(sfx)]
        d = float((fresh.logits[0] - kept[m]).abs().max())
        print("%s member %d (%d ids): |forked append - fresh prefill| %.3e (3 x ROW = %.3e)" % (env.name, m, len(sfx), d, 3 * row))
        assert d <= 3 * row, m
        lg = fresh.logits
        for s in range(4):
            top2 = lg[0].topk(2)
            if float(top2.values[0] - top2.values[1]) < 4 * row:
                break
            assert int(out[m, s]) == int(top2.indices[0]), (m, s)
            lg = DEC.decode_step(model, fresh.cache, top2.indices[:1])


def test_parent_appended_to_after_the_fork_leaves_the_forks_alone(env):
    from halva_amd import decode as DEC
    tok = torch.tensor([5, 9, 11, 5, 9, 11]).cuda()
    ses = _start(env, count=2)
    fk = ses.fork(3, max_new=8)
    want = DEC.decode_step(env.model, fk.cache, tok).clone()
    ses2 = _start(env, count=2)
    fk2 = ses2.fork(3, max_new=8)
    ses2.append(torch.tensor([[7, 8, 9], [10, 11, 12]]))
    ses2.generate(3, eos_token_id=[])
    got = DEC.decode_step(env.model, fk2.cache, tok)
    assert torch.equal(got, want)
    assert fk2.cache.prefix_lens.tolist() == fk.cache.prefix_lens.tolist()
    assert all(a >= b + 5 for a, b in zip(ses2.lens, fk.cache.prefix_lens.tolist()))          # the parent did move on
