"""Contrastive decoding end to end (halva_amd/decode.py:contrast; generate(images_cd= / negative_input_ids= / guidance_scale=) of both
wrappers) on the small d128 models of tests/generate_models_util.py, LLaVA and VILA.

Bounds.  ROW is tests/test_generate_session_gpu.py's: what two cache-free forwards that differ only in row grouping disagree by, the measure
of how far one cached path's logits lie from another's (within 3 x ROW there).  The contrast loop holds its 2 B rows in one cache; the
references below hold B rows, so their logits l and lcd may each differ from the loop's by E = 3 x ROW and x = (1 + a) l - a lcd by
(1 + 2 a) E.  A step of the fp64 reference is decided when its best column is plausible by more than 2 E, and leads every column that could
be plausible (l >= cut - 2 E) by more than 2 (1 + 2 a) E in x; the loop's token must be the reference's on every decided step, and at most a
quarter of the steps may be left undecided."""
import numpy as np
import pytest
import torch

import contrast_ref_util as C
from generate_models_util import build_llava, build_vila, pad_batch
from test_generate_session_gpu import _Env

pytestmark = pytest.mark.gpu

STEPS = 12


@pytest.fixture(scope="module", params=["llava", "vila"])
def env(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    e = _Env(build_llava, "generate_d128.npz") if request.param == "llava" else _Env(build_vila, "generate_vila.npz")
    e.name = request.param
    return e


def _new(env, out, ids):
    """The new tokens of a generate() result: LLaVA returns the prompt in front, VILA does not."""
    return out[:, ids.shape[1]:] if env.name == "llava" else out


def _batch(env, count=2):
    rows, images = env.prompts[:count], env.images[:count]
    ids, mask = pad_batch(rows)
    return rows, images, ids, mask


def _noisy(images, seed=0, step=500):
    from halva_amd.contrast import add_diffusion_noise
    return add_diffusion_noise(images, step, generator=torch.Generator(device=images.device).manual_seed(seed))


def _forced_logits(env, rows, images, toks):
    """The logits in front of each of toks [B, n], teacher-forced through an ordinary session -> fp32 [n, B, V] on the host."""
    n = toks.shape[1]
    ids, mask = pad_batch(rows)
    T = env.spliced(rows, images)[0].shape[1]
    ses = env.model.start_session(ids, images=images, attention_mask=mask, max_len=T + n + 1)
    out = [ses.logits.float().cpu()]
    for s in range(n - 1):
        ses.append(toks[:, s:s + 1].cpu())
        out.append(ses.logits.float().cpu())
    return torch.stack(out)


def test_the_same_images_with_alpha_one_is_plain_greedy(env):
    """images_cd = images, alpha = 1, beta = 0: x = 2 l - l = l exactly, so the loop is greedy decoding on rows of a 2 B batch.  Held to plain
    generate up to the first step whose top-2 gap is below 4 x ROW (the rule of tests/test_generate_beam_gpu.py)."""
    rows, images, ids, mask = _batch(env)
    kw = dict(images=images, attention_mask=mask, max_new_tokens=STEPS, eos_token_id=[])
    plain = _new(env, env.model.generate(ids, **kw), ids)
    got = _new(env, env.model.generate(ids, images_cd=images, cd_alpha=1.0, cd_beta=0.0, **kw), ids)
    assert got.shape == plain.shape == (2, STEPS)
    lg = _forced_logits(env, rows, images, plain).double()
    row = env.row()
    for b in range(2):
        held = STEPS
        for s in range(STEPS):
            top2 = lg[s, b].topk(2).values
            if float(top2[0] - top2[1]) < 4 * row:
                held = s
                break
        print("%s prompt %d: %d of %d steps held to plain greedy" % (env.name, b, held, STEPS))
        assert held >= 1 and got[b, :held].tolist() == plain[b, :held].tolist(), (b, got[b], plain[b])


def _decided(l, lcd, alpha, beta, E):
    """-> (the reference's token, whether the step is decided) for fp64 rows l, lcd (module docstring)."""
    cut = l.max() + (np.log(beta) if beta > 0 else -np.inf)
    x = (1 + alpha) * l - alpha * lcd
    sure = np.where(l >= cut, x, -np.inf)
    maybe = np.where(l >= cut - 2 * E, x, -np.inf)
    best = int(sure.argmax())
    rest = np.delete(maybe, best)
    lead = sure[best] - (rest.max() if len(rest) else -np.inf)
    return best, bool(l[best] >= cut + 2 * E and lead > 2 * (1 + 2 * alpha) * E)


NOISE_SEED = 0          # chosen on the GPU so that the reference leaves at most a quarter of the steps undecided in every case below


def _reference_run(env, alpha, beta, seed):
    """generate(images_cd = the images under diffusion noise) against the fp64 reference on the logits of two ordinary sessions that are
    teacher-forced along the loop's tokens -> (decided steps, steps, [(row, step, got, want)] of decided steps that disagree)."""
    rows, images, ids, mask = _batch(env)
    noisy = _noisy(images, seed=seed)
    assert not torch.equal(noisy, images)
    got = _new(env, env.model.generate(ids, images=images, attention_mask=mask, max_new_tokens=STEPS, eos_token_id=[], images_cd=noisy,
                                       cd_alpha=alpha, cd_beta=beta), ids)
    l = _forced_logits(env, rows, images, got).double().numpy()
    lcd = _forced_logits(env, rows, noisy, got).double().numpy()
    assert float(np.abs(l - lcd).max()) > 0, "the contrast branch saw the same logits"
    E = 3 * env.row()
    n_decided, wrong = 0, []
    for b in range(2):
        for s in range(STEPS):
            want, decided = _decided(l[s, b], lcd[s, b], alpha, beta, E)
            n_decided += decided
            if decided:
                # (the float32 reference of the kernel tests says the same on these logits)
                assert C.contrast_token(l[s, b], lcd[s, b], alpha, beta, 1.0, 1, 1.0, 0.0) == want
                if int(got[b, s]) != want:
                    wrong.append((b, s, int(got[b, s]), want))
    print("%s alpha=%g beta=%g seed=%d: %d of %d steps decided (E = %.3e), %d wrong" % (env.name, alpha, beta, seed, n_decided, 2 * STEPS, E,
                                                                                      len(wrong)))
    return n_decided, 2 * STEPS, wrong


@pytest.mark.parametrize("alpha,beta", [(0.5, 0.1), (1.0, 0.0)])
def test_against_the_reference_on_teacher_forced_logits(env, alpha, beta):
    """Genuinely different images_cd: the loop's token is the reference's on every decided step, and at most a quarter of the steps are
    left undecided."""
    n_decided, n, wrong = _reference_run(env, alpha, beta, NOISE_SEED)
    assert not wrong, (env.name, wrong)
    assert n - n_decided <= n // 4, (n_decided, n)


def test_sampling_with_a_fixed_generator_is_reproducible(env):
    rows, images, ids, mask = _batch(env)
    noisy = _noisy(images, seed=3)
    kw = dict(images=images, attention_mask=mask, max_new_tokens=STEPS, eos_token_id=[], images_cd=noisy, do_sample=True, temperature=1.0,
              top_k=20, top_p=0.9)
    g = lambda seed: torch.Generator(device="cuda").manual_seed(seed)      # noqa: E731
    a = env.model.generate(ids, generator=g(5), **kw)
    b = env.model.generate(ids, generator=g(5), **kw)
    c = env.model.generate(ids, generator=g(6), **kw)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert int(_new(env, a, ids).min()) >= 0


def _padded_after(free, eos, pad):
    """What the loop must return when `eos` ends a row: each row of `free` up to and including its first eos, then pad; cut to the step
    after which every row is done."""
    want = free.clone()
    ends = []
    for b in range(free.shape[0]):
        hit = (free[b] == eos).nonzero()
        at = int(hit[0]) if len(hit) else free.shape[1] - 1
        want[b, at + 1:] = pad
        ends.append(at)
    return want[:, :max(ends) + 1], ends


def test_a_finished_row_does_not_disturb_the_others(env):
    """Three prompts; the EOS id is taken from the free run so that the rows finish at different steps.  Rows are independent in every
    kernel of a step, so the rows that go on must emit exactly what they emitted in the free run."""
    rows, images, ids, mask = _batch(env, 3)
    noisy = _noisy(images, seed=NOISE_SEED)
    kw = dict(images=images, attention_mask=mask, max_new_tokens=STEPS, images_cd=noisy, pad_token_id=0)
    g = lambda: torch.Generator(device="cuda").manual_seed(11)      # noqa: E731
    for skw in (dict(), dict(do_sample=True, temperature=1.0, top_k=0, top_p=1.0)):
        free = _new(env, env.model.generate(ids, eos_token_id=[], generator=g(), **kw, **skw), ids).cpu()
        spread = {t: _padded_after(free, t, 0)[1] for t in sorted(set(free[:, :STEPS - 2].flatten().tolist())) if t != 0}
        eos = max(spread, key=lambda t: (len(set(spread[t])), -min(spread[t])))
        print("%s %s: free run %s, eos %d ends the rows at %s" % (env.name, "sampled" if skw else "greedy", free.tolist(), eos, spread[eos]))
        assert len(set(spread[eos])) > 1, "the fixture needs rows that finish at different steps"
        want, _ = _padded_after(free, eos, 0)
        got = _new(env, env.model.generate(ids, eos_token_id=[eos], generator=g(), **kw, **skw), ids).cpu()
        assert got.tolist() == want.tolist()


def test_negative_prompt_of_another_length_and_the_guidance_alias(env):
    rows, images, ids, mask = _batch(env)
    neg_rows = [r[:len(r) - 5] for r in rows] if env.name == "llava" else [r[:len(r) - 3] for r in rows]
    neg, neg_mask = pad_batch(neg_rows)
    assert neg.shape[1] != ids.shape[1]
    kw = dict(images=images, attention_mask=mask, max_new_tokens=STEPS, eos_token_id=[], negative_input_ids=neg, negative_attention_mask=neg_mask)
    a = env.model.generate(ids, guidance_scale=1.5, **kw)
    b = env.model.generate(ids, cd_alpha=0.5, cd_beta=0.0, **kw)
    assert torch.equal(a, b)
    new = _new(env, a, ids)
    assert new.shape == (2, STEPS) and int(new.min()) >= 0
    # text only, shorter than the prompt's spliced rows
    text = torch.tensor([[5, 6, 7], [9, 8, 0]])
    c = env.model.generate(ids, images=images, attention_mask=mask, max_new_tokens=4, eos_token_id=[], negative_input_ids=text,
                           negative_attention_mask=text != 0, guidance_scale=2.0)
    assert _new(env, c, ids).shape == (2, 4)


def test_output_shapes_per_family(env):
    rows, images, ids, mask = _batch(env, 3)
    out = env.model.generate(ids, images=images, attention_mask=mask, max_new_tokens=5, eos_token_id=[], images_cd=_noisy(images))
    assert out.dtype == torch.long and out.is_cuda
    if env.name == "llava":
        assert out.shape == (3, ids.shape[1] + 5) and torch.equal(out[:, :ids.shape[1]].cpu(), ids)
    else:
        assert out.shape == (3, 5)
    crit_calls = []

    def crit(seq, logits):
        crit_calls.append((tuple(seq.shape), tuple(logits.shape)))
        return len(crit_calls) >= 2
    out = env.model.generate(ids, images=images, attention_mask=mask, max_new_tokens=5, eos_token_id=[], images_cd=_noisy(images),
                             stopping_criteria=[crit])
    assert _new(env, out, ids).shape == (3, 2) and crit_calls[0][0] == (3, (ids.shape[1] if env.name == "llava" else 0) + 1)
    assert crit_calls[0][1][0] == 3


def test_refusals(env):
    rows, images, ids, mask = _batch(env)
    kw = dict(images=images, attention_mask=mask, max_new_tokens=4)
    for bad in (dict(images_cd=images, negative_input_ids=ids), dict(images_cd=images, num_beams=2),
                dict(images_cd=images, num_return_sequences=2, do_sample=True, temperature=1.0), dict(cd_alpha=0.5), dict(guidance_scale=1.5),
                dict(images_cd=images, cd_beta=1.5), dict(images_cd=images, cd_alpha=-1.0), dict(images_cd=images, guidance_scale=0.5),
                dict(images_cd=images, guidance_scale=2.0, cd_alpha=1.0), dict(negative_attention_mask=mask)):
        with pytest.raises(ValueError):
            env.model.generate(ids, **dict(kw, **bad))
    plain = env.model.generate(ids, eos_token_id=[], **kw)                   # and without contrast arguments: the old path, the same bits
    assert torch.equal(plain, env.model.generate(ids, eos_token_id=[], **kw))
