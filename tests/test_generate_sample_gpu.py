"""generate(do_sample=True, ...) of both wrappers (halva_amd/decode.py:sample on halva_sample_top_k_top_p) on the small d128 LLaVA and VILA
models and the prompts of generate_d128.npz / generate_vila.npz.  LLaVA returns [B, T + n], VILA the n new tokens."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from generate_models_util import build_llava, build_vila, pad_batch  # noqa: E402
from sample_ref_util import DELTA, sample_ref  # noqa: E402

N_NEW = 12


class _Wrapper:
    def __init__(self, kind):
        self.kind = kind
        self.model, self.prompts, self.images = (build_llava if kind == "llava" else build_vila)()
        self.ids, self.mask = pad_batch(self.prompts)

    def new_tokens(self, out, T):
        return out[:, T:] if self.kind == "llava" else out

    def one(self, i, **kw):
        p = self.prompts[i]
        kw.setdefault("eos_token_id", [])
        return self.new_tokens(self.model.generate(p[None], images=self.images[i:i + 1], **kw), len(p))

    def batch(self, **kw):
        kw.setdefault("eos_token_id", [])
        return self.new_tokens(self.model.generate(self.ids, images=self.images, attention_mask=self.mask, **kw), self.ids.shape[1])


@pytest.fixture(scope="module", params=["llava", "vila"])
def wr(request):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return _Wrapper(request.param)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def test_top_k_1_is_greedy(wr):
    for i in range(3):
        greedy = wr.one(i, max_new_tokens=N_NEW)
        sampled = wr.one(i, max_new_tokens=N_NEW, do_sample=True, temperature=1.0, top_k=1, generator=_gen(i))
        assert torch.equal(greedy, sampled), (i, greedy.tolist(), sampled.tolist())
    assert torch.equal(wr.batch(max_new_tokens=N_NEW), wr.batch(max_new_tokens=N_NEW, do_sample=True, temperature=1.0, top_k=1, generator=_gen(9)))


def test_the_generator_decides_the_tokens(wr):
    kw = dict(max_new_tokens=N_NEW, do_sample=True, temperature=2.0, top_k=0)
    a, b, c = wr.batch(generator=_gen(1), **kw), wr.batch(generator=_gen(1), **kw), wr.batch(generator=_gen(2), **kw)
    assert a.shape == (3, N_NEW) and a.dtype == torch.long
    assert torch.equal(a, b) and not torch.equal(a, c)
    # the default generator: seeded the same way, the same tokens
    torch.manual_seed(5)
    d = wr.batch(**kw)
    torch.manual_seed(5)
    assert torch.equal(d, wr.batch(**kw))


@pytest.mark.parametrize("T,k,p", [(0.2, None, 0.7), (1.0, 0, 0.9)])
def test_every_sampled_token_lies_in_the_kept_set_of_its_logits(wr, T, k, p):
    """A stopping criterion sees (seq, logits) after every step: the token just appended to row b was drawn from logits[b], so it lies in
    the fp64 kept set of that row, up to the band on the mass above it (top-k, a count, exactly)."""
    seen = []

    def spy(seq, logits):
        seen.append((seq[:, -1].clone(), logits.clone()))
        return False
    out = wr.batch(max_new_tokens=N_NEW, do_sample=True, temperature=T, top_k=k, top_p=p, generator=_gen(3), stopping_criteria=[spy])
    assert len(seen) == N_NEW and out.shape == (3, N_NEW)
    for s, (tok, logits) in enumerate(seen):
        assert torch.equal(tok, out[:, s]) and logits.dtype == torch.float32
        for b in range(3):
            ref = sample_ref(logits[b].cpu().numpy(), T, 50 if k is None else k, p)
            t = int(tok[b])
            assert ref.K1[t] and ref.S[t] < float(np.float32(p)) + DELTA and ref.x[t] > -np.inf, (s, b, t, float(ref.S[t]))


def test_a_row_that_samples_eos_is_padded_and_the_others_do_not_change(wr):
    """One u per row and step whether or not rows are done: ending row 0 early leaves the other rows' tokens as they were."""
    kw = dict(max_new_tokens=N_NEW, do_sample=True, temperature=1.5, top_k=0, top_p=0.95)
    free = wr.batch(generator=_gen(11), **kw)
    eos = int(free[0, 1])
    stopped = wr.batch(generator=_gen(11), eos_token_id=eos, pad_token_id=0, **kw)
    n = stopped.shape[1]
    for b in range(3):
        row = free[b].tolist()
        end = row.index(eos) + 1 if eos in row else N_NEW
        assert stopped[b, :min(end, n)].tolist() == row[:min(end, n)], (b, stopped[b].tolist(), row)
        assert (stopped[b, end:] == 0).all()
    # the batch ends when its last row does
    assert n == max((free[b].tolist().index(eos) + 1 if eos in free[b].tolist() else N_NEW) for b in range(3))


def test_refusals_and_validation(wr):
    with pytest.raises(NotImplementedError, match="explicit temperature"):
        wr.one(0, max_new_tokens=2, do_sample=True)
    with pytest.raises(NotImplementedError):
        wr.one(0, max_new_tokens=2, num_beams=2)
    with pytest.raises(ValueError):
        wr.one(0, max_new_tokens=2, do_sample=True, temperature=0)
    with pytest.raises(ValueError):
        wr.one(0, max_new_tokens=2, do_sample=True, temperature=1.0, top_p=0)
    with pytest.raises(ValueError):
        wr.one(0, max_new_tokens=2, do_sample=True, temperature=1.0, top_k=-1)
    assert torch.equal(wr.one(1, max_new_tokens=N_NEW, do_sample=False, temperature=0), wr.one(1, max_new_tokens=N_NEW))
    assert torch.equal(wr.one(1, max_new_tokens=N_NEW, do_sample=False, temperature=0.2, top_p=0.7), wr.one(1, max_new_tokens=N_NEW))


def test_a_row_without_a_token_to_sample_raises(wr, monkeypatch):
    """NaN logits in a live row: the kernel's -1 rides on the step's host sync and raises, naming the row."""
    from halva_amd import decode as DEC
    head = DEC._lm_head

    def poisoned(st, h):
        out = head(st, h)
        out[1, 7] = float("nan")
        return out
    monkeypatch.setattr(DEC, "_lm_head", poisoned)
    with pytest.raises(RuntimeError, match="row 1"):
        wr.batch(max_new_tokens=3, do_sample=True, temperature=1.0, generator=_gen(0))
