"""Contrastive decoding without a GPU: the reference's own properties (tests/contrast_ref_util.py), its agreement with transformers'
classifier-free guidance, the row builders' margins, the argument checks of generate and of halva_contrast_select, and
halva_amd/contrast.py:add_diffusion_noise."""
import ctypes

import numpy as np
import pytest
import torch

import contrast_ref_util as C
from sample_ref_util import sample_ref

CASES = ((0.5, 0.1), (1.0, 0.0), (0.0, 0.5), (2.0, 1.0))
VS = (1, 5, 4095, 4096, 4097, 32000, 32768)


def _pair(V, seed):
    rng = np.random.default_rng(seed)
    l = (4.0 * rng.standard_normal(V)).astype(np.float32)
    return l, (l + rng.standard_normal(V)).astype(np.float32)


def test_beta_one_keeps_only_the_maxima_and_beta_zero_masks_nothing():
    l, lcd = _pair(257, 1)
    l[[3, 77]] = l.max() + 1.0
    x, plausible = C.contrast_x(l, lcd, 0.5, 1.0)
    assert np.flatnonzero(plausible).tolist() == [3, 77] and (x[~plausible] == -np.inf).all() and np.isfinite(x[plausible]).all()
    l[5] = -np.inf
    x, plausible = C.contrast_x(l, lcd, 0.5, 0.0)
    assert plausible.all() and x[5] == -np.inf and np.isfinite(np.delete(x, 5)).all()
    x, plausible = C.contrast_x(l, lcd, 0.5, 0.1)
    assert np.array_equal(plausible, l.astype(np.float64) >= l.max() + np.log(0.1))


def test_x_is_float32_product_product_difference():
    l, lcd = _pair(4097, 2)
    for alpha in (0.5, 1.0, 2.0, 0.3):
        a = np.float32(alpha)
        g1 = np.float32(1) + a
        want = np.array([np.float32(np.float32(g1 * li) - np.float32(a * ci)) for li, ci in zip(l, lcd)], dtype=np.float32)
        x, _ = C.contrast_x(l, lcd, alpha, 0.0)
        assert x.tobytes() == want.tobytes()
    x, _ = C.contrast_x(l, l, 1.0, 0.0)                   # 2 l - l = l exactly: what the generate test leans on
    assert x.tobytes() == l.tobytes()
    x, _ = C.contrast_x(l, lcd, 0.0, 0.0)                 # alpha = 0: l - 0 = l
    assert x.tobytes() == l.tobytes()


def test_a_masked_columns_lcd_does_not_matter():
    l, lcd = _pair(257, 3)
    x0, plausible = C.contrast_x(l, lcd, 0.5, 0.1)
    masked = np.flatnonzero(~plausible)
    assert len(masked) > 3
    lcd2 = lcd.copy()
    lcd2[masked[:3]] = (np.nan, np.inf, -np.inf)
    assert C.contrast_x(l, lcd2, 0.5, 0.1)[0].tobytes() == x0.tobytes() and C.servable(l, lcd2, 0.5, 0.1)
    lcd2[np.flatnonzero(plausible)[0]] = np.nan
    assert not C.servable(l, lcd2, 0.5, 0.1)


@pytest.mark.parametrize("alpha,beta", CASES)
def test_raw_logit_form_equals_log_softmax_form(alpha, beta):
    """VCD states the rule on logits, HF's guidance on log-softmax: g * (s - s_u) + s_u = (1 + a) s - a s_u.  Tie-free fp64 rows: the same
    kept set and, to fp64 rounding, the same probabilities."""
    rng = np.random.default_rng(11)
    for T, k, p in ((1.0, 0, 1.0), (0.2, 50, 0.7), (1.0, 1, 1.0)):
        l = 4.0 * rng.standard_normal(513)
        lcd = l + rng.standard_normal(513)
        lse = lambda v: v - (np.log(np.exp(v - v.max()).sum()) + v.max())      # noqa: E731
        s, su = lse(l), lse(lcd)
        plausible = l >= l.max() + (np.log(beta) if beta > 0 else -np.inf)
        raw = np.where(plausible, (1 + alpha) * l - alpha * lcd, -np.inf)
        hf = np.where(plausible, (1 + alpha) * (s - su) + su, -np.inf)
        assert np.array_equal(plausible, s >= s.max() + (np.log(beta) if beta > 0 else -np.inf))
        a, b = sample_ref(raw, T, k, p), sample_ref(hf, T, k, p)
        assert np.array_equal(a.K2, b.K2) and np.abs(a.cdf - b.cdf).max() < 1e-12


def test_against_transformers_classifier_free_guidance():
    """HF's UnbatchedClassifierFreeGuidanceLogitsProcessor computes g * (log_softmax(l) - log_softmax(l_u)) + log_softmax(l_u); with
    g = 1 + alpha and beta = 0 the reference keeps the same set and picks the same argmax.  The processor itself needs a model to produce
    l_u, so its arithmetic is taken from the class when transformers has it (the formula is one line of its __call__) and restated here."""
    try:
        from transformers.generation.logits_process import UnbatchedClassifierFreeGuidanceLogitsProcessor as P
    except ImportError:
        P = None
    rng = np.random.default_rng(5)
    for g in (1.0, 1.5, 3.0):
        l = 4.0 * rng.standard_normal(1000)
        lu = l + rng.standard_normal(1000)

        if P is not None:
            class _Stub(P):
                def __init__(self, scale, lu):
                    self.guidance_scale, self._lu = scale, lu

                def get_unconditional_logits(self, input_ids):
                    return self._lu
            out = _Stub(g, torch.as_tensor(lu)[None, None])(torch.zeros(1, 1, dtype=torch.long), torch.as_tensor(l)[None])[0].numpy()
        else:
            s, su = torch.log_softmax(torch.as_tensor(l), -1), torch.log_softmax(torch.as_tensor(lu), -1)
            out = (g * (s - su) + su).numpy()
        for T, k, p in ((1.0, 0, 1.0), (0.7, 50, 0.9), (1.0, 1, 1.0)):
            want = sample_ref(out, T, k, p)
            raw = (1 + (g - 1)) * l - (g - 1) * lu
            got = sample_ref(raw, T, k, p)
            assert np.array_equal(want.K2, got.K2) and np.abs(want.cdf - got.cdf).max() < 1e-12
            assert int(np.argmax(out)) == int(np.argmax(raw))


@pytest.mark.parametrize("V", VS)
def test_the_builders_keep_decisions_clear_of_fp32_rounding(V):
    l, lcd = C.pair_rows(V, 300 + V)
    for alpha, beta in CASES:
        for b in range(l.shape[0]):
            cut_margin, top_margin = C.margins(l[b], lcd[b], alpha, beta)
            assert cut_margin > 0 and top_margin > 0, (V, alpha, beta, b, cut_margin, top_margin)
            x, plausible = C.contrast_x(l[b], lcd[b], alpha, beta)
            xe, pe = C.x_exact(l[b], lcd[b], alpha, beta)
            assert np.array_equal(plausible, pe) and int(x.argmax()) == int(xe.argmax())
            assert (np.abs(x[plausible].astype(np.float64) - xe[plausible]) <= C.x_rounding(l[b], lcd[b], alpha)[plausible]).all()
            assert C.servable(l[b], lcd[b], alpha, beta)
            assert C.contrast_token(l[b], lcd[b], alpha, beta, 1.0, 1, 1.0, 0.0) == int(xe.argmax())


def test_contrast_select_argument_validation_without_gpu():
    """halva_contrast_select validates before launching: each bad argument returns HALVA_ERR_INVALID_ARG with a message."""
    from halva_amd import hip
    lib = hip.load()
    P = ctypes.c_void_p
    ok = dict(logits=P(64), ld=8, logits_cd=P(64), ld_cd=9, u=P(64), token=P(64), thr=None, kept=None, plausible=None, B=2, V=8, alpha=0.5,
              log_beta=-1.0, temperature=1.0, top_k=0, top_p=1.0)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.halva_contrast_select(a["logits"], a["ld"], a["logits_cd"], a["ld_cd"], a["u"], a["token"], a["thr"], a["kept"],
                                         a["plausible"], a["B"], a["V"], a["alpha"], a["log_beta"], a["temperature"], a["top_k"], a["top_p"],
                                         None)
    nan, inf = float("nan"), float("inf")
    for kw, msg in ((dict(logits=None), b"null pointer"), (dict(logits_cd=None), b"null pointer"), (dict(u=None), b"null pointer"),
                    (dict(token=None), b"null pointer"), (dict(V=0), b"V=0"), (dict(B=0), b"B=0"), (dict(ld=7), b"row stride"),
                    (dict(ld_cd=7), b"contrast row stride"), (dict(alpha=-0.5), b"alpha"), (dict(alpha=inf), b"alpha"),
                    (dict(alpha=nan), b"alpha"), (dict(log_beta=0.5), b"log_beta"), (dict(log_beta=nan), b"log_beta"),
                    (dict(top_p=1.5), b"top_p"), (dict(top_p=0.0), b"top_p"), (dict(temperature=0.0), b"temperature"),
                    (dict(temperature=inf), b"temperature"), (dict(temperature=nan), b"temperature"), (dict(top_k=-1), b"top_k")):
        assert rc(**kw) == -1 and msg in lib.halva_last_error(), (kw, lib.halva_last_error())
    cap = lib.halva_sample_max_vocab()
    assert rc(V=cap + 1, ld=cap + 1, ld_cd=cap + 1) == -1 and str(cap).encode() in lib.halva_last_error()


def test_check_contrast_args():
    from halva_amd.decode import check_contrast_args as chk
    none = (False, False, False, None, None, None)
    assert chk(*none, 1, 1) is None and chk(*none, 4, 3) is None           # no contrast argument: the old path, whatever else is asked
    assert chk(True, False, False, None, None, None, 1, 1) == (0.5, 0.1)
    assert chk(False, True, True, 1.0, 0.0, None, None, None) == (1.0, 0.0)
    assert chk(False, True, False, None, None, 1.5, 1, 1) == (0.5, 0.0)
    assert chk(True, False, False, 0, 1, None, 1, 1) == (0.0, 1.0)
    for args in ((True, True, False, None, None, None, 1, 1),              # both branches
                 (False, False, False, 0.5, None, None, 1, 1),             # weights without a branch
                 (False, False, False, None, 0.1, None, 1, 1),
                 (False, False, False, None, None, 2.0, 1, 1),
                 (False, False, True, None, None, None, 1, 1),             # a mask without its ids
                 (True, False, True, None, None, None, 1, 1),
                 (True, False, False, None, None, None, 2, 1),             # beams
                 (True, False, False, None, None, None, 1, 2),             # several returned sequences
                 (True, False, False, 0.5, None, 1.5, 1, 1),               # both spellings
                 (True, False, False, None, None, 0.5, 1, 1),              # g < 1
                 (True, False, False, None, None, float("nan"), 1, 1),
                 (True, False, False, -0.1, None, None, 1, 1),
                 (True, False, False, float("inf"), None, None, 1, 1),
                 (True, False, False, None, 1.5, None, 1, 1),
                 (True, False, False, None, -0.1, None, 1, 1),
                 (True, False, False, None, float("nan"), None, 1, 1)):
        with pytest.raises(ValueError):
            chk(*args)


def test_generate_refuses_before_any_launch():
    """The refusals of section "Public surface" reach the caller from generate itself, on a model that has no device to launch on."""
    from halva_amd.multimodal import MultimodalMixin

    class _NoDevice(MultimodalMixin):
        def __init__(self):
            pass

        def _embed_prompt(self, *a, **k):
            raise AssertionError("generate reached the prompt pass")
    m = _NoDevice()
    ids = torch.tensor([[1, 2, 3]])
    base = (ids, None, None, False, 1, 4, None, None, None)
    for kw in (dict(images_cd=torch.zeros(1), negative_input_ids=ids), dict(images_cd=torch.zeros(1), num_return_sequences=2),
               dict(cd_alpha=0.5), dict(guidance_scale=2.0), dict(negative_input_ids=ids, guidance_scale=0.5),
               dict(negative_input_ids=ids, cd_beta=2.0)):
        with pytest.raises(ValueError):
            m._generate(*base, **kw)
    with pytest.raises(ValueError, match="num_beams"):
        m._generate(ids, None, None, False, 3, 4, None, None, None, images_cd=torch.zeros(1))


def test_add_diffusion_noise():
    from halva_amd.contrast import add_diffusion_noise
    img = torch.randn(2, 3, 24, 24, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    a = add_diffusion_noise(img, 500, generator=torch.Generator().manual_seed(1))
    b = add_diffusion_noise(img, 500, generator=torch.Generator().manual_seed(1))
    c = add_diffusion_noise(img, 500, generator=torch.Generator().manual_seed(2))
    assert a.shape == img.shape and a.dtype == img.dtype and torch.equal(a, b) and not torch.equal(a, c)
    f = img.float()
    z = add_diffusion_noise(f, 0, generator=torch.Generator().manual_seed(3))
    assert z.dtype == torch.float32 and float((z - f).abs().max()) < 0.05          # abar_0 = 1 - 1e-5 - ...: noise of sd ~ 3.5e-3
    # the schedule: 1000 sigmoid steps from 1e-5 to 5e-3; the signal fades monotonically
    betas = torch.sigmoid(torch.linspace(-6, 6, 1000)) * (5e-3 - 1e-5) + 1e-5
    abar = torch.cumprod(1 - betas, 0)
    assert 1e-5 < float(betas[0]) < 3e-5 and 4.9e-3 < float(betas[-1]) < 5e-3
    e500 = add_diffusion_noise(torch.ones(4096), 500, generator=torch.Generator().manual_seed(4))
    assert abs(float(e500.mean()) - float(abar[500].sqrt())) < 4 * float((1 - abar[500]).sqrt()) / 64
    far = add_diffusion_noise(f, 999, generator=torch.Generator().manual_seed(5))
    assert float((far - f).abs().mean()) > float((z - f).abs().mean())
    for bad in (-1, 1000):
        with pytest.raises(ValueError):
            add_diffusion_noise(f, bad)
