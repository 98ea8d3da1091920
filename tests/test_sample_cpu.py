"""Sampling without a GPU: the fp64 restatement (tests/sample_ref_util.py) against transformers' own warpers, the C-ABI argument checks of
halva_sample_top_k_top_p, and generate's argument check (halva_amd/decode.py:check_generate_args)."""
import ctypes

import numpy as np
import pytest
import torch

from sample_ref_util import sample_ref

PARAMS = [(1.0, 0, 1.0), (0.2, 0, 0.7), (1.0, 50, 1.0), (0.7, 50, 0.9), (1.0, 1, 1.0), (1.0, 0, 1e-6), (2.0, 5, 0.5)]


@pytest.mark.parametrize("V", [257, 32000])
def test_the_restatement_keeps_what_transformers_warpers_keep(V):
    """Tie-free fp64 rows: the finite entries after TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper(min_tokens_to_keep=1)
    are the restatement's K2.  (The warpers get the fp32 values of the scalars, as the restatement uses them.)"""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    rng = np.random.default_rng(V)
    for n, (T, k, p) in enumerate(PARAMS):
        row = 4.0 * rng.standard_normal(V)
        assert len(np.unique(row)) == V
        T32, p32 = float(np.float32(T)), float(np.float32(p))
        s = torch.as_tensor(row)[None]
        s = TemperatureLogitsWarper(T32)(None, s)
        if k > 0:
            s = TopKLogitsWarper(top_k=k)(None, s)
        if p32 < 1.0:
            s = TopPLogitsWarper(top_p=p32, min_tokens_to_keep=1)(None, s)
        hf = torch.isfinite(s[0]).numpy()
        ref = sample_ref(row, T, k, p)
        assert np.array_equal(hf, ref.K2), (V, T, k, p, int(hf.sum()), int(ref.K2.sum()))
        assert ref.thr == ref.x[ref.K2].min() and (ref.K2 == (ref.x >= ref.thr)).all()
        if k > 0:
            assert int(ref.K1.sum()) == min(k, V)


def test_the_restatement_keeps_ties_together():
    row = np.array([1.0, 3.0, 3.0, 2.0, 2.0, 2.0, -np.inf, 0.0])
    r = sample_ref(row, 1.0, 1, 1.0)
    assert r.K2.tolist() == [False, True, True, False, False, False, False, False]
    r = sample_ref(row, 1.0, 3, 1.0)                  # two above the 2.0s: all three of them are in
    assert r.K2.tolist() == [False, True, True, True, True, True, False, False]
    r = sample_ref(row, 1.0, 0, 1.0)
    assert r.K2.tolist() == [True, True, True, True, True, True, False, True]
    r = sample_ref(row, 1.0, 0, 1e-6)
    assert r.K2.tolist() == [False, True, True, False, False, False, False, False] and r.cdf[1] == 0.5 and r.cdf[-1] == 1.0


def test_sample_argument_validation_without_gpu():
    """halva_sample_top_k_top_p validates before launching: each bad argument returns HALVA_ERR_INVALID_ARG with a message."""
    from halva_amd import hip
    lib = hip.load()
    P = ctypes.c_void_p
    ok = dict(logits=P(64), ld=8, u=P(64), token=P(64), thr=None, kept=None, B=2, V=8, temperature=1.0, top_k=0, top_p=1.0)

    def rc(**kw):
        a = dict(ok, **kw)
        return lib.halva_sample_top_k_top_p(a["logits"], a["ld"], a["u"], a["token"], a["thr"], a["kept"], a["B"], a["V"], a["temperature"],
                                            a["top_k"], a["top_p"], None)
    for kw, msg in ((dict(logits=None), b"null pointer"), (dict(u=None), b"null pointer"), (dict(token=None), b"null pointer"),
                    (dict(V=0), b"V=0"), (dict(B=0), b"B=0"), (dict(ld=7), b"row stride"), (dict(top_p=1.5), b"top_p"),
                    (dict(top_p=0.0), b"top_p"), (dict(temperature=0.0), b"temperature"), (dict(temperature=float("inf")), b"temperature"),
                    (dict(temperature=float("nan")), b"temperature"), (dict(top_k=-1), b"top_k")):
        assert rc(**kw) == -1 and msg in lib.halva_last_error(), (kw, lib.halva_last_error())
    cap = lib.halva_sample_max_vocab()
    assert cap >= 32003
    assert rc(V=cap + 1, ld=cap + 1) == -1 and str(cap).encode() in lib.halva_last_error()


def test_check_generate_args():
    from halva_amd.decode import check_generate_args as chk
    # greedy: the scripts' temperature=0 call; temperature / top_p / top_k are ignored without do_sample
    assert chk(1, False, 8) is None
    assert chk(1, False, 8, temperature=0, top_p=None) is None
    assert chk(None, False, 8, temperature=0.2, top_p=0.7, top_k=3) is None
    # sampling: HF's defaults filled in
    assert chk(1, True, 8, temperature=0.2, top_p=0.7) == (0.2, 50, 0.7)
    assert chk(1, True, 8, temperature=1, top_k=0) == (1.0, 0, 1.0)
    # the two refusals that stay
    with pytest.raises(NotImplementedError, match="beam"):
        chk(2, False, 8)
    with pytest.raises(NotImplementedError, match="explicit temperature"):
        chk(1, True, 8)
    # the four argument errors
    for kw in (dict(temperature=0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=1.0, top_p=0),
               dict(temperature=1.0, top_p=1.5), dict(temperature=1.0, top_k=-1)):
        with pytest.raises(ValueError):
            chk(1, True, 8, **kw)
    with pytest.raises(ValueError):
        chk(1, False, 0)
