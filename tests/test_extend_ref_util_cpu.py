"""CPU checks of tests/extend_ref_util.py, which the GPU tests of the extend and decode attention (tests/test_extend_attn_gpu.py,
tests/test_decode_kernels_gpu.py) rest on:
  * admissibility: on every wide-score profile and seed, the plain restatement of the kernel's documented arithmetic (emulate) meets the
    row-wise bound on every row - so a GPU failure on these inputs is the kernel's, not the inputs';
  * discrimination: the same restatement with the rescale at a move of m_ref taken out breaks the bound - so the bound would notice;
  * coverage: the boundary sweep's layout reaches every path of the kernel's tiling that the sweep is there for."""
import pytest
import torch

import extend_ref_util as E

PAST, M = 37, 300            # the wide-score case of tests/test_extend_attn_gpu.py
L = PAST + M


@pytest.fixture(scope="module")
def wide():
    """Per seed and profile: the inputs, the float64 reference and the rounding model."""
    out = {}
    for seed in E.WIDE_SEEDS:
        for name in E.WIDE_PROFILES:
            q, K, V = E.wide_inputs(name, L, M, seed=seed)
            out[seed, name] = (q, K, V, E.reference(q, K, V, PAST, M), E.model(q, K, V, PAST, M))
    return out


def _ratios(wide, seed, **kw):
    """worst row error / bound per profile, the bound taken over the five profiles' rows together (as the GPU test's one launch)."""
    ek, em, nr, moves = [], [], [], {}
    for name in E.WIDE_PROFILES:
        q, K, V, ref, mdl = wide[seed, name]
        got, moves[name] = E.emulate(q, K, V, PAST, M, **kw)
        a, b, c = E.row_errors(got, ref, mdl)
        ek.append(a), em.append(b), nr.append(c)
    bound = E.row_bound(torch.cat(em), torch.cat(nr))
    ratio = (torch.cat(ek) / bound).view(len(E.WIDE_PROFILES), M)
    assert not torch.isnan(ratio).any()
    return {name: ratio[k] for k, name in enumerate(E.WIDE_PROFILES)}, moves


def test_wide_scores_have_the_widths_they_claim(wide):
    for name in E.WIDE_PROFILES:
        q, K, V, _, _ = wide[0, name]
        s = torch.einsum("hid,hjd->hij", q.double(), K.double()) / 128 ** 0.5
        want = E.wide_profile(name, L)
        # row i's score on key j is c_i r(j) plus a few nats, c_i = q_i . u / sqrt(D) = 1 +- 0.15 (one sigma) over the rows
        assert float((s[0] - want[None]).abs().max()) <= 0.5 * float(want.max()) + 4.0, name
        assert float(s.abs().max()) < 350.0, name


@pytest.mark.parametrize("seed", E.WIDE_SEEDS)
def test_emulated_kernel_meets_the_row_bound_on_wide_scores(wide, seed):
    ratio, moves = _ratios(wide, seed)
    print("emulate, seed %d: worst row error / bound %s; m_ref moves %s"
          % (seed, {k: round(float(v.max()), 3) for k, v in ratio.items()}, moves))
    for name, r in ratio.items():
        assert bool((r <= 1.0).all()), "%s: row %d at %.3f of the bound" % (name, int(r.argmax()), float(r.max()))
    # the profiles reach the branches they are there for
    # (up: every row whose keys span more than 64 log2 units moves at least once; spike_late: the 70 rows that see the spike)
    assert moves["up"] >= M // 2 and moves["spike_late"] == 70 and moves["down"] == 0 and moves["spike_first"] == 0 and moves["flat"] == 0


@pytest.mark.parametrize("seed", E.WIDE_SEEDS)
def test_a_missing_rescale_breaks_the_row_bound(wide, seed):
    ratio, _ = _ratios(wide, seed, rescale=False)
    print("emulate without the rescale, seed %d: worst row error / bound %s; rows over the bound %s"
          % (seed, {k: round(float(v.max()), 3) for k, v in ratio.items()}, {k: int((v > 1).sum()) for k, v in ratio.items()}))
    assert float(ratio["up"].max()) > 1.0 and float(ratio["spike_late"].max()) > 1.0
    assert bool((ratio["flat"] <= 1.0).all())


def test_emulate_and_model_agree_with_reference_on_flat_scores(wide):
    q, K, V, ref, _ = wide[0, "flat"]
    emu, _ = E.emulate(q, K, V, PAST, M, bf16=False)
    mdl = E.model(q, K, V, PAST, M, bf16=False)
    assert emu.dtype == torch.float32 and mdl.dtype == torch.float32
    # fp32 noise: exp2 of an fp32 score of a few units and sums of at most 337 terms
    assert float((emu.double() - ref).abs().max()) < 1e-5 and float((mdl.double() - ref).abs().max()) < 1e-5
    # with the bf16 roundings the two differ from the reference by bf16 noise, not more
    emu16, _ = E.emulate(q, K, V, PAST, M)
    assert float((emu16.double() - ref).abs().max()) < 2.0 ** -7 * float(ref.abs().max())


def test_reference_masks_by_position_and_ignores_what_lies_beyond():
    q, K, V = E.wide_inputs("flat", 80, 50, seed=1)
    ref = E.reference(q, K, V, 30, 50)
    # row 0 sees keys 0 .. 30 only: garbage behind them changes nothing; rows beyond n_new and slots beyond past + n_new are not read
    K2, V2, q2 = K.clone(), V.clone(), q.clone()
    K2[:, 31:] = 99.0
    V2[:, 31:] = -99.0
    assert torch.equal(E.reference(q, K2, V2, 30, 50)[:, 0], ref[:, 0])
    K3 = torch.cat([K, torch.full((1, 5, 128), float("nan"), dtype=K.dtype)], 1)
    V3 = torch.cat([V, torch.full((1, 5, 128), float("nan"), dtype=V.dtype)], 1)
    q2[:, 40:] = float("nan")
    assert torch.equal(E.reference(q2, K3, V3, 30, 40), E.reference(q, K, V, 30, 40))
    assert torch.equal(E.reference(q, K, V, 30, 40), ref[:, :40])
    s = torch.einsum("d,jd->j", q[0, 7].double(), K[0, :38].double()) / 128 ** 0.5
    assert torch.allclose(ref[0, 7], torch.softmax(s, 0) @ V[0, :38].double(), rtol=0, atol=1e-14)


def test_sweep_layout_reaches_every_path():
    n, Lcap = E.SWEEP_N, E.SWEEP_LCAP
    per_seq = [E.layout_classes(p, m, n, Lcap) for p, m in zip(E.SWEEP_PAST, E.SWEEP_N_NEW)]
    for p, m in zip(E.SWEEP_PAST, E.SWEEP_N_NEW):      # inside the header's contract, and inside the buffers
        assert 0 <= p <= Lcap and 0 <= m <= n
    have = set().union(*per_seq)
    for r in range(64):
        assert ("past_mod64", r, True) in have, r
    for k in (1, 2, 3):
        assert ("blocks", k) in have, k
    for w in (1, 2, 3, 4):
        assert ("last_waves", w) in have, w
    for r in (0, 1, 31):
        assert ("n_new_mod32", r) in have, r
    for r in (0, 1, 63):
        assert ("len_mod64", r) in have, r
    assert ("ntiles", 0) in have and ("ntiles", 1) in have
    for cls in ("skipped", "diag", "len", "unmasked"):
        assert ("tile", cls, True) in have, cls
    assert ("dead_wave", True) in have and ("len_eq_Lcap",) in have
    # the three special sequences are what they are meant to be
    assert ("len_eq_Lcap",) in per_seq[E.SWEEP_FULL] and ("blocks", 3) in per_seq[E.SWEEP_FULL]
    assert per_seq[E.SWEEP_EMPTY] == {("blocks", 0)}
    assert ("clipped",) in per_seq[E.SWEEP_CLIP] and E.ext_rows(E.SWEEP_PAST[E.SWEEP_CLIP], E.SWEEP_N_NEW[E.SWEEP_CLIP], n, Lcap) == 5
    assert [("clipped",) in c for c in per_seq].count(True) == 1


def test_layout_classes_on_hand_worked_layouts():
    # past = 0, 65 rows of n = 65: one block, 3 live waves; len = 65 -> tile 0 (diagonal for waves 0 and 1, unmasked for wave 2, whose
    # first row is 64) and tile 1 (beyond len; skipped by waves 0 and 1, whose last rows are 31 and 63)
    c = E.layout_classes(0, 65, 65, 320)
    assert ("blocks", 1) in c and ("last_waves", 3) in c and ("dead_wave", False) in c and ("ntiles", 0) in c
    assert {x[1] for x in c if x[0] == "tile"} == {"diag", "len", "skipped", "unmasked"} and not any(x[0] == "tile" and x[2] for x in c)
    assert {x[1] for x in E.layout_classes(0, 33, 65, 320) if x[0] == "tile"} == {"len"}
    # past = 255, 64 rows, len = 319: wave 0's rows sit at 255 .. 286 -> tiles 0 .. 3 unmasked (kv0 + 63 <= 255), tile 4 reaches beyond len
    c = E.layout_classes(255, 64, 65, 320)
    assert {x[1] for x in c if x[0] == "tile"} == {"unmasked", "len"} and ("ntiles", 1) in c and ("len_mod64", 63) in c
    # past = 256, 64 rows, len = 320: tile 4 is the diagonal tile of both waves and ends at len
    assert {x[1] for x in E.layout_classes(256, 64, 65, 320) if x[0] == "tile"} == {"unmasked", "diag"}
    # the capacity clips: 9 rows asked, 5 free
    c = E.layout_classes(443, 9, 257, 448)
    assert ("clipped",) in c and ("len_eq_Lcap",) in c and ("n_new_mod32", 5) in c
    assert E.layout_classes(448, 9, 257, 448) == {("blocks", 0), ("clipped",)}
