"""tests/lora_group_ref_util.py proved on the CPU.  With no rounding inserted anywhere its stage references compose to the truth: y to
the peft formula, dx in its three forms, da and the weight-gradient products to what torch.autograd gives for that formula on float64
leaves - at G = 1, 2, 3 with unequal outs and a rank that leaves padding columns, where a transposition, a group offset or a factor of
scale in the references would show.  Then _LoraGroupFn itself in the one configuration that needs no native call (fp32 parameters, no
transposed copy, gradient sink off) is held to the references at fp32 accuracy, and the staleness check of LoraGroup is shown to
see an optimizer step through a flat buffer that no callback follows."""
import pytest
import torch

import gemm_ref_util as R
import lora_group_ref_util as L
from halva_amd import dpa, llama

K_IN, ROWS = 24, 7
CASES = {"G1": ((10,), 4), "G2": ((6, 9), 4), "G3": ((8, 5, 11), 4), "G3-r8": ((8, 5, 11), 8)}
NAMES = ("q_proj", "k_proj", "v_proj")
REL = 1e-12


def _close(name, got, want):
    err = float((got - want).abs().max())
    top = float(want.abs().max())
    assert top > 0, name
    assert err <= REL * top, (name, err, top)


def _leaves(outs, r, seed):
    g = torch.Generator().manual_seed(seed)
    N, G = sum(outs), len(outs)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)
    return dict(x=rnd(ROWS, K_IN), W=rnd(N, K_IN), A=rnd(G * r, K_IN), Bs=[rnd(n, r) for n in outs], res=rnd(ROWS, N), dy=rnd(ROWS, N))


@pytest.mark.parametrize("case", sorted(CASES))
def test_stage_references_compose_to_the_peft_formula_and_its_autograd(case):
    outs, r = CASES[case]
    G, N, K, scale = len(outs), sum(outs), K_IN, 1.5
    z = _leaves(outs, r, 3)
    tail = L.tail_width(G, r)
    assert tail - G * r == {"G1": 4, "G2": 0, "G3": 4, "G3-r8": 0}[case], "G = 1 and G = 3 at r = 4 leave padding columns (12 of 16)"
    leaves = [z["x"], z["A"], z["res"]] + z["Bs"]
    for t in leaves:
        t.requires_grad_(True)
    y, t = L.peft_y(z["x"], z["W"], z["A"], z["Bs"], scale, r, z["res"])
    t.retain_grad()
    y.backward(z["dy"])

    # forward, stage by stage
    t_ref, S_t = L.t_ref(z["x"], z["A"])
    _close("t", t_ref, t.detach())
    xa = torch.zeros(ROWS, K + tail, dtype=torch.float64)
    xa[:, :K], xa[:, K:K + G * r] = z["x"].detach(), t_ref
    T = L.tail_ref(z["Bs"], scale, r)
    assert T.shape == (N, tail) and not bool(T[:, G * r:].any())
    Wc = torch.cat([z["W"], T], 1)
    y_ref, S_y = L.y_ref(xa, Wc, z["res"])
    _close("y", y_ref, y.detach())
    _close("y without the residual", L.y_ref(xa, Wc)[0], y.detach() - z["res"].detach())
    _close("y of the base weight alone", L.y_ref(xa, Wc, cols=K)[0], z["x"].detach() @ z["W"].t())
    assert bool((S_t >= t_ref.abs()).all()) and bool((S_y >= y_ref.abs()).all())

    # backward: da, the three dgrad forms, the weight gradients
    dx_true = z["x"].grad
    da, S_da = L.da_ref(z["dy"], T, outs, r)
    _close("da", da, t.grad)
    _close("da as one product over the block diagonal", da, z["dy"] @ T[:, :G * r])
    merged, S_m = L.merged_ref(z["W"], z["A"], T[:, :G * r].t())
    assert merged.shape == (K, N)
    _close("dx merged", L.dx_merged_ref(z["dy"], merged)[0], dx_true)
    r1, S1, r2, S2 = L.dx_unmerged_ref(z["dy"], z["W"], da, z["A"])
    _close("dx unmerged with copy", r1 + r2, dx_true)
    r1, S1, r2, S2 = L.dx_unmerged_ref(z["dy"], Wc[:, :K], da, z["A"])
    _close("dx no copy", r1 + r2, dx_true)
    assert bool((S1 + S2 >= (r1 + r2).abs()).all()) and bool((S_m >= merged.abs()).all()) and bool((S_da >= da.abs()).all())
    dxa = torch.cat([dx_true, da, torch.zeros(ROWS, tail - G * r, dtype=torch.float64)], 1)
    want = [z["A"].grad] + [B.grad for B in z["Bs"]]
    prods = L.wgrad_operands(z["dy"], xa, dxa, K, outs, r, scale)
    assert len(prods) == G + 1
    for q, (p, w) in enumerate(zip(prods, want)):
        ref, S = L.wgrad_ref(*p)
        _close("weight gradient %d" % q, ref, w)
        assert bool((S >= ref.abs()).all())
    _close("residual gradient", z["res"].grad, z["dy"])


def test_references_see_a_swapped_block_a_transposition_and_a_missing_scale():
    """the composition above is not vacuous: each of these mistakes in a stage reference moves y or dx far beyond 1e-12"""
    outs, r, scale = (8, 8, 11), 4, 1.5
    G, K = len(outs), K_IN
    z = _leaves(outs, r, 5)
    y, _ = L.peft_y(z["x"], z["W"], z["A"], z["Bs"], scale, r)
    t = L.t_ref(z["x"], z["A"])[0]
    xa = torch.cat([z["x"], t, torch.zeros(ROWS, L.tail_width(G, r) - G * r, dtype=torch.float64)], 1)
    good = L.tail_ref(z["Bs"], scale, r)
    wrong = {"blocks of two equal-sized targets swapped": L.tail_ref([z["Bs"][1], z["Bs"][0], z["Bs"][2]], scale, r),
             "scale left out": L.tail_ref(z["Bs"], 1.0, r),
             "columns shifted by one group": torch.roll(good, r, 1)}
    _close("control", L.y_ref(xa, torch.cat([z["W"], good], 1))[0], y)
    for name, T in wrong.items():
        with pytest.raises(AssertionError):
            _close(name, L.y_ref(xa, torch.cat([z["W"], T], 1))[0], y)


def _cpu_group(outs, r, alpha, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    grp = llama.LoraGroup(NAMES[:len(outs)], K_IN, outs, dtype, "cpu")
    grp.weight_cat.data[:, :K_IN].copy_(torch.randn(sum(outs), K_IN, generator=g) * K_IN ** -0.5)
    grp.attach_lora(r, alpha, dtype, "cpu", generator=g)
    for B in grp._Bs():
        B.data.copy_(torch.randn(B.shape, generator=g) * 0.05)
    return grp, g


@pytest.mark.parametrize("residual", [False, True], ids=["no-residual", "residual"])
def test_lora_group_fn_on_the_cpu_matches_the_references_at_fp32_accuracy(residual):
    outs, r = (8, 5, 11), 4
    G, N, K = len(outs), sum(outs), K_IN
    grp, g = _cpu_group(outs, r, 6.0, 11)
    assert grp.weight_cat_t is None and not grp.grad_sink and grp.scale == 1.5 and grp.in_width == K + 16
    x0 = torch.randn(ROWS, grp.in_width, generator=g).requires_grad_(True)
    res0 = torch.randn(ROWS, N, generator=g).requires_grad_(True) if residual else None
    dy = torch.randn(ROWS, N, generator=g)
    xa = x0.clone()
    with torch.no_grad():
        xa[:, K:] = float("nan")
    y = grp(xa, residual=res0)
    y.backward(dy)
    xa = xa.detach()
    Bs, A, Wc = grp._Bs(), grp.A_cat, grp.weight_cat.data

    def held32(name, got, ref, S, n):
        return R.held(None, name, got.detach(), ref, ref, R.delta_det(S, n))
    ref, S = L.t_ref(xa[:, :K], A)
    held32("t", xa[:, K:K + G * r], ref, S, K)
    assert not bool(xa[:, K + G * r:].any()), "padding columns"
    assert torch.equal(Wc[:, K:].double(), L.tail_ref(Bs, grp.scale, r).float().double()), "tail"
    ref, S = L.y_ref(xa, Wc, None if res0 is None else res0)
    held32("y", y, ref, S, K + 16)
    dxa = x0.grad
    ref, S = L.da_ref(dy, Wc[:, K:], outs, r)
    held32("da", dxa[:, K:K + G * r], ref, S, N)
    assert not bool(dxa[:, K + G * r:].any()), "padding columns of dxa"
    r1, S1, r2, S2 = L.dx_unmerged_ref(dy, Wc[:, :K], dxa[:, K:K + G * r], A)
    held32("dx", dxa[:, :K], r1 + r2, S1 + S2, N + G * r)
    for q, (p, P) in enumerate(zip(L.wgrad_operands(dy, xa, dxa, K, outs, r, grp.scale), [A] + Bs)):
        ref, S = L.wgrad_ref(*p)
        held32("weight gradient %d" % q, P.grad, ref, S, ROWS)
    if residual:
        assert torch.equal(res0.grad, dy)
    # and the whole against the truth, loosely: fp32 end to end
    yt, _ = L.peft_y(xa[:, :K].double(), Wc[:, :K].double(), A.detach().double(), [B.detach().double() for B in Bs], grp.scale, r,
                     None if res0 is None else res0.detach().double())
    assert float((y.detach().double() - yt).abs().max()) <= 1e-5 * float(yt.abs().max())


@pytest.mark.parametrize("bound", [True, False], ids=["post-sync-callback", "no-callback"])
def test_a_flat_buffer_step_is_seen_by_the_staleness_check(bound):
    """AdamWFlat.step refreshes the parameters through the flat buffer, which moves no tensor version counter; the epoch of the buffer
    does.  With the callback bind_model installs nothing more happens in the next forward; without it that forward refreshes."""
    outs, r = (8, 5, 11), 4
    G, K = len(outs), K_IN
    grp, g = _cpu_group(outs, r, 8.0, 13, torch.bfloat16)
    params = [grp.A_cat] + grp._Bs()
    flat = dpa.FlatTrainables([("A_cat", grp.A_cat)] + [("B%d" % i, B) for i, B in enumerate(grp._Bs())])
    assert all(p.flat_owner is flat for p in params) and flat.epoch == 0
    calls = []
    refresh = grp.refresh_tail
    grp.refresh_tail = lambda: (calls.append(1), refresh())[1]
    if bound:
        flat.post_sync.append(grp.refresh_tail)
        grp.refresh_tail()
    opt = dpa.AdamWFlat(flat, lr=2e-3)
    x = torch.randn(ROWS, grp.in_width, generator=g).to(torch.bfloat16)
    with torch.no_grad():
        grp(x.clone())
    del calls[:]
    versions = [p._version for p in params]
    for step in (1, 2):
        flat.grad.copy_(torch.randn(flat.total, generator=g))
        before = grp.weight_cat.data[:, K:].clone()
        opt.step()
        assert flat.epoch == step and [p._version for p in params] == versions, "the flat update moved a version counter after all"
        with torch.no_grad():
            grp(x.clone())
            grp(x.clone())
        assert len(calls) == step, "one refresh per step, by the callback or by the first forward - never both, never none"
        want = L.tail_ref(grp._Bs(), grp.scale, r).to(torch.bfloat16)
        assert R.same_bits(grp.weight_cat.data[:, K:], want), "stale tail after step %d" % step
        assert not R.same_bits(before, want), "the step did not move the tail: the check above shows nothing"
