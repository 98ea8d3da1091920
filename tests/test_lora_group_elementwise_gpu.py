"""The layer that strings the GEMMs into the training step - _LoraGroupFn and LoraGroup (halva_amd/llama.py) - held to float64 per
element, and its derived weights held coherent with the trainable factors along every route that changes them.

The older tests of this layer compare whole tensors by one relative norm (2e-2), or compare the weight-gradient routes with each other
on the operands the backward itself used (tests/test_lora_group_wgrad_gpu.py).  Neither asks whether y, xa's LoRA columns, dx or da
are right per element, and an error of one optimizer step's size in a derived weight is far below such a norm.

References: tests/lora_group_ref_util.py - float64, each stage on the operands that stage actually read.  Every element is held to the
form of tests/gemm_ref_util.py,

    |X_kernel - X_ref|  <=  |X_model - X_ref|  +  2 delta,      X_model = bf16(X_ref),  delta = delta_det(S, n) = 2 (n + 2) 2^-24 S

with n the length of the contraction (K for xa's LoRA columns, K + tail for y, N for the merged dx and for da, G r for the merged
rows of the transposed copy).  The two unmerged dgrad forms are held to the bound written for a backward that rounds twice - bf16(dy W),
then the LoRA product added onto it in place:

    |dx - ref|  <=  |model - ref|  +  2^-9 |dy W|_ref  +  2 delta,      model = bf16(bf16(dy W) + da A),  delta = delta_1 + delta_2

(one extra bf16 half-ulp of the intermediate: the stacked-rounding argument of tests/test_sdpa_rowwise_gpu.py's F_X), delta_1 =
delta_det(|dy| |W|, N), delta_2 = delta_det(|da| |A| + |bf16(dy W)|, G r).  No constant here was tuned to a measured figure.

What that bound found (MI355X).  The backward did round twice, and ONE element of 51 200 missed the bound in two cases, identically
under both unmerged forms: qkv-r128-rows200 [14, 27], error / bound 1.215, and single-r4-rows200 [103, 25], 1.022 (every other case
held, worst 0.873).  At [14, 27] dy W = -2423.99922 in float64, 8e-4 from the midpoint -2424 of the bf16 neighbours -2416 and -2432;
the GEMM's fp32 sum fell on the other side and stored -2432.  Such a flip moves the intermediate by a whole bf16 ulp, up to 2^-7 of
it, and the second rounding carried it into dx (got -2208, model -2192, reference -2192.88).  4 to 8 elements of 51 200 flipped per
group; both misses were flips.  A backward that rounds twice cannot keep a 2^-9 term, so _LoraGroupFn.backward now accumulates dy W
and da A in fp32 and rounds once: bf16(ref) is the bf16 value nearest to ref, no farther from it than `model` is, and the bound above
holds with room.  The same elements are also held to the one-rounding form ("rounded once", n = N + G r).

Derived state (`assert_coherent`): weight_cat[:, K:] is blockdiag(scale B_g) rounded once, bit for bit, zeros elsewhere; weight_cat_t[K:]
its transpose bit for bit; weight_cat[:, :K] the frozen W bit for bit; weight_cat_t[:K] the merged rows W^T + A_cat^T tail_rows within
the bound above (W^T bit for bit with DGRAD_MERGED off).  Held after the first forward and after a forward that follows each way the
factors change: copy_ under no_grad, load_state_dict, build_dgrad_copy, AdamWFlat.step with and without a post_sync callback, and the
resume route master.copy_ + sync_compute_copy.  A write through p.data is not detectable and not claimed (LoraGroup's docstring).

Inputs: gemm_ref_util.rand_tensor (rows scaled by 1e3 and 1e-3, one zero row), B ~ 0.05 randn, scale 2 (1.5 in one case: B * 1.5 is
exact in fp32, still one rounding).  xa's right columns, padding included, enter poisoned with NaN / +-Inf.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref_util as R  # noqa: E402
import lora_group_ref_util as L  # noqa: E402
from gemm_ref_util import bf, held, same_bits  # noqa: E402
from halva_amd import dpa, llama  # noqa: E402

DEV = "cuda"
bf16 = torch.bfloat16
K_IN, ROWS = 256, 200
LR = 2e-3             # tests/test_loss_curve_gpu.py's; route 4 asserts on the float64 reference that a step of this size shows
REL_OLD = 2e-2        # the relative-norm budget of the older whole-tensor tests
REPORT = {}
QKV = ("q_proj", "k_proj", "v_proj")
#            names, in_features, outs, r, alpha
GROUPS = {
    "qkv-r128": (QKV, K_IN, (256, 256, 256), 128, 256),
    "qkv-r16": (QKV, K_IN, (256, 256, 256), 16, 32),
    "qkv-r16-scale1.5": (QKV, K_IN, (256, 256, 256), 16, 24),
    "qkv-r4-unequal": (QKV, K_IN, (256, 128, 128), 4, 8),                 # G r = 12, tail 16: 4 padding columns
    "gate-up-r16": (("gate_proj", "up_proj"), K_IN, (384, 384), 16, 32),
    "single-r4": (("o_proj",), K_IN, (256,), 4, 8),                       # tail 8 with 4 padding columns
    "single-k1024-r8": (("down_proj",), 1024, (128,), 8, 16),             # __init__ gave this one 64 spare columns; attach_lora replaces them
}
SHAPES = [(gid, ROWS, None) for gid in GROUPS] + [("qkv-r4-unequal", ROWS, (2, 100)), ("qkv-r4-unequal", 1, None)]
SHAPE_IDS = ["%s-%s" % (g, "x".join(map(str, lead)) if lead else "rows%d" % rows) for g, rows, lead in SHAPES]


class Case:
    """one group with random frozen weight and factors, and a copy of the frozen weight taken before anything ran"""

    def __init__(self, gid, B_std=0.05, seed=0, copy=True):
        names, K, outs, r, alpha = GROUPS[gid]
        self.gen = g = torch.Generator(device=DEV).manual_seed(1000 * seed + sorted(GROUPS).index(gid))
        self.grp = grp = llama.LoraGroup(names, K, outs, bf16, DEV)
        assert grp.in_width == K + (64 if K % 1024 == 0 else 0)
        grp.weight_cat.data[:, :K].copy_(torch.randn(sum(outs), K, generator=g, device=DEV) * K ** -0.5)
        self.W0 = grp.weight_cat.data[:, :K].clone()
        self.K, self.outs, self.r, self.G, self.N = K, outs, r, len(outs), sum(outs)
        self.Gr, self.tail = self.G * r, L.tail_width(self.G, r)
        grp.attach_lora(r, alpha, bf16, DEV, generator=g)
        assert grp.scale == alpha / r and grp.in_width == K + self.tail
        for B in grp._Bs():
            B.data.copy_(torch.randn(B.shape, generator=g, device=DEV) * B_std)       # (before any refresh: nothing is stale yet)
        if copy:
            grp.build_dgrad_copy()

    def inputs(self, rows=ROWS):
        x = R.rand_tensor(rows, self.K, self.gen, DEV)
        res = R.rand_tensor(rows, self.N, self.gen, DEV)
        dy = R.rand_tensor(rows, self.N, self.gen, DEV)
        return x, res, dy

    def flat(self, callback):
        grp = self.grp
        flat = dpa.FlatTrainables([("A_cat", grp.A_cat)] + [("B%d" % i, B) for i, B in enumerate(grp._Bs())])
        if callback:                                   # what dpa.bind_model does, for this one group
            flat.post_sync.append(lambda: grp.refresh_tail())
            grp.refresh_tail()
        return flat, dpa.AdamWFlat(flat, lr=LR)

    def ideal_merged(self):
        """bf16 of the merged rows, in float64 from the factors alone"""
        T = bf(L.tail_ref(self.grp._Bs(), self.grp.scale, self.r))
        return bf(L.merged_ref(self.W0, self.grp.A_cat, T[:, :self.Gr].t())[0])


class Out:
    pass


def run(c, x, res=None, inplace=False, use_lora=True, poisoned=True, lead=None, grad=False):
    """one forward of the group on a fresh operand buffer -> Out(xa as the forward left it, y, the buffer's right columns before,
    and - with grad - the leaves x0 / res0 whose .grad a backward fills)"""
    grp, K = c.grp, c.K
    rows, width = x.shape[0], grp.in_width
    buf = torch.zeros(rows, width, dtype=bf16, device=DEV)
    buf[:, :K] = x
    if poisoned:
        buf[:, K:] = R.poison(rows * (width - K), bf16, DEV).view(rows, width - K)
    o = Out()
    o.right_before = buf[:, K:].clone()
    if lead:
        buf = buf.view(*lead, width)
        res = None if res is None else res.view(*lead, -1)
    o.x0 = buf.requires_grad_(True) if grad else buf
    o.res0 = None if res is None else res.clone().requires_grad_(grad)
    o.xa = o.x0.clone() if grad else o.x0
    rr = None if res is None else o.res0.clone()           # (a buffer of the block's own: contiguous, and with grad not a leaf)
    if grad:
        o.y = grp(o.xa, residual=rr, use_lora=use_lora, res_inplace=inplace)
    else:
        with torch.no_grad():
            o.y = grp(o.xa, residual=rr, use_lora=use_lora, res_inplace=inplace)
    if res is not None and inplace:
        assert o.y.data_ptr() == rr.data_ptr(), "res_inplace: the returned tensor is not the residual buffer itself"
    elif res is not None:
        assert o.y.data_ptr() != rr.data_ptr() and same_bits(rr.detach(), res), "out of place, yet the residual buffer was written"
    assert o.y.shape == o.xa.shape[:-1] + (c.N,)
    torch.cuda.synchronize()
    return o


def flat2(t):
    return t.detach().reshape(-1, t.shape[-1])


def check_forward(tag, c, o, x, res, use_lora=True):
    grp, K, Gr = c.grp, c.K, c.Gr
    xa, y, Wc = flat2(o.xa), flat2(o.y), grp.weight_cat.data
    assert same_bits(xa[:, :K], x), "%s: the forward changed its input columns" % tag
    if use_lora:
        ref, S = L.t_ref(x, grp.A_cat)
        held(REPORT, "xa lora columns", xa[:, K:K + Gr], ref, bf(ref), R.delta_det(S, K))
        assert not bool(xa[:, K + Gr:].any()) and bool(torch.isfinite(xa).all()), "%s: padding columns of xa are not zeros" % tag
        ref, S = L.y_ref(xa, Wc, res)
        held(REPORT, "y" if res is None else "y + residual", y, ref, bf(ref), R.delta_det(S, K + c.tail))
    else:
        assert same_bits(xa[:, K:], o.right_before), "%s: use_lora=False touched the right columns of xa" % tag
        ref, S = L.y_ref(xa, Wc, res, cols=K)
        held(REPORT, "y base only", y, ref, bf(ref), R.delta_det(S, K))


def assert_coherent(c, merged=None, report=REPORT):
    """the three derived copies follow the factors (module docstring)"""
    grp, K, Gr = c.grp, c.K, c.Gr
    merged = llama.DGRAD_MERGED if merged is None else merged
    wc, wct = grp.weight_cat.data, grp.weight_cat_t
    assert wc.shape == (c.N, K + c.tail)
    want = L.tail_ref(grp._Bs(), grp.scale, c.r).to(bf16)          # (scale * B has at most 10 significant bits: one rounding)
    assert same_bits(wc[:, K:], want), "weight_cat's tail is not blockdiag(scale B) rounded once (%d elements differ)" % int(
        (R.bits(wc[:, K:]) != R.bits(want)).sum())
    assert same_bits(wc[:, :K], c.W0), "the frozen weight changed"
    if wct is None:
        return
    assert wct.shape == (K + c.tail, c.N)
    assert same_bits(wct[K:], wc[:, K:].t().contiguous()), "weight_cat_t's tail rows are not the transpose of weight_cat's tail"
    if merged:
        ref, S = L.merged_ref(c.W0, grp.A_cat, wct[K:K + Gr])
        held(report, "merged rows", wct[:K], ref, bf(ref), R.delta_det(S, Gr))
    else:
        assert same_bits(wct[:K], c.W0.t().contiguous()), "DGRAD_MERGED off: the transposed copy's base rows are not W^T"


# ---------------------------------------------------------------------------------------------------------------------------------
# forward
@pytest.mark.parametrize("gid,rows,lead", SHAPES, ids=SHAPE_IDS)
def test_forward_per_element_with_poisoned_scratch(gid, rows, lead):
    c = Case(gid)
    x, res, _ = c.inputs(rows)
    for name, r_, inplace in (("none", None, False), ("out of place", res, False), ("in place", res, True)):
        tag = "%s residual %s" % (gid, name)
        o = run(c, x, r_, inplace, lead=lead)
        check_forward(tag, c, o, x, r_)
        clean = run(c, x, r_, inplace, poisoned=False, lead=lead)
        assert same_bits(o.y, clean.y) and same_bits(o.xa, clean.xa), "%s: poison in xa's scratch columns reached the result" % tag
        o = run(c, x, r_, inplace, use_lora=False, lead=lead)
        check_forward(tag + " base only", c, o, x, r_, use_lora=False)
    assert_coherent(c)


def test_lora_free_group_in_the_spare_column_layout():
    """in_features a multiple of 1024 and no factors: 64 spare columns that the product must neither read nor write"""
    names, K, outs, _, _ = GROUPS["single-k1024-r8"]
    g = torch.Generator(device=DEV).manual_seed(5)
    grp = llama.LoraGroup(names, K, outs, bf16, DEV)
    assert grp.in_width == K + 64
    grp.weight_cat.data.copy_(R.poison(grp.weight_cat.numel(), bf16, DEV).view_as(grp.weight_cat))
    grp.weight_cat.data[:, :K].copy_(torch.randn(sum(outs), K, generator=g, device=DEV) * K ** -0.5)
    x, res = R.rand_tensor(ROWS, K, g, DEV), R.rand_tensor(ROWS, sum(outs), g, DEV)
    xa = R.poison(ROWS * (K + 64), bf16, DEV).view(ROWS, K + 64)
    xa[:, :K] = x
    before = xa.clone()
    for r_ in (None, res):
        with torch.no_grad():
            y = grp(xa, residual=None if r_ is None else r_.clone(), res_inplace=r_ is not None)
        assert same_bits(xa, before)
        ref, S = L.y_ref(xa, grp.weight_cat.data, r_, cols=K)
        held(REPORT, "y base only", y, ref, bf(ref), R.delta_det(S, K))


# ---------------------------------------------------------------------------------------------------------------------------------
# backward
FORMS = (("merged", True, True, "in place"), ("unmerged with copy", False, True, "out of place"), ("no copy", False, False, "none"))


def backward_form(c, form, x, res, dy, lead=None):
    """forward + backward under one dgrad form -> (dxa [rows, width], residual gradient or None); the group is left in that form"""
    name, merged, copy, residual = form
    grp = c.grp
    if copy:
        grp.build_dgrad_copy()          # a fresh W^T: the merged rows of an earlier form must not stay behind
    else:
        grp.weight_cat_t, grp._tail_versions = None, None
    assert grp.dgrad_merged == merged
    o = run(c, x, None if residual == "none" else res, residual == "in place", lead=lead, grad=True)
    o.y.backward(dy.view(o.y.shape))
    torch.cuda.synchronize()
    assert o.x0.grad.shape == o.x0.shape
    return o, flat2(o.x0.grad), None if o.res0 is None else flat2(o.res0.grad)


def bound_of(ref, model, delta, extra=0.0):
    return (model - ref).abs() + extra + 2 * delta


@pytest.mark.parametrize("gid,rows,lead", SHAPES, ids=SHAPE_IDS)
def test_backward_per_element_under_each_dgrad_form(gid, rows, lead, monkeypatch):
    c = Case(gid)
    grp, K, Gr, N = c.grp, c.K, c.Gr, c.N
    x, res, dy = c.inputs(rows)
    seen = {}
    for form in FORMS:
        name, merged, copy, residual = form
        monkeypatch.setattr(llama, "DGRAD_MERGED", merged)
        o, dxa, dres = backward_form(c, form, x, res, dy, lead)
        tag = "%s %s" % (gid, name)
        check_forward(tag, c, o, x, None if residual == "none" else res)
        assert_coherent(c, merged)
        assert (dres is None) == (residual == "none")
        assert dres is None or same_bits(dres, dy), "%s: the residual's gradient is not dy" % tag
        assert not bool(dxa[:, K + Gr:].any()) and bool(torch.isfinite(dxa).all()), "%s: padding columns of dxa are not zeros" % tag
        da = dxa[:, K:K + Gr]
        ref, S = L.da_ref(dy, grp.weight_cat.data[:, K:], c.outs, c.r)
        held(REPORT, "da", da, ref, bf(ref), R.delta_det(S, N))
        if merged:
            ref, S = L.dx_merged_ref(dy, grp.weight_cat_t[:K])
            model, delta, extra = bf(ref), R.delta_det(S, N), 0.0
            held(REPORT, "dx merged", dxa[:, :K], ref, model, delta)
        else:
            W = grp.weight_cat_t[:K].t() if copy else grp.weight_cat.data[:, :K]
            r1, S1, r2, S2 = L.dx_unmerged_ref(dy, W, da, grp.A_cat)
            ref, model = r1 + r2, L.two_rounding_model(r1, r2)
            delta, extra = R.delta_det(S1, N) + R.delta_det(S2 + bf(r1).abs(), Gr), 2.0 ** -9 * r1.abs()
            bound = bound_of(ref, model, delta, extra)
            err = (dxa[:, :K].double() - ref).abs()
            print("[%s] dx against the two-rounding bound: %d of %d elements outside, worst error / bound %.3f" % (
                tag, int((err > bound).sum()), err.numel(), float((err / bound.clamp_min(1e-300)).max())))
            held(REPORT, "dx " + name, dxa[:, :K], ref, model, delta, G=extra)
            # and, tighter, as the backward now forms it: one fp32 sum over N + G r terms, one rounding
            held(REPORT, "dx %s, rounded once" % name, dxa[:, :K], ref, bf(ref), R.delta_det(S1 + S2, N + Gr))
        seen[name] = (dxa[:, :K].double(), ref, bound_of(ref, model, delta, extra))
    # the forms agree within the sum of their own bounds (their references differ by the roundings of the merged rows and of da:
    # that difference is known exactly and added)
    names = [f[0] for f in FORMS]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (ga, ra, ba), (gb, rb, bb) = seen[a], seen[b]
            assert bool(((ga - gb).abs() <= ba + bb + (ra - rb).abs()).all()), "%s: dx of '%s' and '%s' disagree" % (gid, a, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# coherence of the derived state along every route that changes the factors
ROUTE_CASES = [("qkv-r16", True), ("qkv-r4-unequal", True), ("qkv-r16", False)]
ROUTE_IDS = ["%s-%s" % (g, "merged" if m else "unmerged") for g, m in ROUTE_CASES]


@pytest.fixture(params=ROUTE_CASES, ids=ROUTE_IDS)
def live(request, monkeypatch):
    """a group after its first forward and backward, coherent"""
    gid, merged = request.param
    monkeypatch.setattr(llama, "DGRAD_MERGED", merged)
    c = Case(gid)
    c.x, c.res, c.dy = c.inputs()
    c.merged = merged
    forward_is_coherent(c)
    return c


def forward_is_coherent(c):
    o = run(c, c.x, c.res, True)
    assert_coherent(c, c.merged)
    check_forward("after a mutation", c, o, c.x, c.res)


def perturbed(p, gen, by=0.01):
    return (p.detach().float() + by * torch.randn(p.shape, generator=gen, device=DEV)).to(bf16)


def train_pass(c, flat):
    flat.zero_grad()
    c.grp.grad_sink = True
    o = run(c, c.x, c.res, True, grad=True)
    o.y.backward(c.dy)
    torch.cuda.synchronize()
    assert bool(flat.grad.any())
    return flat2(o.x0.grad), flat2(o.y)


def counted_refresh(c, monkeypatch):
    calls, inner = [], c.grp.refresh_tail
    monkeypatch.setattr(c.grp, "refresh_tail", lambda: (calls.append(1), inner())[1])
    return calls


def test_route_1_copy_under_no_grad(live):
    c = live
    with torch.no_grad():
        for B in c.grp._Bs():
            B.copy_(perturbed(B, c.gen))
    forward_is_coherent(c)
    with torch.no_grad():
        c.grp.A_cat.copy_(perturbed(c.grp.A_cat, c.gen))
    forward_is_coherent(c)


def test_route_2_load_state_dict(live):
    c = live
    sd = {k: perturbed(v, c.gen) for k, v in c.grp.state_dict().items() if k == "A_cat" or "lora_B" in k}
    assert len(sd) == c.G + 1
    before = c.ideal_merged()
    missing, unexpected = c.grp.load_state_dict(sd, strict=False)
    assert list(missing) == ["weight_cat"] and not unexpected
    assert all(same_bits(v, c.grp.state_dict()[k]) for k, v in sd.items()) and bool((before != c.ideal_merged()).any())
    forward_is_coherent(c)


def test_route_3_build_dgrad_copy_after_a_forward(live):
    c = live
    c.grp.build_dgrad_copy()
    forward_is_coherent(c)
    with torch.no_grad():
        c.grp._Bs()[0].copy_(perturbed(c.grp._Bs()[0], c.gen))
    c.grp.build_dgrad_copy()
    forward_is_coherent(c)


def test_route_4_flat_adamw_steps_with_post_sync(live, monkeypatch):
    c = live
    calls = counted_refresh(c, monkeypatch)
    flat, opt = c.flat(callback=True)
    forward_is_coherent(c)
    del calls[:]
    for step in (1, 2):
        before = c.ideal_merged()
        train_pass(c, flat)
        opt.step()
        moved = float((before != c.ideal_merged()).double().mean())
        print("[route 4 step %d] %.3f of the elements of bf16(merged_ref) moved" % (step, moved))
        assert moved >= 0.5, "a step of lr %g moves too few elements of the merged weight for a stale copy to show" % LR
        forward_is_coherent(c)
        forward_is_coherent(c)
        assert len(calls) == step, "with a post_sync callback the forward must not refresh again (%d refreshes after %d steps)" % (
            len(calls), step)


def test_route_5_resume_master_copy_and_sync(live):
    c = live
    flat, opt = c.flat(callback=True)
    train_pass(c, flat)
    opt.step()
    saved, ideal = flat.master.clone(), c.ideal_merged()
    train_pass(c, flat)
    opt.step()
    forward_is_coherent(c)
    assert bool((ideal != c.ideal_merged()).any())
    flat.master.copy_(saved)
    flat.sync_compute_copy()
    assert same_bits(flat.flat, saved.to(bf16)) and bool((ideal == c.ideal_merged()).all())
    forward_is_coherent(c)


def test_route_6_flat_adamw_steps_without_any_callback(live, monkeypatch):
    """no bind_model: only the flat buffer's epoch tells the group that its factors moved (tests/test_lora_group_wgrad_gpu.py builds its
    FlatTrainables this way).  Before LoraGroup compared the epoch the tail and the merged rows stayed at their first values here."""
    c = live
    calls = counted_refresh(c, monkeypatch)
    flat, opt = c.flat(callback=False)
    assert not flat.post_sync
    forward_is_coherent(c)
    del calls[:]
    for step in (1, 2):
        before = c.ideal_merged()
        train_pass(c, flat)
        opt.step()
        assert float((before != c.ideal_merged()).double().mean()) >= 0.5
        forward_is_coherent(c)
        forward_is_coherent(c)
        assert len(calls) == step, "the first forward after a step refreshes, the second does not"


# ---------------------------------------------------------------------------------------------------------------------------------
# mismatch tests: what the whole-tensor norm of the older tests lets through and assert_coherent does not
def truth(c):
    """(y, dx) of the peft formula in float64 on the current factors"""
    grp = c.grp
    Bs = [B.detach().double() for B in grp._Bs()]
    y, _ = L.peft_y(c.x.double(), c.W0.double(), grp.A_cat.detach().double(), Bs, grp.scale, c.r, c.res.double())
    T = L.tail_ref(Bs, grp.scale, c.r, c.Gr)
    dx = c.dy.double() @ c.W0.double() + (c.dy.double() @ T) @ grp.A_cat.detach().double()
    return y, dx


def rel(got, want):
    return float((got.double() - want).norm() / want.norm())


def training_like_case(monkeypatch):
    """as in training: B starts at zero (peft's init) and gets its first values from one real optimizer step"""
    monkeypatch.setattr(llama, "DGRAD_MERGED", True)
    c = Case("qkv-r4-unequal", B_std=0.0)
    assert c.outs[1] == c.outs[2]
    c.x, c.res, c.dy = c.inputs()
    c.merged = True
    flat, opt = c.flat(callback=True)
    forward_is_coherent(c)
    return c, flat, opt


def step_and_measure(c, flat, opt):
    train_pass(c, flat)
    opt.step()
    dx, y = train_pass(c, flat)
    yt, dxt = truth(c)
    return rel(y, yt), rel(dx[:, :c.K], dxt)


def test_mismatch_control_passes_both_checks(monkeypatch):
    c, flat, opt = training_like_case(monkeypatch)
    ry, rdx = step_and_measure(c, flat, opt)
    print("[mismatch control] relative norm error: y %.2e, dx %.2e" % (ry, rdx))
    assert ry < REL_OLD and rdx < REL_OLD
    assert_coherent(c, True, report=None)


def test_mismatch_stale_merged_rows_is_caught_by_coherence_only(monkeypatch):
    c, flat, opt = training_like_case(monkeypatch)
    K, inner = c.K, llama.LoraGroup.refresh_tail

    def skips_the_merged_rows(self):
        keep = self.weight_cat_t[:K].clone()
        inner(self)
        self.weight_cat_t[:K].copy_(keep)
    monkeypatch.setattr(llama.LoraGroup, "refresh_tail", skips_the_merged_rows)
    ry, rdx = step_and_measure(c, flat, opt)
    print("[mismatch stale merged rows] relative norm error: y %.2e, dx %.2e" % (ry, rdx))
    assert ry < REL_OLD and rdx < REL_OLD, "the whole-tensor norm was expected to let this through"
    with pytest.raises(AssertionError, match="merged rows"):
        assert_coherent(c, True, report=None)


def test_mismatch_swapped_tail_blocks_is_caught_by_coherence_only(monkeypatch):
    c, flat, opt = training_like_case(monkeypatch)
    K, r, inner = c.K, c.r, llama.LoraGroup.refresh_tail
    n, o1 = c.outs[1], c.outs[0]
    o2 = o1 + n

    def swaps_two_blocks(self):
        inner(self)
        wc, wct = self.weight_cat.data, self.weight_cat_t
        a, b = wc[o1:o1 + n, K + r:K + 2 * r].clone(), wc[o2:o2 + n, K + 2 * r:K + 3 * r].clone()
        wc[o1:o1 + n, K + r:K + 2 * r], wc[o2:o2 + n, K + 2 * r:K + 3 * r] = b, a
        wct[K + r:K + 2 * r, o1:o1 + n], wct[K + 2 * r:K + 3 * r, o2:o2 + n] = b.t(), a.t()
    monkeypatch.setattr(llama.LoraGroup, "refresh_tail", swaps_two_blocks)
    ry, rdx = step_and_measure(c, flat, opt)
    print("[mismatch swapped tail blocks] relative norm error: y %.2e, dx %.2e" % (ry, rdx))
    assert ry < REL_OLD and rdx < REL_OLD, "the whole-tensor norm was expected to let this through"
    with pytest.raises(AssertionError, match="weight_cat's tail"):
        assert_coherent(c, True, report=None)


def test_zz_report_worst_ratios():
    """(runs last in the file) the worst ratio error / bound of every quantity over the tests above"""
    print("worst error / bound per quantity: " + ", ".join("%s %.3g" % kv for kv in sorted(REPORT.items())))
    for k, v in REPORT.items():
        assert v <= 1.0, k
