"""The beam-search kernels alone (halva_amd/csrc/beam.hip; the table-reading own pass of csrc/kvcache.hip, beam_advance_kernel of csrc/fork.hip): H = 2, D = 128.

halva_beam_select against tests/beam_ref_util.py's float64 reference on inputs whose float64 top C + 1 per prompt are more than 1e-3 apart
(asserted on the host): tokens and beams exactly, scores within beam_ref_util.select_bound; the tie rule, the -1 rule, row independence,
the limits.  halva_beam_advance exactly against the host reference.  halva_beam_decode_attn without a tolerance: bitwise
halva_fork_decode_attn with the identity table, and with random tables (real beam histories) bitwise halva_fork_decode_attn on own caches
materialised by that gather; NaN in every slot the launch must not read; one configuration per element against float64 under the decode
bound in use (2^-8 |ref| + 1e-4); a wrong table entry changes exactly that member."""
import pytest
import torch

import beam_ref_util as R
import fork_ref_util as F

pytestmark = pytest.mark.gpu

H, D = 2, 128
INVALID = -1         # HALVA_ERR_INVALID_ARG (include/halva_hip.h)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda"


def _t(v, dev="cuda"):
    return torch.tensor(v, dtype=torch.int32, device=dev)


def _i16(t):
    return t.contiguous().view(torch.int16)


def _strided(logits, pad, dev):
    """The rows inside a wider buffer (row stride V + pad), the pad columns NaN."""
    M, V = logits.shape
    buf = torch.full((M, V + pad), float("nan"), dtype=torch.float32, device=dev)
    buf[:, :V] = logits.to(dev)
    return buf[:, :V]


# ------------------------------------------------------------------------------------------------
# select
SELECT_CASES = [(V, K, C, kind) for V in (97, 1000, 32000, 32768) for K in (1, 3, 5, 16) for C in sorted({min(2 * K, 64), min(3 * K, 64)})
                for kind in ("first", "mixed")]


@pytest.mark.parametrize("V,K,C,kind", SELECT_CASES)
def test_select_against_float64(V, K, C, kind):
    from halva_amd import kernels as KR
    dev = _dev()
    B = 2
    logits, scores, ref = R.select_inputs(B, K, C, V, kind, gap=1e-3, seed=V + 7 * K + C)
    assert R.min_gap(ref) > 1e-3
    got_s, got_t, got_b = KR.beam_select(_strided(logits, 3, dev), scores.to(dev), K, C)
    got_s, got_t, got_b = got_s.cpu().double(), got_t.cpu().long(), got_b.cpu().long()
    assert torch.equal(got_t, ref["token"]) and torch.equal(got_b, ref["beam"])
    if kind == "first":
        assert not bool(got_b.any())          # every candidate comes from beam 0
    rows = torch.arange(B)[:, None] * K + ref["beam"]
    bound = R.select_bound(ref["score"], scores.double()[rows], logits.double().abs().amax(1)[rows], ref["lse"][rows])
    err = (got_s - ref["score"]).abs()
    worst = float((err / bound).max())
    print("beam_select V=%d K=%d C=%d %s: worst |err| %.3e, worst err / bound %.3f" % (V, K, C, kind, float(err.max()), worst))
    assert bool((err <= bound).all()), worst


def test_select_four_prompts_at_the_vocabulary_size_in_use():
    """B = 4, K = 5, C = 10, V = 32000 (the shape tools/bench_decode.py --beam times) against float64, and against log_softmax + topk in torch
    on the same inputs: the gaps decide, so all three agree."""
    from halva_amd import kernels as KR
    dev = _dev()
    B, K, C, V = 4, 5, 10, 32000
    logits, scores, ref = R.select_inputs(B, K, C, V, "mixed", gap=1e-3, seed=77)
    s, t, b = KR.beam_select(logits.to(dev), scores.to(dev), K, C)
    assert torch.equal(t.cpu().long(), ref["token"]) and torch.equal(b.cpu().long(), ref["beam"])
    top = (torch.log_softmax(logits.to(dev), -1) + scores.to(dev)[:, None]).view(B, K * V).topk(C, 1)
    assert torch.equal(top.indices.cpu(), ref["beam"] * V + ref["token"])
    rows = torch.arange(B)[:, None] * K + ref["beam"]
    bound = R.select_bound(ref["score"], scores.double()[rows], logits.double().abs().amax(1)[rows], ref["lse"][rows])
    assert bool(((s.cpu().double() - ref["score"]).abs() <= bound).all())


def test_select_ties_inside_rows_at_the_vocabulary_size_in_use():
    """B = 4, K = 5, C = 10, V = 32000 on logits rounded to multiples of 0.5: equal logits inside a row are equal scores (one lse, one beam
    score), in fp32 as in float64, so the float64 reference's stable sort - ties by the lower flat index - is held exactly.  The draw must
    put ties among the returned candidates, and every gap between distinct scores of the top C + 1 must decide (re-seeded until so).
    (torch.topk leaves the order of equal values open, so log_softmax + topk may list such candidates in another order.)"""
    from halva_amd import kernels as KR
    dev = _dev()
    B, K, C, V = 4, 5, 10, 32000
    for seed in range(200):
        g = torch.Generator().manual_seed(9000 + seed)
        logits = torch.round(torch.randn(B * K, V, generator=g) * 8.0 * 2) / 2
        scores = R.beam_scores_for(B, K, "mixed", g)
        ref = R.select_reference(logits, scores, K, C)
        d = torch.cat([ref["score"], ref["next"][:, None]], 1)
        d = d[:, :-1] - d[:, 1:]
        ties = int((d[:, :C - 1] == 0).sum())
        if ties >= 2 and float(d[d > 0].min()) > 1e-3:
            break
    else:
        raise AssertionError("no draw with ties among the candidates and deciding gaps elsewhere")
    s, t, b = KR.beam_select(logits.to(dev), scores.to(dev), K, C)
    print("beam_select on half-integer logits: %d ties among the returned candidates" % ties)
    assert torch.equal(t.cpu().long(), ref["token"]) and torch.equal(b.cpu().long(), ref["beam"])


def test_select_ties_at_the_cut_go_by_lowest_index():
    """One row of equal values, and a row whose ties straddle the cut: the lower columns win, whatever fp32 makes of lse."""
    from halva_amd import kernels as KR
    dev = _dev()
    one = torch.full((1, 97), 1.0)
    s, t, b = KR.beam_select(one.to(dev), torch.zeros(1, device=dev), 1, 3)
    assert t.cpu()[0].tolist() == [0, 1, 2] and len(set(s.cpu()[0].tolist())) == 1
    row = torch.full((1, 32768), -5.0)
    row[0, [30000, 17, 4096, 4095, 32767, 9000]] = 3.0          # six equal values for four places, over several lanes, waves and groups
    row[0, 12345] = 4.0
    s, t, b = KR.beam_select(row.to(dev), torch.zeros(1, device=dev), 1, 5)
    assert t.cpu()[0].tolist() == [12345, 17, 4095, 4096, 9000] and not bool(b.any())
    s = s.cpu()[0]
    assert float(s[0]) > float(s[1]) and len(set(s[1:].tolist())) == 1


def test_select_equal_rows_tie_across_beams():
    """K identical rows under equal beam scores: every value ties across the beams; the order is beam 0 first, then 1, ... per value."""
    from halva_amd import kernels as KR
    dev = _dev()
    K, C, V = 3, 7, 97
    row = torch.linspace(-3, 3, V)
    logits = row[None].repeat(K, 1)
    s, t, b = KR.beam_select(logits.to(dev), torch.zeros(K, device=dev), K, C)
    assert t.cpu()[0].tolist() == [96, 96, 96, 95, 95, 95, 94] and b.cpu()[0].tolist() == [0, 1, 2, 0, 1, 2, 0]
    dup = logits.clone()
    dup[:, 10] = dup[:, 96]          # the same value twice inside every row: the lower column first
    s, t, b = KR.beam_select(dup.to(dev), torch.zeros(K, device=dev), K, C)
    assert t.cpu()[0].tolist() == [10, 96, 10, 96, 10, 96, 95] and b.cpu()[0].tolist() == [0, 0, 1, 1, 2, 2, 0]


@pytest.mark.parametrize("what", ["nan", "inf", "all-neg-inf"])
def test_select_flags_only_the_prompt_it_cannot_serve(what):
    from halva_amd import kernels as KR
    dev = _dev()
    B, K, C, V = 3, 3, 6, 1000
    logits, scores, ref = R.select_inputs(B, K, C, V, "mixed", seed=3)
    bad = logits.clone()
    if what == "nan":
        bad[4, 999] = float("nan")
    elif what == "inf":
        bad[4, 0] = float("inf")
    else:
        bad[4] = float("-inf")
    s, t, b = KR.beam_select(bad.to(dev), scores.to(dev), K, C)
    t, b = t.cpu().long(), b.cpu().long()
    assert t[1].tolist() == [-1] * C
    for p in (0, 2):
        assert torch.equal(t[p], ref["token"][p]) and torch.equal(b[p], ref["beam"][p])
    # a row with some -inf columns is served
    some = logits.clone()
    some[4, ::2] = float("-inf")
    s, t, b = KR.beam_select(some.to(dev), scores.to(dev), K, C)
    r2 = R.select_reference(some, scores, K, C)
    assert torch.equal(t.cpu().long(), r2["token"]) and torch.equal(b.cpu().long(), r2["beam"])


def test_select_group_alone_equals_itself_among_eight():
    from halva_amd import kernels as KR
    dev = _dev()
    K, C, V = 5, 15, 32000
    logits, scores, _ = R.select_inputs(8, K, C, V, "mixed", seed=21)
    full = KR.beam_select(_strided(logits, 5, dev), scores.to(dev), K, C)
    for p in (0, 5):
        one = KR.beam_select(logits[p * K:(p + 1) * K].to(dev).contiguous(), scores[p * K:(p + 1) * K].to(dev), K, C)
        for a, f in zip(one, full):
            assert torch.equal(a[0].view(torch.int32), f[p].view(torch.int32)), p


def test_select_limits():
    from halva_amd import hip, kernels as KR
    from halva_amd.beam import MAX_BEAMS, MAX_CANDIDATES
    dev = _dev()
    assert KR.beam_select_limits() == (32768, MAX_BEAMS, MAX_CANDIDATES)
    lib = hip.load()
    buf = torch.zeros(17 * 32769, dtype=torch.float32, device=dev)
    out = torch.zeros(4096, dtype=torch.int32, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)

    def rc(K, C, V):
        return lib.halva_beam_select(buf.data_ptr(), V, buf.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                     1, K, C, V, None)
    assert rc(2, 4, 32769) == INVALID and rc(17, 34, 1000) == INVALID and rc(16, 65, 1000) == INVALID and rc(4, 3, 1000) == INVALID
    assert rc(1, 3, 2) == INVALID          # more candidates than continuations
    assert rc(2, 4, 1000) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------
# advance
def test_advance_against_the_host_reference():
    from halva_amd import hip, kernels as KR
    dev = _dev()
    Lown = 12
    g = torch.Generator().manual_seed(4)
    sizes = [3, 4, 2]
    M = sum(sizes)
    src = torch.randint(0, M, (M, Lown), generator=g, dtype=torch.int32)
    parents = {
        "all-to-one": [0, 0, 0, 3, 3, 3, 3, 7, 7],
        "swap": [1, 0, 2, 4, 3, 6, 5, 8, 7],
        "identity": list(range(M)),
        "mixed": [2, 2, 0, 3, 6, 6, 4, 8, 8],
        "out-of-range": [0, -1, 2, M, 4, 5, 99, 7, 8],
    }
    lens = {"t0": [0] * M, "last": [Lown - 1] * M, "mid": [5] * M, "full": [5, Lown, 5, 0, Lown, 5, 5, 5, Lown + 3]}
    for pname, parent in parents.items():
        for lname, t in lens.items():
            dst = torch.full((M, Lown), -99, dtype=torch.int32)
            want = R.advance_reference(src, parent, t, dst)
            got = KR.beam_advance(src.to(dev), dst.to(dev), _t(parent), _t(t)).cpu()
            assert torch.equal(got, want), (pname, lname)
            for m in range(M):
                ok = 0 <= parent[m] < M and 0 <= t[m] < Lown
                keep = got[m, t[m] + 1:] if ok else got[m]
                assert bool((keep == -99).all()), (pname, lname, m)          # rows j > t, and whole rows that are refused, keep the sentinel
    lib = hip.load()
    a = src.to(dev)
    assert lib.halva_beam_advance(a.data_ptr(), a.data_ptr(), _t([0] * M).data_ptr(), _t([0] * M).data_ptr(), M, Lown, None) == INVALID
    with pytest.raises(hip.HalvaHipError):
        KR.beam_advance(a, a, _t([0] * M), _t([0] * M))


# ------------------------------------------------------------------------------------------------
# attention
PLENS = [1, 256, 300]
SIZES = [1, 3, 5, 16]
OWN_OF_GROUP = {0: [257, 0, 513, 255], 1: [1, 256, 0, 513], 2: [513, 255, 257, 1]}      # per launch: the own length of each group
LPRE, LOWN = 304, 516


def _attn(fn_name, q, pk, pv, plens, prefix_of, kc, vc, own, anc=None, ws_fill=float("nan")):
    from halva_amd import kernels as KR
    M = q.shape[0]
    ws = torch.empty(KR.fork_ws_bytes(M, H, pk.shape[2], kc.shape[2]), dtype=torch.uint8, device=q.device)
    ws.view(torch.float32).fill_(ws_fill)
    if anc is None:
        return KR.fork_decode_attention(q, pk, pv, _t(plens), _t(prefix_of), kc, vc, _t(own), ws, H, D)
    return KR.beam_decode_attention(q, pk, pv, _t(plens), _t(prefix_of), kc, vc, _t(own), anc.to(q.device).contiguous(), ws, H, D)


@pytest.fixture(scope="module")
def att():
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(9)
    hg = torch.Generator().manual_seed(9)
    # groups on prefix rows 0, 1, 2, 0: prefix_of must be non-decreasing, so the groups are laid out sorted by prefix row
    order = sorted(range(len(SIZES)), key=lambda i: i % len(PLENS))
    sizes = [SIZES[i] for i in order]
    prefix_of = [i % len(PLENS) for i in order for _ in range(SIZES[i])]
    M = sum(sizes)
    mk = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)      # noqa: E731
    r = dict(q=(torch.randn(M, 3 * H * D, device=dev, generator=g) * 2).to(torch.bfloat16), pk=mk(len(PLENS), H, LPRE, D), pv=mk(len(PLENS), H, LPRE, D),
             kc=mk(M, H, LOWN, D), vc=mk(M, H, LOWN, D), sizes=sizes, prefix_of=prefix_of, M=M, launches=[])
    first = [sum(sizes[:i]) for i in range(len(sizes))]
    for li in sorted(OWN_OF_GROUP):
        own, table = [], torch.full((M, LOWN), -7, dtype=torch.int32)
        for gi, (f, n) in enumerate(zip(first, sizes)):
            L = OWN_OF_GROUP[li][gi]
            own += [L] * n
            table[f:f + n] = _shifted(R.histories([n], L, LOWN, hg), f)
        r["launches"].append((own, table))
    return r


def _shifted(table, first):
    return torch.where(table >= 0, table + first, table)


def test_attention_layout_covers_the_cases(att):
    assert sorted(att["sizes"]) == [1, 3, 5, 16] and att["prefix_of"] == sorted(att["prefix_of"]) and set(att["prefix_of"]) == {0, 1, 2}
    assert {L for own, _ in att["launches"] for L in own} == {0, 1, 255, 256, 257, 513}
    for own, table in att["launches"]:
        for m, L in enumerate(own):
            lo = sum(n for n in att["sizes"][:_group_of(att, m)])
            assert bool(((table[m, :L] >= lo) & (table[m, :L] < lo + att["sizes"][_group_of(att, m)])).all())      # histories stay inside the group
    assert any(bool((table[m, :L] != m).any()) for own, table in att["launches"] for m, L in enumerate(own) if L)


def _group_of(att, m):
    acc = 0
    for gi, n in enumerate(att["sizes"]):
        acc += n
        if m < acc:
            return gi
    raise IndexError(m)


def test_attention_identity_table_is_the_fork_attention_bitwise(att):
    r = att
    ident = torch.arange(r["M"], dtype=torch.int32)[:, None].expand(r["M"], LOWN).contiguous()
    for own, _ in r["launches"]:
        a = _attn("fork", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own)
        b = _attn("beam", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own, ident)
        assert torch.isfinite(a.float()).all() and torch.equal(_i16(a), _i16(b))


def test_attention_random_tables_equal_the_fork_attention_on_materialised_caches(att):
    r = att
    for own, table in r["launches"]:
        km, vm = R.materialise(r["kc"], table, own), R.materialise(r["vc"], table, own)
        want = _attn("fork", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], km, vm, own)
        got = _attn("beam", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own, table)
        assert torch.isfinite(want.float()).all() and torch.equal(_i16(got), _i16(want))


def test_attention_reads_nothing_it_must_not(att):
    """NaN in every own slot that no table entry of the launch names, in every slot at or beyond the lengths (prefix rows too), NaN / Inf in
    the unused workspace: the outputs do not change by a bit."""
    r = att
    own, table = r["launches"][0]
    clean = _attn("beam", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own, table, ws_fill=0.0)
    named = torch.zeros(r["M"], LOWN, dtype=torch.bool)
    for m, L in enumerate(own):
        named[table[m, :L].long(), torch.arange(L)] = True
    kc, vc, pk, pv = r["kc"].clone(), r["vc"].clone(), r["pk"].clone(), r["pv"].clone()
    mask = (~named).to(kc.device)[:, None, :, None].expand_as(kc)
    kc[mask], vc[mask] = float("nan"), float("nan")
    for p, L in enumerate(PLENS):
        pk[p, :, L:], pv[p, :, L:] = float("nan"), float("nan")
    tb = table.clone()
    for m, L in enumerate(own):
        tb[m, L:] = 10 ** 6          # table entries at or beyond the length are never read either
    got = _attn("beam", r["q"], pk, pv, PLENS, r["prefix_of"], kc, vc, own, tb, ws_fill=float("inf"))
    assert int(named.sum()) < named.numel() // 2 and torch.isfinite(clean.float()).all()
    assert torch.equal(_i16(got), _i16(clean))


def test_attention_against_float64(att):
    r = att
    own, table = r["launches"][2]
    got = _attn("beam", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own, table).view(r["M"], H, D).double()
    km, vm = R.materialise(r["kc"], table, own), R.materialise(r["vc"], table, own)
    ref = torch.stack([F.decode_reference(r["q"][m, :H * D].view(H, D), r["pk"][p, :, :PLENS[p]], r["pv"][p, :, :PLENS[p]], km[m, :, :own[m]],
                                          vm[m, :, :own[m]]) for m, p in enumerate(r["prefix_of"])])
    err, tol = (got - ref).abs(), F.decode_tol(ref)
    print("beam decode attention: worst error / tolerance %.3f" % float((err / tol).max()))
    assert bool((err <= tol).all())


def test_attention_sees_a_wrong_table_entry(att):
    r = att
    own, table = r["launches"][0]
    base = _attn("beam", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own, table)
    gi = att["sizes"].index(5) if OWN_OF_GROUP[0][att["sizes"].index(5)] else att["sizes"].index(16)
    lo = sum(att["sizes"][:gi])
    m, t = lo + 1, own[lo + 1] // 2
    wrong = table.clone()
    wrong[m, t] = lo + (int(table[m, t]) - lo + 1) % att["sizes"][gi]          # a sibling: other rows in that slot
    got = _attn("beam", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own, wrong)
    changed = [i for i in range(r["M"]) if not torch.equal(_i16(got[i]), _i16(base[i]))]
    assert changed == [m], changed
    # a table entry outside [0, M) is clamped: the launch stays inside the caches and only that member differs
    wild = table.clone()
    wild[m, t] = 2 ** 30
    got = _attn("beam", r["q"], r["pk"], r["pv"], PLENS, r["prefix_of"], r["kc"], r["vc"], own, wild)
    torch.cuda.synchronize()
    assert all(torch.equal(_i16(got[i]), _i16(base[i])) for i in range(r["M"]) if i != m)
