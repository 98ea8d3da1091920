"""The fork kernels (the fork entries of halva_amd/csrc/kvcache.hip) alone: H = 2, D = 128.

Decode attention (halva_fork_decode_attn) per element against float64 under the tolerance tests/test_decode_kernels_gpu.py holds
halva_decode_attn to, |err| <= 2^-8 |ref| + 1e-4 (fork_ref_util.decode_tol): one launch over prefix rows of 1, 255, 256, 257 and 513 rows
(and one without a member), groups of 1, 2, 16, 17 and 33 members, own rows of 0, 1, 255, 256 and 257, everything inside NaN / Inf-poisoned
guarded buffers; the bitwise properties; extend_ref_util's wide-score profiles split at three places; three input mismatches.

Extend attention (halva_fork_extend_attn): every new row against float64 under extend_ref_util.row_bound (C = 2, F = 2^-8, G = 2^-14).

The appends: bit for bit what halva_decode_rope_append / halva_extend_rope_append write for the same row at the same absolute position."""

import pytest
import torch

import extend_ref_util as E
import fork_ref_util as F

pytestmark = pytest.mark.gpu

H, D = 2, 128


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda"


def _i16(t):
    return t.contiguous().view(torch.int16)


def _t(v, dev="cuda"):
    return torch.tensor(v, dtype=torch.int32, device=dev)


# ------------------------------------------------------------------------------------------------
# decode attention
PLENS = [1, 255, 100, 256, 257, 513]          # row 2 has no member
SIZES = [1, 2, 16, 17, 33]
PREFIX_OF = F.groups(SIZES, skip=(2,))
OWN_POOL = [0, 1, 255, 256, 257]
OWN = [OWN_POOL[(m + 2) % 5] for m in range(len(PREFIX_OF))]
LPRE, LOWN = 516, 260


def _decode(q, pk, pv, plens, prefix_of, kc, vc, own, ws_fill=float("nan"), Hh=H):
    from halva_amd import kernels as K
    M = q.shape[0]
    ws = torch.empty(K.fork_ws_bytes(M, Hh, pk.shape[2], kc.shape[2]), dtype=torch.uint8, device=q.device)
    ws.view(torch.float32).fill_(ws_fill)
    return K.fork_decode_attention(q, pk, pv, _t(plens), _t(prefix_of), kc, vc, _t(own), ws, Hh, D)


def _poison(pk, pv, plens, kc, vc, own, kval=float("nan"), vval=float("inf")):
    for p, L in enumerate(plens):
        pk[p, :, L:], pv[p, :, L:] = kval, vval
    for m, L in enumerate(own):
        kc[m, :, L:], vc[m, :, L:] = kval, vval


@pytest.fixture(scope="module")
def dec():
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(5)
    M, P = len(PREFIX_OF), len(PLENS)
    bufs = {}
    bufs["pk"], pk = F.guarded((P, H, LPRE, D), dev)
    bufs["pv"], pv = F.guarded((P, H, LPRE, D), dev)
    bufs["kc"], kc = F.guarded((M, H, LOWN, D), dev)
    bufs["vc"], vc = F.guarded((M, H, LOWN, D), dev)
    for t in (pk, pv, kc, vc):
        t.copy_(torch.randn(t.shape, device=dev, generator=g))
    clean = [t.clone() for t in (pk, pv, kc, vc)]
    _poison(pk, pv, PLENS, kc, vc, OWN)
    q = (torch.randn(M, 3 * H * D, device=dev, generator=g) * 2).to(torch.bfloat16)
    out = _decode(q, pk, pv, PLENS, PREFIX_OF, kc, vc, OWN)
    torch.cuda.synchronize()
    return dict(q=q, pk=pk, pv=pv, kc=kc, vc=vc, out=out, clean=clean, bufs=bufs)


def _dec_ref(r, m, plens=PLENS, prefix_of=PREFIX_OF, own=OWN, Hh=H):
    p = prefix_of[m]
    return F.decode_reference(r["q"][m, :Hh * D].view(Hh, D), r["pk"][p, :, :plens[p]], r["pv"][p, :, :plens[p]], r["kc"][m, :, :own[m]],
                              r["vc"][m, :, :own[m]])


def test_decode_layout_covers_the_cases():
    assert {PLENS[p] for p in PREFIX_OF} == {1, 255, 256, 257, 513} and 2 not in PREFIX_OF
    assert sorted(PREFIX_OF.count(p) for p in set(PREFIX_OF)) == [1, 2, 16, 17, 33]
    for p in (3, 4, 5):          # every own length under every group of 16 or more
        assert {OWN[m] for m, pp in enumerate(PREFIX_OF) if pp == p} == set(OWN_POOL)
    assert PREFIX_OF == sorted(PREFIX_OF)


def test_decode_attention_against_float64(dec):
    r = dec
    M = len(PREFIX_OF)
    got = r["out"].view(M, H, D).double()
    assert torch.isfinite(got).all()
    ref = torch.stack([_dec_ref(r, m) for m in range(M)])
    err, tol = (got - ref).abs(), F.decode_tol(ref)
    worst = (err / tol).amax((1, 2))
    print("fork decode attention: worst error / tolerance %.3f (member %d; max err %.3e)" % (float(worst.max()), int(worst.argmax()), float(err.max())))
    assert bool((err <= tol).all()), "members over: %s" % (worst > 1).nonzero().flatten().tolist()
    assert all(F.guards_intact(b) for b in r["bufs"].values())


def test_decode_poison_and_workspace_change_nothing(dec):
    r = dec
    pk, pv, kc, vc = [t.clone() for t in r["clean"]]
    a = _decode(r["q"], pk, pv, PLENS, PREFIX_OF, kc, vc, OWN, ws_fill=0.0)
    _poison(pk, pv, PLENS, kc, vc, OWN, float("nan"), float("nan"))
    b = _decode(r["q"], pk, pv, PLENS, PREFIX_OF, kc, vc, OWN, ws_fill=float("inf"))
    torch.cuda.synchronize()
    assert torch.equal(_i16(a), _i16(r["out"])) and torch.equal(_i16(b), _i16(r["out"]))


def _subset(r, members, lpre, lown):
    """The given members of the full launch (all of one prefix row, or any) in a launch of their own, in caches of other capacities."""
    dev = r["q"].device
    rows = sorted({PREFIX_OF[m] for m in members})
    pk = torch.full((len(rows), H, lpre, D), float("nan"), dtype=torch.bfloat16, device=dev)
    pv = torch.full_like(pk, float("nan"))
    kc = torch.full((len(members), H, lown, D), float("nan"), dtype=torch.bfloat16, device=dev)
    vc = torch.full_like(kc, float("nan"))
    for i, p in enumerate(rows):
        pk[i, :, :PLENS[p]], pv[i, :, :PLENS[p]] = r["pk"][p, :, :PLENS[p]], r["pv"][p, :, :PLENS[p]]
    for j, m in enumerate(members):
        kc[j, :, :OWN[m]], vc[j, :, :OWN[m]] = r["kc"][m, :, :OWN[m]], r["vc"][m, :, :OWN[m]]
    q = r["q"][members].contiguous()
    return _decode(q, pk, pv, [PLENS[p] for p in rows], [rows.index(PREFIX_OF[m]) for m in members], kc, vc, [OWN[m] for m in members])


def test_decode_member_alone_equals_itself_in_the_launch(dec):
    for m in (0, 2, 19, 35, 36, 68):
        one = _subset(dec, [m], PLENS[PREFIX_OF[m]] + 5, max(OWN[m], 1) + 2)
        assert torch.equal(_i16(one[0]), _i16(dec["out"][m])), m


def test_decode_member_at_another_offset_in_its_block(dec):
    first = PREFIX_OF.index(5)                         # the group of 33
    members = [first + 20, first + 5, first + 32] + [first + 5] * 15 + [first + 5, first + 16]      # first + 5 at many offsets of two blocks
    out = _subset(dec, members, LPRE + 3, LOWN + 1)
    torch.cuda.synchronize()
    for j, m in enumerate(members):
        assert torch.equal(_i16(out[j]), _i16(dec["out"][m])), (j, m)


def test_decode_wide_scores_against_float64():
    """extend_ref_util's five profiles over 700 keys, one query row each, the keys split into prefix and own rows at 2, 400 and 650: the spike of
    `spike_first` (key 3) and of `spike_late` (key 630) falls on either side of the boundary."""
    dev = _dev()
    L, splits = 700, (2, 400, 650)
    ins = [E.wide_inputs(name, L, 1, seed=E.WIDE_SEEDS[0]) for name in E.WIDE_PROFILES]
    cases = [(i, s) for i in range(len(ins)) for s in splits]
    M = len(cases)
    pk = torch.full((M, 1, 653, D), float("nan"), dtype=torch.bfloat16, device=dev)
    pv = torch.full((M, 1, 653, D), float("inf"), dtype=torch.bfloat16, device=dev)
    kc = torch.full((M, 1, 701, D), float("nan"), dtype=torch.bfloat16, device=dev)
    vc = torch.full((M, 1, 701, D), float("inf"), dtype=torch.bfloat16, device=dev)
    for m, (i, s) in enumerate(cases):
        _, Kb, Vb = ins[i]
        pk[m, :, :s], pv[m, :, :s] = Kb[:, :s].to(dev), Vb[:, :s].to(dev)
        kc[m, :, :L - s], vc[m, :, :L - s] = Kb[:, s:].to(dev), Vb[:, s:].to(dev)
    q = torch.cat([ins[i][0][0] for i, _ in cases]).to(dev).contiguous()
    out = _decode(q, pk, pv, [s for _, s in cases], list(range(M)), kc, vc, [L - s for _, s in cases], Hh=1)
    torch.cuda.synchronize()
    ref = torch.stack([E.reference(*ins[i], L - 1, 1)[:, 0] for i, _ in cases]).to(dev)      # the last row sees every key
    got = out.view(M, 1, D).double()
    assert torch.isfinite(got).all()
    err, tol = (got - ref).abs(), F.decode_tol(ref)
    print("fork decode attention, wide scores: worst error / tolerance %.3f" % float((err / tol).max()))
    assert bool((err <= tol).all()), [(E.WIDE_PROFILES[cases[m][0]], cases[m][1]) for m in ((err / tol).amax((1, 2)) > 1).nonzero().flatten().tolist()]


# ---- input mismatches: the kernel is given an input that differs from the reference's; only the affected members may be reported
MM_PLENS, MM_OF, MM_OWN = [40, 37], [0, 0, 0, 1, 1], [5, 9, 3, 7, 4]


@pytest.fixture(scope="module")
def mm():
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(71)
    mk = lambda *s: torch.randn(*s, device=dev, generator=g).to(torch.bfloat16)      # noqa: E731
    return dict(q=mk(5, H * D), pk=mk(2, H, 48, D), pv=mk(2, H, 48, D), kc=mk(5, H, 16, D), vc=mk(5, H, 16, D))


def _mm_violations(mm, plens=MM_PLENS, **changed):
    a = dict(mm, **changed)
    out = _decode(a["q"], a["pk"], a["pv"], plens, MM_OF, a["kc"], a["vc"], MM_OWN)
    torch.cuda.synchronize()
    ref = torch.stack([_dec_ref(mm, m, MM_PLENS, MM_OF, MM_OWN) for m in range(5)])
    err = (out.view(5, H, D).double() - ref).abs()
    return {m for m in range(5) if bool((err[m] > F.decode_tol(ref[m])).any())}


def test_mismatch_control_has_no_violation(mm):
    assert _mm_violations(mm) == set()


def test_mismatch_swapped_prefix_key_rows(mm):
    pk = mm["pk"].clone()
    pk[0, :, [11, 12]] = mm["pk"][0][:, [12, 11]]
    assert _mm_violations(mm, pk=pk) == {0, 1, 2}


def test_mismatch_prefix_lens_off_by_one(mm):
    assert _mm_violations(mm, plens=[40, 38]) == {3, 4}


def test_mismatch_scaled_own_value_row(mm):
    vc = mm["vc"].clone()
    vc[1, :, 4] = (vc[1, :, 4].float() * 1.5).to(torch.bfloat16)
    assert _mm_violations(mm, vc=vc) == {1}


# ------------------------------------------------------------------------------------------------
# extend attention: prefix_lens mod 64 in {0, 1, 63} x own_lens mod 64 in {0, 1, 63}, n_new in {0, 1, 31, 33, 129}, one block clipped by Lown
X_PLENS = [64, 129, 63]
X_OF = [0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2]
X_PAST = [64, 1, 63, 195, 0, 65, 63, 64, 1, 63, 17]
X_NEW = [129, 31, 33, 9, 129, 1, 129, 33, 129, 31, 0]
X_N, X_LPRE, X_LOWN = 129, 132, 200


def test_extend_layout_covers_the_cases():
    combos = {(X_PLENS[p] % 64, past % 64) for p, past, n in zip(X_OF, X_PAST, X_NEW) if n and past < 195}
    assert combos == {(a, b) for a in (0, 1, 63) for b in (0, 1, 63)}
    assert set(X_NEW) == {0, 1, 31, 33, 129, 9}
    rows = [E.ext_rows(p, n, X_N, X_LOWN) for p, n in zip(X_PAST, X_NEW)]
    assert rows[3] == 5 and rows[:3] == X_NEW[:3] and max(p + r for p, r in zip(X_PAST, rows)) <= X_LOWN


@pytest.fixture(scope="module")
def ext():
    dev = _dev()
    from halva_amd import kernels as K
    g = torch.Generator(device=dev).manual_seed(29)
    M, P = len(X_OF), len(X_PLENS)
    rows = [E.ext_rows(p, n, X_N, X_LOWN) for p, n in zip(X_PAST, X_NEW)]
    cos, sin = K.rope_tables(D, X_LPRE + X_LOWN, device=dev)
    bufs = {}
    bufs["pk"], pk = F.guarded((P, H, X_LPRE, D), dev)
    bufs["pv"], pv = F.guarded((P, H, X_LPRE, D), dev)
    bufs["kc"], kc = F.guarded((M, H, X_LOWN, D), dev)
    bufs["vc"], vc = F.guarded((M, H, X_LOWN, D), dev)
    for t in (pk, pv, kc, vc):
        t.copy_(torch.randn(t.shape, device=dev, generator=g))
    x = torch.randn(M, X_N, 3 * H * D, device=dev, generator=g).to(torch.bfloat16)
    for p, L in enumerate(X_PLENS):
        pk[p, :, L:], pv[p, :, L:] = float("nan"), float("inf")
    for m in range(M):
        x[m, X_NEW[m]:] = float("nan")
        kc[m, :, X_PAST[m]:], vc[m, :, X_PAST[m]:] = float("nan"), float("inf")
    k0, v0 = kc.clone(), vc.clone()
    plens, of, own, n_new = _t(X_PLENS), _t(X_OF), _t(X_PAST), _t(X_NEW)
    qkv = x.clone()
    K.fork_extend_rope_append(qkv, cos, sin, plens, of, kc, vc, own, n_new, H, D)
    width = H * D + 8
    out = torch.full((M, X_N, width), F.SENTINEL, dtype=torch.bfloat16, device=dev)
    K.fork_extend_attention(qkv, pk, pv, plens, of, kc, vc, own, n_new, H, D, out_width=width, out=out)
    own_before = own.clone()
    K.extend_advance(own, n_new, X_LOWN)
    torch.cuda.synchronize()
    return dict(cos=cos, sin=sin, x=x, k0=k0, v0=v0, pk=pk, pv=pv, kc=kc, vc=vc, qkv=qkv, out=out, rows=rows, own=own, own_before=own_before,
                plens=plens, of=of, n_new=n_new, bufs=bufs)


def _ext_ratios(out, qkv, r, members=None):
    eks, ems, nrs, cnt = [], [], [], []
    for j, m in enumerate(range(len(X_OF)) if members is None else members):
        n = r["rows"][m]
        cnt.append(n)
        if n == 0:
            continue
        p = X_OF[m]
        Kc, Vc, past = F.extend_operands(r["pk"][p], r["pv"][p], X_PLENS[p], r["kc"][m], r["vc"][m], X_PAST[m], n)
        assert torch.isfinite(Kc.float()).all() and torch.isfinite(Vc.float()).all(), m
        qm = qkv[j, :n, :H * D].view(n, H, D).transpose(0, 1)
        got = out[j, :n, :H * D].view(n, H, D).transpose(0, 1)
        assert torch.isfinite(got.float()).all(), m
        ek, em, nr = E.row_errors(got, E.reference(qm, Kc, Vc, past, n), E.model(qm, Kc, Vc, past, n))
        eks.append(ek), ems.append(em), nrs.append(nr)
    ratio = torch.cat(eks) / E.row_bound(torch.cat(ems), torch.cat(nrs))
    return torch.split(ratio, [H * n for n in cnt if n])


def test_extend_rows_against_float64(ext):
    r = ext
    ratios = _ext_ratios(r["out"], r["qkv"], r)
    worst = [float(q.max()) for q in ratios]
    print("fork extend attention: worst row error / bound %.3f over %d rows" % (max(worst), sum(q.numel() for q in ratios)))
    assert max(worst) <= 1.0, worst
    for m, n in enumerate(r["rows"]):      # rows at or beyond the new ones and the columns beyond H*D keep the sentinel
        assert (r["out"][m, n:] == F.SENTINEL).all() and (r["out"][m, :, H * D:] == F.SENTINEL).all(), m
    assert all(F.guards_intact(b) for b in r["bufs"].values())
    assert r["own_before"].tolist() == X_PAST and r["own"].tolist() == [min(p + n, X_LOWN) for p, n in zip(X_PAST, X_NEW)]


def test_extend_append_is_the_plain_append_at_the_absolute_position(ext):
    """halva_extend_rope_append on a plain cache whose lens are prefix_lens + own_lens: the same rotated q, the same k / v rows."""
    from halva_amd import kernels as K
    r = ext
    M, Lcap = len(X_OF), X_LPRE + X_LOWN
    pos = [X_PLENS[p] + past for p, past in zip(X_OF, X_PAST)]
    kp = torch.full((M, H, Lcap, D), float("nan"), dtype=torch.bfloat16, device="cuda")
    vp = torch.full_like(kp, float("nan"))
    qkv = r["x"].clone()
    K.extend_rope_append(qkv, r["cos"], r["sin"], kp, vp, _t(pos), _t(r["rows"]), H, D)
    torch.cuda.synchronize()
    for m, n in enumerate(r["rows"]):
        assert torch.equal(_i16(qkv[m, :n]), _i16(r["qkv"][m, :n])), m
        assert torch.equal(_i16(r["qkv"][m, n:]), _i16(r["x"][m, n:])), m                  # rows without a slot are left as they were
        a, b = X_PAST[m], X_PAST[m] + n
        assert torch.equal(_i16(kp[m, :, pos[m]:pos[m] + n]), _i16(r["kc"][m, :, a:b])), m
        assert torch.equal(_i16(vp[m, :, pos[m]:pos[m] + n]), _i16(r["vc"][m, :, a:b])), m
        assert torch.equal(_i16(r["kc"][m, :, :a]), _i16(r["k0"][m, :, :a])) and torch.equal(_i16(r["kc"][m, :, b:]), _i16(r["k0"][m, :, b:])), m
        assert torch.equal(_i16(r["vc"][m, :, :a]), _i16(r["v0"][m, :, :a])) and torch.equal(_i16(r["vc"][m, :, b:]), _i16(r["v0"][m, :, b:])), m


@pytest.mark.parametrize("m", [0, 6, 8])
def test_extend_member_alone_equals_its_rows_in_the_batch(ext, m):
    from halva_amd import kernels as K
    r = ext
    p, n = X_OF[m], r["rows"][m]
    assert n == 129
    kc, vc, qkv = r["k0"][m:m + 1].clone(), r["v0"][m:m + 1].clone(), r["x"][m:m + 1].clone()
    pk, pv = r["pk"][p:p + 1].clone(), r["pv"][p:p + 1].clone()
    plens, of, own, n_new = _t([X_PLENS[p]]), _t([0]), _t([X_PAST[m]]), _t([X_NEW[m]])
    K.fork_extend_rope_append(qkv, r["cos"], r["sin"], plens, of, kc, vc, own, n_new, H, D)
    out = K.fork_extend_attention(qkv, pk, pv, plens, of, kc, vc, own, n_new, H, D)
    assert torch.equal(_i16(kc), _i16(r["kc"][m:m + 1])) and torch.equal(_i16(qkv), _i16(r["qkv"][m:m + 1]))
    assert torch.equal(_i16(out[0, :n]), _i16(r["out"][m, :n, :H * D]))


def test_extend_strides_with_gaps_through_the_c_abi(ext):
    """ldseq > n ldrow and ld_out_seq > n ld_out_row: append and attention equal the contiguous call's, bit for bit, and leave the gaps alone."""
    from halva_amd import hip
    r = ext
    lib, P, dev = hip.load(), hip.ptr, "cuda"
    M, n = len(X_OF), X_N
    ldrow, ldo = 3 * H * D + 8, H * D + 8
    ldseq, ldos = n * ldrow + 16, n * ldo + 24
    qbuf = torch.full((M * ldseq,), float("nan"), dtype=torch.bfloat16, device=dev)
    obuf = torch.full((M * ldos,), F.SENTINEL, dtype=torch.bfloat16, device=dev)
    qv = qbuf.as_strided((M, n, 3 * H * D), (ldseq, ldrow, 1))
    ov = obuf.as_strided((M, n, H * D), (ldos, ldo, 1))
    qv.copy_(r["x"])
    qgap = torch.ones(M * ldseq, dtype=torch.bool, device=dev)
    qgap.as_strided((M, n, 3 * H * D), (ldseq, ldrow, 1)).fill_(False)
    ogap = torch.ones(M * ldos, dtype=torch.bool, device=dev)
    ogap.as_strided((M, n, H * D), (ldos, ldo, 1)).fill_(False)
    k2, v2 = r["k0"].clone(), r["v0"].clone()
    own = _t(X_PAST)
    assert lib.halva_fork_extend_rope_append(P(qbuf), ldrow, ldseq, P(r["cos"]), P(r["sin"]), r["cos"].shape[0], P(r["plens"]), P(r["of"]), P(k2), P(v2),
                                             P(own), P(r["n_new"]), M, n, len(X_PLENS), H, D, X_LOWN, hip.stream_ptr()) == 0, lib.halva_last_error()
    assert lib.halva_fork_extend_attn(P(qbuf), ldrow, ldseq, P(r["pk"]), P(r["pv"]), P(r["plens"]), P(r["of"]), P(k2), P(v2), P(own), P(r["n_new"]),
                                      P(obuf), ldo, ldos, M, n, len(X_PLENS), H, D, X_LPRE, X_LOWN, 0.0, hip.stream_ptr()) == 0, lib.halva_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_i16(k2), _i16(r["kc"])) and torch.equal(_i16(v2), _i16(r["vc"]))
    assert torch.equal(_i16(qv.contiguous()), _i16(r["qkv"]))
    assert torch.equal(_i16(ov.contiguous()), _i16(r["out"][..., :H * D]))
    assert torch.isnan(qbuf[qgap].float()).all() and (obuf[ogap] == F.SENTINEL).all()
    assert lib.halva_fork_extend_attn(P(qbuf), ldrow, n * ldrow - 8, P(r["pk"]), P(r["pv"]), P(r["plens"]), P(r["of"]), P(k2), P(v2), P(own),
                                      P(r["n_new"]), P(obuf), ldo, ldos, M, n, len(X_PLENS), H, D, X_LPRE, X_LOWN, 0.0, hip.stream_ptr()) == -1
    assert b"sequence stride" in lib.halva_last_error()


def test_extend_wide_scores_against_float64():
    """extend_ref_util's profiles (37 + 300 keys behind a prefix of 128): the first 128 keys of each profile are the prefix row, own past = 37.
    tests/test_fork_cpu.py shows these inputs admissible through extend_ref_util.emulate with the prefix tiles in front."""
    dev = _dev()
    from halva_amd import kernels as K
    plen, past, m = 128, 37, 300
    L = plen + past + m
    ins = [E.wide_inputs(name, L, m, seed=E.WIDE_SEEDS[0]) for name in E.WIDE_PROFILES]
    B = len(ins)
    pk = torch.full((B, 1, plen + 3, D), float("nan"), dtype=torch.bfloat16, device=dev)
    pv = torch.full_like(pk, float("inf"))
    kc = torch.full((B, 1, past + m + 7, D), float("nan"), dtype=torch.bfloat16, device=dev)
    vc = torch.full_like(kc, float("inf"))
    qq = torch.empty(B, m, D, dtype=torch.bfloat16, device=dev)
    for b, (qb, Kb, Vb) in enumerate(ins):
        pk[b, :, :plen], pv[b, :, :plen] = Kb[:, :plen].to(dev), Vb[:, :plen].to(dev)
        kc[b, :, :past + m], vc[b, :, :past + m] = Kb[:, plen:].to(dev), Vb[:, plen:].to(dev)
        qq[b] = qb[0].to(dev)
    out = K.fork_extend_attention(qq, pk, pv, _t([plen] * B), _t(list(range(B))), kc, vc, _t([past] * B), _t([m] * B), 1, D)
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    worst = {}
    for b, (qb, Kb, Vb) in enumerate(ins):
        qd, Kd, Vd = qb.to(dev), Kb.to(dev), Vb.to(dev)
        ek, em, nr = E.row_errors(out[b].view(m, 1, D).transpose(0, 1), E.reference(qd, Kd, Vd, plen + past, m), E.model(qd, Kd, Vd, plen + past, m))
        worst[E.WIDE_PROFILES[b]] = round(float((ek / E.row_bound(em, nr)).max()), 3)
    print("fork extend attention, wide scores: worst row error / bound %s" % worst)
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------
# the single-row append
def test_rope_append_is_the_plain_append_at_the_absolute_position():
    """halva_fork_rope_append against halva_decode_rope_append on a plain cache with lens = prefix_lens + own_lens, on tables with VILA's
    linear scaling that run past max_position_embeddings = 48; a full own cache and a position beyond the tables write nothing."""
    dev = _dev()
    from halva_amd import kernels as K
    Hh, Lown, max_pos = 4, 12, 96
    cos, sin = K.rope_tables(D, max_pos, 10000.0, dev, 2.0)
    plens_l, of_l = [1, 47, 80, 90], [0, 0, 1, 1, 2, 2, 3, 3]
    own_l = [0, 5, 0, 11, 3, 12, 5, 6]                 # member 5: own cache full; member 7: position 96 = max_pos
    M = len(of_l)
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(M, 3 * Hh * D, device=dev, generator=g).to(torch.bfloat16)
    kc = torch.full((M, Hh, Lown, D), float("nan"), dtype=torch.bfloat16, device=dev)
    vc = torch.full_like(kc, float("nan"))
    qkv, own = x.clone(), _t(own_l)
    K.fork_rope_append(qkv, cos, sin, _t(plens_l), _t(of_l), kc, vc, own, Hh, D)
    pos = [plens_l[p] + t for p, t in zip(of_l, own_l)]
    ok = [t < Lown and a < max_pos for t, a in zip(own_l, pos)]
    assert ok == [True, True, True, True, True, False, True, False] and max(a for a, o in zip(pos, ok) if o) > 48
    kp = torch.full((M, Hh, 128, D), float("nan"), dtype=torch.bfloat16, device=dev)
    vp = torch.full_like(kp, float("nan"))
    ref, lens = x.clone(), _t([a if o else 128 for a, o in zip(pos, ok)])          # (a full plain cache is left as it is)
    K.decode_rope_append(ref, cos, sin, kp, vp, lens, Hh, D)
    torch.cuda.synchronize()
    assert torch.equal(_i16(qkv), _i16(ref))
    assert own.tolist() == [t + 1 if o else t for t, o in zip(own_l, ok)]
    for m in range(M):
        if ok[m]:
            assert torch.equal(_i16(kc[m, :, own_l[m]]), _i16(kp[m, :, pos[m]])) and torch.equal(_i16(vc[m, :, own_l[m]]), _i16(vp[m, :, pos[m]])), m
            assert int(torch.isnan(kc[m].float()).all(-1).sum()) == Hh * (Lown - 1)
        else:
            assert torch.isnan(kc[m].float()).all() and torch.isnan(vc[m].float()).all() and torch.equal(_i16(qkv[m]), _i16(x[m])), m
