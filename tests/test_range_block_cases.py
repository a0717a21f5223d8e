"""CPU tests of range_block_cases.py: every case for the batched ExGETRF / ExGETRS / ExPOTRF / ExPOTRS has, through the
exact models, the property it is named for, the counter formula, and is SENSITIVE: at the named entry the plain fp64
restatement gives other bits or other pivots ("plain"), or the total is an exact tie ("tie"; "reference" where the
reference rounding takes it the other way: on the ties of range_rows_trsv it does not, the two rules agree there, so the
planted ties of the neighbours tell the modes apart in the GPU tests), or it is a tie or lies where the register certificate
may not decide ("settle": the GPU tests then find it in the accumulator's counter), or it is a zero whose sign is the
statement ("zero").  No GPU involved."""
import math
from fractions import Fraction

import numpy as np
import pytest

import bjacobi_cases as J
import blas1_cases as B
import exact_cases as E
import getrf_cases as G
import potrf_cases as P
import range_block_cases as R


def _bits(a, b):
    return G.J_same(np.array([a], dtype=np.float64), np.array([b], dtype=np.float64))


def _reference(oracle, t):
    """the reference rule's rounding of the exact total t"""
    T = t * B.ONE
    assert T.denominator == 1
    return oracle.round_limbs(B.canon_from_int(int(T)), mode=oracle.ROUND_REFERENCE)


def _threshold(t):
    return abs(t) == Fraction(2 ** 1024 - 2 ** 970)


def _sensitivity(oracle, e):
    """the ways in which case entry e tells a wrong kernel from a right one"""
    c, out = e.case, set()
    W, ipiv, info = G.plain_getrf(e.A)
    if not _bits(W[c.at], e.W[c.at]) or (ipiv != e.ipiv).any() or info != e.info:
        out.add("plain")
    t = getattr(c, "total", None)
    if t is None:
        t = e.totals.get(c.at)
    if t is not None:
        if R.is_tie(t) or _threshold(t):
            out.add("tie")
            if not _bits(_reference(oracle, t), P._round(t)):
                out.add("reference")
        if R.settles(t):
            out.add("settle")
        if t == 0:
            out.add("zero")
    if c.row == "total just above 2^-960":
        out.add("control")               # the inner member of its pair: one settled rounding fewer than its neighbour below
    if e.W[c.at] != 0 and abs(e.W[c.at]) < 2.0 ** -1022:
        out.add("settle")                # a subnormal quotient
    return out


def test_the_rows_and_the_short_list_of_rows_left_out():
    names = [r[0] for r in R.rows()]
    assert set(E.range_rows_trsv(0).names) <= set(names) and len(set(names)) == len(names) == 15
    print("left out:", R.LEFT_OUT)
    assert set(R.LEFT_OUT) <= set(names)
    built = {c.row for c in R.getrf_cases(0)}
    assert built == (set(names) - set(R.LEFT_OUT)) | {"rounding decides the pivot"} | {c.row for c in R.hand_made()}
    for form in ("cand", "U"):
        assert {c.cls for c in R.getrf_cases(0) if c.form == form} == {1, 2, 3, 4, 5, 6}, form
    # the sizes: p - q covers the four residues mod 4, so that the range products meet every slot of the inner loop
    res = {(p - (R.NSUP + 2 + s)) % 4 for p, s in R.EMBED} | {0}
    assert res == {0, 1, 2, 3}
    for shift in (1, 2, 3):
        assert [c.name for c in R.getrf_cases(shift)] == [c.name for c in R.getrf_cases(0)]


@pytest.mark.parametrize("shift", [0, 3])
def test_every_getrf_case_has_its_property_and_is_sensitive(oracle, shift):
    r = E.range_rows_trsv(0)
    seen = {}
    for e in R.getrf_entries(shift):
        c = e.case
        q = e.A.shape[0]
        sens = _sensitivity(oracle, e)
        print(c.cls, c.name, "info", e.info, "pivots", e.ipiv.tolist()[-2:], "at", c.at, repr(e.W[c.at]), "settle", e.settle,
              sorted(sens))
        assert sens, c.name
        assert e.roundings == G.roundings(q, e.info)
        if c.want is not None:
            assert _bits(e.W[c.at], c.want), (c.name, e.W[c.at], c.want)
        # the model's own totals round to the model's own entries: the identity P A = L U on the doubles
        for (i, j), t in e.totals.items():
            v = P._round(t)
            with np.errstate(all="ignore"):
                got = v if j >= i or e.info == q and j == q - 1 else float(np.float64(v) / np.float64(e.W[j, j]))
            assert _bits(got, e.W[i, j]), (c.name, i, j)
        assert all(R.in_domain(e.W[i, k], e.W[k, j]) for i in range(q) for j in range(q) for k in range(min(i, j))), c.name
        if hasattr(c, "total"):
            s = R.NSUP + c.shift
            assert (e.ipiv[:s] == np.arange(1, s + 1)).all()
            if c.cls == 6 and c.form == "cand":   # the larger of the two candidates is the pivot, the other one lies below it
                assert c.total in (e.totals[s, s], e.totals[s + 1, s]) and c.total != Fraction(e.A[s, s])
            else:
                assert e.totals[c.at if c.form == "U" or c.pivot else (s + 1, s)] == c.total
            if c.form == "U":
                assert e.info == (q if math.isinf(c.want) else 0) and _bits(e.W[s + 1, s], c.l) and e.ipiv[s] == s + 1
                assert math.isnan(e.W[q - 1, q - 1]) == math.isinf(c.want)
            elif c.pivot is True:
                assert e.info == 0 and e.ipiv[s] == s + 1 and _bits(e.W[s + 1, s], c.l)
            elif c.pivot is False:
                assert e.info == 0 and e.ipiv[s] == s + 2
                if c.row in r.rows:           # the multiplier is what ExTRSV's row gives
                    assert _bits(e.W[c.at], r.want[r.rows[c.row]]), c.name
        if c.cls == 1:
            assert "settle" in sens
            assert e.W[c.at] in (math.inf, R.DMAX)
        if c.cls == 2:
            assert R.is_tie(c.total) and "settle" in sens and 2.0 ** 1000 <= abs(e.W[c.at]) < 2.0 ** 1001
        if c.cls == 4:
            assert c.total == 0 and "zero" in sens and e.W[c.at] == 0
            assert math.copysign(1.0, e.W[c.at]) == (math.copysign(1.0, c.l) if c.form == "cand" else 1.0)
            assert math.copysign(1.0, e.W[R.NSUP + c.shift + 1, R.NSUP + c.shift]) == (1.0 if "positive" in c.name else -1.0)
        if c.cls == 5:
            assert "plain" in sens and len(rowdict(c.row)) >= 6
            ex = [math.frexp(a * R.support()[k])[1] for k, a in rowdict(c.row).items()]
            assert max(ex) - min(ex) > 4 * 53
        if c.cls == 6:
            assert "plain" in sens
            if c.form == "cand":
                assert e.ipiv[R.NSUP + c.shift] == c.exact_pivot != G.plain_getrf(e.A)[1][R.NSUP + c.shift] == c.plain_pivot
        seen.setdefault(c.cls, set()).update(sens)
    assert seen[3] >= {"settle", "plain"} and "plain" in seen[1] and "tie" in seen[1] and "tie" in seen[2] and seen[4] == {"zero"}
    named = {c.row: e for e in R.getrf_entries(shift) for c in [e.case] if c.form == "cand"}
    assert named["total just below 2^-960"].settle == named["total just above 2^-960"].settle + 1
    assert named["2 x 2 pivot among subnormal candidates"].ipiv[0] == 2
    assert named["3 x 3 subnormal candidate and quotient"].W[2, 1] == -3 * R.TINY


def rowdict(name):
    return next(r[4] for r in R.rows() if r[0] == name)


@pytest.mark.parametrize("p", [9, 20, 33])
def test_embedded_entries_are_what_the_model_gives(p):
    """the composition of blockdiag(dominant, case) from its two factorisations is getrf_exact of the whole; the row shuffle
    either keeps the factors with other pivots or it does not, and then the copy is dropped"""
    kept = 0
    for e in R.getrf_at(p):
        W, ipiv, info = G.getrf_exact(e.A)
        assert G.J_same(W, e.W) and (ipiv == e.ipiv).all() and info == e.info, e.name
        assert e.roundings == G.roundings(p, info) and e.settle >= e.parts[1].settle
        s = R.shuffled_entry(e)
        if s is not None:
            W2, ipiv2, info2 = G.getrf_exact(s.A)
            assert (s.ipiv != e.ipiv).any() and G.J_same(s.W, e.W) and G.J_same(W2, W) and (ipiv2 == s.ipiv).all() and info2 == info
            assert (np.sort(s.A, axis=0) == np.sort(e.A, axis=0)).all() and (s.A != e.A).any()
            kept += 1
        else:
            small = e.parts[1]
            W2, _, info2 = G.getrf_exact(G.shuffled(small.A, 7))
            assert info2 != small.info or not G.J_same(W2, small.W)
    print(p, "shuffled copies kept", kept, "of", len(R.getrf_at(p)))
    assert kept >= 10


def test_potrf_cases_and_roots():
    for p in (2, 3, 4, 9, 20, 33):
        names = [e.name for e in R.potrf_at(p)]
        for e in R.potrf_at(p):
            Rm, info = P.potrf_exact(e.G, "U")
            assert info == e.info and G.J_same(np.triu(Rm), np.triu(e.R)), e.name
            assert e.fixed == P.fixed_entries(p, info)
            pr, pinfo = J.plain_factor(e.G)
            print(p, e.name, "info", e.info, "settle", e.settle,
                  "plain differs", pinfo != info or not G.J_same(np.triu(pr), np.triu(e.R)))
            if e.name.startswith("subnormal"):
                assert e.info == 0 and e.settle >= 1 and (pinfo != info or not G.J_same(np.triu(pr), np.triu(e.R)))
            if e.name.startswith("overflow"):
                assert e.info == p and e.R[p - 2, p - 1] == np.inf and e.R[p - 1, p - 1] == -np.inf and e.settle >= 1
            if e.name.startswith("inf"):
                assert e.info == 0 and np.isinf(e.R).sum() == 1
            if e.name.startswith("roots"):
                v = np.diag(e.G)
                assert (np.diag(e.R).view(np.int64) == np.array([math.sqrt(x) for x in v]).view(np.int64)).all()
        if p >= 9:
            assert len(names) == 7 and sum(n.startswith("roots") for n in names) == 3
    v = np.diag(R.root_diagonal(64, 2))
    assert {5e-324, R.DMAX, 2.0 ** -1022, float(np.nextafter(2.0 ** -1022, 0.0))} <= set(v.tolist())
    k = np.sqrt(np.diag(R.root_diagonal(64, 1))[10:50])
    assert (k == np.round(k)).all()                                   # perfect squares
    assert R.potrf_at(64)[-1].settle == 4


@pytest.mark.parametrize("lead", [0, 14, 46])
def test_range_blocks_for_the_apply(oracle, lead):
    r = E.range_rows_trsv(lead)
    p = lead + 18
    assert r.n == p
    full, safe, half = (R.range_block(lead, v) for v in R.VARIANTS)
    print(p, "dropped from half:", half.dropped)
    assert full.dropped == () and safe.dropped == ("tie at the overflow threshold",) and 0 < len(half.dropped) <= 4
    x, tot = R.trsv_ieee(full.L, full.B[:, 0])
    xe, tote = E.trsv_exact(r.L, r.b)
    assert G.J_same(x, xe) and tot == tote and G.J_same(x, r.want) and x[-1] == np.inf
    for c in range(1, R.NPAT):
        xc, _ = R.trsv_ieee(full.L, full.B[:, c])
        assert np.isfinite(xc).all() and (xc[:-1] == x[:-1] * (1, -1, 1, -1, 1)[c]).all()      # (an exact zero is +0 either way)
    # sensitive: the ties go the other way under the reference rounding, and something differs from plain fp64
    ties = [i for i, t in enumerate(tot) if R.is_tie(t) or _threshold(t)]
    assert len(ties) >= 6
    flipped = [i for i in ties if not _bits(oracle.round_limbs(B.canon_from_int(int(tot[i] * B.ONE)), mode=oracle.ROUND_REFERENCE),
                                            P._round(tot[i]))]
    print("ties", len(ties), "of which the reference rounding takes the other way:", len(flipped))
    assert not G.J_same(J.plain_solve(np.ascontiguousarray(full.L.T), full.B[:, 0], "1"), x)
    assert sum(R.settles(t) for t in tot) >= 10
    xh, toth = R.trsv_ieee(half.L, half.B[:, 0])
    assert np.isfinite(xh).all() and xh[-1] == 2.0 ** 1023 and R.is_tie(toth[-1])
    # the two sweeps of ExPOTRS and the two directions of ExGETRS meet the same totals
    for sweep in ("1", "2"):
        seven = R.potrs_seven(p, sweep)
        assert [e.name.split()[0] for e in seven] == ["healthy", "range", "planted", "range", "healthy", "range", "nan"]
        for rows in (p, lead + 6, lead + 12):
            fullF, X0, want, settle = R.potrs_case(seven, p, 6 * p + rows, 5, sweep, "U")
            # the healthy and the planted blocks are what bjacobi_cases.solve_model gives
            for b, kind in ((0, 0), (2, 5 if sweep == "1" else 6), (4, 1)):
                Xm, _ = J.solve_model(p, kind, p, sweep)
                assert G.J_same(want[b * p:(b + 1) * p], Xm)
            blk = want[p:2 * p, 0] if sweep == "1" else want[p:2 * p, 0][::-1]
            assert G.J_same(blk, r.want)
            assert np.isnan(want[6 * p:, :]).all() and settle >= 10
            plain = J.plain_solve(np.triu(np.nan_to_num(fullF[1])), X0[p:2 * p, 0], sweep)
            assert not G.J_same(plain, want[p:2 * p, 0])
    for turn in (0, 1):
        seven = R.getrs_seven(p, turn)
        for rows in (p, lead + 6, lead + 12):
            LU, ipiv, X0, want, settle = R.getrs_case(seven, p, 6 * p + rows, 5)
            for b in (0, 2, 4):                                           # finite blocks: getrs_model itself
                for c in range(5):
                    xm, _ = G.getrs_model(LU[b], ipiv[b], X0[b * p:(b + 1) * p, c])
                    assert G.J_same(want[b * p:(b + 1) * p, c], xm)
            assert settle >= 10
            for b in (1, 3, 5):
                e = seven[b]
                col = want[b * p:(b + 1) * p, 0]
                if "forward" in e.name:
                    assert (ipiv[b] != np.arange(1, p + 1)).sum() == p // 2          # every row changes places
                    if "full" in e.name:      # the overflow poisons its own column, and that column alone
                        assert np.isnan(col[:-1]).all() and np.isinf(col[-1]) and np.isfinite(want[b * p:(b + 1) * p, 1:]).all()
                    if "half" not in e.name:  # (halved, the totals below the overflow threshold are exact in plain fp64 too)
                        assert not G.J_same(G.plain_getrs(LU[b], ipiv[b], X0[b * p:(b + 1) * p, 1]), want[b * p:(b + 1) * p, 1])
                elif "full" in e.name:
                    assert G.J_same(col[::-1], r.want)
    # the planted blocks: the ties the model counts
    for part in ("L", "U"):
        e = R.getrs_planted(p, part)
        X, st = R._getrs_solve(e, p)
        LU, ip, X0 = e.lu(p)
        assert (ip != np.arange(1, p + 1)).sum() >= p // 2
        xm, ties = G.getrs_model(LU, ip, X0[:, 0])
        assert G.J_same(xm, X[:, 0]) and st[0] >= ties >= 3, (part, st, ties)
        assert G.J_same(X[:, 0] if part == "L" else X[::-1, 0], e.case.want[:p])
        if p >= 32:                      # (the six planted rows of the 18-row part have short mantissas: plain fp64 gets them)
            assert not G.J_same(G.plain_getrs(LU, ip, X0[:, 0]), X[:, 0])
