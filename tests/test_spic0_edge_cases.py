"""The ExSpIC0 edge cases hold what the GPU tests rely on (CPU only): every transplant carries exactly row_total(row) to
the entry it names and divides it by |dia|, at the lengths, slots and kc positions the kernel's branches need, whatever
the pad, the wide rows and the reader; the padded dense and planted variants keep their totals and classes in long rows;
the block-diagonal composition is the model of the whole; and each section can see a routine that breaks ties away from
even, rounds every product, flushes subnormals, takes a sloppy root or sums in plain fp64."""
import math

import numpy as np
import pytest

import exact_cases as E
import potrf_cases as P
import range_block_cases as R
import spic0_cases as C
import spic0_edge_cases as X
from helpers import assert_bits, bits

VARIANTS = X.variants()
WRONG = ("each", "away", "flush")


def _same_double(a, b):
    return bits(np.array([a]))[0] == bits(np.array([b]))[0] or (math.isnan(a) and math.isnan(b))


def _rows_of(csr):
    crow, col, _ = csr
    return [col[crow[r]:crow[r + 1]].tolist() for r in range(len(crow) - 1)]


def _differs(got, want):
    return bool(((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any())


def _wrong(name, csr, want):
    if name == "away":
        return C.ic0_exact(*csr, rounder=C.round_away)[0]
    if name == "flush":
        return C.ic0_exact(*csr, rounder=X.flush_round)[0]
    try:
        return C.ic0_exact(*csr, round_products=True)[0]
    except OverflowError:             # a partial sum rounded to Inf (the model keeps Fractions): the total is not finite
        return np.full(len(want), math.inf)


# ---------------------------------------------------------------------------------------------
# 1. the transplants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,wide,reader", VARIANTS)
def test_every_transplant_carries_row_total_and_divides_it_by_the_root(length, wide, reader):
    trsv = E.range_rows_trsv(0)
    cases = X.range_cases(length, wide, reader)
    plain = X.range_cases()
    assert len(cases) == 15 and not X.LEFT_OUT and sorted({c.cls for c in cases}) == [1, 2, 3, 4, 5]
    for c, base in zip(cases, plain):
        crow, col, val = c.csr
        ll, i0, i1, d = X.model(c)
        rows = _rows_of(c.csr)
        assert i0 == 0 and c.m == len(crow) - 1 == c.carrier + 1 <= 1100, c.name      # the carrier is the last row
        assert max(len(r) for r in rows) <= C.MAX_ROW
        assert col[c.at] == c.target and crow[c.carrier] <= c.at < crow[c.carrier + 1], c.name
        # the root of the target is |dia| exactly, so the fixed entry is fl(Round(T) / |dia|): ExTRSV's quotient
        diag = {r: int(crow[r]) + rows[r].index(r) for r in range(c.m)}
        assert ll[diag[c.s]] == c.dia, (c.name, ll[diag[c.s]], c.dia)
        assert c.rounded == P._round(c.total) and _same_double(float(ll[c.at]), c.want), (c.name, ll[c.at], c.want)
        if c.row in trsv.rows:
            assert _same_double(c.want, c.sign * float(trsv.want[trsv.rows[c.row]])), c.name
        # the total is the same whatever the pad, the wide rows and the reader
        assert _same_double(float(ll[c.at]), float(X.model(base)[0][base.at])), c.name
        # where a square of the carrier overflows its radicand is -Inf: the diagonal is NaN and info[1] names the carrier
        assert i1 == (c.carrier + 1 if c.cls in (1, 2) else 0), (c.name, i1)
        assert math.isnan(ll[diag[c.carrier]]) == (c.cls in (1, 2)) and (c.cls in (1, 2) or ll[diag[c.carrier]] > 0), c.name
        # the slot: the range entry is the last of the carrier's L part
        mine = [j for j in rows[c.carrier] if j <= c.carrier]
        assert c.length == len(mine) and c.e == len(mine) - 2 and mine[c.e] == c.s, c.name
        if length:
            assert c.length == length and c.pad == length - len(c.ks) - 2 and c.m == length + X.NSUP - len(c.ks), c.name
            assert c.pad > 0 or length == 8
            # what the settled total strides: misses (the idle columns, which the target does not store) and hits
            target = set(rows[c.s])
            hit = [k for k in mine[:c.e] if k in target]
            miss = [k for k in mine[:c.e] if k not in target]
            assert hit == [c.pad + k for k in c.ks] and miss == list(range(c.pad)), c.name
        # no product but the a_k x_k reaches a total off the diagonal: two rows that store each other store no common
        # column in front, except target and carrier
        low = [set(j for j in rows[r] if j < r) for r in range(c.m)]
        for r in range(c.m):
            for j in low[r]:
                common = {k for k in low[r] & low[j] if k < j}
                assert (not common) or (r, j) == (c.carrier, c.s), (c.name, r, j)
        assert low[c.carrier] & low[c.s] == {c.pad + k for k in c.ks}
        assert d.terms == d.owned - c.m + len(c.ks)      # one square per L entry, and the a_k x_k
        # the wide rows: perfect squares, small integers; the support rows the carrier reads are wide
        w0 = c.pad + X.NSUP
        for t in range(wide):
            r = w0 + t
            assert ll[diag[r]] == 2 + t % 5 and rows[r][-1] == r, (c.name, t)
            assert (ll[crow[r]:diag[r]] == val[crow[r]:diag[r]]).all() and len(rows[r]) == X.NSUP + 1 - (1 if reader and t % 6 < X.NSUP else 0)
        for k in c.ks:
            upper = [j for j in rows[c.pad + k] if j > c.pad + k]
            assert upper[-2:] == [c.s, c.carrier], (c.name, k)
            left_out = len([t for t in range(wide) if t % 6 == k]) if reader else 0
            assert len(upper) == wide - left_out + 2 and upper.index(c.s) == wide - left_out
            assert (not reader) or left_out >= 33


def test_the_lengths_reach_every_slot_class_the_seam_and_the_limit():
    """the step kk = e at which the owner of the range entry certifies it (lane e % 64, slot e / 64 in the several-entries
    form), and the diagonal behind it"""
    row = R.rows()[0]
    at = {n: X.transplant(row, X.pad_for(row, n)).e for n in X.LENGTHS}
    assert at == {8: 6, 63: 61, 64: 62, 65: 63, 66: 64, 128: 126, 129: 127, 512: 510}
    assert sorted({kk >> 6 for kk in at.values()}) == [0, 1, 7] and 64 in at.values()
    assert sorted({n - 1 >> 6 for n in X.LENGTHS}) == [0, 1, 2, 7]          # the slot of the diagonal
    assert C.MAX_ROW in X.LENGTHS and {64, 65} <= set(X.LENGTHS)


def test_wide_sources_are_staged_in_one_to_four_passes():
    seen = {}
    for wide in X.WIDES:
        c = X.range_cases(0, wide)[14]                       # the wide-range cancellation reads all six support rows
        assert c.ks == tuple(range(X.NSUP))
        rows = _rows_of(c.csr)
        seen[wide] = {-(-len([j for j in rows[k] if j > k]) // 64) for k in range(X.NSUP)}
    assert seen == {62: {1}, 63: {2}, 64: {2}, 200: {4}}      # nu = wide + 2: 64, 65, 66 and 202 columns in kc
    c = X.range_cases(0, X.WIDES[-1], True)[14]
    rows = _rows_of(c.csr)
    assert len({len(rows[k]) for k in range(X.NSUP)}) > 1 and min(len(rows[k]) for k in range(X.NSUP)) > 128


def test_the_block_diagonal_composition_is_the_model_of_the_whole():
    picks = [X.range_cases(0)[9], X.range_cases(65)[11], X.range_cases(0, 62)[5], X.range_cases(66)[14]]
    for c in picks:
        for reference in (False, True):
            whole = X.behind(C.tridiagonal(X.LEAD), c.csr)
            got = X.behind_model(c, reference)
            if got is None:
                assert reference and c.cls == 3
                continue
            want, i0, i1, d = got
            if reference:
                ll, j0, j1 = C.ic0_exact(*whole, rounder=X.reference_round)
            else:
                ll, j0, j1, dd = C.ic0_exact(*whole, detail=True)
                assert (dd.terms, dd.ties, dd.nears, dd.owned, dd.wide) == (d.terms, d.ties, d.nears, d.owned, d.wide)
            assert (i0, i1) == (j0, j1), c.name
            assert_bits(ll, want, c.name)
    assert picks[1].cls == 1 and X.behind_model(picks[1])[2] == X.LEAD + picks[1].carrier + 1


def test_the_settled_totals_are_named():
    """settle: the model's ties (every entry outside the certificate's range is one) and the range entry where settles()
    holds: 12 of the 15 rows; the two zeros by cancellation and the wide-range cancellation may stay in registers"""
    cases = X.range_cases(65)
    named = [c.row for c in cases if R.settles(c.total)]
    assert len(named) == 11 and all(c.cls in (4, 5) or "above" in c.row for c in cases if c.row not in named)
    for c in cases:
        d = X.model(c)[3]
        assert d.settle >= (1 if c.row in named else 0) and d.settle == d.ties + (c.row in named and d.kind[c.at] != C.TIE)


# ---------------------------------------------------------------------------------------------
# 2. radicands and roots
# ---------------------------------------------------------------------------------------------
def test_root_values_are_held_to_the_correctly_rounded_root():
    crow, col, val = X.root_diagonal()
    v = P.root_values()
    assert len(v) == 512 == len(val) and (np.diff(crow) == 1).all() and (val > 0).all()
    ll, i0, i1, d = C.ic0_exact(crow, col, val, detail=True)
    assert (i0, i1, d.terms, d.owned, d.wide) == (0, 0, 0, 512, 0)
    assert_bits(ll, np.array([math.sqrt(x) for x in v]), "roots")
    assert {5e-324, float(np.finfo(np.float64).max), 2.0 ** -1022, float(np.nextafter(2.0 ** -1022, 0.0))} <= set(v.tolist())
    k = np.sqrt(v[120:160])
    assert (k * k == v[120:160]).all() and (k == np.floor(k)).all()
    for x in v[:120].tolist():                           # a neighbour of a perfect square, not a square itself
        near = [float(np.nextafter(x, math.inf)), float(np.nextafter(x, 0.0))]
        assert any(n == int(n) and math.isqrt(int(n)) ** 2 == int(n) for n in near), x
        assert not (x == int(x) and math.isqrt(int(x)) ** 2 == int(x)), x
    # a root from an fp32 estimate and one Newton step is seen
    sloppy = np.array([X.sloppy_root(x) for x in v])
    assert int((bits(sloppy) != bits(ll)).sum()) >= 16


@pytest.mark.parametrize("name", X.DENSE_NAMES)
def test_dense_range_cases_keep_their_factor_behind_idle_rows(name):
    Gm = X.dense_matrix(name)
    q = Gm.shape[0]
    Rm, pinfo = P.potrf_exact(Gm, "L")
    assert (pinfo > 0) == (name in X.DENSE_STOPPED)
    first = None
    for pad in X.DENSE_PADS:
        c = X.dense_case(name, pad)
        crow, col, val = c.csr
        ll, i0, i1, d = X.dense_model(name, pad)
        lens = np.diff(crow)
        assert i0 == 0 and lens[pad:].tolist() == [pad + q] * q and lens.max() <= C.MAX_ROW
        assert (val[col < pad] == 0).sum() == pad * q and (val == 0).sum() >= 2 * pad * q
        L = np.tril(C.dense_of(crow, col, ll)[pad:, pad:])
        if name in X.DENSE_STOPPED:
            assert i1 == pad + pinfo and math.isnan(L[pinfo - 1, pinfo - 1])       # ExSpIC0 goes on: sqrt(-Inf)
        else:
            assert i1 == 0
            assert_bits(L, np.tril(Rm), c.name)
        first = L if first is None else first
        assert_bits(L, first, c.name)
        assert (C.dense_of(crow, col, ll)[pad:, :pad] == 0).all()
    assert pad + q >= 510 and [X.DENSE_PADS[1] + q <= 64 < X.DENSE_PADS[2] + q]


@pytest.mark.parametrize("what", ["zero", "neg"])
@pytest.mark.parametrize("owned", [65, C.MAX_ROW])
def test_breakdowns_at_the_end_of_long_rows(what, owned):
    c = X.long_breakdown(what, owned)
    crow, col, val = c.csr
    ll, i0, i1, d = C.ic0_exact(crow, col, val, detail=True)
    r = c.row
    assert i0 == 0 and i1 == r + 1 and d.wide == 1 and np.diff(crow).max() <= C.MAX_ROW
    assert (col[crow[r]:crow[r + 1]] <= r).sum() == owned
    rad = ll[crow[r] + owned - 1]
    assert (rad == 0 and not np.signbit(rad)) if what == "zero" else math.isnan(rad)
    if owned < C.MAX_ROW:                                # the row behind it divides by the broken pivot
        assert len(crow) - 1 == r + 2 and not math.isfinite(ll[crow[r + 1]])


# ---------------------------------------------------------------------------------------------
# 3. planted ties in long rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", list(X.PLANTED_ALL))
def test_planted_variants_keep_their_classes_in_long_rows(length):
    ties = nears = 0
    for spec in X.PLANTED_ALL[length]:
        p, pad, seed = spec
        crow, col, val = X.planted(*spec)
        m = len(crow) - 1
        assert m <= 1100 and C.structure(crow, col, m) == 0
        ll, i0, i1, d = X.planted_model(spec)
        bcrow, bcol, bval = X.planted_base(p, seed)
        bll, b0, b1, bd = X.planted_base_model(p, seed)
        assert (i0, i1, b0, b1) == (0, 0, 0, 0) and np.isfinite(ll).all()
        rows = np.repeat(np.arange(m), np.diff(crow))
        keep = (rows >= pad) & (col >= pad) & (rows < pad + p)
        # the planted part is untouched: the same entries, the same classes
        assert_bits(ll[keep], bll, spec)
        assert (d.kind[keep] == bd.kind).all() and (col[keep] - pad == bcol).all()
        cold = (rows >= pad) & (col < pad)
        assert (ll[cold] == 0).all() and (d.kind[cold] == C.CLEAR).all() and cold.sum() == pad * (X.planted_rows(p) + 2)
        # the block behind: the subnormal radicand of potrf_cases.range_cases()
        Rm, pinfo = P.potrf_exact(X.dense_matrix(X.TAIL), "L")
        assert pinfo == 0 and ll[-1] == Rm[1, 1] and 0 < ll[-1] ** 2 < 2.0 ** -1020
        # where the planted entries lie: position pad + 4 of the owned part, in rows that own up to pad + block entries
        hot = (d.kind != C.CLEAR) & (rows < pad + p) & (col <= rows)
        e = (np.arange(len(col)) - crow[rows])[hot]
        first_block = 4 + P.BLOCKS[p][0]
        plants = np.zeros(len(col), dtype=bool)
        for r, c, *_ in C.planted(p)[1].plants:
            plants |= (rows == pad + c) & (col == pad + r)        # (upper orientation there: the entry (c, r) of L)
        assert plants.sum() == len(C.planted(p)[1].plants) and (e[plants[hot]] == pad + 4 + 0).sum() >= P.BLOCKS[p][0]
        lens = np.diff(crow)
        assert (lens[pad:pad + first_block] == pad + first_block).all()
        if length in X.PLANTED:
            assert pad + first_block == length or (length == C.MAX_ROW and lens.max() == C.MAX_ROW)
            ties += int((d.kind[keep] == C.TIE).sum())
            nears += int((d.kind[keep] == C.NEAR).sum())
        else:
            assert (pad + 4) >> 6 == {192: 2, 256: 3, 320: 4, 384: 5}[length]
        assert (d.ties, d.nears) == (bd.ties + 1, bd.nears)          # (the subnormal radicand lies outside the range)
    if length in X.PLANTED:
        assert ties >= 16 and nears >= 16, (length, ties, nears)
    slots = {(X.PLANTED_ALL[n][0][1] + 4) >> 6 for n in X.PLANTED_ALL}
    assert slots == {0, 1, 2, 3, 4, 5, 6}
    big = X.planted(*X.PLANTED[C.MAX_ROW][0])
    assert np.diff(big[0]).max() == C.MAX_ROW                        # slot 7: the rows at the limit own 449 .. 512 entries


# ---------------------------------------------------------------------------------------------
# 4. sensitivity: every section sees each wrong routine
# ---------------------------------------------------------------------------------------------
def test_the_range_cases_see_each_wrong_routine_and_the_plain_form():
    seen = {w: [] for w in WRONG + ("plain",)}
    for c in X.range_cases():
        want = X.model(c)[0]
        for w in WRONG:
            if _differs(_wrong(w, c.csr, want), want):
                seen[w].append(c.cls)
        if _differs(C.plain_ic0(*c.csr), want):
            seen["plain"].append(c.cls)
    assert all(seen[w] for w in seen), seen
    assert 2 in seen["away"] and 3 in seen["flush"] and 5 in seen["each"] and {4, 5} & set(seen["plain"]), seen


def test_the_dense_cases_see_each_wrong_routine():
    seen = {w: [] for w in WRONG}
    for name in X.DENSE_NAMES:
        for pad in X.DENSE_PADS[:2]:
            c = X.dense_case(name, pad)
            want = X.dense_model(name, pad)[0]
            for w in WRONG:
                if _differs(_wrong(w, c.csr, want), want):
                    seen[w].append(c.name)
    assert all(len(seen[w]) >= 2 for w in WRONG), seen


@pytest.mark.parametrize("length", [12, 192])
def test_the_planted_variants_see_each_wrong_routine(length):
    spec = X.PLANTED_ALL[length][0]
    want = X.planted_model(spec)[0]
    for w in WRONG:
        assert _differs(_wrong(w, X.planted(*spec), want), want), (length, w)
    assert _differs(C.plain_ic0(*X.planted(*spec)), want)


def test_reference_rounding_is_seen_on_the_range_and_the_planted_cases():
    moved, held = 0, set()
    for length in (0, 65):
        for c in X.range_cases(length):
            ref = X.model(c, True)
            if ref is not None:
                held.add(c.cls)
                moved += int(_differs(ref[0], X.model(c)[0]))
    assert {4, 5} <= held and 3 not in held and moved >= 2, (held, moved)
    for length in (12, 65):                              # (the GPU tests assert it for every length they run)
        for spec in X.PLANTED[length]:
            ref = X.planted_model(spec, True)
            assert ref is not None and ref[1:3] == (0, 0)
            assert int((bits(ref[0]) != bits(X.planted_model(spec)[0])).sum()) >= 30, spec


# ---------------------------------------------------------------------------------------------
# 5. small structures, the value sets of the replays
# ---------------------------------------------------------------------------------------------
def test_small_structures():
    ll, i0, i1, d = C.ic0_exact(*X.one_row(), detail=True)
    assert (i0, i1, d.terms) == (0, 0, 0) and ll.tolist() == [math.sqrt(3.0)]
    crow, col, val = X.diagonal()
    ll, i0, i1, d = C.ic0_exact(crow, col, val, detail=True)
    assert len(crow) == 301 and (i0, i1, d.terms, d.owned) == (0, 0, 0, 300)
    assert_bits(ll, np.array([math.sqrt(x) for x in val]), "diagonal")
    csr = X.negative_zero()
    ll, i0, i1 = C.ic0_exact(*csr)
    plain = C.plain_ic0(*csr)
    assert (i0, i1) == (0, X.SMALL_INFO["negative zero"]) == (0, 3) and (ll == plain).all()
    zero = np.nonzero(csr[2] == 0)[0]
    assert zero.tolist() == [1, 2, 4] and np.signbit(csr[2][zero]).all()
    assert not np.signbit(ll[zero]).any() and np.signbit(plain[zero]).all()
    assert (np.nonzero(bits(ll) != bits(plain))[0] == zero).all()


def test_value_sets_on_the_replay_pattern():
    crow, col = X.replay_pattern()
    m = len(crow) - 1
    assert m == 8 and C.structure(crow, col, m) == 0
    sets = X.replay_sets()
    assert [n for n, _ in sets] == ["healthy", "zero radicand", "healthy again", "tie at the overflow threshold",
                                    "subnormal total, quotient a tie"]
    got = [C.ic0_exact(crow, col, v) for _, v in sets]
    assert [g[1:] for g in got] == [(0, 0), (0, 2), (0, 0), (0, 3), (0, 0)]
    assert np.isfinite(got[0][0]).all() and np.isfinite(got[2][0]).all() and _differs(got[0][0], got[2][0])
    at = int(crow[2]) + 1                                  # (2, 1): the carrier's entry in the target's column
    for (name, v), g in zip(sets[3:], got[3:]):
        row = next(r for r in R.rows() if r[0] == name)
        assert R.settles(R.row_total(row))
        assert _same_double(float(g[0][at]), float(np.float64(P._round(R.row_total(row))) / np.float64(abs(row[3])))), name
    assert got[3][0][at] == math.inf and got[4][0][at] == 2 * 5e-324 and np.isfinite(got[4][0]).all()
    # every set is symmetric
    for _, v in sets:
        D = C.dense_of(crow, col, v)
        assert (bits(D) == bits(D.T)).all()
