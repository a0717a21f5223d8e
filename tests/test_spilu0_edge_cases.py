"""The ExSpILU0 edge cases hold what the GPU tests rely on (CPU only): every transplant carries exactly row_total(row) to
the entry it names, inside the product domain, at the lengths, slots and kc positions the kernel's branches need; the
planted variants keep their ties in long rows; the block-diagonal composition is the model of the whole; and the cases
can see a routine that breaks ties away from even, rounds every product or sums in plain fp64, class by class."""
import math

import numpy as np
import pytest

import exact_cases as E
import potrf_cases as P
import range_block_cases as R
import spilu0_cases as S
import spilu0_edge_cases as X
from helpers import assert_bits, bits

VARIANTS = X.variants()


def _same_double(a, b):
    return bits(np.array([a]))[0] == bits(np.array([b]))[0] or (math.isnan(a) and math.isnan(b))


# ---------------------------------------------------------------------------------------------
# 1. the transplants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,length,wide,reader", VARIANTS)
def test_every_transplant_carries_row_total_inside_the_product_domain(form, length, wide, reader):
    trsv = E.range_rows_trsv(0)
    cases = X.range_cases(form, length, wide, reader)
    assert len(cases) == 15 and sorted({c.cls for c in cases}) == [1, 2, 3, 4, 5] and X.LEFT_OUT == ()
    for c in cases:
        crow, col, val = c.csr
        lu, i0, i1, d = X.model(c)
        assert i0 == 0 and c.m == len(crow) - 1 <= 1100, c.name
        assert col[c.at] == c.target and crow[c.carrier] <= c.at < crow[c.carrier + 1], c.name
        assert c.rounded == P._round(c.total) and _same_double(float(lu[c.at]), c.want), (c.name, lu[c.at], c.want)
        if form == "L" and c.row in trsv.rows:          # the one division: what ExTRSV's own row expects
            assert _same_double(c.want, float(trsv.want[trsv.rows[c.row]])), c.name
        # a zero by cancellation in the pivot is reported, the Inf of the overflow tie is not
        assert i1 == (c.carrier + 1 if form == "D" and c.rounded == 0 else 0), (c.name, i1)
        assert all(R.in_domain(a, b) for a, b in X.products(c.csr, lu)), c.name
        assert len(X.products(c.csr, lu)) == d.terms
        # nothing multiplies the carrier's outputs: no later row stores one of its columns in its L part
        later = [r for r in range(c.carrier + 1, c.m) if any(c.carrier <= j < r for j in col[crow[r]:crow[r + 1]])]
        assert later == [], c.name
        assert c.length == crow[c.carrier + 1] - crow[c.carrier]
        if length:
            assert c.length == length and c.e == length - (2 if form == "L" else 1), c.name
        else:
            assert c.pad == 0


def test_the_lengths_reach_every_slot_class_and_the_seam():
    """the entry that carries the total: its position e in the carrier (lane e % 64, slot e / 64 in the several-entries
    form), and in form "L" the step kk = e at which its owner certifies it"""
    row = R.rows()[0]
    at = {form: {n: X.transplant(row, form, X.pad_for(row, form, n)).e for n in X.lengths(form)} for form in X.FORMS}
    for form in ("U", "D"):
        assert at[form] == {8: 7, 63: 62, 64: 63, 65: 64, 128: 127, 129: 128, 512: 511}
        assert sorted({e >> 6 for e in at[form].values()}) == [0, 1, 2, 7]
    assert at["L"] == {8: 6, 63: 61, 64: 62, 65: 63, 66: 64, 128: 126, 129: 127, 512: 510}     # kk
    assert sum(1 for kk in at["L"].values() if kk >= 64) == 4 and sorted({kk >> 6 for kk in at["L"].values()}) == [0, 1, 7]
    assert S.MAX_ROW in X.LENGTHS and {64, 65} <= set(X.LENGTHS)


def test_wide_sources_are_consumed_and_the_reader_hits_and_misses():
    for form in X.FORMS:
        seen, consumed = {}, set()
        for wide in X.WIDES:
            for c in X.range_cases(form, 0, wide):
                crow, col, _ = c.csr
                for k in c.ks:                      # the support rows the carrier reads
                    r = k                           # (pad = 0)
                    upper = col[crow[r] + 1:crow[r + 1]].tolist()
                    assert col[crow[r]] == r and len(upper) == c.nu[k] == wide + 1
                    assert upper.index(c.target) == c.kc_index[k] == wide
                    consumed.add(c.nu[k])
                seen[wide] = -(-(wide + 1) // 64)
        assert seen == {62: 1, 63: 1, 64: 2, 200: 4}                      # passes of the wave that stage kc
        assert consumed == {63, 64, 65, 201}, "no consumed row with nu >= 64"
        c = X.range_cases(form, 0, X.WIDES[-1], True)[-1]
        crow, col, _ = c.csr
        rd = c.m - 1
        mine = col[crow[rd]:crow[rd + 1]].tolist()
        assert mine[-1] == rd and mine[:X.NSUP] == list(range(X.NSUP))
        for k in range(X.NSUP):
            upper = col[crow[k] + 1:crow[k + 1]].tolist()
            assert len(upper) >= 64
            hit = [upper.index(j) for j in mine[k + 1:] if j in upper]
            miss = [j for j in mine[k + 1:] if j not in upper]
            assert min(hit) < 8 and max(hit) > 128 and len(hit) > 30, (k, hit)
            assert len(miss) >= X.NSUP - k and (k not in (0, 3) or len(miss) > 20), (k, miss)


def test_the_block_diagonal_composition_is_the_model_of_the_whole():
    picks = [X.range_cases("D", 0)[9], X.range_cases("U", 65)[11], X.range_cases("L", 0, 62)[5]]
    for c in picks:
        for reference in (False, True):
            whole = X.behind(S.tridiagonal(X.LEAD), c.csr)
            want, i0, i1, d = X.behind_model(c, reference)
            if reference:
                lu, j0, j1 = S.ilu0_exact(*whole, rounder=X.reference_round)
            else:
                lu, j0, j1, dd = S.ilu0_exact(*whole, detail=True)
                assert (dd.terms, dd.ties, dd.nears) == (d.terms, d.ties, d.nears)
            assert (i0, i1) == (j0, j1), c.name
            assert_bits(lu, want, c.name)
    assert picks[0].cls == 4 and X.behind_model(picks[0])[2] == X.LEAD + picks[0].carrier + 1


def test_a_later_row_meets_the_inf_of_the_overflow_tie_with_a_zero_multiplier():
    c = X.inf_meets_zero()
    crow, col, val = c.csr
    lu, i0, i1, d = X.model(c)
    assert i0 == 0 and lu[c.at] == math.inf
    last = c.m - 1
    assert col[crow[last]:crow[last + 1]].tolist() == [c.s, c.s + 1, last]
    assert lu[crow[last]] == 0.0 and math.isnan(lu[crow[last] + 1]) and lu[crow[last] + 2] == 1.0


# ---------------------------------------------------------------------------------------------
# 2. planted ties in long rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", X.PLANTED_LENGTHS)
def test_planted_variants_keep_their_classes_in_rows_of_every_length(length):
    pad = X.planted_pad(length)
    crow, col, val = X.planted(pad)
    m = len(crow) - 1
    assert m <= 1100 and S.structure(crow, col, m) == 0
    lu, i0, i1, d = X.planted_model(pad)
    base = S.expected("planted")[3]
    assert (i0, i1) == (0, 0) and np.isfinite(lu).all()
    assert min(d.ties_l, d.ties_u, d.nears_l, d.nears_u) >= 16, vars(d)
    assert (d.ties_l, d.ties_u, d.nears_l, d.nears_u, d.terms) == (base.ties_l, base.ties_u, base.nears_l, base.nears_u, base.terms)
    lens = np.diff(crow)
    first = pad + S.PLANTED_SRC + S.PLANTED_MID
    assert lens[first:].tolist() == [length] * (S.PLANTED_ROWS - 3) + [length - 1, length - 2, length - 3]
    assert lens.max() == max(length, 23) and (lens[:pad] == 1).all()          # (a source row has 23 entries)
    # where the planted entries lie in their rows: from position pad + 4 on
    rows = np.repeat(np.arange(m), lens)
    e = np.arange(len(col)) - crow[rows]
    hot = d.kind != S.CLEAR
    assert hot.sum() == d.ties + d.nears and (rows[hot] >= first).all() and e[hot].min() == pad + 4
    if length > 64:
        assert (e[hot] >> 6).min() >= (pad + 4) >> 6 and (e[hot] >> 6).max() == (length - 1) >> 6
        low = hot & (col < rows)
        if length == 65:                    # the seam: the planted U entries lie on both sides of it, the last in slot 1
            assert (e[low] < 64).all() and (e[hot & ~low] == 63).any() and (e[hot & ~low] == 64).any()
        else:
            assert low.any() and (e[low] >= 64).all(), "no planted L entry is owned by a slot >= 1"
    # the pads: exact quotients, and no product under them (an idle row has no U part)
    cold = (rows >= first) & (col < pad)
    assert (d.kind[cold] == S.CLEAR).all() and (lu[cold] * np.array([X._pow2(int(j)) for j in col[cold]]) == val[cold]).all()
    # the untouched part is the planted matrix itself
    keep = (rows >= pad) & (col >= pad)
    assert_bits(lu[keep], S.expected("planted")[0], length)
    # the reference rounding is seen
    ref = X.planted_model(pad, True)[0]
    assert int((bits(ref) != bits(lu)).sum()) == 30


# ---------------------------------------------------------------------------------------------
# 3. sensitivity
# ---------------------------------------------------------------------------------------------
def _wrong(name, csr, want, at=None):
    if name == "away":
        return S.ilu0_exact(*csr, rounder=S.round_away)[0]
    if name == "plain":
        return S.plain_ilu0(*csr)
    try:
        return S.ilu0_exact(*csr, round_products=True)[0]
    except OverflowError:             # a partial sum rounded to Inf (the model keeps Fractions): the total is not finite
        got = want.copy()
        got[at] = math.inf
        return got


# the (class, wrong routine) pairs that change no bit, by name, with the reason
BLIND = {
    (1, "away"): "the one tie of the class lies at the overflow threshold: both roundings give Inf",
    (2, "each"): "one product per row: there is no partial sum to round",
    (2, "plain"): "one product per row, itself a double: b - a x in fp64 is the one rounding",
    (4, "away"): "the total is zero: no tie",
    (4, "plain"): "v w and w v round alike and every partial sum of the row is exact in fp64: plain arithmetic cancels too",
    (5, "away"): "the cancellation leaves the error term of v w, far from a tie",
}


def test_every_class_sees_each_wrong_routine_or_names_why_not():
    seen = {}
    for form in X.FORMS:
        for c in X.range_cases(form):
            want = X.model(c)[0]
            for wrong in ("away", "each", "plain"):
                got = _wrong(wrong, c.csr, want, c.at)
                diff = bool(((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).any())
                seen[c.cls, wrong] = seen.get((c.cls, wrong), False) or diff
    assert len(seen) == 15
    assert {k for k, v in seen.items() if not v} == set(BLIND), seen
    for cls in (1, 2, 3, 4, 5):                # no class is blind to everything
        assert any(seen[cls, w] for w in ("away", "each", "plain")), cls


@pytest.mark.parametrize("length", X.PLANTED_LENGTHS)
def test_every_planted_variant_sees_each_wrong_routine(length):
    csr = X.planted(X.planted_pad(length))
    want = X.planted_model(X.planted_pad(length))[0]
    for wrong in ("away", "each", "plain"):
        assert (bits(_wrong(wrong, csr, want)) != bits(want)).any(), (length, wrong)


# ---------------------------------------------------------------------------------------------
# 4. small structures, the reserved NaN, the value sets of the replays
# ---------------------------------------------------------------------------------------------
def test_small_structures():
    lu, i0, i1, d = S.ilu0_exact(*X.one_row(), detail=True)
    assert (i0, i1, d.terms) == (0, 0, 0) and lu.tolist() == [3.0]
    crow, col, val = X.diagonal()
    lu, i0, i1, d = S.ilu0_exact(crow, col, val, detail=True)
    assert len(crow) == 301 and (i0, i1, d.terms) == (0, 0, 0)
    assert_bits(lu, val, "diagonal")
    csr = X.negative_zero()
    lu, i0, i1 = S.ilu0_exact(*csr)
    plain = S.plain_ilu0(*csr)
    assert (i0, i1) == (0, 0) and (lu == plain).all()
    zero = np.nonzero(csr[2] == 0)[0]
    assert zero.tolist() == [1, 3, 6] and np.signbit(csr[2][zero]).all()
    assert np.signbit(lu[zero]).tolist() == [False, False, True]          # +0, +0 / 2, +0 / -3
    assert np.signbit(plain[zero]).tolist() == [True, True, False]        # -0, -0 / 2, -0 / -3
    assert (np.nonzero(bits(lu) != bits(plain))[0] == zero).all()
    crow, col, val = X.empty_row()
    assert crow[6] == crow[7] and S.ilu0_exact(crow, col, val)[1:] == (7, 0)
    assert "empty" not in " ".join(S.defects())


@pytest.mark.parametrize("where,first", [("pivot", 1), ("upper", 2)])
def test_the_all_ones_nan_poisons_everything_behind_it(where, first):
    crow, col, val = X.empty_pattern_nan(where)
    assert int(val.view(np.uint64)[0 if where == "pivot" else 1]) == X.ALL_ONES and np.isnan(val).sum() == 1
    lu, i0, i1 = S.ilu0_exact(crow, col, val)
    assert (i0, i1) == (0, first)
    # u_{i,i+1} = a_{i,i+1} has no product under it; "upper": u_00 and l_10 = a_10 / u_00 come before the NaN
    clean = {"pivot": [1, 4, 7], "upper": [0, 2, 4, 7]}[where]
    assert np.nonzero(~np.isnan(lu))[0].tolist() == clean
    assert np.isnan(S.plain_ilu0(crow, col, val)).tolist() == np.isnan(lu).tolist()


def test_value_sets_on_the_zero_pivot_pattern():
    crow, col, _ = S.zero_pivot()
    sets = X.zero_pivot_sets()
    assert [n for n, _ in sets][:3] == ["healthy", "zero pivot", "healthy again"]
    infos = [S.ilu0_exact(crow, col, v)[1:] for _, v in sets]
    assert infos[:3] == [(0, 0), (0, 5), (0, 0)]
    pivot = int(crow[4]) + 1
    for (name, v), info in zip(sets[3:], infos[3:]):
        row = next(r for r in R.rows() if r[0] == name)
        lu = S.ilu0_exact(crow, col, v)[0]
        assert _same_double(float(lu[pivot]), P._round(R.row_total(row))) and R.settles(R.row_total(row)), name
        assert info[0] == 0
    assert S.ilu0_exact(crow, col, sets[3][1])[0][pivot] == math.inf


def test_reference_rounding_agrees_on_the_range_totals():
    """all 15 totals fit the oracle's canonical limbs, and the reference rounding gives what nearest-even gives"""
    for row in R.rows():
        t = R.row_total(row)
        assert _same_double(X.reference_round(t), P._round(t)), row[0]
