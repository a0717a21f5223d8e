"""Edge cases for ExSpILU0: totals at the ends of the double range and planted ties in every row class of the kernel, wide
source rows, the small structures and the mailbox's reserved NaN.  Nothing here calls the code under test: every
expectation comes from spilu0_cases.ilu0_exact, plain_ilu0 and apply_exact.

`transplant(row, form, pad, wide)` carries one row of range_block_cases.rows() (T = b - sum_k a_k x_k over the support values
x = 2^511, 2^-537, v, w, 1, 2^-600) into a CSR matrix, by the trick of range_block_cases.transplant:

    rows 0 .. pad - 1          IDLE: a power of two on the diagonal and nothing else
    rows pad + k, k = 0 .. 5   SUPPORT: d_k = _delta(a_k) on the diagonal (1 where the row has no a_k), `wide` small
                               integers in the idle columns behind it, d_k x_k (exact) in the TARGET column
    `wide` rows                the rows of those idle columns: a power of two on the diagonal and nothing else
    the CARRIER                a small integer in every idle row's column in front (l = integer / power of two, exact, and
                               an idle row has no U part: no product), a_k in column pad + k (l_k = a_k / d_k exact), so
                               that its total in the target column is b - sum_k a_k x_k = row_total(row), exactly

form "U": the carrier is row s, the target column s + 1: the total is u_{s,s+1} under the diagonal `dia`; row s + 1 holds 1.
form "D": the target column is s itself: the total is the pivot u_ss.  A zero by cancellation is reported (info[1] = s + 1),
          the Inf of the overflow tie is not.
form "L": row s holds the row's own diagonal `dia` (3, 5, ...: no powers of two) and nothing else, the carrier is row s + 1
          and the target column s: the total is c_{s+1,s}, and l = fl(c / dia) is the one IEEE division, on subnormal and
          huge numerators (what ExTRSV's row gives: asserted against range_rows_trsv's own expectation).
Nothing multiplies the carrier's outputs afterwards, but for `inf_meets_zero()`.  The carrier has pad + (the number of the
row's a_k) + 2 entries (+ 1 in form "D") and the range entry is its last ("U", "D") or its last but one ("L": position
kk = length - 2, its diagonal behind it); `pad_for` gives the pad for a length, so with the lengths of LENGTHS the entry
lies in every slot class of the several-entries form.

With wide > 0 a support row has nu = wide + 1 entries right of its diagonal and the carrier finds the target as the last
of them (index `wide` from 0: the 63rd, 64th, 65th and 201st column of kc for WIDES), kc being staged in 1, 1, 2 and 4
passes of the wave.  `reader=True` adds a last row that stores every support column and every third idle column, while
support row k leaves out the idle columns t with t % 6 == k: the binary search hits and misses all over a wide kc.

`planted(pad)` is spilu0_cases.planted() behind `pad` idle rows, every planted row storing a small integer in each of their
columns: an idle row has no U part, so still no other product reaches a planted total, the ties and near-ties are the
same and the planted entries move to position pad + 4 and beyond of rows of pad + 12 entries (the last three planted rows
lose one entry each at the edge of the matrix: pad + 11, pad + 10, pad + 9)."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import potrf_cases as P
import range_block_cases as R
import spilu0_cases as S

NSUP = R.NSUP
FORMS = ("U", "D", "L")
LENGTHS = (8, 63, 64, 65, 128, 129, S.MAX_ROW)      # of the carrier: below, at and past the seam, two slots, the limit
EXTRA_L = (66,)                                     # form "L" only: the range entry itself at kk = 64, the first of slot 1
WIDES = (62, 63, 64, 200)
PLANTED_LENGTHS = (12, 64, 65, 130, S.MAX_ROW)      # of a planted row
ALL_ONES = 0xffffffffffffffff                       # ST_EMPTY: the NaN the mailbox reserves for "not posted"
# rows of range_block_cases.rows() that cannot be carried: none
LEFT_OUT = ()


def lengths(form):
    return LENGTHS + (EXTRA_L if form == "L" else ())


def pad_for(row, form, length):
    """the idle rows in front that give the carrier of `row` that many entries (its a_k, the total, its diagonal)"""
    pad = length - (len(row[4]) + (1 if form == "D" else 2))
    assert pad >= 0
    return pad


def _pow2(i):
    return 2.0 ** (i % 5 - 2)


def _small(i):
    return float((1 + i % 7) * (1 if i % 2 else -1))


def transplant(row, form, pad=0, wide=0, reader=False):
    """the case that carries `row` in `form` (module docstring)"""
    name, cls, b, dia, ent = row
    sup = R.support()
    i0 = pad + NSUP                      # the first idle column behind the support rows
    s = i0 + wide                        # the row whose entry is the total ("U", "D"), or whose diagonal divides it ("L")
    carrier = s + 1 if form == "L" else s
    target = s + 1 if form == "U" else s
    m = s + (1 if form == "D" else 2)
    rows = [dict() for _ in range(m)]
    for i in range(pad):
        rows[i][i] = _pow2(i)
        rows[carrier][i] = _small(i)
    nu = []
    for k in range(NSUP):
        a = ent.get(k)
        d = R._delta(a) if a is not None else 1.0
        u = d * sup[k]
        assert math.isfinite(u) and Fraction(u) == R.F(d) * R.F(sup[k]), (name, k)
        r = rows[pad + k]
        r[pad + k] = d
        for t in range(wide):
            if not (reader and t % 6 == k):
                r[i0 + t] = _small(3 * t + k)
        r[target] = u
        nu.append(len(r) - 1)
        if a is not None:
            assert Fraction(a / d) * R.F(d) == R.F(a), (name, k)
            rows[carrier][pad + k] = a
    for t in range(wide):
        rows[i0 + t][i0 + t] = _pow2(t)
    if form == "U":
        rows[s][s], rows[s][s + 1], rows[s + 1][s + 1] = dia, b, 1.0
    elif form == "D":
        rows[s][s] = b
    else:
        rows[s][s], rows[s + 1][s], rows[s + 1][s + 1] = dia, b, 1.0
    if reader:
        rd = {m: 64.0}
        for k in range(NSUP):
            rd[pad + k] = float(k - 3 if k != 3 else 2) * rows[pad + k][pad + k]
        for t in range(0, wide, 3):
            rd[i0 + t] = _small(t + 1)
        rows.append(rd)
    csr = S.from_rows(rows)
    crow, col, _ = csr
    e = sorted(rows[carrier]).index(target)
    t = R.row_total(row)
    c = P._round(t)
    with np.errstate(all="ignore"):
        want = float(np.float64(c) / np.float64(dia)) if form == "L" else c
    tag = f"{name} [{form}, pad {pad}, wide {wide}{', reader' if reader else ''}]"
    return SimpleNamespace(name=tag, row=name, cls=cls, form=form, pad=pad, wide=wide, reader=reader, csr=csr, s=s,
                           carrier=carrier, target=target, at=int(crow[carrier]) + e, e=e, length=len(rows[carrier]),
                           total=t, rounded=c, want=want, nu=tuple(nu), kc_index=tuple(n - 1 for n in nu),
                           ks=tuple(sorted(ent)), m=len(rows))


def inf_meets_zero():
    """the overflow tie in form "U", and one row more: row s + 2 stores a ZERO in column s (l = 0 / dia = 0) and column
    s + 1, so that its total there meets 0 * Inf = NaN: the model decides (ilu0_exact: a non-finite operand decides the
    totals it meets in IEEE arithmetic)"""
    row = next(r for r in R.rows() if r[0] == "tie at the overflow threshold")
    c = transplant(row, "U")
    crow, col, val = c.csr
    m = len(crow) - 1
    rows = [{int(col[p]): float(val[p]) for p in range(int(crow[r]), int(crow[r + 1]))} for r in range(m)]
    rows.append({c.s: 0.0, c.s + 1: 2.0, m: 1.0})
    c.csr, c.m, c.name = S.from_rows(rows), m + 1, c.name + " + a row that meets the Inf with l = 0"
    return c


@lru_cache(maxsize=None)
def range_cases(form, length=0, wide=0, reader=False):
    """the 15 rows of range_block_cases.rows() in one form, with a carrier of `length` entries (0: no idle row in front)"""
    out = tuple(transplant(row, form, pad_for(row, form, length) if length else 0, wide, reader) for row in R.rows())
    assert len(out) == 15 and not LEFT_OUT
    return out


def variants():
    """every (form, length, wide, reader) the tests run: the row classes, the wide sources, the reader row"""
    out = []
    for form in FORMS:
        out += [(form, n, 0, False) for n in lengths(form)]
        out += [(form, 0, w, False) for w in WIDES]
        out.append((form, 0, WIDES[-1], True))
    return tuple(out)


# ---- models ------------------------------------------------------------------------------------------------------------
def products(csr, lu):
    """every product (l_ik, u_kj) the definition forms, from the finished factor"""
    crow, col, _ = csr
    m = len(crow) - 1
    col = col.tolist()
    diag = [col.index(r, int(crow[r]), int(crow[r + 1])) for r in range(m)]
    upper = {r: {col[p]: p for p in range(diag[r] + 1, int(crow[r + 1]))} for r in range(m) if diag[r] + 1 < crow[r + 1]}
    out = []
    for i in range(m):
        p0, p1 = int(crow[i]), int(crow[i + 1])
        for pk in range(p0, diag[i]):
            k = col[pk]
            if k in upper:
                out += [(float(lu[pk]), float(lu[upper[k][col[p]]])) for p in range(pk + 1, p1) if col[p] in upper[k]]
    return out


_MODEL = {}
# (the idle entries repeat a few small values: the oracle is asked once per total)
reference_round = lru_cache(maxsize=None)(S.reference_round)


def model(c, reference=False):
    """(lu, info0, info1, detail) of a case, once per process; detail.settle: the least number of entries that the
    accumulator must round (the model's ties and out-of-range entries, and the case's own total where settles() holds)"""
    key = (c.name, reference)
    if key not in _MODEL:
        if reference:
            _MODEL[key] = S.ilu0_exact(*c.csr, rounder=reference_round) + (None,)
        else:
            lu, i0, i1, d = S.ilu0_exact(*c.csr, detail=True)
            d.settle = d.ties + (1 if R.settles(c.total) and d.kind[c.at] != S.TIE else 0)
            _MODEL[key] = (lu, i0, i1, d)
    return _MODEL[key]


def behind(lead, csr):
    """blockdiag(lead, csr) as CSR"""
    (c0, j0, v0), (c1, j1, v1) = lead, csr
    m0 = len(c0) - 1
    return np.concatenate([c0, c1[1:] + c0[-1]]), np.concatenate([j0, j1 + m0]), np.concatenate([v0, v1])


LEAD = 255


@lru_cache(maxsize=None)
def lead_model(reference=False):
    """the model of tridiagonal(LEAD), the healthy block in front: (lu, detail)"""
    lu, i0, i1, d = S.ilu0_exact(*S.tridiagonal(LEAD), detail=True)
    assert (i0, i1) == (0, 0)
    if reference:
        lu = S.ilu0_exact(*S.tridiagonal(LEAD), rounder=reference_round)[0]
    return lu, d


def behind_model(c, reference=False):
    """the model of behind(tridiagonal(LEAD), c.csr), composed: the off-diagonal blocks store nothing, so the two factors
    do not meet (test_spilu0_edge_cases.py holds the composition to the model of the whole)"""
    lu, i0, i1, d = model(c, reference)
    llu, ld = lead_model(reference)
    assert i0 == 0
    if d is not None:
        d = SimpleNamespace(terms=ld.terms + d.terms, ties=ld.ties + d.ties, nears=ld.nears + d.nears, settle=ld.ties + d.settle)
    return np.concatenate([llu, lu]), 0, (i1 + LEAD if i1 else 0), d


# ---- planted ties in long rows -------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def planted(pad=0):
    """spilu0_cases.planted() behind `pad` idle rows (module docstring)"""
    crow, col, val = S.planted()
    m = len(crow) - 1
    rows = [{i: _pow2(i)} for i in range(pad)]
    for r in range(m):
        new = {int(col[p]) + pad: float(val[p]) for p in range(int(crow[r]), int(crow[r + 1]))}
        if r >= S.PLANTED_SRC + S.PLANTED_MID:
            new.update({i: _small(i + r) for i in range(pad)})
        rows.append(new)
    return S.from_rows(rows)


@lru_cache(maxsize=None)
def planted_model(pad, reference=False):
    if reference:
        return S.ilu0_exact(*planted(pad), rounder=reference_round)
    return S.ilu0_exact(*planted(pad), detail=True)


def planted_pad(length):
    return length - 12


# ---- small structures ------------------------------------------------------------------------------------------------------
def one_row():
    return S.from_rows([{0: 3.0}])


def diagonal(m=300):
    """nothing is ever fetched: no row has an L part"""
    return S.from_rows([{i: float((i % 9 + 1) * (-1) ** i)} for i in range(m)])


def negative_zero():
    """A stored -0.0 with no product under it: (0, 1) in U, (1, 0) and (2, 1) in L.  The exact paths round the exact total
    0, which is +0.0 (and l = +0.0 / u_jj: -0.0 under the negative u_11), the plain fp64 form of fpe = 1 keeps the stored
    sign: plain_ilu0 gives -0.0 in U and -0.0 / u_jj in L.  The two models differ in the sign bits alone."""
    return S.from_rows([{0: 2.0, 1: -0.0, 2: 5.0}, {0: -0.0, 1: -3.0, 2: 1.0}, {1: -0.0, 2: 7.0}])


SMALL = {"one row": one_row, "diagonal": diagonal, "negative zero": negative_zero}


def empty_row():
    """an eighth structural defect: row 6 of a tridiagonal matrix stores nothing at all (so no diagonal either)"""
    rows = [{c: 1.0 + (c == i) for c in (i - 1, i, i + 1) if 0 <= c < 12} for i in range(12)]
    rows[6] = {}
    return S.from_rows(rows)


def empty_pattern_nan(where):
    """a 4-row matrix with one lower and one upper diagonal whose u_00 ("pivot") or u_01 ("upper") is the all-ones NaN, the
    pattern the mailbox reserves for "not posted": row 0 posts it as it stands, and everything behind depends on it"""
    rows = [{c: 4.0 if c == i else -1.0 for c in (i - 1, i, i + 1) if 0 <= c < 4} for i in range(4)]
    crow, col, val = S.from_rows(rows)
    v = val.view(np.uint64)
    v[{"pivot": 0, "upper": 1}[where]] = ALL_ONES
    return crow, col, val


# ---- value sets on the pattern of spilu0_cases.zero_pivot() (capture and replay) -----------------------------------------
def zero_pivot_sets():
    """[(name, val)] on zero_pivot()'s pattern, in the order of the replays: healthy, the zero pivot, healthy again (other
    values), then two range rows with one product (row 4 is the carrier in form "D": u_33 = d, u_34 = d x, a_43 = a)"""
    crow, col, val = S.zero_pivot()
    p3, p4 = int(crow[3]), int(crow[4])
    assert col[p3:p4 + 3].tolist() == [3, 4, 3, 4, 5]
    healthy = val.copy()
    healthy[p4 + 1] = 5.0
    other = val * 1.25
    other[p4 + 1] = -7.0
    out = [("healthy", healthy), ("zero pivot", val.copy()), ("healthy again", other)]
    sup = R.support()
    for name in ("tie at the overflow threshold", "subnormal total, quotient a tie"):
        _, _, b, dia, ent = next(r for r in R.rows() if r[0] == name)
        (k, a), = ent.items()
        v = healthy.copy()
        d = R._delta(a)
        v[p3], v[p3 + 1], v[p4], v[p4 + 1] = d, d * sup[k], a, b
        out.append((name, v))
    return out
