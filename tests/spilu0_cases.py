"""Cases for the ExSpILU0 tests (the exact-sum ILU(0) factor of a CSR matrix).  Nothing here calls the code under test:
every expectation comes from ilu0_exact below, the definition in exact integer / Fraction arithmetic.

The definition.  Every row has strictly ascending columns and a stored diagonal, S is the set of stored positions, the
factor has the same pattern.  For every stored (i, j), rows in ascending order:
    c_ij = Round(a_ij - sum_k l_ik u_kj)        k < min(i, j), (i, k) in S, (k, j) in S; the sum exact, rounded once
    j <  i: l_ij = fl(c_ij / u_jj)              one IEEE division
    j >= i: u_ij = c_ij
This is getrf_cases.getrf_exact without the pivot search, on the pattern.  info0: 0 or r + 1 for the smallest row with a
structural defect (row_ptr decreasing or leaving [0, row_ptr[m]], a column outside [0, m), columns not strictly ascending,
no stored diagonal, more than MAX_ROW entries); info1: 0 or r + 1 for the smallest row whose pivot is zero or NaN.

The planted matrix (`planted`).  Rows 0 .. 3 are SOURCE rows without an L part, so u_kj = a_kj: small integers, the pivots
1, 2, 4 and 2^40.  Then eight MIDDLE rows that hold a power of two on the diagonal and nothing else, then the PLANTED rows:
a_ik for k < 4 are small multiples of the pivots, so l_ik is a small integer (2^-40 for k = 3) and the sum
s = sum_k l_ik u_kj is an odd integer, plus or minus 2^-40 in the NEAR columns, where u_3j = +-1.  a_ij = t + (the integer
part of s) with t an odd integer just above 2^53 is an even integer below 2^54, i.e. a double, and the exact total is t (a
tie) or t -+ 2^-40 (a near-tie, 2^-40 of the half unit away: far inside the margin of the register certificate).  Planted
entries lie in the middle columns (the L part: the divisor there is a power of two) and on and right of the diagonal (the
U part).  A middle row has no U part and a planted row no L entry in a planted column, so no other product reaches a
planted total.  The classes are asserted through the model in test_spilu0_cases.py."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import getrf_cases as G
import potrf_cases as P

CLEAR, TIE, NEAR = P.CLEAR, P.TIE, P.NEAR
MAX_ROW = 512                            # EXBLAS_SPILU0_MAX_ROW
NAN_BITS = 0x7ff8dead0000beef            # what an lu that must not be written is pre-filled with
_ONE = G._ONE


# ---- the model ---------------------------------------------------------------------------------------------------------
def structure(crow, col, m):
    """info0: 0, or r + 1 for the smallest row r with a structural defect"""
    crow, col = [int(v) for v in crow], [int(v) for v in col]
    cap = crow[m]
    for r in range(m):
        p0, p1 = crow[r], crow[r + 1]
        if p0 < 0 or p1 < p0 or p1 > cap or p1 > len(col) or p1 - p0 > MAX_ROW:
            return r + 1
        cs = col[p0:p1]
        if any(c < 0 or c >= m for c in cs) or any(b <= a for a, b in zip(cs, cs[1:])) or r not in cs:
            return r + 1
    return 0


def _round_even(t):
    return P._round(t)


def round_away(t):
    """the one rounding with ties broken AWAY from even: a defect the cases must be able to see"""
    v = P._round(t)
    if t == 0 or not math.isfinite(v):
        return v
    err = t - Fraction(v)
    if abs(err) * 2 == Fraction(math.ulp(v)):
        return float(np.nextafter(v, math.copysign(math.inf, err)))
    return v


def reference_round(t):
    """the reference's rounding of an exact total: the oracle's restatement on the canonical limbs"""
    import blas1_cases as B
    from oracle import pyoracle
    T = t * 2 ** 1074
    assert T.denominator == 1 and B.canon_fits(T.numerator)
    return float(pyoracle.round_limbs(B.canon_matrix([T.numerator])[0], pyoracle.ROUND_REFERENCE))


def ilu0_exact(crow, col, val, detail=False, rounder=None, round_products=False):
    """(lu, info0, info1): the definition.  Every total is summed exactly (integers at a fixed binary scale), `rounder`
    (default: nearest even) does the one rounding, the quotient of two np.float64 the division.  A non-finite operand
    decides the totals it meets in IEEE arithmetic: Inf - Inf and 0 * Inf are NaN.  With a structural defect lu is a copy
    of val (nothing is computed).  detail: also a namespace with kind (CLEAR / TIE / NEAR per stored entry), terms (the
    number of products, i.e. of triples (i, k, j)) and the counts ties_l, ties_u, nears_l, nears_u.
    round_products: the running sum is rounded after every product (a defect the cases must be able to see)."""
    rounder = rounder or _round_even
    crow, col = np.asarray(crow).astype(np.int64), np.asarray(col).astype(np.int64)
    lu = np.array(val, dtype=np.float64, copy=True)
    m = len(crow) - 1
    info0 = structure(crow, col, m)
    kind = np.zeros(len(lu), dtype=np.int8)
    if info0:
        out = (lu, info0, 0)
        return out + (SimpleNamespace(kind=kind, terms=0),) if detail else out
    fin = np.isfinite(lu)
    li = [G._int(v) if f else 0 for v, f in zip(lu.tolist(), fin.tolist())]
    where = [dict() for _ in range(m)]          # row k: {column: position}
    diag = [0] * m
    for r in range(m):
        for p in range(int(crow[r]), int(crow[r + 1])):
            where[r][int(col[p])] = p
        diag[r] = where[r][r]
    info1, terms = 0, 0
    rows = np.repeat(np.arange(m), np.diff(crow))
    with np.errstate(all="ignore"):
        for i in range(m):
            p0, p1 = int(crow[i]), int(crow[i + 1])
            lpart = [(p, int(col[p])) for p in range(p0, p1) if col[p] < i]
            for p in range(p0, p1):
                j = int(col[p])
                pairs = [(pk, where[k][j]) for pk, k in lpart if k < j and j in where[k]]
                terms += len(pairs)
                if not fin[p] or any(not (fin[a] and fin[b]) for a, b in pairs):
                    special = [] if fin[p] else [float(lu[p])]
                    special += [-float(np.float64(lu[a]) * np.float64(lu[b])) for a, b in pairs if not (fin[a] and fin[b])]
                    v, kd = float(np.sum(np.array(special))), TIE
                else:
                    if round_products:
                        t = Fraction(float(lu[p]))
                        for n, (a, b) in enumerate(pairs):
                            t -= Fraction(float(lu[a])) * Fraction(float(lu[b]))
                            if n + 1 < len(pairs):
                                t = Fraction(P._round(t))
                    else:
                        t = Fraction(li[p] * _ONE - sum(li[a] * li[b] for a, b in pairs), _ONE * _ONE)
                    v = rounder(t)
                    kd = P._kind(t, v)
                if j < i:
                    v = float(np.float64(v) / np.float64(lu[diag[j]]))
                lu[p], kind[p] = v, kd
                fin[p] = math.isfinite(v)
                li[p] = G._int(v) if fin[p] else 0
            u = lu[diag[i]]
            if info1 == 0 and (u == 0 or math.isnan(u)):
                info1 = i + 1
    if detail:
        low = col < rows
        d = SimpleNamespace(kind=kind, terms=terms, ties=int((kind == TIE).sum()), nears=int((kind == NEAR).sum()),
                            ties_l=int(((kind == TIE) & low).sum()), ties_u=int(((kind == TIE) & ~low).sum()),
                            nears_l=int(((kind == NEAR) & low).sum()), nears_u=int(((kind == NEAR) & ~low).sum()))
        return lu, info0, info1, d
    return lu, info0, info1


def restate(crow, col, val):
    """a second, naive restatement for small finite sound cases: dictionaries of Fractions, k over the whole range"""
    m = len(crow) - 1
    a = {}
    for r in range(m):
        for p in range(int(crow[r]), int(crow[r + 1])):
            a[(r, int(col[p]))] = float(val[p])
    f = {}
    for i in range(m):
        for j in sorted(c for (r, c) in a if r == i):
            t = Fraction(a[(i, j)])
            for k in range(min(i, j)):
                if (i, k) in a and (k, j) in a:
                    t -= Fraction(f[(i, k)]) * Fraction(f[(k, j)])
            c = P._round(t)
            f[(i, j)] = float(np.float64(c) / np.float64(f[(j, j)])) if j < i else c
    return np.array([f[(r, int(col[p]))] for r in range(m) for p in range(int(crow[r]), int(crow[r + 1]))])


def plain_ilu0(crow, col, val):
    """the fp64 restatement of fpe == 1: s = a_ij, then s -= l_ik * u_kj for k ascending"""
    lu = np.array(val, dtype=np.float64, copy=True)
    m = len(crow) - 1
    where = [{int(col[p]): p for p in range(int(crow[r]), int(crow[r + 1]))} for r in range(m)]
    with np.errstate(all="ignore"):
        for i in range(m):
            p0, p1 = int(crow[i]), int(crow[i + 1])
            lpart = [(p, int(col[p])) for p in range(p0, p1) if col[p] < i]
            for p in range(p0, p1):
                j = int(col[p])
                s = np.float64(lu[p])
                for pk, k in lpart:
                    if k < j and j in where[k]:
                        s = s - np.float64(lu[pk]) * np.float64(lu[where[k][j]])
                lu[p] = s / np.float64(lu[where[j][j]]) if j < i else s
    return lu


def dense_of(crow, col, val):
    m = len(crow) - 1
    D = np.zeros((m, m))
    for r in range(m):
        for p in range(int(crow[r]), int(crow[r + 1])):
            D[r, int(col[p])] = val[p]
    return D


def apply_exact(crow, col, lu, b):
    """U^-1 L^-1 b: exact_cases.trsv_exact twice on the densified factor (the upper sweep as a lower one, reversed)"""
    import exact_cases as E
    D = dense_of(crow, col, lu)
    m = D.shape[0]
    y, _ = E.trsv_exact(np.tril(D, -1) + np.eye(m), b, unit=True)
    x, _ = E.trsv_exact(np.ascontiguousarray(np.triu(D)[::-1, ::-1]), y[::-1].copy())
    return x[::-1].copy()


# ---- builders: (crow, col, val) with int64 indices, sorted unique columns, a stored diagonal ---------------------------------
def from_rows(rows):
    """rows: one {column: value} per row"""
    crow, col, val = [0], [], []
    for r in rows:
        for c in sorted(r):
            col.append(c)
            val.append(r[c])
        crow.append(len(col))
    return np.array(crow, dtype=np.int64), np.array(col, dtype=np.int64), np.array(val, dtype=np.float64)


def as_width(csr, itype):
    return csr[0].astype(itype), csr[1].astype(itype), csr[2]


def _values(rows, rng):
    """full-mantissa nonsymmetric values: off the diagonal in (-1, 0), the diagonal above the row's and the column's sums"""
    m = len(rows)
    colsum = np.zeros(m)
    for r in rows:
        for c in r:
            r[c] = -float(rng.random()) - 2.0 ** -10
            colsum[c] += 1.0
    for i, r in enumerate(rows):
        r[i] = max(len(r), colsum[i]) + 1.0 + float(rng.random())
    return rows


@lru_cache(maxsize=None)
def tridiagonal(m=257):
    rng = np.random.default_rng([m, 1, 70])
    return from_rows(_values([{c: 0.0 for c in (i - 1, i, i + 1) if 0 <= c < m} for i in range(m)], rng))


@lru_cache(maxsize=None)
def stencil(dims, points):
    """the 5-point (2-D), 7-point or 27-point (3-D) stencil on a grid of `dims`"""
    rng = np.random.default_rng([points, 2, 70, *dims])
    dims = tuple(dims)
    idx = np.arange(int(np.prod(dims))).reshape(dims)
    rows = []
    for at in np.ndindex(*dims):
        r = {}
        for off in np.ndindex(*(3,) * len(dims)):
            d = tuple(o - 1 for o in off)
            if points in (5, 7) and sum(abs(x) for x in d) > 1:
                continue
            to = tuple(a + x for a, x in zip(at, d))
            if all(0 <= t < n for t, n in zip(to, dims)):
                r[int(idx[to])] = 0.0
        rows.append(r)
    return from_rows(_values(rows, rng))


@lru_cache(maxsize=None)
def dense(p):
    """a dense pattern, diagonally dominant by rows and columns: partial pivoting never swaps (asserted on the CPU)"""
    A = G.dominant(p, seed=3)
    return from_rows([{c: float(A[r, c]) for c in range(p)} for r in range(p)]), A


@lru_cache(maxsize=None)
def random_pattern(m=300, per_row=8, seed=4):
    rng = np.random.default_rng([m, seed, 70])
    rows = []
    for i in range(m):
        cs = set(rng.choice(m, per_row - 1, replace=False).tolist()) | {i}
        rows.append({int(c): 0.0 for c in cs})
    return from_rows(_values(rows, rng))


@lru_cache(maxsize=None)
def arrow_band(m=520, long_rows=(65, 130, 512)):
    """a band with a stored last column, and last rows of 65, 130 and 512 entries: the several-entries-per-lane form, its
    exact limit included (a row of 512 distinct columns needs m >= 512)"""
    rng = np.random.default_rng([m, 5, 70])
    rows = [{c: 0.0 for c in (i - 1, i, i + 1, m - 1) if 0 <= c < m} for i in range(m)]
    for q, n in enumerate(long_rows):
        i = m - len(long_rows) + q
        cs = set(np.linspace(0, i - 1, n - 1 - (m - 1 - i)).astype(int).tolist()) | set(range(i, m))
        extra = iter(range(i - 1, -1, -1))
        while len(cs) < n:
            cs.add(next(extra))
        assert len(cs) == n
        rows[i] = {int(c): 0.0 for c in cs}
    return from_rows(_values(rows, rng))


@lru_cache(maxsize=None)
def random_earlier(m=4096, seed=6):
    """every row depends on a few random earlier rows and stores a few later columns: many waves wait on the mailbox"""
    rng = np.random.default_rng([m, seed, 70])
    rows = []
    for i in range(m):
        cs = {i}
        if i:
            cs |= set(rng.choice(i, min(i, 4), replace=False).tolist())
        if i < m - 1:
            cs |= set((i + 1 + rng.choice(m - 1 - i, min(m - 1 - i, 3), replace=False)).tolist())
        rows.append({int(c): 0.0 for c in cs})
    return from_rows(_values(rows, rng))


PLANTED_SRC, PLANTED_MID, PLANTED_ROWS = 4, 8, 14


@lru_cache(maxsize=None)
def planted():
    """the planted matrix of the module docstring"""
    rng = np.random.default_rng([7, 70])
    B, M, R = PLANTED_SRC, PLANTED_MID, PLANTED_ROWS
    m = B + M + R
    piv = (1.0, 2.0, 4.0, 2.0 ** 40)
    rows = [dict() for _ in range(m)]
    for k in range(B):
        rows[k][k] = piv[k]
        for j in range(B, m):
            if k == 0:
                rows[k][j] = float(2 * int(rng.integers(1, 9)) + 1)       # odd
            elif k < 3:
                rows[k][j] = float(int(rng.integers(-9, 10)))
            else:
                rows[k][j] = float((-1) ** (j // 2)) if j % 2 else 0.0        # odd columns: NEAR
    for j in range(B, B + M):
        rows[j][j] = 2.0 ** (j % 3)
    tees = (2 ** 53 + 1, 2 ** 53 + 3, -(2 ** 53 + 1), 2 ** 53 + 5)
    for r in range(R):
        i = B + M + r
        l = (2 * int(rng.integers(1, 9)) + 1, 2 * int(rng.integers(-4, 5)), 2 * int(rng.integers(-4, 5)))   # odd, even, even
        for k in range(3):
            rows[i][k] = float(l[k]) * piv[k]
        rows[i][3] = 1.0                                 # l_i3 = 2^-40
        cols = [B + (r + q) % M for q in range(4)] + [c for c in range(i, i + 4) if c < m]
        for j in cols:
            s = sum(l[k] * int(rows[k][j]) for k in range(3))
            assert s % 2 == 1
            a = tees[(i + j) % 4] + s
            assert a % 2 == 0 and abs(a) < 2 ** 54
            rows[i][j] = float(a)
    return from_rows(rows)


@lru_cache(maxsize=None)
def zero_pivot():
    """row 4's pivot cancels exactly: u_44 = 2 - (4 / 2) * 1 = 0; the rows behind it meet Inf and NaN"""
    m = 9
    rows = [{i: 3.0 + i, **({i + 1: 1.0} if i + 1 < m else {})} for i in range(m)]
    rows[3] = {3: 2.0, 4: 1.0}
    rows[4] = {3: 4.0, 4: 2.0, 5: 1.0}
    for i in range(5, m):
        rows[i][i - 1] = 1.0
    return from_rows(rows)


@lru_cache(maxsize=None)
def nonfinite():
    """the 5-point stencil with a NaN and an Inf among its values"""
    crow, col, val = stencil((6, 6), 5)
    val = val.copy()
    val[int(crow[7]) + 1] = math.nan
    val[int(crow[20]) + 2] = math.inf
    return crow, col, val


def defects():
    """{name: (crow, col, val)}: one matrix for each structural defect"""
    out = {}
    base = tridiagonal(12)
    crow, col, val = (a.copy() for a in base)
    crow[5] = crow[4] - 1
    out["row_ptr decreasing"] = (crow, col, val)
    crow, col, val = (a.copy() for a in base)
    col[int(crow[6]) + 2] = 12
    out["column past the end"] = (crow, col, val)
    crow, col, val = (a.copy() for a in base)
    col[int(crow[3])] = -1
    out["negative column"] = (crow, col, val)
    crow, col, val = (a.copy() for a in base)
    p = int(crow[7])
    col[p], col[p + 1] = col[p + 1], col[p]
    out["columns not ascending"] = (crow, col, val)
    crow, col, val = (a.copy() for a in base)
    col[int(crow[9]) + 1] = col[int(crow[9])]
    out["duplicate column"] = (crow, col, val)
    rows = [{c: 1.0 for c in (i - 1, i, i + 1) if 0 <= c < 12} for i in range(12)]
    del rows[8][8]
    out["no stored diagonal"] = from_rows(rows)
    m, r = 520, 515
    rows = [{i: 2.0} for i in range(m)]
    rows[r] = {c: 1.0 for c in range(MAX_ROW)}
    rows[r][r] = 2.0
    assert len(rows[r]) == MAX_ROW + 1
    out["a row of 513 entries"] = from_rows(rows)
    return out


SOUND = {
    "tridiagonal": lambda: tridiagonal(257),
    "stencil5": lambda: stencil((12, 12), 5),
    "stencil7": lambda: stencil((6, 6, 6), 7),
    "stencil27": lambda: stencil((5, 5, 5), 27),
    "dense24": lambda: dense(24)[0],
    "dense64": lambda: dense(64)[0],
    "random": lambda: random_pattern(300),
    "arrow_band": lambda: arrow_band(520),
    "random_earlier": lambda: random_earlier(4096),
    "planted": planted,
    "zero_pivot": zero_pivot,
    "nonfinite": nonfinite,
}
SMALL = ("stencil5", "dense24", "planted")       # what the naive restatement is run on


@lru_cache(maxsize=None)
def expected(name):
    """(lu, info0, info1, detail) of a sound case, computed once per session"""
    return ilu0_exact(*SOUND[name](), detail=True)
