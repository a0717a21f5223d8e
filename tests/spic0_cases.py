"""Cases for the ExSpIC0 tests (the exact-sum IC(0) factor of a symmetric CSR matrix).  Nothing here calls the code under
test: every expectation comes from ic0_exact below, the definition in exact integer / Fraction arithmetic.

The definition.  Every row has strictly ascending columns and a stored diagonal, the pattern S is structurally symmetric,
only the entries on and below the diagonal are read.  For every stored (i, j) with j <= i, rows in ascending order:
    c_ij = Round(a_ij - sum_k l_ik l_jk)        k < j, (i, k) in S, (j, k) in S; the sum exact, rounded once
    j <  i: l_ij = fl(c_ij / l_jj)              one IEEE division
    j == i: l_ii = fl(sqrt(c_ii))               one correctly rounded square root
The factor lies on A's pattern: L on and below the diagonal, every stored (j, i) above it holds l_ij.  This is
potrf_cases.potrf_exact on the pattern, except at a breakdown: a radicand that is not > 0 gives sqrt(c_ii) by IEEE
arithmetic and the factorisation goes on.  info0: 0, or r + 1 for the smallest row with one of ExSpILU0's structural
defects (phase 1, spilu0_cases.structure); when there is none, r + 1 for the smallest row r that stores an (r, j) without
(j, r) (phase 2).  info1: 0, or r + 1 for the smallest row whose radicand is not > 0.

Every builder returns symmetric values (int64 indices, sorted unique columns, a stored diagonal); the healthy ones are
diagonally dominant with a positive diagonal, hence positive definite, so IC(0) exists."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import getrf_cases as G
import potrf_cases as P
import spilu0_cases as S

CLEAR, TIE, NEAR = P.CLEAR, P.TIE, P.NEAR
MAX_ROW = S.MAX_ROW                      # EXBLAS_SPIC0_MAX_ROW
NAN_BITS = S.NAN_BITS                    # what an ll that must not be written is pre-filled with
MAILBOX_NAN = np.array([0xFFFFFFFFFFFFFFFF], dtype=np.uint64).view(np.float64)[0]   # the mailbox's "not posted"
_ONE = G._ONE
from_rows, as_width, dense_of, round_away, reference_round = S.from_rows, S.as_width, S.dense_of, S.round_away, S.reference_round


# ---- the model ---------------------------------------------------------------------------------------------------------
def mirror_defect(crow, col, m):
    """phase 2: 0, or r + 1 for the smallest row r that stores some (r, j) with no stored (j, r)"""
    rows = [set(int(c) for c in col[int(crow[r]):int(crow[r + 1])]) for r in range(m)]
    for r in range(m):
        if any(r not in rows[j] for j in rows[r]):
            return r + 1
    return 0


def structure(crow, col, m):
    """info0: phase 1 (ExSpILU0's defects), then, only when it found nothing, phase 2"""
    return S.structure(crow, col, m) or mirror_defect(crow, col, m)


def _root(v):
    """the correctly rounded square root; IEEE's for a radicand that is not > 0 (zero: the zero, else NaN)"""
    if v > 0:
        return math.sqrt(v)
    with np.errstate(all="ignore"):
        return float(np.sqrt(np.float64(v)))


def in_range(x):
    """the register certificate's range: a non-zero finite double at or above 2^-960 and below 2^1000"""
    a = abs(float(x))
    return a == 0.0 or (math.isfinite(a) and 2.0 ** -960 <= a < 2.0 ** 1000)


def ic0_exact(crow, col, val, detail=False, rounder=None, round_products=False):
    """(ll, info0, info1): the definition.  Every total is summed exactly (integers at a fixed binary scale), `rounder`
    (default: nearest even) does the one rounding, the quotient of two np.float64 the division, math.sqrt the root.  A
    non-finite operand decides the totals it meets in IEEE arithmetic: Inf - Inf and 0 * Inf are NaN.  Only the values on
    and below the diagonal are read.  With a structural defect ll is a copy of val (nothing is computed).  detail: also a
    namespace with kind (CLEAR / TIE / NEAR per entry on and below the diagonal, 0 above), terms (the number of products,
    i.e. of triples (i, k, j) with j <= i), owned (entries on and below the diagonal), wide (rows with more than 64 of
    them), ties / nears and their split ties_l, ties_d, nears_l, nears_d (off the diagonal / on it), and ranged (every
    operand and every fixed entry lies in the register certificate's range).
    round_products: the running sum is rounded after every product (a defect the cases must be able to see)."""
    rounder = rounder or S._round_even
    crow, col = np.asarray(crow).astype(np.int64), np.asarray(col).astype(np.int64)
    ll = np.array(val, dtype=np.float64, copy=True)
    m = len(crow) - 1
    info0 = structure(crow, col, m)
    kind = np.zeros(len(ll), dtype=np.int8)
    if info0:
        out = (ll, info0, 0)
        return out + (SimpleNamespace(kind=kind, terms=0),) if detail else out
    rows = np.repeat(np.arange(m), np.diff(crow))
    low = col <= rows
    ll[~low] = 0.0                                       # (never read: the mirror overwrites it below)
    fin = np.isfinite(ll)
    li = [G._int(v) if f else 0 for v, f in zip(ll.tolist(), fin.tolist())]
    where = [dict() for _ in range(m)]                   # row r: {column: position} of its owned part
    for r in range(m):
        for p in range(int(crow[r]), int(crow[r + 1])):
            if col[p] <= r:
                where[r][int(col[p])] = p
    diag = [where[r][r] for r in range(m)]
    info1, terms, ranged = 0, 0, all(in_range(v) for v in np.asarray(val)[low])
    with np.errstate(all="ignore"):
        for i in range(m):
            lpart = [(p, int(col[p])) for p in range(int(crow[i]), diag[i])]
            for p in range(int(crow[i]), diag[i] + 1):
                j = int(col[p])
                pairs = [(pk, where[j][k]) for pk, k in lpart if k < j and k in where[j]]
                terms += len(pairs)
                if not fin[p] or any(not (fin[a] and fin[b]) for a, b in pairs):
                    special = [] if fin[p] else [float(ll[p])]
                    special += [-float(np.float64(ll[a]) * np.float64(ll[b])) for a, b in pairs if not (fin[a] and fin[b])]
                    v, kd = float(np.sum(np.array(special))), TIE
                else:
                    if round_products:
                        t = Fraction(float(ll[p]))
                        for n, (a, b) in enumerate(pairs):
                            t -= Fraction(float(ll[a])) * Fraction(float(ll[b]))
                            if n + 1 < len(pairs):
                                t = Fraction(P._round(t))
                    else:
                        t = Fraction(li[p] * _ONE - sum(li[a] * li[b] for a, b in pairs), _ONE * _ONE)
                    v = rounder(t)
                    kd = P._kind(t, v)
                if j < i:
                    v = float(np.float64(v) / np.float64(ll[diag[j]]))
                else:
                    if info1 == 0 and not v > 0:
                        info1 = i + 1
                    v = _root(v)
                ll[p], kind[p] = v, kd
                fin[p] = math.isfinite(v)
                li[p] = G._int(v) if fin[p] else 0
                ranged = ranged and in_range(v)
    for r in range(m):                                   # the mirror: (j, i) above the diagonal holds l_ij
        for p in range(int(crow[r]), int(crow[r + 1])):
            c = int(col[p])
            if c > r:
                ll[p] = ll[where[c][r]]
    if detail:
        on = col == rows
        d = SimpleNamespace(kind=kind, terms=terms, owned=int(low.sum()), ranged=ranged,
                            wide=int(sum(1 for r in range(m) if diag[r] + 1 - int(crow[r]) > 64)),
                            ties=int((kind == TIE).sum()), nears=int((kind == NEAR).sum()),
                            ties_l=int(((kind == TIE) & ~on).sum()), ties_d=int(((kind == TIE) & on).sum()),
                            nears_l=int(((kind == NEAR) & ~on).sum()), nears_d=int(((kind == NEAR) & on).sum()))
        return ll, info0, info1, d
    return ll, info0, info1


def restate(crow, col, val):
    """a second, naive restatement for finite sound cases: dictionaries of Fractions, k over the whole range, the lower
    triangle only (the mirror is filled in at the end)"""
    m = len(crow) - 1
    a = {}
    for r in range(m):
        for p in range(int(crow[r]), int(crow[r + 1])):
            a[(r, int(col[p]))] = float(val[p])
    f = {}
    for i in range(m):
        for j in sorted(c for (r, c) in a if r == i and c <= i):
            t = Fraction(a[(i, j)])
            for k in range(j):
                if (i, k) in a and (j, k) in a:
                    t -= Fraction(f[(i, k)]) * Fraction(f[(j, k)])
            c = P._round(t)
            f[(i, j)] = float(np.float64(c) / np.float64(f[(j, j)])) if j < i else _root(c)
    return np.array([f[(r, c) if c <= r else (c, r)] for r in range(m)
                     for c in (int(col[p]) for p in range(int(crow[r]), int(crow[r + 1])))])


def plain_ic0(crow, col, val):
    """the fp64 restatement of fpe == 1: s = a_ij, then s -= l_ik * l_jk for k ascending, then the division or the root"""
    ll = np.array(val, dtype=np.float64, copy=True)
    m = len(crow) - 1
    where = [{int(col[p]): p for p in range(int(crow[r]), int(crow[r + 1])) if col[p] <= r} for r in range(m)]
    with np.errstate(all="ignore"):
        for i in range(m):
            lpart = [(p, k) for k, p in sorted(where[i].items()) if k < i]
            for j, p in sorted(where[i].items()):
                s = np.float64(ll[p])
                for pk, k in lpart:
                    if k < j and k in where[j]:
                        s = s - np.float64(ll[pk]) * np.float64(ll[where[j][k]])
                ll[p] = s / np.float64(ll[where[j][j]]) if j < i else np.sqrt(s)
        for r in range(m):
            for p in range(int(crow[r]), int(crow[r + 1])):
                if col[p] > r:
                    ll[p] = ll[where[int(col[p])][r]]
    return ll


def apply_exact(crow, col, ll, b):
    """L^-T L^-1 b: exact_cases.trsv_exact with the lower triangle of the densified factor, then with its upper one (the
    mirror L^T) as a lower system in reversed order"""
    import exact_cases as E
    D = dense_of(crow, col, ll)
    y, _ = E.trsv_exact(np.tril(D), b)
    x, _ = E.trsv_exact(np.ascontiguousarray(np.triu(D)[::-1, ::-1]), y[::-1].copy())
    return x[::-1].copy()


# ---- builders ----------------------------------------------------------------------------------------------------------
def _symmetric(pairs, m, rng):
    """rows of the symmetric pattern {(i, i)} + pairs (+ mirrors): off the diagonal in (-1, 0), the same value on both
    sides; the diagonal above the row's count plus one: diagonally dominant, positive definite"""
    rows = [{i: 0.0} for i in range(m)]
    for i, j in sorted({(max(a, b), min(a, b)) for a, b in pairs if a != b}):
        v = -float(rng.random()) - 2.0 ** -10
        rows[i][j] = rows[j][i] = v
    for i, r in enumerate(rows):
        r[i] = float(len(r)) + 1.0 + float(rng.random())
    return from_rows(rows)


@lru_cache(maxsize=None)
def tridiagonal(m=257):
    return _symmetric([(i, i - 1) for i in range(1, m)], m, np.random.default_rng([m, 1, 71]))


@lru_cache(maxsize=None)
def stencil(n, points):
    """the 7-point or 27-point stencil on an n^3 grid"""
    idx = np.arange(n ** 3).reshape(n, n, n)
    pairs = []
    for at in np.ndindex(n, n, n):
        for off in np.ndindex(3, 3, 3):
            d = tuple(o - 1 for o in off)
            if points == 7 and sum(abs(x) for x in d) != 1:
                continue
            to = tuple(a + x for a, x in zip(at, d))
            if all(0 <= t < n for t in to):
                pairs.append((int(idx[at]), int(idx[to])))
    return _symmetric(pairs, n ** 3, np.random.default_rng([points, 2, 71, n]))


@lru_cache(maxsize=None)
def random_pattern(m=300, per_row=4, seed=4):
    rng = np.random.default_rng([m, seed, 71])
    pairs = [(i, int(c)) for i in range(m) for c in rng.choice(m, per_row, replace=False)]
    return _symmetric(pairs, m, rng)


@lru_cache(maxsize=None)
def dense(p):
    """(csr, G): a dense symmetric diagonally dominant G with full mantissas on the full pattern"""
    csr = _symmetric([(i, j) for i in range(p) for j in range(i)], p, np.random.default_rng([p, 3, 71]))
    return csr, dense_of(*csr)


def block_pattern(Gm, blocks):
    """the CSR of Gm on the pattern of its dense diagonal blocks (sizes `blocks` from row 0 on, then 1 x 1 blocks), zeros
    inside a block included"""
    p = Gm.shape[0]
    rows, at = [dict() for _ in range(p)], 0
    for n in list(blocks) + [1] * (p - sum(blocks)):
        for r in range(at, at + n):
            rows[r] = {c: float(Gm[r, c]) for c in range(at, at + n)}
        at += n
    return from_rows(rows)


@lru_cache(maxsize=None)
def planted(p):
    """(csr, potrf_cases.planted(p)): the planted system on its block pattern"""
    c = P.planted(p)
    return block_pattern(c.G, [4 + n for n in P.BLOCKS[p]]), c


@lru_cache(maxsize=None)
def arrow_first(m=512):
    """a dense first row and column and a band: row 0 stores 512 entries (its 511 upper columns are staged in 8 passes of
    64), every other row finds itself among them"""
    return _symmetric([(i, 0) for i in range(1, m)] + [(i, i - 1) for i in range(2, m)], m, np.random.default_rng([m, 5, 71]))


@lru_cache(maxsize=None)
def arrow_last(m=512):
    """a dense last row and column and a band: the last row owns 512 entries, every slot of the several-entries form"""
    return _symmetric([(m - 1, i) for i in range(m - 1)] + [(i, i - 1) for i in range(1, m - 1)], m,
                      np.random.default_rng([m, 6, 71]))


@lru_cache(maxsize=None)
def breakdown(r, what, m=40):
    """row r's radicand is exactly 0 ("zero") or -1 ("neg").  Rows: a first column of small integers a_i (l_00 = 1, so
    l_i0 = a_i exactly) and a band whose totals are small; row r has no band entry to its left, so its radicand is
    a_rr - a_r^2 exactly; the band entry (r + 1, r) carries the broken pivot onwards."""
    rng = np.random.default_rng([m, r, 8, 71])
    a = [0] + [int(rng.integers(1, 9)) for _ in range(1, m)]
    rows = [{0: 1.0}] + [{0: float(a[i])} for i in range(1, m)]
    for i in range(1, m):
        rows[0][i] = float(a[i])
    for i in range(2, m):
        if i != r:
            v = float(a[i] * a[i - 1]) + float(rng.random()) - 0.5
            rows[i][i - 1] = rows[i - 1][i] = v
    for i in range(1, m):
        rows[i][i] = float(a[i] * a[i]) + 8.0 + float(rng.random())
    rows[r][r] = float(a[r] * a[r]) - {"zero": 0.0, "neg": 1.0}[what]
    return from_rows(rows)


@lru_cache(maxsize=None)
def mailbox_nan(where):
    """the mailbox's reserved all-ones NaN as a_00 ("a00") or as a_10 (and a_01: "a10") of tridiagonal(12)"""
    crow, col, val = (x.copy() for x in tridiagonal(12))
    if where == "a00":
        val[0] = MAILBOX_NAN
    else:
        val[1] = val[int(crow[1])] = MAILBOX_NAN
    return crow, col, val


def _with_entries(base, extra, drop=()):
    """base (crow, col, val) with the stored entries `extra` {(r, c): v} added and the positions `drop` [(r, c)] removed"""
    crow, col, val = base
    m = len(crow) - 1
    rows = [{int(col[p]): float(val[p]) for p in range(int(crow[r]), int(crow[r + 1]))} for r in range(m)]
    for (r, c), v in extra.items():
        rows[r][c] = v
    for r, c in drop:
        del rows[r][c]
    return from_rows(rows)


def defects():
    """{name: (crow, col, val)}: every phase-1 defect (spilu0_cases.defects), a missing mirror on each side of the
    diagonal, and a phase-1 defect in a later row than a missing mirror"""
    out = dict(S.defects())
    base = tridiagonal(12)
    out["missing mirror above"] = _with_entries(base, {(3, 7): -0.5})              # (3, 7) without (7, 3): row 3
    out["missing mirror below"] = _with_entries(base, {(7, 3): -0.5})              # (7, 3) without (3, 7): row 7
    out["phase 1 after a missing mirror"] = _with_entries(base, {(3, 7): -0.5}, drop=[(9, 9)])   # row 9: no diagonal
    return out


DEFECT_INFO = {"missing mirror above": 4, "missing mirror below": 8, "phase 1 after a missing mirror": 10}

SOUND = {
    "tridiagonal": lambda: tridiagonal(257),
    "stencil7": lambda: stencil(8, 7),
    "stencil27": lambda: stencil(6, 27),
    "random": lambda: random_pattern(300),
    "dense24": lambda: dense(24)[0],
    "dense64": lambda: dense(64)[0],
    "dense65": lambda: dense(65)[0],
    "planted40": lambda: planted(40)[0],
    "planted64": lambda: planted(64)[0],
    "planted65": lambda: planted(65)[0],
    "planted130": lambda: planted(130)[0],
    "arrow_first": lambda: arrow_first(512),
    "arrow_last": lambda: arrow_last(512),
    "breakdown_zero": lambda: breakdown(17, "zero"),
    "breakdown_neg": lambda: breakdown(17, "neg"),
    "mailbox_nan_a00": lambda: mailbox_nan("a00"),
    "mailbox_nan_a10": lambda: mailbox_nan("a10"),
}
PLANTED = ("planted40", "planted64", "planted65", "planted130")
DENSE = {"dense24": 24, "dense64": 64, "dense65": 65}
BREAKDOWN_INFO = {"breakdown_zero": 18, "breakdown_neg": 18, "mailbox_nan_a00": 1, "mailbox_nan_a10": 2}
HEALTHY = tuple(n for n in SOUND if n not in BREAKDOWN_INFO)
NAIVE = ("tridiagonal", "stencil7", "random", "arrow_first")   # what the naive restatement is run on


@lru_cache(maxsize=None)
def expected(name):
    """(ll, info0, info1, detail) of a sound case, computed once per session"""
    return ic0_exact(*SOUND[name](), detail=True)
