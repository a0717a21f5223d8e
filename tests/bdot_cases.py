"""Constructed ExBDOT inputs (row-major block pairs) whose exact column inner products are known as Python integers or
Fractions -- the block counterpart of tests/blas1_cases.py, whose cases it packs into columns.

Nothing here touches the GPU, the library or the oracle.  Every product x * y of a construction is exactly representable
as a double (asserted), so the exact inner product is the sum of those doubles and TwoProd has nothing to add.

  planted_d    up to 64 ExSUM cases (families A..D), one per column, for mode 'D': column j of X holds case j's terms
               divided by +-2^e_r, column j of Y the matching +-2^e_r, e_r from SCALES wherever the scaled term is still
               exactly representable (else 0).  Columns are zero-padded to a common n; the first term of a column sits at
               row 0, inside the block, so that the last term is the last row, or halfway to that, by the column's index.
               Expected: the case's `want`.
  planted_g    the same columns, unscaled, in X for mode 'G'; column j of Y is the constant 2^s_j.  Expected:
               round_nearest_even(T_i 2^s_j / 2^1074), kept (`keep`) only where every term times 2^s_j is exactly
               representable and the result is finite and normal.
  integer_blocks  random entries m 2^s, |m| < 2^26, s in [-400, 400]; the exact Gram matrix from Fractions.  Planted: row 0
               of C cancels to zero everywhere (the rows come in pairs with equal Y rows and opposite X[:, 0]), C[1, 1] is
               a tie that rounds down to even, C[2, 2] a tie that rounds up to even.
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import blas1_cases as B
import exact_cases as E

SCALES = (0, 1, -1, 20, -20)
MAX_COLS = 64
PAD_ROWS = 67          # rows beyond the longest column: room for the start offsets


def sample(count):
    """`count` or a few more cases of families A..D, none of their kinds left out"""
    return B.stride_sample(B.sum_cases(), count)


def _start(j, n, length):
    """first row of column j's terms: the first rows, an interior, flush with the last row, halfway to that"""
    room = n - length
    return (0, min(37, room), room, room // 2)[j % 4]


def _scaled(x, e):
    """(x 2^-e, 2^e) when that is exact and finite, else (x, 1.0)"""
    if e:
        try:
            xs = math.ldexp(x, -e)
        except OverflowError:
            xs = math.inf
        if math.isfinite(xs) and math.ldexp(xs, e) == x and xs * math.ldexp(1.0, e) == x:
            return xs, math.ldexp(1.0, e)
    return x, 1.0


def planted_d(cases):
    cases = list(cases)
    assert 0 < len(cases) <= MAX_COLS
    k = len(cases)
    n = max(len(c.terms) for c in cases) + PAD_ROWS
    X, Y = np.zeros((n, k)), np.zeros((n, k))
    scaled = 0
    for j, c in enumerate(cases):
        r0 = _start(j, n, len(c.terms))
        for t, x in enumerate(c.terms):
            r = r0 + t
            xs, ys = _scaled(x, SCALES[(r + j) % len(SCALES)])
            sign = -1.0 if (r + 2 * j) % 3 == 0 else 1.0
            X[r, j], Y[r, j] = sign * xs, sign * ys
            scaled += ys != 1.0
    want = np.array([c.want for c in cases])
    return SimpleNamespace(X=X, Y=Y, n=n, k=k, want=want, T=[c.T for c in cases], scaled=scaled)


def planted_g(cases, shifts):
    cases = list(cases)
    assert 0 < len(cases) <= MAX_COLS and len(shifts) > 0
    p, q = len(cases), len(shifts)
    n = max(len(c.terms) for c in cases) + PAD_ROWS
    X, Y = np.zeros((n, p)), np.zeros((n, q))
    for j, s in enumerate(shifts):
        Y[:, j] = math.ldexp(1.0, s)
    want, keep = np.zeros((p, q)), np.zeros((p, q), dtype=bool)
    for i, c in enumerate(cases):
        r0 = _start(i, n, len(c.terms))
        X[r0:r0 + len(c.terms), i] = c.terms
        distinct = set(c.terms)
        for j, s in enumerate(shifts):
            v = E.round_nearest_even(Fraction(c.T, B.ONE) * Fraction(2) ** s)
            want[i, j] = v
            prods = [x * math.ldexp(1.0, s) for x in distinct]
            exact = all(math.isfinite(v) for v in prods) and all(
                Fraction(v) == Fraction(x) * Fraction(2) ** s for v, x in zip(prods, distinct))
            keep[i, j] = exact and math.isfinite(v) and (v == 0.0 or abs(v) >= 2.0 ** -1022)
    return SimpleNamespace(X=X, Y=Y, n=n, p=p, q=q, want=want, keep=keep, T=[c.T for c in cases], shifts=tuple(shifts))


def exact_inner(x, y):
    """sum(Fraction(x_r) * Fraction(y_r)) over the rows where both are non-zero"""
    nz = np.nonzero((x != 0) & (y != 0))[0]
    return sum((Fraction(float(x[r])) * Fraction(float(y[r])) for r in nz), Fraction(0))


def integer_blocks(rng, n, p, q):
    assert n >= 20 and n % 2 == 0 and p >= 3 and q >= 3
    h = n // 2

    def entries(rows, cols):
        m = rng.integers(-(1 << 26) + 1, 1 << 26, size=(rows, cols))
        s = rng.integers(-400, 401, size=(rows, cols))
        return np.ldexp(m.astype(np.float64), s)

    X, Y = entries(n, p), entries(n, q)
    # row 0 of C cancels: the second half of Y repeats the first, X[:, 0] changes sign
    Y[h:] = Y[:h]
    X[h:, 0] = -X[:h, 0]
    # C[1, 1] = (2^53 + 1) 2^t, C[2, 2] = (2^53 + 3) 2^t: ties, to even downwards and upwards
    # (the planted rows lie in the first half and Y keeps its two equal halves, so row 0 of C still cancels)
    for col, t, exps in ((1, -77, (53, 0)), (2, 130, (53, 0, 1))):
        X[:, col] = 0.0
        a = int(rng.integers(-300, 300))
        for r, e in zip(range(3 * col, 3 * col + len(exps)), exps):
            X[r, col] = math.ldexp(1.0, a)
            Y[r, col] = Y[h + r, col] = math.ldexp(1.0, t + e - a)
    G = np.empty((p, q), dtype=object)
    for i in range(p):
        for j in range(q):
            G[i, j] = exact_inner(X[:, i], Y[:, j])
    want = np.array([[E.round_nearest_even(G[i, j]) for j in range(q)] for i in range(p)])
    return SimpleNamespace(X=X, Y=Y, n=n, p=p, q=q, G=G, want=want, zeros=[(0, j) for j in range(q)],
                           ties=[(1, 1, -77, 1), (2, 2, 130, 3)])
