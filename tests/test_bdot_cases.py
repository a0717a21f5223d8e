"""CPU tests of the constructed ExBDOT blocks (tests/bdot_cases.py): every construction meets its own integer / Fraction
arithmetic, and the oracle's ExDOT on the strided columns returns the expected bits in both rounding modes -- the
statement that the bits the GPU tests expect are ExDOT's.  No GPU involved."""
from fractions import Fraction

import numpy as np
import pytest

import bdot_cases as D
import blas1_cases as B
from helpers import same_double

SHIFTS = (0, 7, -13, 40)


def _batches(cases):
    return [cases[i:i + D.MAX_COLS] for i in range(0, len(cases), D.MAX_COLS)]


def _inner_units(x, y):
    """(sum of x_r y_r in units of 2^-1074, or None when it is no whole number of them; every product exact as a double)"""
    total, exact = 0, True
    for r in np.nonzero((x != 0) & (y != 0))[0]:
        a, b = float(x[r]), float(y[r])
        prod = B.units(a) * B.units(b)          # units of 2^-2148
        exact = exact and prod % B.ONE == 0 and np.isfinite(a * b) and B.units(a * b) * B.ONE == prod
        total += prod
    return (total // B.ONE if total % B.ONE == 0 else None), exact


def _ref_round(oracle, T):
    """the reference rule's rounding of T units, from the canonical limbs"""
    return oracle.round_limbs(B.canon_from_int(T), mode=oracle.ROUND_REFERENCE)


@pytest.fixture(scope="module")
def d_blocks():
    return [D.planted_d(b) for b in _batches(D.sample(2048))]


@pytest.fixture(scope="module")
def g_blocks():
    return [D.planted_g(b, SHIFTS) for b in _batches(D.sample(256))]


def test_planted_d_is_its_cases(d_blocks):
    assert sum(d.k for d in d_blocks) >= 2048 and sum(d.scaled for d in d_blocks) > 1000
    last_row = interior = 0
    for d in d_blocks:
        assert d.X.shape == d.Y.shape == (d.n, d.k) and d.k <= 64
        for j in range(d.k):
            T, exact = _inner_units(d.X[:, j], d.Y[:, j])
            assert exact and T == d.T[j], (j, d.T[j])
            assert same_double(d.want[j], B.X.round_nearest_even(Fraction(d.T[j], B.ONE)))
        last_row += int(np.count_nonzero(d.X[-1]))
        interior += int(np.count_nonzero(d.X[37]))
    assert last_row > 100 and interior > 100


def test_planted_d_is_exdot(oracle, d_blocks):
    for d in d_blocks:
        xf, yf = d.X.ravel(), d.Y.ravel()
        for j in range(d.k):
            got = oracle.exdot(xf, yf, inca=d.k, offa=j, incb=d.k, offb=j, n=d.n)
            assert same_double(got, d.want[j]), (j, got, d.want[j])
            if B.canon_fits(d.T[j]):
                ref = oracle.exdot(xf, yf, inca=d.k, offa=j, incb=d.k, offb=j, n=d.n, mode=oracle.ROUND_REFERENCE)
                assert same_double(ref, _ref_round(oracle, d.T[j])), (j, ref)


def test_planted_g_is_its_cases(g_blocks):
    kept = sum(int(g.keep.sum()) for g in g_blocks)
    assert sum(g.p for g in g_blocks) >= 256 and kept >= 600
    for g in g_blocks:
        assert g.q == len(SHIFTS) and (g.Y == np.ldexp(1.0, np.array(SHIFTS))[None, :]).all()
        for i, j in np.argwhere(g.keep):
            T, exact = _inner_units(g.X[:, i], g.Y[:, j])
            s = SHIFTS[j]
            assert exact and Fraction(T) == Fraction(g.T[i]) * Fraction(2) ** s, (i, j)
            assert same_double(g.want[i, j], B.X.round_nearest_even(Fraction(T, B.ONE)))
            assert np.isfinite(g.want[i, j]) and (g.want[i, j] == 0 or abs(g.want[i, j]) >= 2.0 ** -1022)


def test_planted_g_is_exdot(oracle, g_blocks):
    for g in g_blocks:
        xf, yf = g.X.ravel(), g.Y.ravel()
        for i, j in np.argwhere(g.keep):
            i, j = int(i), int(j)
            got = oracle.exdot(xf, yf, inca=g.p, offa=i, incb=g.q, offb=j, n=g.n)
            assert same_double(got, g.want[i, j]), (i, j, got, g.want[i, j])
            T = g.T[i] << SHIFTS[j] if SHIFTS[j] >= 0 else g.T[i] >> -SHIFTS[j]
            if B.canon_fits(T):
                ref = oracle.exdot(xf, yf, inca=g.p, offa=i, incb=g.q, offb=j, n=g.n, mode=oracle.ROUND_REFERENCE)
                assert same_double(ref, _ref_round(oracle, T)), (i, j, ref)


def test_integer_blocks(oracle):
    c = D.integer_blocks(np.random.default_rng(7), 200, 9, 9)
    for x in (c.X, c.Y):   # m 2^s with |m| < 2^26
        m, e = np.frexp(x)
        assert (np.ldexp(m, 26) == np.rint(np.ldexp(m, 26))).all() and (np.abs(x[x != 0]) >= 2.0 ** -427).all()
    for i, j in c.zeros:
        assert c.G[i, j] == 0 and c.want[i, j] == 0.0 and not np.signbit(c.want[i, j])
    for i, j, t, low in c.ties:
        assert c.G[i, j] == ((1 << 53) + low) * Fraction(2) ** t                 # half a unit in the last place
        assert c.want[i, j] == float(((1 << 53) + low + (1 if low == 3 else -1)) * Fraction(2) ** t)
    assert sum(c.G[i, j] != 0 and Fraction(c.want[i, j]) != c.G[i, j] for i in range(c.p) for j in range(c.q)) > 40
    xf, yf = c.X.ravel(), c.Y.ravel()
    for i in range(c.p):
        for j in range(c.q):
            assert c.G[i, j] == D.exact_inner(c.X[:, i], c.Y[:, j])
            got = oracle.exdot(xf, yf, inca=c.p, offa=i, incb=c.q, offb=j, n=c.n)
            assert same_double(got, c.want[i, j]), (i, j, got, c.want[i, j])
            T = c.G[i, j] * B.ONE
            assert T.denominator == 1
            ref = oracle.exdot(xf, yf, inca=c.p, offa=i, incb=c.q, offb=j, n=c.n, mode=oracle.ROUND_REFERENCE)
            assert same_double(ref, _ref_round(oracle, int(T))), (i, j, ref)
