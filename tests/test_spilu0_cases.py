"""The ExSpILU0 cases hold what the GPU tests rely on (CPU only): the model against getrf_exact and against a naive
restatement, the planted classes, the cancellation pivot, the defects, and that the cases can see a routine that rounds
every product or breaks ties away from even."""
import numpy as np
import pytest

import exact_cases as E
import getrf_cases as G
import spilu0_cases as S
from helpers import assert_bits, bits


@pytest.mark.parametrize("p", [24, 64])
def test_model_equals_getrf_exact_where_pivoting_never_swaps(p):
    csr, A = S.dense(p)
    W, ipiv, info = G.getrf_exact(A)
    assert info == 0 and (ipiv == np.arange(1, p + 1)).all(), "partial pivoting swapped"
    lu, i0, i1 = S.ilu0_exact(*csr)
    assert (i0, i1) == (0, 0)
    assert_bits(lu.reshape(p, p), W, p)


@pytest.mark.parametrize("name", S.SMALL)
def test_model_equals_the_naive_restatement(name):
    lu, i0, i1, _ = S.expected(name)
    assert (i0, i1) == (0, 0)
    assert_bits(lu, S.restate(*S.SOUND[name]()), name)


def test_every_builder_is_sound_sorted_and_has_its_diagonal():
    for name, make in S.SOUND.items():
        crow, col, val = make()
        m = len(crow) - 1
        assert S.structure(crow, col, m) == 0, name
        assert crow[0] == 0 and crow[-1] == len(col) == len(val), name
    crow = S.arrow_band()[0]
    assert sorted(np.diff(crow)[-3:].tolist()) == [65, 130, S.MAX_ROW]
    assert np.diff(S.random_pattern()[0]).mean() > 7


def test_planted_classes_and_the_cancellation_pivot():
    lu, i0, i1, d = S.expected("planted")
    assert (i0, i1) == (0, 0) and np.isfinite(lu).all()
    assert min(d.ties_l, d.ties_u, d.nears_l, d.nears_u) >= 16, vars(d)
    crow, col, _ = S.zero_pivot()
    lu, i0, i1, _ = S.expected("zero_pivot")
    assert (i0, i1) == (0, 5)
    assert lu[int(crow[4]) + 1] == 0.0 and col[int(crow[4]) + 1] == 4, "the pivot of row 4 is not exactly zero"
    assert not np.isfinite(lu[int(crow[5]):]).all()
    lu, i0, i1, _ = S.expected("nonfinite")
    assert i0 == 0 and np.isnan(lu).any()


def test_the_cases_see_rounded_products_and_ties_broken_away_from_even():
    csr = S.planted()
    want = S.expected("planted")[0]
    each = S.ilu0_exact(*csr, round_products=True)[0]
    away = S.ilu0_exact(*csr, rounder=S.round_away)[0]
    assert (bits(each) != bits(want)).any(), "rounding every product goes unseen"
    assert (bits(away) != bits(want)).any(), "ties broken away from even go unseen"
    plain = S.plain_ilu0(*csr)
    assert (bits(plain) != bits(want)).any(), "the plain fp64 form goes unseen"


def test_defects_name_their_first_row():
    want = {"row_ptr decreasing": 5, "column past the end": 7, "negative column": 4, "columns not ascending": 8,
            "duplicate column": 10, "no stored diagonal": 9, "a row of 513 entries": 516}
    cases = S.defects()
    assert set(cases) == set(want)
    for name, (crow, col, val) in cases.items():
        lu, i0, i1 = S.ilu0_exact(crow, col, val)
        assert i0 == want[name] and i1 == 0, (name, i0)
        assert_bits(lu, val, name)
    assert np.diff(cases["a row of 513 entries"][0]).max() == S.MAX_ROW + 1


def test_the_chain_on_the_tridiagonal_case():
    """trsv_exact applied twice to the densified factor: L y = b with the unit diagonal, then U x = y"""
    crow, col, _ = S.tridiagonal()
    lu = S.expected("tridiagonal")[0]
    m = len(crow) - 1
    b = np.random.default_rng(11).random(m) - 0.5
    x = S.apply_exact(crow, col, lu, b)
    D = S.dense_of(crow, col, lu)
    y, _ = E.trsv_exact(np.tril(D, -1) + np.eye(m), b, unit=True)
    # the upper sweep by hand: rows m - 1 .. 0 of a bidiagonal U
    z = np.zeros(m)
    from fractions import Fraction
    for i in range(m - 1, -1, -1):
        t = Fraction(float(y[i]))
        if i + 1 < m:
            t -= Fraction(float(D[i, i + 1])) * Fraction(float(z[i + 1]))
        z[i] = E.round_nearest_even(t) / D[i, i]
    assert_bits(x, z, "chain")
    r = np.abs(S.dense_of(crow, col, S.tridiagonal()[2]) @ x - b).max()
    assert r < 1e-12, r          # ILU(0) of a tridiagonal matrix is its LU: the chain solves the system
