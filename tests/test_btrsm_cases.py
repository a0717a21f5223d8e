"""CPU suite: the case helpers of the ExBTRSM GPU tests (tests/btrsm_cases.py) against exact_cases.trsv_exact and against
arithmetic done by hand."""
import numpy as np
import pytest

import btrsm_cases as R
import exact_cases as X
import sptrsv_cases as S
from helpers import bits


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
def test_alpha_one_is_trsv_exact_on_every_row(unit):
    """x M = b is M^T x^T = b^T: with alpha = 1 every row is trsv_exact on the logical lower L = M^T"""
    rng = np.random.default_rng([9, int(unit)])
    s = S._system(23, rng, lambda i: np.arange(i))
    B = S.rand53(rng, (6, 23)) * rng.choice((-1.0, 1.0), (6, 23))
    got = R.btrsm_exact(s.L.T, B, 1.0, unit)
    for r in range(6):
        assert (bits(got[r]) == bits(X.trsv_exact(s.L, B[r], unit)[0])).all(), r


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
def test_row_block_is_the_planted_block_transposed(unit):
    """rows of every kind, the planted expectation (the exactly scaled want) included, follow btrsm_exact; the block
    repeats cyclically and a prefix of a taller block is the shorter one"""
    c, blk = R.row_block(0, unit, 7)
    assert blk.B.shape == blk.want.shape == (7, c.n) and blk.kinds[:3] == ["b", "control", "random"] and blk.from_b == 3
    assert (bits(R.btrsm_exact(c.L.T, blk.B, 1.0, unit)) == bits(blk.want)).all()
    for r in range(7):
        assert (bits(X.trsv_exact(c.L, blk.B[r], unit)[0]) == bits(blk.want[r])).all()
    _, tall = R.row_block(0, unit, R.KMAX + 4)
    assert (bits(tall.B[:7]) == bits(blk.B)).all() and (bits(tall.B[R.KMAX:]) == bits(tall.B[:4])).all()
    assert (bits(tall.want[R.KMAX:]) == bits(tall.want[:4])).all() and tall.from_b == 22 + 2


def test_operands_flip_the_trans_of_extrsv():
    """reading the storage as ExBTRSM does -- op(T)(i, j) of the column-major triangle, columns through idx -- gives the
    logical upper M = L^T in every orientation, with NaN wherever nothing may be read"""
    rng = np.random.default_rng(4)
    s = S._system(6, rng, lambda i: np.arange(i))
    M = s.L.T
    for uplo, transt in R.ORIENT:
        for diag in ("N", "U"):
            t, ldt, idx = R.operands(s.L, uplo, transt, diag, ldt_pad=2)
            assert ldt == 8
            T = t.reshape(6, ldt)[:, :6].T                       # T[i, j] of the column-major storage
            op = T.T if transt == "T" else T
            logical = op[np.ix_(idx, idx)]
            tri = np.triu(np.ones((6, 6), dtype=bool), 1 if diag == "U" else 0)
            assert (logical[tri] == M[tri]).all() and np.isnan(logical[~tri]).all(), (uplo, transt, diag)
            forward = (uplo, transt) in (("U", "N"), ("L", "T"))
            assert (idx == (np.arange(6) if forward else np.arange(5, -1, -1))).all()
            assert np.isnan(t.reshape(6, ldt)[:, 6:]).all()


def test_alpha_scales_exactly_and_zero_does_not_read_b():
    rng = np.random.default_rng(11)
    s = S._system(9, rng, lambda i: np.arange(i))
    B = S.rand53(rng, (3, 9)) * rng.choice((-1.0, 1.0), (3, 9))
    one = R.btrsm_exact(s.L.T, B)
    for e in (-7, 1, 30):
        assert (bits(R.btrsm_exact(s.L.T, B, 2.0 ** e)) == bits(one * 2.0 ** e)).all()
        assert (bits(R.btrsm_exact(s.L.T, B * 2.0 ** e)) == bits(one * 2.0 ** e)).all()
    assert (bits(R.btrsm_exact(s.L.T, B, -1.0)) == bits(-one)).all()
    zero = R.btrsm_exact(s.L.T, np.full((2, 9), np.nan), 0.0)
    assert (zero == 0.0).all() and not np.signbit(zero).any()    # + 0 over a positive diagonal
    M = s.L.T.copy()
    M[4, 4] = -M[4, 4]
    zero = R.btrsm_exact(M, np.full((1, 9), np.nan), 0.0)
    assert (zero == 0.0).all() and np.signbit(zero[0]).tolist() == [j == 4 for j in range(9)]
    # alpha that is no power of two: the product alpha * b enters exactly
    got = R.btrsm_exact(np.eye(1), np.array([[3.0]]), 0.1, True)
    assert got[0, 0] == 0.30000000000000004 and got[0, 0] == 0.1 * 3.0


def test_the_error_term_of_alpha_b_decides():
    got = R.btrsm_exact(R.ERR_M, R.ERR_B[None, :], R.ERR_ALPHA, True)[0]
    assert (got == R.ERR_WANT).all() and got[0] == 2.0 ** 54 + 2.0 ** 28 and got[1] == 1.0
    rounded_first = R.btrsm_exact(R.ERR_M, (R.ERR_ALPHA * R.ERR_B)[None, :], 1.0, True)[0]
    assert rounded_first[0] == R.ERR_WANT[0] and rounded_first[1] == 0.0     # what the construction tells apart
    M, b, want = R.embedded_error_term()
    assert M.shape == (70, 70) and (np.triu(M) == M).all() and (np.diag(M) == 1.0).all()
    assert want[62] == want[63] == R.ERR_WANT[0] and want[64] == want[65] == 1.0
    rest = np.ones(70, dtype=bool)
    rest[[62, 63, 64, 65]] = False
    assert (want[rest] == R.ERR_ALPHA * b[rest]).all()            # exact: small integers times 2^27 + 1


def test_overflow_rounds_to_infinity_and_division_by_zero_is_ieee():
    big = float(2 ** 1023)
    got = R.btrsm_exact(np.array([[1.0, -1.0], [0.0, 1.0]]), np.array([[big, big]]), 1.0, True)[0]
    assert got[0] == big and got[1] == np.inf
    got = R.btrsm_exact(np.array([[0.0]]), np.array([[1.0], [-1.0], [0.0]]).reshape(3, 1))
    assert got[0, 0] == np.inf and got[1, 0] == -np.inf and np.isnan(got[2, 0])
