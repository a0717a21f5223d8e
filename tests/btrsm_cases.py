"""Cases for the ExBTRSM tests: the exact right-side substitution, and the planted ExTRSV systems as blocks of rows.

ExBTRSM solves X op(T) = alpha B row by row; in substitution order op(T) is a logical UPPER triangle M, and row r is
    x_j = Round(alpha b_j - sum_{i < j} x_i M[i, j]) / M[j, j].
That is ExTRSV's substitution on the logical lower system L = M^T, so the planted systems of exact_cases.planted_trsv
serve as they are: a block of right-hand-side columns of sptrsm_cases.planted_block, transposed, is a block of rows here
(row_block repeats them cyclically to reach a wanted n), and ExTRSV's operands for (uplo, trans) are ExBTRSM's for (uplo,
the other trans).  Nothing here calls the code under test."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import exact_cases as X
from helpers import bits
from sptrsm_cases import planted_block

KMAX = 65                              # the width of the planted blocks that the ExTRSM tests build too (one cache)
ORIENT = (("U", "N"), ("L", "T"), ("L", "N"), ("U", "T"))     # (uplo, transt): the first two run forward


def flip(trans):
    return "T" if trans in ("N", "n") else "N"


def _round(total):
    """the one rounding of an exact total: float() of a Fraction rounds to nearest even; beyond the range it is +-inf"""
    try:
        return float(total)
    except OverflowError:
        return float("inf") if total > 0 else float("-inf")


def btrsm_exact(M, B, alpha=1.0, unit=False):
    """Plain Fraction substitution per row for the logical upper system x M = alpha b (M: p x p, its upper triangle; B:
    n x p in substitution order).  The total alpha b_j - sum_{i<j} x_i M[i, j] is exact (alpha b_j as the exact product,
    B not read for alpha == 0), rounded once by float(), then divided as the quotient of two doubles (not under `unit`).
    Zero entries of M are skipped, so a non-finite x_i may only sit where nothing consumes it."""
    M, B = np.asarray(M, dtype=np.float64), np.atleast_2d(np.asarray(B, dtype=np.float64))
    n, p = B.shape
    out = np.zeros((n, p))
    cols = [np.nonzero(M[:j, j])[0].tolist() for j in range(p)]
    fa = Fraction(float(alpha))
    with np.errstate(all="ignore"):
        for r in range(n):
            xf = [None] * p
            for j in range(p):
                total = fa * Fraction(float(B[r, j])) if alpha != 0.0 else Fraction(0)
                for i in cols[j]:
                    if xf[i] is None:
                        xf[i] = Fraction(float(out[r, i]))
                    total -= xf[i] * Fraction(float(M[i, j]))
                v = np.float64(_round(total))
                out[r, j] = v if unit else v / np.float64(M[j, j])
    return out


def row_block(case, unit, n):
    """n rows for the planted system TRSV_CASES[case]: the KMAX columns of its planted block as rows, repeated
    cyclically.  Returns c (the system; the logical upper triangle is c.L.T) and B, want (n x p), kinds (per row) and
    from_b, the number of rows that derive from the planted b."""
    c, blk = planted_block(case, unit, KMAX)
    pick = np.arange(n) % KMAX
    kinds = [blk.kinds[k] for k in pick]
    return c, SimpleNamespace(B=np.ascontiguousarray(blk.B.T[pick]), want=np.ascontiguousarray(blk.want.T[pick]),
                              kinds=kinds, from_b=sum(kd == "b" for kd in kinds), n=n)


def operands(L, uplo, transt, diag="N", ldt_pad=0):
    """ExBTRSM's triangle for the logical lower system L (the logical upper M = L^T) under (uplo, transt): ExTRSV's
    storage for (uplo, the other trans), NaN in everything that must not be read.  Returns (t, ldt, idx): column-major
    storage, and logical column j of a row is physical column idx[j]."""
    p = np.asarray(L).shape[0]
    t, ldt, _, idx = X.trsv_operands(L, np.zeros(p), uplo, flip(transt), diag, lda_pad=ldt_pad)
    return t, ldt, idx


def solve_rows(call, info, B, idx, pad=0, sentinel=-7.25):
    """logical B (n x p) in, logical X out, and the counters.  call(x) solves the device block x in place and returns it;
    info() returns the counters; logical column j is physical column idx[j]; pad: X is the view [:, :p] of a block pad
    columns wider, filled with the sentinel"""
    import torch
    B = np.asarray(B)
    n, p = B.shape
    wide = np.full((n, p + pad), sentinel)
    wide[:, idx] = B
    full = torch.from_numpy(wide).cuda()
    x = full[:, :p] if pad else full
    out = call(x)
    assert out is x
    counters = info()
    back = full.cpu().numpy()
    if pad:
        assert (bits(back[:, p:]) == bits(np.full((n, pad), sentinel))).all(), "the padding was written"
    return back[:, idx], counters


# the error term of alpha * b: unit diagonal, T = [[1, 1], [0, 1]] upper, alpha = b_0 = b_1 = 2^27 + 1.  x_0 =
# Round((2^27 + 1)^2) = 2^54 + 2^28 (the 1 is lost), x_1 = (2^27 + 1)^2 - x_0 = 1 exactly; a routine that rounds alpha * b
# before it sums gives x_1 = 0
ERR_ALPHA = float(2 ** 27 + 1)
ERR_M = np.array([[1.0, 1.0], [0.0, 1.0]])
ERR_B = np.array([ERR_ALPHA, ERR_ALPHA])
ERR_WANT = np.array([float(2 ** 54 + 2 ** 28), 1.0])


def embedded_error_term(p=70, at=(62, 63, 64, 65)):
    """the same construction inside a p x p unit upper triangle, twice: M[at0, at3] = M[at1, at2] = 1 (identity
    elsewhere), b = ERR_ALPHA in those four columns and j + 1 elsewhere.  With at = 62..65 the dependencies cross the
    64-column seam.  Returns (M, b, want) with want from btrsm_exact"""
    M = np.eye(p)
    M[at[0], at[3]] = 1.0
    M[at[1], at[2]] = 1.0
    b = np.arange(1.0, p + 1.0)
    b[list(at)] = ERR_ALPHA
    want = btrsm_exact(M, b[None, :], ERR_ALPHA, True)[0]
    assert want[at[0]] == want[at[1]] == ERR_WANT[0] and want[at[2]] == want[at[3]] == 1.0
    return M, b, want
