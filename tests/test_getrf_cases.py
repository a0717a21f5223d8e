"""CPU suite: the models of getrf_cases held to their claims.  Nothing here calls the library."""
import math

import numpy as np
import pytest

import bjacobi_cases as J
import getrf_cases as G

try:
    from scipy.linalg import lu_factor as _lu_factor
except ImportError:                      # the numpy restatement below serves
    _lu_factor = None


def _split(W):
    return np.tril(W, -1) + np.eye(W.shape[0]), np.triu(W)


def _permuted(A, ipiv):
    PA = np.array(A, copy=True)
    for j, pv in enumerate(ipiv):
        PA[[j, pv - 1]] = PA[[pv - 1, j]]
    return PA


def _plain_pivots(A):
    """partial pivoting in fp64 (what LAPACK's unblocked LU does), 1-based"""
    W = np.array(A, dtype=np.float64, copy=True)
    p = W.shape[0]
    ipiv = np.arange(1, p + 1)
    for j in range(p):
        piv = j + int(np.argmax(np.abs(W[j:, j])))
        ipiv[j] = piv + 1
        W[[j, piv]] = W[[piv, j]]
        W[j + 1:, j] /= W[j, j]
        W[j + 1:, j + 1:] -= np.outer(W[j + 1:, j], W[j, j + 1:])
    return ipiv


@pytest.mark.parametrize("p", [1, 2, 5, 16, 33, 64])
def test_p_a_equals_l_u_to_a_few_ulps_and_pivots_are_lapacks(p):
    for seed in (0, 1):
        A = G.random_matrix(p, seed)
        W, ipiv, info = G.getrf_exact(A)
        assert info == 0 and (np.abs(np.tril(W, -1)) <= 1.0).all()
        L, U = _split(W)
        err = np.abs(L @ U - _permuted(A, ipiv)).max()
        # every entry of L U - P A is a sum of at most p roundings of partial sums bounded by the growth of U
        assert err <= 4 * p * np.abs(U).max() * 2.0 ** -53, (p, seed, err)
        # |c| has no near-ties on random full-mantissa matrices: any correct partial pivoting picks the same rows
        if _lu_factor is not None:
            assert (_lu_factor(A)[1] + 1 == ipiv).all()
        assert (_plain_pivots(A) == ipiv).all()
        Wp, ipp, infop = G.plain_getrf(A)
        assert infop == 0 and (ipp == ipiv).all() and np.abs(Wp - W).max() <= 64 * p * np.abs(U).max() * 2.0 ** -53


@pytest.mark.parametrize("p", [1, 2, 3, 4, 5, 7, 8])
def test_the_two_restatements_agree(p):
    for e in G.factor_seven(p)[:5]:      # the finite ones
        W, ipiv, info = G.restate(e.A)
        assert G.J_same(W, e.W) and (ipiv == e.ipiv).all() and info == e.info, (p, e.name)


@pytest.mark.parametrize("p,rows", [(4, 1), (7, 3), (16, 9), (33, 20)])
def test_a_block_padded_with_an_identity_factors_to_the_leading_part(p, rows):
    """[[A, 0], [0, I]]: the leading rows x rows part of W and the first rows pivots are those of A alone"""
    A = G.random_matrix(rows, 7)
    D = np.eye(p)
    D[:rows, :rows] = A
    W, ipiv, info = G.getrf_exact(D)
    Wa, ipa, infa = G.getrf_exact(A)
    assert info == infa == 0
    assert G.J_same(W[:rows, :rows], Wa) and (ipiv[:rows] == ipa).all() and (ipiv[rows:] == np.arange(rows + 1, p + 1)).all()
    assert (W[rows:, rows:] == np.eye(p - rows)).all() and (W[:rows, rows:] == 0).all() and (W[rows:, :rows] == 0).all()


@pytest.mark.parametrize("p", [1, 2, 3, 9, 16, 40])
def test_breakdown_rule(p):
    seven = G.factor_seven(p)
    for e in seven[4:]:
        j = e.info - 1
        assert j >= 0 and (e.ipiv[j:] == np.arange(j + 1, p + 1)).all(), e.name
        # the candidates are stored in column j, rows j .. p - 1; to the right of column j the rows are original entries in
        # the row order reached so far, with the rows of U above
        cand = e.W[j:, j]
        assert all(c == 0 or math.isnan(c) for c in cand) or any(math.isnan(c) for c in cand), e.name
        PA = np.array(e.A, copy=True)
        for s in range(j):
            PA[[s, e.ipiv[s] - 1]] = PA[[e.ipiv[s] - 1, s]]
        assert G.J_same(e.W[j:, j + 1:], PA[j:, j + 1:]), e.name
        assert e.roundings == G.roundings(p, e.info)
    z = seven[4]
    assert (z.W[z.info - 1:, z.info - 1] == 0).all() and not np.signbit(z.W[z.info - 1:, z.info - 1]).any()
    # an infinite pivot is no breakdown: IEEE arithmetic goes on (Inf / Inf and 0 * Inf are NaN)
    if p >= 2:
        A = G.dominant(p)
        A[0, 0] = np.inf
        W, ipiv, info = G.getrf_exact(A)
        assert ipiv[0] == 1 and W[0, 0] == np.inf and (W[1:, 0] == 0).all() and info == 0
        assert np.isfinite(W.ravel()[1:]).all()
        A[1, 0] = np.inf                 # the first of two infinite candidates wins; Inf / Inf = NaN meets step 1
        W, ipiv, info = G.getrf_exact(A)
        assert ipiv[0] == 1 and math.isnan(W[1, 0]) and info == 2 and math.isnan(W[1, 1])
    # a signed zero pivot
    for z0 in (0.0, -0.0):
        W, ipiv, info = G.plain_getrf(np.array([[z0]]))
        assert info == 1 and W[0, 0] == 0 and np.signbit(W[0, 0]) == np.signbit(z0)
        W, ipiv, info = G.getrf_exact(np.array([[z0]]))
        assert info == 1 and W[0, 0] == 0 and not np.signbit(W[0, 0])     # an exact zero total rounds to + 0


def test_counter_formula_and_pivot_tie():
    for p in (1, 2, 5, 16):
        assert G.roundings(p, 0) == p * p
        assert G.roundings(p, 1) == p
        assert G.roundings(p, p) == p * p    # a breakdown at the last step: only its one candidate is left
    assert G.roundings(5, 3) == 9 + 7 + 3
    for p in (2, 3, 8, 33):
        e = G.factor_seven(p)[3]
        lo = 0 if p == 2 else p // 2
        assert e.info == 0 and e.ipiv[0] == lo + 1 and e.W[0, 0] == -0.75
        assert (np.abs(e.A[:, 0]) == 0.75).sum() == 2


@pytest.mark.parametrize("p", [9, 17, 40, 63, 64])
def test_planted_ties_and_batches(p):
    c = G.planted(p)
    assert c.ties >= 1 and (c.ipiv == np.arange(1, p + 1)).all() and (c.ipiv_shuffled != c.ipiv).any()
    for batch in J.batches(p)[:4]:
        A, W, ipiv, info, ent = G.factor_batch(p, batch)
        assert A.shape == W.shape == (batch, p, p) and sum(e.ties for e in ent) >= 1
        assert len({e.name for e in ent}) == min(batch, 7)


@pytest.mark.parametrize("p", [1, 2, 7, 16])
def test_getrs_model_solves_and_skips_pivots_out_of_range(p):
    n, k = 6 * p + p // 2, 7                 # six whole blocks (the hand-made one is the sixth) and a short one
    LU, ipiv, X0, want, ties = G.solve_case(p, n, k)
    for b in range(-(-n // p)):
        rows = min(p, n - b * p)
        blk = G.solve_seven(p)[b % 7]
        L, U = _split(blk.LU[:rows, :rows])
        if rows == p and b % 7 != 5:
            PB = _permuted(X0[b * p:b * p + rows], ipiv[b][:rows])
            res = np.abs(L @ U @ want[b * p:b * p + rows] - PB).max()
            assert res <= 1e-9 * max(1.0, np.abs(want[b * p:b * p + rows]).max()), (p, b, res)
        for j in range(k):
            x = G.plain_getrs(LU[b], ipiv[b], X0[b * p:b * p + rows, j])
            assert np.allclose(x, want[b * p:b * p + rows, j], rtol=1e-6, atol=1e-9)
    if p >= 2:
        assert ties >= 1
        x, t = G.getrs_model(G.solve_seven(p)[5].LU, G.solve_seven(p)[5].ipiv, G.solve_seven(p)[5].B[:, 0])
        assert t == 1 and x[0] == 1.0 - 2.0 ** -53 and x[1] == 1.0
    # garbage pivots move nothing
    b = np.arange(1.0, p + 1.0)
    x, _ = G.getrs_model(np.eye(p), np.full(p, 2 ** 31 - 1, dtype=np.int64), b)
    assert (x == b).all()
    x, _ = G.getrs_model(np.eye(p), np.full(p, 0), b)
    assert (x == b).all()


def test_chain_matrix_is_nonsymmetric_and_its_blocks_factor():
    A = G.convection_diffusion(6)
    assert (A != A.T).any() and (np.count_nonzero(A, axis=1) <= 5).all()
    X0 = np.random.default_rng(3).random((36, 2)) - 0.5
    for p in (4, 7):
        W, ipiv, X = G.chain_model(A, p, X0)
        D = J.diag_blocks(A, p)
        for b in range(D.shape[0]):
            r = min(p, 36 - b * p)
            assert np.allclose(D[b][:r, :r] @ X[b * p:b * p + r], X0[b * p:b * p + r], rtol=1e-10, atol=1e-12)
