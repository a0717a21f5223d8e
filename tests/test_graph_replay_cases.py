"""The builders of tests/graph_replay_cases.py without a GPU: every case is built (the builders assert that results are
finite, that ties are present and that the data changes from call to call), the exact-scaling argument behind the
right-hand sides is checked against trsv_exact itself, and the planted and the oracle's ExBDOT expectations against
Fractions."""
from fractions import Fraction

import numpy as np
import pytest

import bdot_cases as D
import exact_cases as X
import graph_replay_cases as G
import sptrsv_cases as S
from helpers import bits


@pytest.mark.parametrize("tris,sets,ks", [(G.dense_triangles, G.dense_sets, (65, 9)), (G.sparse_triangles, G.sparse_sets, (1, 65, 9))],
                         ids=["dense", "sparse"])
def test_solve_sets_carry_ties_and_change_from_call_to_call(tris, sets, ks):
    t0, t1 = tris()
    assert t0.n == t1.n and t0.ties >= 10 and t0.pool[0][2] and not any(c[2] for c in t0.pool[1:])
    for k in ks:
        six = sets(k)
        assert [s[0] for s in six] == list(G.TRIANGLE_OF_CALL)
        assert all(s[1].shape == (t0.n, k) == s[2].shape for s in six)
        # the planted b (ties) is in the first replay's block, on the planted triangle
        assert six[0][3] >= 1 and six[0][3] == sum(G.column(t0, j, 0)[2] for j in range(k))
        for a in range(6):
            for b in range(a):
                assert (bits(six[a][1]) != bits(six[b][1])).mean() > 0.99, (k, a, b)


@pytest.mark.parametrize("tris", [G.dense_triangles, G.sparse_triangles], ids=["dense", "sparse"])
def test_scaled_columns_are_what_trsv_exact_gives(tris):
    """one column per pool entry and triangle, at the call and position where its scale is not 1: the scaled solution is
    trsv_exact's of the scaled right-hand side, bit for bit (and on the planted b every tie is still a tie: the totals
    scale exactly)"""
    checked = 0
    for tri in tris():
        P = len(tri.pool)
        for i in range(P):
            r = 3
            j = next(j for j in range(4 * P) if (j + 2 * r) % P == i and G.SCALES[(j // P + r) % len(G.SCALES)] != 0)
            b, want, tie = G.column(tri, j, r)
            assert tie == tri.pool[i][2] and (bits(b) != bits(tri.pool[i][0])).all()
            got, totals = X.trsv_exact(tri.L, b)
            assert (bits(got) == bits(want)).all(), (i, j)
            if i == 0 and tri.ties:
                base = X.trsv_exact(tri.L, tri.pool[0][0])[1]
                s = b[0] / tri.pool[0][0][0]
                assert all(t == u * Fraction(s) for t, u in zip(totals, base))
            checked += 1
    assert checked >= 9


@pytest.mark.parametrize("uplo", ["L", "U"])
def test_sparse_csr_pairs_share_a_budget_and_cover_both_row_classes(uplo):
    budget = G.sparse_budget(uplo)
    seen = []
    for t in (0, 1):
        crow, col, val, idx, skipped = G.sparse_csr(t, uplo)
        pc, pcol, pval = G.padded_csr(t, uplo)
        assert len(pcol) == len(pval) == budget and int(pc[-1]) == len(col) <= budget and pc.dtype == pcol.dtype
        dense, outside = S.densify(crow, col, val, uplo)
        assert (bits(dense) == bits(np.tril(G.sparse_triangles()[t].L))).all() and len(outside) == skipped
        assert all(np.isnan(v) for _, _, v in outside)
        seen.append(np.diff(crow))
    assert seen[0].max() <= 64 < seen[1].max() and not np.array_equal(seen[0], seen[1])


def test_planted_bdot_pairs_against_fractions():
    Xg, Yg, wg = G.planted_g_pair()
    assert Xg.shape == Yg.shape == (G.BDOT_N, G.BDOT_G) and np.isfinite(wg).all()
    for i, j in ((0, 0), (3, 64), (64, 0), (64, 64), (17, 33), (40, 5)):
        assert bits(np.array(X.round_nearest_even(D.exact_inner(Xg[:, i], Yg[:, j]))))[()] == bits(wg)[i, j], (i, j)
    Xd, Yd, wd = G.planted_d_pair()
    assert Xd.shape == Yd.shape == (G.BDOT_N, G.BDOT_D) and wd.shape == (G.BDOT_D,)
    for j in range(G.BDOT_D):
        assert bits(np.array(X.round_nearest_even(D.exact_inner(Xd[:, j], Yd[:, j]))))[()] == bits(wd)[j], j
    # ties: exact totals that lie half way between two doubles
    halves = 0
    for j in range(G.BDOT_D):
        T = D.exact_inner(Xd[:, j], Yd[:, j])
        if T and np.isfinite(wd[j]) and wd[j] != 0.0:
            lo, hi = sorted((Fraction(float(wd[j])), Fraction(float(np.nextafter(wd[j], np.inf if T > wd[j] else -np.inf)))))
            halves += (T - lo) * 2 == hi - lo
    assert halves >= 5


@pytest.mark.parametrize("mode", ["G", "D"])
def test_bdot_sets_against_fractions(oracle, mode):
    """the oracle's expectations of the unplanted pairs, sampled, against Fraction sums"""
    sets = G.bdot_sets(mode)
    assert len(sets) == 4 and G.BDOT_KINDS[1] is None
    p = G.BDOT_G if mode == "G" else G.BDOT_D
    for r in (0, 2, 3):
        Xr, Yr, want = sets[r]
        for i, j in ((0, 0), (p - 1, p - 1), (7, 64)):
            j = j if mode == "G" else i
            w = want[i, j] if mode == "G" else want[i]
            assert bits(np.array(X.round_nearest_even(D.exact_inner(Xr[:, i], Yr[:, j]))))[()] == bits(np.array(w))[()], (r, i, j)


def test_bdot_uneven_sets_against_fractions(oracle):
    sets = G.bdot_uneven_sets()
    assert len(sets) == 4 and all(s[0].shape == (G.BDOT_N, G.UNEVEN_P) and s[1].shape == (G.BDOT_N, G.UNEVEN_Q) for s in sets)
    for r, (Xr, Yr, want) in enumerate(sets):
        for i, j in ((0, 0), (63, 2), (64, 0), (66, 2)):
            assert bits(np.array(X.round_nearest_even(D.exact_inner(Xr[:, i], Yr[:, j]))))[()] == bits(want)[i, j], (r, i, j)
