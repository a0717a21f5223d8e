"""CPU suite: the constructions of potrf_cases hold their claims, the Fraction factorisation agrees with a second
restatement, and the cases bite: a factorisation that rounds its products (numpy's) misses them."""
import math

import numpy as np
import pytest

import potrf_cases as P

SIZES = tuple(P.BLOCKS)


def test_two_by_two_case_and_its_sibling():
    R, info = P.potrf_exact(P.G2)
    assert info == 0 and R[0, 0] == 1.0 and R[0, 1] == P.A2 and R[1, 1] == math.sqrt(3.0)
    assert R[1, 0] == P.A2                                   # the other triangle comes back as it was
    L, info = P.potrf_exact(P.G2, "L")
    assert info == 0 and L[1, 0] == P.A2 and L[1, 1] == math.sqrt(3.0) and L[0, 1] == P.A2
    assert np.linalg.cholesky(P.G2)[1, 1] == 2.0             # a^2 rounded first: 4, not 3
    R, info = P.potrf_exact(P.G7)
    assert info == 0 and R[1, 1] == math.sqrt(7.0)
    assert int(P.A7) ** 2 + 7 == int(P.G7[1, 1]) and float(int(P.A7) ** 2) == P.G7[1, 1]   # the rounded product is g
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(P.G7)
    for at in ((2, 3), (3, 4), (3, 5), (62, 63), (63, 64), (64, 65), (60, 69)):
        for g2, rad in ((P.G2, 3.0), (P.G7, 7.0)):
            R, info = P.potrf_exact(P.embedded(70, at, g2))
            assert info == 0 and R[at[1], at[1]] == math.sqrt(rad) and R[at[0], at[1]] == g2[0, 1]


@pytest.mark.parametrize("p", SIZES)
def test_planted_systems_hold_their_claims(p):
    """(the builder asserts class and rounding of every plant while it refactors the doubles)"""
    c = P.planted(p)
    assert c.info == 0 and c.G.shape == (p, p) and (c.G == c.G.T).all() and np.isfinite(c.G).all()
    cols = sorted(col for _, col, *_ in c.plants)
    assert len(set(cols)) == len(cols)                       # one planted total per column
    assert len(cols) == sum(P.BLOCKS[p])
    ties = sum(n for cls, n in c.counts.items() if cls.split(":")[-1] in ("tie", "tie_odd", "carry"))
    assert (c.kind == P.TIE).sum() >= ties > 0
    pure = P.planted(p, True)
    assert not (pure.kind == P.NEAR).any() and not any("near" in cls for cls in pure.counts)
    assert (pure.kind == P.TIE).sum() >= ties
    assert ((pure.kind != 0) == np.triu(np.ones((p, p), dtype=bool))).all()


def test_every_class_is_planted_off_the_diagonal_and_on_it():
    tot = {}
    for p in SIZES:
        for cls, n in P.planted(p).counts.items():
            tot[cls] = tot.get(cls, 0) + n
    for cls in P.OFF_SEQ:
        assert tot.get(cls, 0) >= 30, (cls, tot)
    for cls in ("tie", "tie_odd", "carry", "near", "ctrl+", "ctrl-"):
        assert tot.get("d:" + cls, 0) >= 1, (cls, tot)
    gaps = {(cls, gap) for p in SIZES for _, _, cls, gap, _ in P.planted(p).plants if "near" in cls}
    for g in P.GAPS:
        assert ("near+", g) in gaps and ("near-", g) in gaps
    assert len({g for cls, g in gaps if cls == "d:near"}) >= 2


def test_numpy_misses_planted_outputs_of_every_tie_class():
    missed = {}
    for p in SIZES:
        c = P.planted(p)
        L = np.linalg.cholesky(c.G).T
        for r, col, cls, _, _ in c.plants:
            if L[r, col] != c.R[r, col]:
                missed[cls.split(":")[-1]] = missed.get(cls.split(":")[-1], 0) + 1
    for cls in ("tie", "tie_odd", "carry"):
        assert missed.get(cls, 0) >= 1, missed


@pytest.mark.parametrize("p", [1, 2, 5, 9, 17])
def test_potrf_exact_agrees_with_the_plain_restatement(p):
    for G in (P.gram(p), P.gram(p, bits=20), P.banded(p) if p > 2 else P.gram(p, 3)):
        for uplo in ("U", "L"):
            R, info = P.potrf_exact(G if uplo == "U" else G.T.copy(), uplo)
            R2, info2 = P.restate(G)
            assert info == info2 == 0
            tri = np.triu(R) if uplo == "U" else np.tril(R).T
            assert (tri.view(np.int64) == np.triu(R2).view(np.int64)).all()
    G = P.breakdown(max(p, 2), max(p, 2) - 1, "neg")
    R, info = P.potrf_exact(G)
    R2, info2 = P.restate(G)
    assert info == info2 == max(p, 2) and (R.view(np.int64) == R2.view(np.int64)).all()


@pytest.mark.parametrize("p", [8, 16, 40])
def test_factor_reproduces_g_and_numpy_differs_in_bits(p):
    G = P.gram(p)
    R, info = P.potrf_exact(G)
    assert info == 0
    U = np.triu(R)
    assert np.allclose(U.T @ U, G, rtol=1e-12, atol=0.0)
    N = np.linalg.cholesky(G).T
    assert np.allclose(np.triu(N), U, rtol=1e-9)
    iu = np.triu_indices(p)
    assert (N[iu] != U[iu]).mean() > 0.05                     # plain fp64 sums give other bits


@pytest.mark.parametrize("what", ["zero", "neg", "nan"])
def test_breakdown_cases(what):
    for p in (66, 70):
        for j in P.breakdown_pivots(p):
            G = P.breakdown(p, j, what)
            R, info = P.potrf_exact(G)
            assert info == j + 1
            v = R[j, j]
            assert (v == 0.0) if what == "zero" else (v == -1.0) if what == "neg" else math.isnan(v)
            # row j beyond the diagonal and the later rows are as they were; the earlier rows were fixed
            assert (R[j, j + 1:] == G[j, j + 1:]).all() and (R[j + 1:, :] == G[j + 1:, :]).all()
            assert P.fixed_entries(p, info) == sum(p - r for r in range(j)) + 1
    assert P.fixed_entries(5, 0) == 15
