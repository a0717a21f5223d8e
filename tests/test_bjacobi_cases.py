"""CPU suite: the builders and models of bjacobi_cases hold what the GPU tests of the batched ExPOTRF / ExPOTRS rely on."""
import math

import numpy as np
import pytest

import bjacobi_cases as J
import exact_cases as E
import potrf_cases as P


@pytest.mark.parametrize("q,ties,near", [(9, 4, 0), (17, 4, 1), (32, 11, 3), (40, 16, 9)])
def test_leading_parts_of_the_planted_system_factor_to_leading_parts(q, ties, near):
    G, R, t, nr = J.planted_lead(q)
    assert (t, nr) == (ties, near)
    R2, info, d = P.potrf_exact(G, "U", detail=True)
    assert info == 0 and (np.triu(R2).view(np.int64) == np.triu(R).view(np.int64)).all()
    assert int((d.kind == P.TIE).sum()) == ties and int((d.kind == P.NEAR).sum()) == near


def test_planted_64_serves_the_widest_block():
    G, R, ties, _ = J.planted_lead(64)
    assert ties >= 16 and G.shape == (64, 64)
    G, R, ties63, _ = J.planted_lead(63)
    R2, info = P.potrf_exact(G, "U")
    assert info == 0 and (np.triu(R2).view(np.int64) == np.triu(R).view(np.int64)).all() and ties63 >= 16


def test_leading_part_of_a_gram_factor_is_the_factor_of_the_leading_part():
    G, R, _ = J.gram64(0)
    for q in (1, 5, 17):
        R2, info = P.potrf_exact(G[:q, :q], "U")
        assert info == 0 and (np.triu(R2).view(np.int64) == np.triu(R[:q, :q]).view(np.int64)).all()


@pytest.mark.parametrize("p", J.SIZES)
def test_the_seven_matrices_are_distinct_and_cover_the_kinds(p):
    seven = J.factor_seven(p)
    assert len(seven) == 7
    infos = [e.info for e in seven]
    assert infos[-1] == 1 and infos[4] >= 1 and sum(1 for i in infos if i == 0) == 5
    keys = {np.nan_to_num(e.G, nan=-7.0).tobytes() for e in seven}
    assert len(keys) == 7 or p == 1                                # (one entry: a breakdown at 0 can repeat a value)
    for e in seven:
        assert e.fixed == P.fixed_entries(p, e.info) and e.G.shape == (p, p)
        if e.info == 0:
            assert (np.diag(e.R) > 0).all()
    if p >= 9:
        assert seven[1].name == "planted" and seven[1].ties >= 4
    full, want, infos, entries = J.factor_batch(p, 16, "L")
    assert (infos == [seven[b % 7].info for b in range(16)]).all() and entries[8] is seven[1]
    m = J.tri_mask(p, "L")
    assert np.isnan(full[:, ~m]).all() and np.isnan(want[:, ~m]).all()
    J.same_bits(want[3], seven[3].R.T, m, "the lower triangle holds the transpose")


def test_batches_sit_at_the_seams_of_the_packing():
    assert J.pw_of(1) == 1 and J.pw_of(3) == 4 and J.pw_of(16) == 16 and J.pw_of(17) == 32 and J.pw_of(33) == 64
    assert J.batches(4) == [1, 15, 16, 17, 65, 304]
    assert J.batches(64) == [1, 2, 5, 364] and J.batches(17) == [1, 2, 3, 9, 317]
    for p in J.SIZES:
        assert all(math.gcd(7, 64 // J.pw_of(p)) == 1 for _ in (0,))


@pytest.mark.parametrize("layout", ["col", "row"])
def test_pack_and_unpack(layout):
    p, batch = 5, 4
    rng = np.random.default_rng(5)
    m = J.tri_mask(p, "U")
    full = np.where(m, rng.random((batch, p, p)), np.nan)
    buf, ld, stride, strides = J.pack(full, layout, 2, 3)
    assert ld == 7 and stride == 38 and buf.shape == (batch, stride)
    assert int((~np.isnan(buf)).sum()) == batch * 15
    # matrix 2, entry (1, 3)
    at = 1 + 3 * ld if layout == "col" else 1 * ld + 3
    assert buf[2, at] == full[2, 1, 3]
    got = J.unpack(buf, batch, p, strides, m)
    J.same_bits(got, full, m, "round trip")
    buf[1, stride - 1] = 0.0                                       # the gap
    with pytest.raises(AssertionError):
        J.unpack(buf, batch, p, strides, m)
    buf[1, stride - 1] = np.nan
    J._view(buf, batch, p, strides)[0, 3, 1] = 1.0                 # the other triangle
    with pytest.raises(AssertionError):
        J.unpack(buf, batch, p, strides, m)


def test_plain_factor_restates_the_definition_in_fp64():
    G = J.gram64(1)[0][:9, :9]
    R, info = J.plain_factor(G)
    assert info == 0 and np.allclose(np.triu(R), np.linalg.cholesky(G).T, rtol=1e-10)
    R, info = J.plain_factor(P.breakdown(6, 3, "neg"))
    assert info == 4 and R[3, 3] == -1.0


@pytest.mark.parametrize("sweep", ["1", "2", "B"])
@pytest.mark.parametrize("p", [2, 8, 16, 33])
def test_solve_models_agree_with_a_dense_solve_and_meet_their_ties(p, sweep):
    seven = J.solve_seven(p, sweep)
    for kind in (0, 5, 6):
        X, ties = J.solve_model(p, kind, p, sweep)
        F, B = seven[kind].F, seven[kind].B
        assert (np.tril(F, -1) == 0).all()
        ref = B.copy()
        if sweep in ("1", "B"):
            ref = np.linalg.solve(F.T, ref)
        if sweep in ("2", "B"):
            ref = np.linalg.solve(F, ref)
        planted = (kind == 5 and sweep in ("1", "B")) or (kind == 6 and sweep in ("2", "B"))
        if not (planted and p >= 16 and sweep != "B"):             # (the planted systems are ill-conditioned on purpose)
            assert np.allclose(X, ref, rtol=1e-6, atol=1e-9), (kind, sweep)
        if planted:
            assert ties[0] >= 1, (p, kind, sweep, ties)
    # 'B' is '1' then '2': the second sweep of the model on the first sweep's result
    if sweep == "B":
        F, B = seven[2].F, seven[2].B
        y, _ = E.trsv_exact(np.ascontiguousarray(F.T), B[:, 1])
        z, _ = E.trsv_exact(np.ascontiguousarray(F[::-1, ::-1]), y[::-1])
        assert (J.solve_model(p, 2, p, "B")[0][:, 1].view(np.int64) == z[::-1].view(np.int64)).all()


def test_the_planted_substitutions_carry_their_classes():
    """leading parts (p >= 16) of the planted ExTRSV systems plant sweep 1, their index reversal sweep 2"""
    c = E.planted_trsv_case(40, 40, 20, False, False)
    assert int((c.classes[:12] == "anchor").all()) and int(c.planted[12:].sum()) >= 25
    for p, least in ((16, 1), (17, 1), (32, 6), (40, 10)):
        X1, t1 = J.solve_model(p, 5, p, "1")
        assert (X1[:, 0].view(np.int64) == c.want[:p].view(np.int64)).all() and t1[0] >= least, (p, t1)
        X2, t2 = J.solve_model(p, 6, p, "2")
        assert (X2[:, 0].view(np.int64) == c.want[:p][::-1].view(np.int64)).all() and t2[0] == t1[0]
    c = E.planted_trsv_case(64, 400, 53, False, False)
    X1, t1 = J.solve_model(64, 5, 64, "1")
    assert (X1[:, 0].view(np.int64) == c.want.view(np.int64)).all() and t1[0] >= 10


def test_the_hand_made_ties():
    u = 2.0 ** -52
    X, t = J.solve_model(2, 5, 2, "1")
    assert X[0, 0] == 1.0 and X[1, 0] == 1.0 and t[0] == 1          # 1 + u - 2^-53 is a tie: to even
    X, t = J.solve_model(2, 6, 2, "2")
    assert X[1, 0] == 1.0 and X[0, 0] == 1.0 and t[0] == 1
    X, t = J.solve_model(7, 6, 7, "B")
    assert X[1, 0] == 1.0 and X[0, 0] == 1.0 and t[0] == 1 and J.solve_seven(7, "B")[6].B[1, 0] == 1.0 + u


def test_solve_case_lays_blocks_and_patterns_out():
    p, n, k = 4, 4 * 9 + 3, 7
    X0, want, ties = J.solve_case(p, n, k, "B")
    assert X0.shape == want.shape == (n, k) and ties >= 2
    seven = J.solve_seven(p, "B")
    assert (X0[8 * p:8 * p + 4, 6] == seven[1].B[:, 1]).all()
    assert (X0[9 * p:, 5] == seven[2].B[:3, 0]).all()
    short = J.solve_model(p, 2, 3, "B")[0]
    assert (want[9 * p:, 5].view(np.int64) == short[:, 0].view(np.int64)).all()
    full = J.solve_model(p, 2, 4, "B")[0]
    assert (short[:, 0] != full[:3, 0]).any()                       # sweep 2 of a short block starts at its own last row
    Fs = J.solve_factors(p, n, "L", "B")
    assert Fs.shape == (10, 4, 4) and np.isnan(Fs[9, 3, :]).all() and np.isnan(Fs[0][~J.tri_mask(4, "L")]).all()
    assert (Fs[1][J.tri_mask(4, "L")] == seven[1].F.T[J.tri_mask(4, "L")]).all()


def test_plain_solve_restates_the_substitution():
    F, B = J.solve_seven(9, "B")[0].F, J.solve_seven(9, "B")[0].B
    x = J.plain_solve(F, B[:, 0], "B")
    assert np.allclose(x, np.linalg.solve(F, np.linalg.solve(F.T, B[:, 0])), rtol=1e-10)


def test_chain_model_is_block_jacobi():
    A = J.laplacian(6)
    assert (A == A.T).all() and (np.linalg.eigvalsh(A) > 0).all()
    for p in (8, 7):
        D = J.diag_blocks(A, p)
        n = A.shape[0]
        assert D.shape == (-(-n // p), p, p)
        X0 = np.random.default_rng(p).random((n, 3))
        R, X = J.chain_model(A, p, X0)
        M = np.zeros_like(A)
        for b in range(D.shape[0]):
            r = min(p, n - b * p)
            M[b * p:b * p + r, b * p:b * p + r] = D[b, :r, :r]
            assert (D[b, r:, r:] == np.eye(p - r)).all()
        assert np.allclose(X, np.linalg.solve(M, X0), rtol=1e-10)
