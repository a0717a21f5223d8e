"""Inputs and expected bits for tests/test_gpu_graph_replay_solves.py: the mailbox solves (ExTRSM, ExSpTRSV, ExSpTRSM) on
two triangles and six right-hand sides, and ExBDOT on four pairs of blocks of which one is planted.

Nothing here touches the GPU or the library.  Expected bits come from exact_cases.trsv_exact (Fraction substitution),
from the planted cases of exact_cases / bdot_cases, or from the CPU oracle's ExDOT per output.  Every builder asserts
that its case is not vacuous (finite results, ties where they are wanted, data that differs from call to call);
tests/test_graph_replay_cases.py runs the builders without a GPU.

Right-hand sides.  A triangle owns a pool of a few solved columns (for a planted triangle the planted b, whose solution
is the construction's, and b_control; then random columns of full mantissas, each solved once by trsv_exact).  Column j
of the block of call r is a pool column times +-2^e, (pool index, sign, e) walking with j and r.  A power-of-two scaling
or a negation of b scales the whole substitution exactly (every product, every exact total, its rounding and the
quotient scale with it; solve_sets holds the values hundreds of binades inside the double range), so the expected column is the
pool's solution scaled the same way and every planted tie stays a tie -- tests/test_graph_replay_cases.py checks scaled
columns against trsv_exact itself.  So a block of 65 columns costs no Fraction arithmetic beyond its pool."""
import functools
import math
from types import SimpleNamespace

import numpy as np

import bdot_cases as D
import blas1_cases as B
import exact_cases as X
import sptrsv_cases as S
from helpers import bits

SCALES = (0, -3, 5, 40, -60)
TRIANGLE_OF_CALL = (0, 0, 1, 1, 1, 0)      # replays 0 .. 3, the eager call beside the graph, the second context's call
PREVIOUS_ON_DEFAULT = {1: 4, 2: 1, 3: 2}   # replay -> the call whose x the default context's mailbox still holds
POOL_RANDOM = 3

DENSE_N = 203                              # not a multiple of TR_R = 4 or TR_CH = 64: a partial item, a partial tile
SPARSE_N = 700
WIDE_EVERY, WIDE_LEN = 50, 100             # triangle 1 of the sparse pair: every 50th row holds 100 entries (> 64)


def _pool(L, unit, named, seed):
    """[(b, want, derives from the planted b)]: the named columns (want None: solve it), then POOL_RANDOM random ones"""
    n = L.shape[0]
    rng = np.random.default_rng([seed, n, 4177])
    cols = list(named) + [(S.rand53(rng, n) * rng.choice((-1.0, 1.0), n), None, False) for _ in range(POOL_RANDOM)]
    out = []
    for b, want, tie in cols:
        if want is None:
            want = X.trsv_exact(L, b, unit)[0]
        assert np.isfinite(want).all() and (bits(want) != bits(b)).any()
        out.append((b, want, tie))
    return out


def _planted_triangle(c, seed):
    ties = int(((c.classes == "tie") | (c.classes == "carry")).sum())
    assert ties >= 10
    return SimpleNamespace(n=c.n, L=c.L, ties=ties, pool=_pool(c.L, False, [(c.b, c.want, True), (c.b_control, None, False)], seed))


@functools.lru_cache(maxsize=None)
def dense_triangles():
    """two planted systems of DENSE_N rows: a sparse strict triangle, and one that the filler makes dense"""
    t0 = _planted_triangle(X.planted_trsv(DENSE_N, seed=31, W=40, mbits=53, filler=False), 1)
    t1 = _planted_triangle(X.planted_trsv(DENSE_N, seed=32, W=40, mbits=53, filler=True), 2)
    assert (bits(t0.L) != bits(t1.L)).sum() > DENSE_N
    return t0, t1


@functools.lru_cache(maxsize=None)
def sparse_triangles():
    """triangle 0: the planted system of TRSV_CASES[5] (700 rows of at most a few dozen entries: the 8-lane form, ties);
    triangle 1: random earlier columns, 6 to a row and WIDE_LEN in every WIDE_EVERY-th row (the 64-lane form)"""
    t0 = _planted_triangle(X.planted_trsv_case(*X.TRSV_CASES[5], False), 3)
    assert t0.n == SPARSE_N
    rng = np.random.default_rng([SPARSE_N, 9])
    s = S._system(SPARSE_N, rng, lambda i: rng.choice(i, min(i, WIDE_LEN if i % WIDE_EVERY == WIDE_EVERY - 1 else 6),
                                                      replace=False) if i else [])
    t1 = SimpleNamespace(n=SPARSE_N, L=s.L, ties=0, pool=_pool(s.L, False, [(s.b, None, False)], 4))
    return t0, t1


def column(tri, j, r):
    """(b, want, derives from the planted b) of column j of call r on triangle `tri`"""
    P = len(tri.pool)
    b, want, tie = tri.pool[(j + 2 * r) % P]
    t = j // P + r
    s = math.ldexp(-1.0 if t % 2 else 1.0, SCALES[t % len(SCALES)])
    return b * s, want * s, tie


def solve_sets(tris, k):
    """six (triangle index, B [n, k], want [n, k], columns that derive from the planted b), by TRIANGLE_OF_CALL"""
    out = []
    for r, t in enumerate(TRIANGLE_OF_CALL):
        cols = [column(tris[t], j, r) for j in range(k)]
        Bk, want = np.stack([c[0] for c in cols], axis=1), np.stack([c[1] for c in cols], axis=1)
        # (a random b does not cancel the planted +-G 2^150 pairs: such a column grows to 2^430 on the filler triangle;
        # with entries of L between 2^-305 and 2^151 every product and its TwoProd error stay far inside the range)
        assert (np.abs(want) > 2.0 ** -70).all() and (np.abs(want) < 2.0 ** 500).all()
        out.append((t, Bk, want, sum(c[2] for c in cols)))
    assert out[0][3] >= 1 and tris[out[0][0]].ties > 0, "no replay carries the planted ties"
    for r, prev in PREVIOUS_ON_DEFAULT.items():
        # a mailbox that was not reset hands over the previous call's x: it must differ from this call's everywhere
        assert (bits(out[r][2]) != bits(out[prev][2])).all(), (r, prev)
    for r in range(1, 4):
        assert (bits(out[r][1]) != bits(out[r - 1][2])).all()     # (nor is the solution left in X the next input)
    return out


@functools.lru_cache(maxsize=None)
def dense_sets(k):
    return solve_sets(dense_triangles(), k)


@functools.lru_cache(maxsize=None)
def sparse_sets(k):
    return solve_sets(sparse_triangles(), k)


@functools.lru_cache(maxsize=None)
def sparse_csr(t, uplo):
    """(crow, col, val, idx, skipped) of sparse triangle t: int64 indices under 'L', int32 under 'U', the entries of a
    row shuffled and up to three NaN entries per row in the other triangle; skipped: those entries, counted here"""
    tri = sparse_triangles()[t]
    crow, col, val, idx = S.csr_of_triangular(tri.L, uplo, np.int64 if uplo == "L" else np.int32, shuffle=True, junk=True,
                                              seed=t)
    skipped = len(col) - int(np.count_nonzero(np.tril(tri.L)))
    assert skipped == int(np.isnan(val).sum()) > SPARSE_N
    lens = np.diff(crow)
    if t == 1:      # both forms of k_sptrsv: items (8 rows) with a row beyond 64 entries, and items without
        assert (lens > 64).sum() >= 10 and np.convolve(lens <= 64, np.ones(16), "valid").max() == 16   # (16 rows in a
        #                                                                     run hold a whole item wherever they lie)
    else:
        assert lens.max() <= 64
    return crow, col, val, idx, skipped


def sparse_budget(uplo):
    """entries the captured col / val buffers hold: the larger of the two triangles' counts"""
    return max(len(sparse_csr(t, uplo)[1]) for t in (0, 1))


def padded_csr(t, uplo):
    """(crow, col, val) of sparse_csr(t, uplo) with col / val filled up to sparse_budget: column 0 and NaN, which no row
    reaches (crow[n] is the triangle's own count)"""
    crow, col, val = sparse_csr(t, uplo)[:3]
    room = sparse_budget(uplo) - len(col)
    return crow, np.concatenate([col, np.zeros(room, dtype=col.dtype)]), np.concatenate([val, np.full(room, np.nan)])


# ---------------------------------------------------------------------------------------------
# ExBDOT
# ---------------------------------------------------------------------------------------------
BDOT_N = 1000
BDOT_G, BDOT_D = 65, 70                    # 'G': 65 x 65 outputs, four batches over one workspace block; 'D': 70 outputs
G_SHIFTS = tuple(range(65))               # column j of Y in the planted 'G' pair is the constant 2^s_j (a term of one
#                                            unit, 2^-1074, stays exact under s >= 0 only)
A_POSITIONS = (700, 1074, 1075, 1330, 1900)    # leading bits of the Family A totals: 2^-374 .. 2^826
BDOT_KINDS = (("lognormal", 0.0, 50.0), None, ("fpuniform_signed", 60, 30), ("lognormal", 0.0, 2.0))   # None: planted
UNEVEN_P, UNEVEN_Q = 67, 3                 # 'G': a batch of 64 x 3 outputs in 192 sets (one group), then one of 3 x 3 in 252 (28
#                                            groups): the later batch accumulates into sets the first one never touched


def _sum_cases(count, with_d):
    """`count` ExSUM cases of at most a few terms: Family A at A_POSITIONS (every kind, mantissa and sign, strided), and
    for mode 'D' also every fifth case of Families B and C (totals of a few units of 2^-1074, runs of ones)"""
    a = B.family_a(positions=A_POSITIONS)
    extra = (B.family_b() + B.family_c())[::5] if with_d else []
    take = count - len(extra)
    cases = [a[(i * len(a)) // take] for i in range(take)] + extra
    assert len(cases) == count and sum(c.kind == "tie" for c in cases) >= 5
    return cases


def _rows(a, n):
    out = np.zeros((n, a.shape[1]))
    out[:a.shape[0]] = a
    return out


@functools.lru_cache(maxsize=None)
def planted_g_pair():
    """bdot_cases.planted_g on 64 + 1 cases (its limit is 64 columns), side by side, in BDOT_N rows: (X, Y, want)"""
    cases = _sum_cases(BDOT_G, False)
    parts = [D.planted_g(cases[:D.MAX_COLS], G_SHIFTS), D.planted_g(cases[D.MAX_COLS:], G_SHIFTS)]
    assert all(g.keep.all() and g.n <= BDOT_N for g in parts), "a planted output left the model's domain"
    Xp = np.hstack([_rows(g.X, BDOT_N) for g in parts])
    Yp = _rows(parts[0].Y, BDOT_N)
    Yp[parts[0].n:] = Yp[0]                 # (the constant columns go on; X is zero there)
    want = np.vstack([g.want for g in parts])
    assert Xp.shape == (BDOT_N, BDOT_G) and Yp.shape == (BDOT_N, BDOT_G) and want.shape == (BDOT_G, BDOT_G)
    return Xp, Yp, want


@functools.lru_cache(maxsize=None)
def planted_d_pair():
    cases = _sum_cases(BDOT_D, True)
    parts = [D.planted_d(cases[:D.MAX_COLS]), D.planted_d(cases[D.MAX_COLS:])]
    assert all(d.n <= BDOT_N for d in parts) and parts[0].scaled > 0
    Xp, Yp = (np.hstack([_rows(getattr(d, name), BDOT_N) for d in parts]) for name in ("X", "Y"))
    return Xp, Yp, np.concatenate([d.want for d in parts])


def _oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


@functools.lru_cache(maxsize=None)
def bdot_sets(mode):
    """four (X, Y, want) for mode 'G' (65 x 65) or 'D' (70): wide-range lognormal data (the small expansions spill into
    the sets), the planted pair (ties), wide-range signed data, plain data; the unplanted ones from the oracle's ExDOT
    on the strided columns, one call per output"""
    O = _oracle()
    p = BDOT_G if mode == "G" else BDOT_D
    out = []
    for r, kind in enumerate(BDOT_KINDS):
        if kind is None:
            Xr, Yr, want = planted_g_pair() if mode == "G" else planted_d_pair()
            assert np.isfinite(want).sum() >= want.size - 8
        else:
            Xr = O.gen(kind[0], BDOT_N * p, 8100 + r, kind[1], kind[2]).reshape(BDOT_N, p)
            Yr = O.gen(kind[0], BDOT_N * p, 8200 + r, kind[1], kind[2]).reshape(BDOT_N, p)
            xf, yf = Xr.ravel(), Yr.ravel()
            if mode == "G":
                want = np.array([[O.exdot(xf, yf, inca=p, offa=i, incb=p, offb=j, n=BDOT_N) for j in range(p)]
                                 for i in range(p)])
            else:
                want = np.array([O.exdot(xf, yf, inca=p, offa=j, incb=p, offb=j, n=BDOT_N) for j in range(p)])
            assert np.isfinite(want).all()
        out.append((Xr, Yr, want))
    for r in range(1, 4):
        assert (bits(out[r][2]) != bits(out[r - 1][2])).mean() > 0.9
    spread = np.log2(np.abs(out[0][0])).max() - np.log2(np.abs(out[0][0])).min()
    assert spread > 300, "the wide set is not wide"
    return out


def _gram_want(O, Xr, Yr):
    p, q = Xr.shape[1], Yr.shape[1]
    xf, yf = Xr.ravel(), Yr.ravel()
    return np.array([[O.exdot(xf, yf, inca=p, offa=i, incb=q, offb=j, n=Xr.shape[0]) for j in range(q)] for i in range(p)])


@functools.lru_cache(maxsize=None)
def bdot_uneven_sets():
    """four (X [n, 67], Y [n, 3], want [67, 3]) from the oracle, the kinds of bdot_sets with plain signed data in the
    planted pair's place.  bdot.hip keeps max(1, min(32, 256 // outputs)) groups of sets per batch: the figures of
    UNEVEN_P, UNEVEN_Q are asserted here from that rule, so that the case cannot go vacuous unnoticed"""
    O = _oracle()
    groups = lambda nout: max(1, min(32, 256 // nout))  # noqa: E731
    first, later = 64 * UNEVEN_Q, (UNEVEN_P - 64) * UNEVEN_Q
    assert groups(first) * first == 192 < groups(later) * later == 252
    out = []
    for r, kind in enumerate(BDOT_KINDS):
        kind = kind or ("fpuniform_signed", 10, 0)
        Xr = O.gen(kind[0], BDOT_N * UNEVEN_P, 8300 + r, kind[1], kind[2]).reshape(BDOT_N, UNEVEN_P)
        Yr = O.gen(kind[0], BDOT_N * UNEVEN_Q, 8400 + r, kind[1], kind[2]).reshape(BDOT_N, UNEVEN_Q)
        want = _gram_want(O, Xr, Yr)
        assert np.isfinite(want).all() and (want != 0).all()
        out.append((Xr, Yr, want))
    return out
