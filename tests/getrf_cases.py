"""Cases for the batched ExGETRF / ExGETRS tests (the factor and the apply of a block-Jacobi preconditioner with general
blocks).  Nothing here calls the code under test: every expectation comes from getrf_exact below (the definition in exact
rational arithmetic) and exact_cases.trsv_exact.

The definition, step j = 0 .. p - 1 on the working matrix W (A on entry, rows swapped as the steps go):
    candidates  c_i = Round(w_ij - sum_{k<j} l_ik u_kj), i >= j        every sum exact, rounded once
    pivot       the smallest i >= j with the largest |c_i|, a NaN above +Inf; ipiv[j] = piv + 1
    breakdown   c_piv zero or NaN: the candidates are stored, no swap, ipiv[i] = i + 1 for i >= j, info = j + 1, stop
    column of L rows j and piv swapped whole, u_jj = c_piv, l_ij = fl(c_i / u_jj)
    row of U    u_ji = Round(w_ji - sum_{k<j} l_jk u_ki), i > j

A batch CYCLES SEVEN DISTINCT MATRICES (seven is coprime to every packing factor), each expectation computed once and
cached: bjacobi_cases.pack / unpack lay them out with NaN in every padding and gap."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import exact_cases as E
import potrf_cases as P
import bjacobi_cases as J

SIZES, VARIANTS, NAN_BITS = J.SIZES, J.VARIANTS, J.NAN_BITS
LAYOUTS = (("col", 0, 0), ("row", 3, 5), ("col", 2, 0), ("row", 0, 7), ("col", 5, 1), ("row", 0, 0), ("col", 0, 3),
           ("row", 1, 0))   # (layout, padding of ld, gap between matrices)
CLEAR, TIE, NEAR = P.CLEAR, P.TIE, P.NEAR
_SH = 1100                              # every double is an integer multiple of 2^-1074: x 2^_SH is an integer
_ONE = 1 << _SH


def _int(x):
    """the finite double x times 2^_SH, exactly, as a Python integer"""
    num, den = float(x).as_integer_ratio()
    return num * (_ONE // den)


def roundings(p, info):
    """the counter formula: p^2 for a complete matrix, sum_{s<j} (2 (p - s) - 1) + (p - j) for a breakdown at step j"""
    if info == 0:
        return p * p
    j = info - 1
    return sum(2 * (p - s) - 1 for s in range(j)) + (p - j)


def _rank(c):
    """the pivot order of a candidate: a NaN above +Inf, else |c|"""
    return (1, 0.0) if math.isnan(c) else (0, abs(c))


def getrf_exact(A, detail=False):
    """(W, ipiv, info): the definition on a copy of A.  Every total is summed exactly (integers at a fixed binary scale,
    handed to potrf_cases._kind as a Fraction), float() does the one rounding, the quotient of two np.float64 the division.
    A non-finite operand decides the totals it meets in IEEE arithmetic: Inf - Inf and 0 * Inf are NaN.  detail: also a
    namespace with ckind / ukind (CLEAR / TIE / NEAR of the candidate of working row i at step j, before the swap, and of
    u_ji; 0 where nothing was rounded), ties, nears and the number of roundings."""
    W = np.array(A, dtype=np.float64, copy=True)
    p = W.shape[0]
    ipiv = np.arange(1, p + 1, dtype=np.int32)
    ckind, ukind = np.zeros((p, p), dtype=np.int8), np.zeros((p, p), dtype=np.int8)
    fin = np.isfinite(W)
    Wi = np.empty((p, p), dtype=object)
    for r in range(p):
        for c in range(p):
            Wi[r, c] = _int(W[r, c]) if fin[r, c] else 0

    def fix(r, c, v):
        W[r, c] = v
        fin[r, c] = math.isfinite(v)
        Wi[r, c] = _int(v) if fin[r, c] else 0

    def total(r, c, j):
        """Round(w_rc - sum_{k<j} w_rk w_kc) and its kind"""
        if not (fin[r, c] and fin[r, :j].all() and fin[:j, c].all()):
            special = [] if fin[r, c] else [float(W[r, c])]
            special += [-float(np.float64(W[r, k]) * np.float64(W[k, c])) for k in range(j)
                        if not (fin[r, k] and fin[k, c])]
            return float(np.sum(np.array(special))), TIE
        t = Wi[r, c] * _ONE
        for k in range(j):
            t -= Wi[r, k] * Wi[k, c]
        t = Fraction(t, _ONE * _ONE)
        v = P._round(t)
        return v, P._kind(t, v)

    info = 0
    with np.errstate(all="ignore"):
        for j in range(p):
            cand = []
            for i in range(j, p):
                v, ckind[i, j] = total(i, j, j)
                cand.append(v)
            piv = j + max(range(len(cand)), key=lambda q: (_rank(cand[q]), -q))
            cp = cand[piv - j]
            for i in range(j, p):
                fix(i, j, cand[i - j])
            if cp == 0 or math.isnan(cp):
                info = j + 1
                break
            ipiv[j] = piv + 1
            if piv != j:
                for M in (W, fin, Wi):
                    M[[j, piv]] = M[[piv, j]]
            for i in range(j + 1, p):
                fix(i, j, float(np.float64(W[i, j]) / np.float64(W[j, j])))
            for i in range(j + 1, p):
                v, ukind[j, i] = total(j, i, j)
                fix(j, i, v)
    if detail:
        both = np.concatenate([ckind.ravel(), ukind.ravel()])
        return W, ipiv, info, SimpleNamespace(ckind=ckind, ukind=ukind, ties=int((both == TIE).sum()),
                                              nears=int((both == NEAR).sum()), roundings=int((both != 0).sum()))
    return W, ipiv, info


def restate(A):
    """a second, dense restatement of the definition for small finite cases: Fractions, no skipping, the permutation kept
    as a row list"""
    A = np.asarray(A, dtype=np.float64)
    p = A.shape[0]
    rows = [[float(v) for v in A[r]] for r in range(p)]
    ipiv = list(range(1, p + 1))
    for j in range(p):
        c = [P._round(Fraction(rows[i][j]) - sum(Fraction(rows[i][k]) * Fraction(rows[k][j]) for k in range(j)))
             for i in range(j, p)]
        best = 0
        for q in range(1, len(c)):
            if abs(c[q]) > abs(c[best]):
                best = q
        for i in range(j, p):
            rows[i][j] = c[i - j]
        if c[best] == 0:
            return np.array(rows), np.array(ipiv, dtype=np.int32), j + 1
        piv = j + best
        ipiv[j] = piv + 1
        rows[j], rows[piv] = rows[piv], rows[j]
        for i in range(j + 1, p):
            rows[i][j] = float(np.float64(rows[i][j]) / np.float64(rows[j][j]))
        for i in range(j + 1, p):
            rows[j][i] = P._round(Fraction(rows[j][i]) - sum(Fraction(rows[j][k]) * Fraction(rows[k][i]) for k in range(j)))
    return np.array(rows), np.array(ipiv, dtype=np.int32), 0


def plain_getrf(A):
    """the fp64 restatement of fpe == 1: the same structure with s = w, then s -= l * u for k ascending"""
    W = np.array(A, dtype=np.float64, copy=True)
    p = W.shape[0]
    ipiv = np.arange(1, p + 1, dtype=np.int32)

    def total(r, c, j):
        s = np.float64(W[r, c])
        for k in range(j):
            s = s - np.float64(W[r, k]) * np.float64(W[k, c])
        return float(s)

    with np.errstate(all="ignore"):
        for j in range(p):
            cand = [total(i, j, j) for i in range(j, p)]
            piv = j + max(range(len(cand)), key=lambda q: (_rank(cand[q]), -q))
            W[j:, j] = cand
            if cand[piv - j] == 0 or math.isnan(cand[piv - j]):
                return W, ipiv, j + 1
            ipiv[j] = piv + 1
            W[[j, piv]] = W[[piv, j]]
            W[j + 1:, j] = W[j + 1:, j] / W[j, j]
            for i in range(j + 1, p):
                W[j, i] = total(j, i, j)
    return W, ipiv, 0


# ---- the seven matrices ----------------------------------------------------------------------------------------------
def random_matrix(p, seed):
    """full-mantissa entries of either sign in (-1, 1)"""
    rng = np.random.default_rng([p, seed, 90])
    return (rng.random((p, p)) - 0.5) * 2


def dominant(p, seed=0):
    """strictly diagonally dominant, nonsymmetric, full mantissas: no interchange"""
    rng = np.random.default_rng([p, seed, 91])
    return (rng.random((p, p)) - 0.5) + np.diag((p + rng.random(p)) * rng.choice((-1.0, 1.0), p))


def shuffled(M, seed=0):
    """the rows of M in another order (never the identity for p >= 2)"""
    p = M.shape[0]
    perm = np.random.default_rng([p, seed, 92]).permutation(p)
    if p >= 2 and (perm == np.arange(p)).all():
        perm = np.roll(perm, 1)
    return np.ascontiguousarray(M[perm])


@lru_cache(maxsize=None)
def planted(q):
    """The leading q x q part of potrf_cases.planted(40) (planted(64) beyond q = 40) with its identity rows scaled by 2^24.
    Those rows are then the pivots of their columns (every other entry of such a column lies below 2^24), l = b / 2^24 and
    u = 2^24 b are exact, so l u = b_k0 b_ki as in the Cholesky case: the planted totals reappear as the candidates of the
    planted column AND, the matrix being symmetric but for the scaling, in the planted row of U.  Asserted through
    getrf_exact: no interchange, the planted ties in both places, and a row shuffle gives the same W with another ipiv."""
    c = P.planted(40 if q <= 40 else 64)
    G = c.G[:q, :q].copy()
    ident = np.flatnonzero(np.diag(G) == 1.0)
    G[ident] *= 2.0 ** 24
    W, ipiv, info, d = getrf_exact(G, detail=True)
    assert info == 0 and (ipiv == np.arange(1, q + 1)).all(), "the planted matrix must need no interchange"
    want_ties = 0
    for r, col, cls, gap, want in c.plants:
        if r >= q or col >= q:
            continue
        name = cls.split(":")[-1]
        if name in ("tie", "tie_odd", "carry"):
            # (r, col) of the upper orientation: u_{r,col}, and by symmetry the candidate of row col at step r
            assert d.ukind[r, col] == TIE or col == r, (r, col, cls)
            assert d.ckind[col, r] == TIE, (r, col, cls)
            assert (W[r, col] == want) if col > r else True
            want_ties += 1 if col == r else 2
    assert d.ties >= want_ties
    if q in (40, 64):
        assert d.ties == {40: 31, 64: 57}[q], d.ties
    S = shuffled(G, 5)
    W2, ipiv2, info2 = getrf_exact(S)
    assert info2 == 0 and J_same(W2, W) and (q < 2 or (ipiv2 != np.arange(1, q + 1)).any())
    return SimpleNamespace(A=G, shuffled=S, W=W, ipiv=ipiv, ipiv_shuffled=ipiv2, ties=d.ties, nears=d.nears)


def J_same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def pivot_tie(p, seed=0):
    """a random matrix whose column 0 holds its largest magnitude twice, with opposite signs, the negative one first: the
    first index must win"""
    A = random_matrix(p, 40 + seed)
    if p >= 2:
        hi, lo = (p - 1, p // 2) if p // 2 != p - 1 else (1, 0)
        A[:, 0] *= 0.5
        A[lo, 0], A[hi, 0] = -0.75, 0.75
    return A


def zero_pivot(p, j):
    """A = [[2^10 I_j, 2^10 B], [C, D]] with small non-zero integers in B and C: the first j steps need no interchange,
    l = C / 2^10 and u = 2^10 B are exact, so the candidates of step j are D[:, 0] - C B[:, 0] exactly.  D[:, 0] is set to that
    product: every candidate of step j cancels to an exact zero (j = 0: a zero column), a breakdown at step j."""
    rng = np.random.default_rng([p, j, 93])
    A = rng.integers(1, 9, (p, p)).astype(np.float64) * rng.choice((-1.0, 1.0), (p, p))
    A[:j, :j] = np.eye(j)
    A[:j] *= 2.0 ** 10
    A[j:, j] = A[j:, :j] @ (A[:j, j] / 2.0 ** 10) if j else 0.0
    return A


def nan_pivot(p, j):
    """dominant(p) with a single NaN on the diagonal at j: no interchange before, the NaN ranks first at step j"""
    A = dominant(p, 3)
    A[j, j] = np.nan
    return A


def _entry(name, A):
    W, ipiv, info, d = getrf_exact(A, detail=True)
    p = A.shape[0]
    assert d.roundings == roundings(p, info), (name, p, info, d.roundings)
    return SimpleNamespace(name=name, A=A, W=W, ipiv=ipiv, info=info, ties=d.ties, nears=d.nears, roundings=d.roundings)


def breakdown_step(p, shift=0):
    """first / inner / last, chosen by p (shift: another choice for the same p)"""
    return (0, p // 2, p - 1)[(p + shift) % 3]


@lru_cache(maxsize=None)
def factor_seven(p):
    """the seven distinct matrices of size p, each with its model W, ipiv, info, ties and roundings: the planted matrix (its
    row shuffle for odd p; p >= 9, else random), a random one, a row-shuffled dominant matrix, a pivot tie, a zero-pivot
    breakdown, a NaN-pivot breakdown and a matrix of NaNs"""
    if p >= 9:   # first, so that every batch holds it
        c = planted(p)
        e = _entry("planted", c.shuffled if p % 2 else c.A)
        assert J_same(e.W, c.W) and e.ties == c.ties >= 1
        out = [e]
    else:
        out = [_entry("random1", random_matrix(p, 1))]
    out += [_entry("random0", random_matrix(p, 0)), _entry("shuffled", shuffled(dominant(p)))]
    out.append(_entry("pivot_tie", pivot_tie(p)))
    j = breakdown_step(p)
    e = _entry(f"zero_pivot({j})", zero_pivot(p, j))
    assert e.info == j + 1, (p, j, e.info)
    out.append(e)
    j = breakdown_step(p, 1)
    e = _entry(f"nan_pivot({j})", nan_pivot(p, j))
    assert e.info == j + 1 and math.isnan(e.W[j, j]), (p, j, e.info)
    out.append(e)
    e = _entry("nan", np.full((p, p), np.nan))
    assert e.info == 1
    out.append(e)
    assert len(out) == 7
    return tuple(out)


def factor_batch(p, batch, seven=None):
    """the batch that cycles factor_seven(p): (A [batch, p, p], W, ipiv [batch, p], info [batch], entries); asserts that
    the batch holds a TIE wherever p >= 9"""
    own = seven is None
    seven = seven or factor_seven(p)
    ent = [seven[b % 7] for b in range(batch)]
    A = np.array([e.A for e in ent]).reshape(batch, p, p)
    W = np.array([e.W for e in ent]).reshape(batch, p, p)
    ipiv = np.array([e.ipiv for e in ent], dtype=np.int32).reshape(batch, p)
    info = np.array([e.info for e in ent], dtype=np.int32)
    if own and p >= 9 and batch >= 1:
        assert sum(e.ties for e in ent) >= 1
    return A, W, ipiv, info, ent


# ---- the apply side --------------------------------------------------------------------------------------------------
NPAT = 5                                # column patterns of the right-hand sides


@lru_cache(maxsize=None)
def solve_seven(p):
    """seven factored blocks for the apply: LU and ipiv from getrf_exact of healthy matrices (random, shuffled dominant,
    pivot ties), one of them hand-made so that both sweeps meet a tie, and B (p x NPAT right-hand sides)"""
    out = []
    mats = [random_matrix(p, 10), shuffled(dominant(p, 1), 1), pivot_tie(p, 1), random_matrix(p, 11), shuffled(dominant(p, 2), 2),
            random_matrix(p, 12), shuffled(dominant(p, 4), 4)]
    for s, A in enumerate(mats):
        W, ipiv, info = getrf_exact(A)
        assert info == 0
        rng = np.random.default_rng([p, s, 94])
        out.append(SimpleNamespace(LU=W, ipiv=ipiv, B=(rng.random((p, NPAT)) - 0.5) * 4))
    if p >= 2:
        # L = [[1, 0], [2^-53, 1]] ..., U = diag(1, 1, 3, 4, ...) with U[0, 1] = 2^-53, pivots (2, 2, 3, ...): the right-hand
        # side (1 + u, 1), u = 2^-52, becomes (1, 1 + u) by the interchange; forward row 1 meets 1 + u - 2^-53, a tie
        # (-> 1); backward row 0 then meets 1 - 2^-53 exactly
        LU = np.diag(np.arange(1.0, p + 1.0))
        LU[0, 0] = LU[1, 1] = 1.0
        LU[0, 1] = LU[1, 0] = 2.0 ** -53
        ip = np.arange(1, p + 1, dtype=np.int32)
        ip[0] = 2
        out[5].LU, out[5].ipiv = LU, ip
        out[5].B[0, 0], out[5].B[1, 0] = 1.0 + 2.0 ** -52, 1.0
    return tuple(out)


def getrs_model(LU, ipiv, b):
    """one column through the definition: the interchanges (an index outside 1 .. rows is skipped), then
    exact_cases.trsv_exact twice: the unit-lower sweep forward and the upper sweep, as the same substitution on the
    index-reversed system.  Returns (x, ties among the totals)."""
    rows = len(b)
    x = np.array(b, dtype=np.float64, copy=True)
    for j in range(rows):
        pv = int(ipiv[j]) - 1
        if 0 <= pv < rows and pv != j:
            x[j], x[pv] = x[pv], x[j]
    LU = np.asarray(LU, dtype=np.float64)[:rows, :rows]
    y, t1 = E.trsv_exact(np.tril(LU, -1) + np.eye(rows), x, unit=True)
    zr, t2 = E.trsv_exact(np.ascontiguousarray(np.triu(LU)[::-1, ::-1]), y[::-1])
    ties = sum(1 for t in list(t1) + list(t2) if P._kind(t, E.round_nearest_even(t)) == TIE)
    return zr[::-1].copy(), ties


@lru_cache(maxsize=None)
def solve_model(p, kind, rows):
    """(X [rows, NPAT], ties [NPAT]) of block `kind` of solve_seven(p) with its first `rows` rows"""
    blk = solve_seven(p)[kind]
    X, ties = np.zeros((rows, NPAT)), np.zeros(NPAT, dtype=np.int64)
    for c in range(NPAT):
        X[:, c], ties[c] = getrs_model(blk.LU, blk.ipiv, blk.B[:rows, c])
    return X, ties


def solve_case(p, n, k):
    """(LU [nb, p, p], ipiv [nb, p], X0 [n, k], the expected X, the ties the call meets): block b is solve_seven(p)[b % 7],
    column j its pattern j % NPAT.  A short last block uses its leading part: the rest of its LU is NaN, the rest of its
    pivots garbage.  Its pivots inside the leading part may point beyond it: such an index is skipped."""
    nb = -(-n // p)
    cols = np.arange(k) % NPAT
    LU, ipiv = np.full((nb, p, p), np.nan), np.zeros((nb, p), dtype=np.int32)
    X0, want, ties = np.zeros((n, k)), np.zeros((n, k)), 0
    for b in range(nb):
        rows = min(p, n - b * p)
        blk = solve_seven(p)[b % 7]
        LU[b, :rows, :rows] = blk.LU[:rows, :rows]
        ipiv[b] = blk.ipiv
        ipiv[b, rows:] = -(2 ** 31) + 5
        Xm, tm = solve_model(p, b % 7, rows)
        X0[b * p:b * p + rows] = blk.B[:rows][:, cols]
        want[b * p:b * p + rows] = Xm[:, cols]
        ties += int(tm[cols].sum())
    return LU, ipiv, X0, want, ties


def plain_getrs(LU, ipiv, b):
    """the fp64 restatement of fpe == 1 on one column: s = b_i, then s -= a x over the solved rows ascending"""
    x = np.array(b, dtype=np.float64, copy=True)
    r = len(x)
    for j in range(r):
        pv = int(ipiv[j]) - 1
        if 0 <= pv < r and pv != j:
            x[j], x[pv] = x[pv], x[j]
    for i in range(r):
        s = np.float64(x[i])
        for c in range(i):
            s = s - np.float64(LU[i, c]) * x[c]
        x[i] = s
    for i in range(r - 1, -1, -1):
        s = np.float64(x[i])
        for c in range(i + 1, r):
            s = s - np.float64(LU[i, c]) * x[c]
        x[i] = s / np.float64(LU[i, i])
    return x


# ---- the chain -------------------------------------------------------------------------------------------------------
def convection_diffusion(m, seed=0):
    """the five-point upwind convection-diffusion operator on m x m, dense and nonsymmetric: diffusion -1 to every
    neighbour, convection (full-mantissa, position dependent) added to the west and south couplings, a perturbed diagonal"""
    rng = np.random.default_rng([m, seed, 95])
    n = m * m
    A = np.zeros((n, n))
    for r in range(m):
        for c in range(m):
            i = r * m + c
            A[i, i] = 4.0 + rng.random() * 3
            for rr, cc, conv in ((r - 1, c, 1.0), (r + 1, c, 0.0), (r, c - 1, 1.0), (r, c + 1, 0.0)):
                if 0 <= rr < m and 0 <= cc < m:
                    A[i, rr * m + cc] = -1.0 - conv * rng.random() * 2.5
    return A


def chain_model(A, p, X0):
    """block-Jacobi by the models: (W [nb, p, p], ipiv [nb, p], X = blockdiag(D_b)^-1 X0)"""
    D = J.diag_blocks(A, p)
    n, k = X0.shape
    W, ipiv, X = np.zeros_like(D), np.zeros((D.shape[0], p), dtype=np.int32), np.zeros_like(X0)
    for b in range(D.shape[0]):
        W[b], ipiv[b], info = getrf_exact(D[b])
        assert info == 0
        r = min(p, n - b * p)
        for j in range(k):
            X[b * p:b * p + r, j], _ = getrs_model(W[b], ipiv[b], X0[b * p:b * p + r, j])
    return W, ipiv, X
