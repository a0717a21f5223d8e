"""Cases for the batched ExPOTRF / ExPOTRS tests (the factor and the apply of a block-Jacobi preconditioner).  Nothing here
calls the code under test: every expectation comes from the Fraction models of potrf_cases (potrf_exact) and exact_cases
(trsv_exact; sweep 2 is the same substitution on the index-reversed system).

Every matrix of a batch is independent, so a batch CYCLES SEVEN DISTINCT MATRICES (seven is coprime to every packing
factor, which are powers of two): each expectation is computed once and cached, and a mix-up between neighbours still
shows.  The right-hand sides of the apply cycle seven blocks by five column patterns in the same way.

Buffers: `pack` lays the logical [batch, p, p] triangles out column- or row-major with a padded leading dimension and a gap
between matrices; everything that is not a stored triangle entry is NaN, and `unpack` checks that it still is."""
import math
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import exact_cases as E
import potrf_cases as P

SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 40, 63, 64)
VARIANTS = ((0, False), (4, True), (8, True))
LAYOUTS = (("U", "col", 0, 0), ("L", "row", 3, 5), ("L", "col", 2, 0), ("U", "row", 0, 7), ("U", "col", 5, 1),
           ("L", "row", 0, 0), ("L", "col", 0, 3), ("U", "row", 1, 0))   # (uplo, layout, padding of ld, gap between matrices)
NAN_BITS = np.array(np.nan).view(np.int64)
NPAT = 5                                # column patterns of the right-hand sides


def pw_of(p):
    """p rounded up to a power of two: the lanes a matrix takes"""
    return 1 << max(p - 1, 0).bit_length()


def batches(p):
    """the seams of the packing (64 / pw matrices per wave, four waves per workgroup item) and one of a few hundred"""
    g = max(64 // pw_of(p), 1)
    return sorted({1, max(g - 1, 1), g, g + 1, 4 * g + 1, 300 + p})


def tri_mask(p, uplo):
    return np.triu(np.ones((p, p), dtype=bool)) if uplo == "U" else np.tril(np.ones((p, p), dtype=bool))


# ---- buffers ---------------------------------------------------------------------------------------------------------
def geometry(p, layout, pad, gap):
    """(ld, stride, element strides of the logical [batch, i, j] view)"""
    ld = max(p, 1) + pad
    stride = ld * p + gap
    return ld, stride, ((stride, 1, ld) if layout == "col" else (stride, ld, 1))


def _view(buf, batch, p, strides):
    return np.lib.stride_tricks.as_strided(buf, shape=(batch, p, p), strides=tuple(8 * s for s in strides))


def pack(full, layout, pad, gap):
    """full: [batch, p, p] logical matrices (NaN wherever nothing must be read).  Returns (buf, ld, stride, strides): a
    NaN-filled [batch, stride] buffer holding them."""
    batch, p = full.shape[0], full.shape[1]
    ld, stride, strides = geometry(p, layout, pad, gap)
    buf = np.full((batch, stride), np.nan)
    if batch and p:
        _view(buf, batch, p, strides)[...] = full
    return buf, ld, stride, strides


def unpack(buf, batch, p, strides, written):
    """the logical [batch, p, p] matrices of a buffer, after checking that nothing outside `written` (a [batch, p, p] or
    [p, p] mask of the entries a routine may store) holds anything but the NaN it was filled with"""
    buf = np.array(buf, copy=True)
    got = np.array(_view(buf, batch, p, strides), copy=True) if batch and p else np.zeros((batch, p, p))
    if batch and p:
        v = _view(buf, batch, p, strides)
        v[np.broadcast_to(written, v.shape)] = np.nan
    assert (buf.view(np.int64) == NAN_BITS).all(), "something outside the stored triangles was written"
    return got


def same_bits(got, want, mask, what):
    """bit for bit where mask holds; a NaN is a NaN"""
    mask = np.broadcast_to(mask, np.asarray(got).shape)
    g, w = np.asarray(got)[mask], np.asarray(want)[mask]
    ok = (g.view(np.int64) == w.view(np.int64)) | (np.isnan(g) & np.isnan(w))
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), g[~ok][:4], w[~ok][:4])


# ---- the factor side -------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def gram64(seed):
    """a random full-mantissa Gram matrix of size 64 and its factor: the factor of a leading part is the leading part"""
    G = P.gram(64, seed=seed)
    R, info, d = P.potrf_exact(G, "U", detail=True)
    assert info == 0
    return G, R, d.kind


@lru_cache(maxsize=None)
def planted_lead(q):
    """the leading q x q part of potrf_cases.planted(40) (planted(64) beyond): (G, R, ties, near-ties)"""
    c = P.planted(40 if q <= 40 else 64)
    kind = c.kind[:q, :q]
    return c.G[:q, :q], c.R[:q, :q], int((kind == P.TIE).sum()), int((kind == P.NEAR).sum())


def _entry(name, G, R, info, ties):
    p = G.shape[0]
    return SimpleNamespace(name=name, G=G, R=R, info=info, ties=ties, fixed=P.fixed_entries(p, info))


@lru_cache(maxsize=None)
def factor_seven(p):
    """the seven distinct matrices of size p: random Gram matrices, a planted leading part (p >= 9), a banded matrix
    (p >= 3), a breakdown (zero / neg / nan at the first, an inner or the last pivot, by p) and a matrix of NaNs.  Each with
    its model R (upper orientation, symmetric G), info, the ties among its fixed entries and their number."""
    out = []
    for s in (0, 1, 2):
        G, R, kind = gram64(s)
        out.append(_entry(f"gram{s}", G[:p, :p], R[:p, :p], 0, int((kind[:p, :p] == P.TIE).sum())))
    if p >= 9:
        G, R, ties, _ = planted_lead(p)
        out.insert(1, _entry("planted", G, R, 0, ties))
    else:
        G, R, kind = gram64(3)
        out.insert(1, _entry("gram3", G[:p, :p], R[:p, :p], 0, int((kind[:p, :p] == P.TIE).sum())))
    if p >= 3:
        G = P.banded(p)
        R, info, d = P.potrf_exact(G, "U", detail=True)
        assert info == 0
        out.insert(2, _entry("banded", G, R, 0, int((d.kind == P.TIE).sum())))
    else:
        G, R, kind = gram64(4)
        out.insert(2, _entry("gram4", G[:p, :p], R[:p, :p], 0, int((kind[:p, :p] == P.TIE).sum())))
    j = (0, p // 2, p - 1)[p % 3]
    what = ("zero", "neg", "nan")[(p // 3) % 3]
    G = P.breakdown(p, j, what)
    R, info = P.potrf_exact(G, "U")
    assert info == j + 1
    out.insert(4, _entry(f"breakdown({j},{what})", G, R, info, 0))
    G = np.full((p, p), np.nan)
    R, info = P.potrf_exact(G, "U")
    assert info == 1 and math.isnan(R[0, 0])
    out.append(_entry("nan", G, R, 1, 0))
    assert len(out) == 7
    return tuple(out)


def factor_batch(p, batch, uplo, seven=None):
    """the batch that cycles factor_seven(p): (full [batch, p, p] with NaN in the other triangle, want, infos, entries)"""
    seven = seven or factor_seven(p)
    mask = tri_mask(p, uplo)
    full, want = np.full((batch, p, p), np.nan), np.full((batch, p, p), np.nan)
    infos = np.zeros(batch, dtype=np.int32)
    for b in range(batch):
        e = seven[b % 7]
        full[b][mask] = e.G[mask]
        want[b][mask] = (e.R if uplo == "U" else e.R.T)[mask]
        infos[b] = e.info
    return full, want, infos, [seven[b % 7] for b in range(batch)]


def plain_factor(G):
    """the fp64 restatement of fpe == 1 (upper orientation): s = g_ji, then s -= r_kj r_ki for k ascending"""
    G = np.asarray(G, dtype=np.float64)
    p = G.shape[0]
    R = G.copy()
    for j in range(p):
        s = float(G[j, j])
        for k in range(j):
            s -= float(R[k, j]) * float(R[k, j])
        if not s > 0:
            R[j, j] = s
            return R, j + 1
        rjj = math.sqrt(s)
        R[j, j] = rjj
        for i in range(j + 1, p):
            s = float(G[j, i])
            for k in range(j):
                s -= float(R[k, j]) * float(R[k, i])
            R[j, i] = np.float64(s) / np.float64(rjj)
    return R, 0


# ---- the apply side --------------------------------------------------------------------------------------------------
def _random_triangle(p, seed):
    """an upper triangle of full-mantissa doubles: a diagonal of either sign in [1, 2), the rest in (-1/4, 1/4)"""
    rng = np.random.default_rng([p, seed, 77])
    F = np.triu((rng.random((p, p)) - 0.5) / 2, 1)
    F += np.diag((1.0 + rng.random(p)) * rng.choice((-1.0, 1.0), p))
    return F


def _hand_made(p, b0, b1):
    """F = diag(1, 1, 3, 4, ...) with F[0, 1] = 2^-53, and the right-hand side (b0, b1, ...) of column pattern 0.  With
    u = 2^-52: sweep 1 on (1, 1 + u) meets the total 1 + u - 2^-53, a tie; sweep 2 on (1 + u, 1) meets the same tie; 'B' on
    (1 + u, 1 + u) meets the near-tie 1 + 2^-53 - 2^-105 in sweep 1, which leaves (1 + u, 1), and then the tie."""
    F = np.diag(np.arange(1.0, p + 1.0))
    F[0, 0] = F[1, 1] = 1.0
    F[0, 1] = 2.0 ** -53
    return F, b0, b1


@lru_cache(maxsize=None)
def solve_seven(p, sweep):
    """the seven distinct blocks of an apply with `sweep`: F (upper p x p, zeros below) and B (p x NPAT right-hand sides).
    Random full-mantissa triangles, and (the hand-made ties in column pattern 0, the planted systems in every column)
      sweep '1': block 5 is the leading part of a planted ExTRSV system (p >= 16), else the hand-made tie (p >= 2);
      sweep '2': block 6 is the index reversal of that leading part, else the hand-made tie;
      sweep 'B': blocks 5 and 6 are the hand-made ties of sweep 1 and of sweep 2 (the planted systems are built for one
                 direction: solved in the other, their large cancelling entries overflow)."""
    out = []
    for s in range(7):
        rng = np.random.default_rng([p, s, 78])
        out.append(SimpleNamespace(F=_random_triangle(p, s), B=(rng.random((p, NPAT)) - 0.5) * 4))
    u = 2.0 ** -52
    hand = {"1": ((5, 1.0, 1.0 + u),), "2": ((6, 1.0 + u, 1.0),), "B": ((5, 1.0, 1.0 + u), (6, 1.0 + u, 1.0 + u))}[sweep]
    if p >= 16 and sweep != "B":
        c = E.planted_trsv_case(40, 40, 20, False, False) if p <= 40 else E.planted_trsv_case(64, 400, 53, False, False)
        L, b = c.L[:p, :p], c.b[:p]
        # every column of a planted block is the planted right-hand side times a power of two (the totals scale with it,
        # ties stay ties): under any other right-hand side the large cancelling entries of these systems would not cancel
        scale = 2.0 ** np.arange(NPAT)
        if sweep == "1":
            out[5].F, out[5].B = np.ascontiguousarray(L.T), np.outer(b, scale)
        else:
            out[6].F, out[6].B = np.ascontiguousarray(L[::-1, ::-1]), np.outer(b[::-1], scale)
    elif p >= 2:
        for s, b0, b1 in hand:
            out[s].F, out[s].B[0, 0], out[s].B[1, 0] = _hand_made(p, b0, b1)
    return tuple(out)


def _stage(Lmat, b):
    """one substitution of the model and the ties among its totals"""
    x, totals = E.trsv_exact(Lmat, b)
    return x, sum(1 for t in totals if P._kind(t, E.round_nearest_even(t)) == P.TIE)


@lru_cache(maxsize=None)
def solve_model(p, kind, rows, sweep):
    """(X [rows, NPAT], ties [NPAT]) of block `kind` of solve_seven(p, sweep) with its first `rows` rows: sweep '1' is the
    substitution on F^T, sweep '2' the same substitution on the index-reversed system F[::-1, ::-1], 'B' one after the
    other"""
    blk = solve_seven(p, sweep)[kind]
    F = blk.F[:rows, :rows]
    X, ties = np.zeros((rows, NPAT)), np.zeros(NPAT, dtype=np.int64)
    for c in range(NPAT):
        x = blk.B[:rows, c].copy()
        if sweep in ("1", "B"):
            x, t = _stage(np.ascontiguousarray(F.T), x)
            ties[c] += t
        if sweep in ("2", "B"):
            xr, t = _stage(np.ascontiguousarray(F[::-1, ::-1]), x[::-1])
            x = xr[::-1]
            ties[c] += t
        X[:, c] = x
    return X, ties


def solve_case(p, n, k, sweep):
    """X0 (n x k), the expected X and the number of ties the call meets; block b is solve_seven(p, sweep)[b % 7], column j
    its pattern j % NPAT"""
    nb = -(-n // p)
    cols = np.arange(k) % NPAT
    X0, want, ties = np.zeros((n, k)), np.zeros((n, k)), 0
    for b in range(nb):
        rows = min(p, n - b * p)
        Xm, tm = solve_model(p, b % 7, rows, sweep)
        X0[b * p:b * p + rows] = solve_seven(p, sweep)[b % 7].B[:rows][:, cols]
        want[b * p:b * p + rows] = Xm[:, cols]
        ties += int(tm[cols].sum())
    return X0, want, ties


def solve_factors(p, n, uplo, sweep):
    """the [ceil(n / p), p, p] logical factors of solve_case: F in the upper triangle ('U') or F^T in the lower ('L'), NaN in
    the other triangle and in the unused trailing part of a short last block"""
    nb = -(-n // p)
    full = np.full((nb, p, p), np.nan)
    mask = tri_mask(p, uplo)
    for b in range(nb):
        rows = min(p, n - b * p)
        F = solve_seven(p, sweep)[b % 7].F
        M = np.full((p, p), np.nan)
        M[:rows, :rows] = F[:rows, :rows] if uplo == "U" else F[:rows, :rows].T
        full[b][mask] = M[mask]
    return full


def plain_solve(F, b, sweep):
    """the fp64 restatement of fpe == 1 on one column: s = b_i, then s -= F x over the solved rows ascending"""
    x = np.array(b, dtype=np.float64)
    r = len(x)
    if sweep in ("1", "B"):
        for i in range(r):
            s = float(x[i])
            for c in range(i):
                s -= float(F[c, i]) * float(x[c])
            x[i] = np.float64(s) / np.float64(F[i, i])
    if sweep in ("2", "B"):
        for i in range(r - 1, -1, -1):
            s = float(x[i])
            for c in range(i + 1, r):
                s -= float(F[i, c]) * float(x[c])
            x[i] = np.float64(s) / np.float64(F[i, i])
    return x


# ---- the chain -------------------------------------------------------------------------------------------------------
def laplacian(m, seed=0):
    """the 2-D five-point Laplacian on m x m with a full-mantissa perturbation of the diagonal, dense (SPD: strictly
    diagonally dominant)"""
    rng = np.random.default_rng([m, seed, 79])
    n = m * m
    A = np.zeros((n, n))
    for r in range(m):
        for c in range(m):
            i = r * m + c
            A[i, i] = 4.0 + rng.random()
            for rr, cc in ((r - 1, c), (r + 1, c), (r, c - 1), (r, c + 1)):
                if 0 <= rr < m and 0 <= cc < m:
                    A[i, rr * m + cc] = -1.0
    return A


def diag_blocks(A, p):
    """the dense restatement of csr_diag_blocks_dev: [ceil(n / p), p, p], the last block padded with an identity diagonal"""
    n = A.shape[0]
    nb = -(-n // p)
    D = np.zeros((nb, p, p))
    for b in range(nb):
        r = min(p, n - b * p)
        D[b, :r, :r] = A[b * p:b * p + r, b * p:b * p + r]
        for i in range(r, p):
            D[b, i, i] = 1.0
    return D


def chain_model(A, p, X0):
    """block-Jacobi by the models: (R [nb, p, p] upper orientation, X = blockdiag(D_b)^-1 X0)"""
    D = diag_blocks(A, p)
    n, k = X0.shape
    R, X = np.zeros_like(D), np.zeros_like(X0)
    for b in range(D.shape[0]):
        R[b], info = P.potrf_exact(D[b], "U")
        assert info == 0
        r = min(p, n - b * p)
        F = np.triu(R[b])[:r, :r]
        for j in range(k):
            y, _ = E.trsv_exact(np.ascontiguousarray(F.T), X0[b * p:b * p + r, j])
            z, _ = E.trsv_exact(np.ascontiguousarray(F[::-1, ::-1]), y[::-1])
            X[b * p:b * p + r, j] = z[::-1]
    return R, X
