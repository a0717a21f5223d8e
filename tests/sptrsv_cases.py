"""CSR forms of logical lower-triangular systems for the ExSpTRSV tests, and a few structures.

Every system is a dense logical lower-triangular (L, b) in substitution order, as exact_cases.planted_trsv and
range_rows_trsv build them; the expected bits always come from exact_cases.trsv_exact on that dense matrix.  Nothing
here does arithmetic on the values: the functions only place them."""
import functools
from types import SimpleNamespace

import numpy as np

import exact_cases as X


def csr_of_triangular(L, uplo="L", itype=np.int64, shuffle=False, junk=False, diag_nan=False, keep=None, seed=0):
    """CSR of the logical lower system L: its stored entries are the non-zeros of the lower triangle (or the positions
    of `keep`, a boolean mask inside the lower triangle: explicit zeros).  'U' reverses rows and columns, as
    exact_cases.trsv_operands does: logical row i is physical row idx[i].  shuffle permutes the entries inside each
    row; junk adds NaN-valued entries strictly inside the OTHER triangle (up to 3 per row); diag_nan (for diag = 'U')
    stores NaN on the diagonal.  Returns (crow, col, val, idx)."""
    L = np.asarray(L, dtype=np.float64)
    n = L.shape[0]
    rng = np.random.default_rng([seed, n, int(shuffle), int(junk), 97])
    tri = np.tri(n, dtype=bool)
    mask = ((L != 0) if keep is None else np.asarray(keep, dtype=bool)) & tri
    M = L.copy()
    if diag_nan:
        M[np.arange(n), np.arange(n)] = np.nan
        mask[np.arange(n), np.arange(n)] = True
    forward = uplo == "L"
    idx = np.arange(n) if forward else np.arange(n - 1, -1, -1)
    if not forward:
        M, mask = M[::-1, ::-1], mask[::-1, ::-1]
    crow, col, val = [0], [], []
    for r in range(n):
        cs = np.nonzero(mask[r])[0]
        vs = M[r, cs]
        if junk:
            other = np.arange(r + 1, n) if forward else np.arange(0, r)
            if len(other):
                js = rng.choice(other, min(3, len(other)), replace=False)
                cs, vs = np.concatenate([cs, js]), np.concatenate([vs, np.full(len(js), np.nan)])
        if shuffle and len(cs) > 1:
            p = rng.permutation(len(cs))
            cs, vs = cs[p], vs[p]
        col.extend(cs.tolist())
        val.extend(vs.tolist())
        crow.append(len(col))
    return (np.array(crow, dtype=itype), np.array(col, dtype=itype), np.array(val, dtype=np.float64), idx)


def densify(crow, col, val, uplo="L"):
    """The inverse: (logical dense lower matrix of the entries inside the triangle, duplicates must not occur there;
    list of (physical row, physical column, value) of the entries outside it)."""
    n = len(crow) - 1
    P = np.zeros((n, n))
    outside = []
    for r in range(n):
        for p in range(int(crow[r]), int(crow[r + 1])):
            c = int(col[p])
            inside = c <= r if uplo == "L" else c >= r
            if inside:
                assert P[r, c] == 0.0, "duplicate entry"
                P[r, c] = val[p]
            else:
                outside.append((r, c, float(val[p])))
    return (P if uplo == "L" else P[::-1, ::-1]), outside


def rand53(rng, size=None):
    """doubles in [1, 2) with a random 52-bit fraction and the last bit set: full 53-bit mantissas"""
    k = rng.integers(0, 1 << 51, size=size, dtype=np.int64) * 2 + 1
    return 1.0 + k.astype(np.float64) * 2.0 ** -52


def _system(n, rng, cols_of):
    """L with a diagonal in [1, 2) and, in row i, entries +-[1, 2) / 16 in the columns cols_of(i); b in +-[1, 2)"""
    L = np.zeros((n, n))
    L[np.arange(n), np.arange(n)] = rand53(rng, n)
    for i in range(n):
        cs = np.asarray(cols_of(i), dtype=np.int64)
        if len(cs):
            L[i, cs] = rand53(rng, len(cs)) * rng.choice((-1.0, 1.0), len(cs)) * 2.0 ** -4
    b = rand53(rng, n) * rng.choice((-1.0, 1.0), n)
    return SimpleNamespace(n=n, L=L, b=b)


def chain(n, seed=1):
    """bidiagonal: row i depends on row i - 1 alone"""
    return _system(n, np.random.default_rng([seed, n, 1]), lambda i: [i - 1] if i else [])


def arrow(n, seed=2):
    """a dense first column (every row waits for row 0) and a dense last row (n entries: many steps of the 64-lane form)"""
    return _system(n, np.random.default_rng([seed, n, 2]), lambda i: np.arange(i) if i == n - 1 else ([0] if i else []))


def random_earlier(n, per_row=6, seed=3):
    rng = np.random.default_rng([seed, n, 3])
    return _system(n, rng, lambda i: rng.choice(i, min(i, per_row), replace=False) if i else [])


def block_diagonal(blocks=64, size=5, seed=4):
    """independent dense lower blocks"""
    return _system(blocks * size, np.random.default_rng([seed, blocks, size]), lambda i: np.arange(i - i % size, i))


def diagonal_only(n, seed=5):
    return _system(n, np.random.default_rng([seed, n, 5]), lambda i: [])


def with_duplicates(crow, col, val, every=3):
    """every `every`-th off-diagonal entry a is stored twice, as its upper 26 mantissa bits and the rest: two doubles
    whose exact sum is a.  Returns (crow, col, val, number of entries added)."""
    n = len(crow) - 1
    ncrow, ncol, nval, added, t = [0], [], [], 0, 0
    for r in range(n):
        for p in range(int(crow[r]), int(crow[r + 1])):
            c, a = int(col[p]), float(val[p])
            t += 1
            hi = float((np.array([a]).view(np.int64) & ~np.int64((1 << 27) - 1)).view(np.float64)[0])
            lo = a - hi                                    # exact: hi is a with its low mantissa bits cleared
            if c != r and t % every == 0 and lo != 0.0:
                assert hi + lo == a and hi != 0.0
                ncol += [c, c]
                nval += [hi, lo]
                added += 1
            else:
                ncol.append(c)
                nval.append(a)
        ncrow.append(len(ncol))
    return (np.array(ncrow, dtype=crow.dtype), np.array(ncol, dtype=col.dtype), np.array(nval), added)


def with_second_diagonal(crow, col, val, value=np.nan):
    """a second diagonal entry (`value`) at the END of every row: the first one stays the divisor"""
    n = len(crow) - 1
    ncrow, ncol, nval = [0], [], []
    for r in range(n):
        ncol += col[int(crow[r]):int(crow[r + 1])].tolist() + [r]
        nval += val[int(crow[r]):int(crow[r + 1])].tolist() + [value]
        ncrow.append(len(ncol))
    return np.array(ncrow, dtype=crow.dtype), np.array(ncol, dtype=col.dtype), np.array(nval)


@functools.lru_cache(maxsize=None)
def planted_csr(n, W, mbits, filler, unit, uplo, itype, messy):
    """csr_of_triangular of a planted system (exact_cases.planted_trsv_case), built once per session; messy: the entries
    of each row shuffled, NaN junk in the other triangle and, under diag = 'U', NaN on the stored diagonal"""
    c = X.planted_trsv_case(n, W, mbits, filler, unit)
    return csr_of_triangular(c.L, uplo, itype, shuffle=messy, junk=messy, diag_nan=unit and messy, seed=n)


def upload(csr, n):
    """the device operand (crow, col, val, shape) of a CSR tuple"""
    import torch
    crow, col, val = csr[:3]
    return (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), (n, n))
