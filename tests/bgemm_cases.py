"""Case helpers of the ExBGEMM tests (no GPU needed here): the dense block X as the CSR matrix of the routine's contract,
the shapes of the planted cases with what is rotated over them, the covering subset of the sizes for the bit identity
with ExSpMM, random blocks with wide exponents."""
import numpy as np

import exact_cases as X

# (rows, q, p) of the planted cases: G = 1 .. 64, a ragged second tile (q = 65), two and three chunks of C (p = 70, 130),
# several row blocks, rows that are no multiple of the rows of a wave
PLANTED_SHAPES = ((67, 1, 5), (67, 5, 12), (130, 17, 16), (67, 33, 33), (67, 64, 64), (40, 65, 7), (40, 9, 70), (24, 3, 130))
PLANTED_S = (54, 63, 80)
PLANTED_YTERM = ((None, 0), ("H", 1), ("d", -0.75))
ALPHAS = (1.0, -1.0, 2.0 ** -7, 2.0 ** 40)
PATHS = (0, 1, 2, 3)

IDENTITY_N = (1, 63, 64, 65, 257, 1031)
IDENTITY_Q = (1, 2, 3, 4, 5, 8, 31, 32, 33, 63, 64, 65, 130)
IDENTITY_P = (0, 1, 3, 4, 5, 63, 64, 65, 129)
IDENTITY_COUNT = 39


def dense_csr(n, p, itype=np.int64):
    """(row_ptr, col_idx) of the n x p CSR matrix that stores every entry of a dense block: row_ptr[r] = r p,
    col_idx = 0 .. p-1 in every row.  The values are the block itself, row by row."""
    crow = (np.arange(n + 1, dtype=np.int64) * p).astype(itype)
    col = np.tile(np.arange(p, dtype=np.int64), n).astype(itype)
    return crow, col


def planted_rotation(i):
    """(S, layout, (plant, beta)) of the i-th planted shape: rotated over the shapes, not crossed, and not in step"""
    return PLANTED_S[i % 3], X.LAYOUTS[(i + i // 3) % 3], PLANTED_YTERM[(i + 2 * (i // 3)) % 3]


def identity_shapes():
    """IDENTITY_COUNT triples (n, q, p): every value of each list occurs, and so does every pair of a q and a p taken from
    the two sides of a seam (4 | 5: path 3; 64 | 65: tiles and chunks of every path)."""
    out = [(IDENTITY_N[i % 6], IDENTITY_Q[i % 13], IDENTITY_P[(2 * i + i // 13) % 9]) for i in range(IDENTITY_COUNT - 8)]
    seams = [(q, p) for q in (4, 5) for p in (4, 5)] + [(q, p) for q in (64, 65) for p in (64, 65)]
    out += [(IDENTITY_N[(i + 2) % 6], q, p) for i, (q, p) in enumerate(seams)]
    return out


def wide_block(rng, rows, cols, span=200):
    """53-bit random mantissas of either sign times 2^e, e uniform in [-span, span]"""
    m = rng.standard_normal((rows, cols))
    return np.ldexp(m, rng.integers(-span, span + 1, (rows, cols)))
