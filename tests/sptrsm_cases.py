"""Blocks of right-hand sides for the ExSpTRSM and ExTRSM tests, built from one planted system of exact_cases.planted_trsv.

Column j of the block is, by j % 3, the planted b scaled by s * 2^e, the control b_control scaled the same way, or a
random column of full 53-bit mantissas; (s, e) walks through the signs and SCALES with j // 3.  A power-of-two scaling or
a negation of b scales the whole substitution exactly (every product, every exact total, its rounding and the quotient
scale with it, and nothing here comes near the ends of the double range), so every planted tie stays a tie and the
expected column is s * 2^e * want; tests/test_sptrsm_api.py asserts that through trsv_exact.  The expected control and
random columns always come from exact_cases.trsv_exact.  A column depends on (the system, j) alone, so the block of k
columns is a prefix of every wider one.  Nothing here does arithmetic on the values beyond that exact scaling.

planted_block is the widest block of a planted system with its expected solution, built once per session; solve_block
is the one way both GPU test files put a logical block on the device, solve it in place and read it back."""
import functools
from types import SimpleNamespace

import numpy as np

import exact_cases as X
from helpers import bits
from sptrsv_cases import rand53

SCALES = (0, -3, 5, 40, -200)
KINDS = ("b", "control", "random")


def column_plan(j):
    """(kind, s, e) of column j"""
    t = j // 3
    return KINDS[j % 3], (-1.0 if t % 2 else 1.0), SCALES[t % len(SCALES)]


def rhs_block(case, k, seed=0):
    """B (n x k, C order) for the planted system `case`, with kinds (per column), scale (per column: s * 2^e, 1.0 for a
    random column) and from_b, the number of columns that derive from case.b."""
    n = case.n
    B = np.zeros((n, k))
    kinds, scale = [], np.ones(k)
    for j in range(k):
        kind, s, e = column_plan(j)
        kinds.append(kind)
        if kind == "random":
            rng = np.random.default_rng([seed, n, j, 811])
            B[:, j] = rand53(rng, n) * rng.choice((-1.0, 1.0), n)
        else:
            scale[j] = s * 2.0 ** e
            src = case.b if kind == "b" else case.b_control
            B[:, j] = src * scale[j]                       # exact: a sign and a power of two
            assert (B[:, j] / scale[j] == src).all()
    return SimpleNamespace(B=B, kinds=kinds, scale=scale, from_b=sum(kd == "b" for kd in kinds), k=k)


def expected_block(case, blk, exact_b=False):
    """the expected solution of every column: s * 2^e * case.want for the columns that derive from b (trsv_exact too with
    exact_b), trsv_exact for the control and random columns"""
    want = np.zeros_like(blk.B)
    for j, kind in enumerate(blk.kinds):
        if kind == "b" and not exact_b:
            want[:, j] = case.want * blk.scale[j]
        else:
            want[:, j] = X.trsv_exact(case.L, blk.B[:, j], case.unit)[0]
    return want


@functools.lru_cache(maxsize=None)
def planted_block(case, unit, kmax):
    """(the planted system of TRSV_CASES[case], its widest block with the expected solution in blk.want); narrower blocks
    are prefixes of it"""
    c = X.planted_trsv_case(*X.TRSV_CASES[case], unit)
    blk = rhs_block(c, kmax)
    blk.want = expected_block(c, blk)
    return c, blk


def solve_block(call, clear, B, idx, pad=0, sentinel=-7.25):
    """logical B (n x k) in, logical X out, and the counters.  call(x) solves the device block x in place and returns it,
    clear() asserts that the routine's watchdog is clear and returns its counters; logical row i is physical row idx[i];
    pad: X is the view [:, :k] of a block pad columns wider, filled with the sentinel"""
    import torch
    B = np.asarray(B)
    n, k = B.shape
    wide = np.full((n, k + pad), sentinel)
    wide[idx, :k] = B
    full = torch.from_numpy(wide).cuda()
    x = full[:, :k] if pad else full
    out = call(x)
    assert out is x
    info = clear()
    back = full.cpu().numpy()
    if pad:
        assert (bits(back[:, k:]) == bits(np.full((n, pad), sentinel))).all(), "the padding was written"
    return back[idx, :k], info
