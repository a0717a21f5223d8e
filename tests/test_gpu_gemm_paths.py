"""ExGEMM's path table (exblas_set_gemm_path) at every knob value, both rounding modes and all four transposes.

Operands hold integers in [-8, 8] with k = 64, so every path qualifies and the exact product is an int64 product.  Per
call: the path exblas_last_gemm_info reports, every bit of C, and the untouched padding of C (ldc = n + 2).  The table:

    knob 0            residues when min(m, n) >= 192 (CRT_MIN_EDGE), digit slices below
    knob 4            residues
    knob 1            scalar kernel
    knob 3            fp64 slices in exact rounding mode, scalar kernel in reference mode
    knob 2, any other digit slices (-1 and 5 included)
"""
import ctypes as C

import numpy as np
import pytest

from helpers import assert_bits, bits

pytestmark = pytest.mark.gpu

K = 64
SHAPES = [(191, 200), (192, 192)]
KNOBS = [-1, 0, 1, 2, 3, 4, 5]
PAD = -7.25                                   # the padding of C: any value the call must leave alone


def expected_path(knob, m, n, round_mode):
    """exblas_last_gemm_info out[0]: 0 scalar kernel, 1 fp64 slices, 2 int8 digit slices, 4 int8 residues"""
    if knob == 1:
        return 0
    if knob == 3:
        return 1 if round_mode == 0 else 0
    if knob == 4 or (knob == 0 and min(m, n) >= 192):
        return 4
    return 2


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    return exblas_amd


@pytest.fixture(scope="module")
def operands():
    """per shape: A (m x k), B (k x n) and their exact product, shared by every case"""
    rng = np.random.default_rng(20261020)
    out = {}
    for m, n in SHAPES:
        a = rng.integers(-8, 9, size=(m, K)).astype(np.int64)
        b = rng.integers(-8, 9, size=(K, n)).astype(np.int64)
        out[(m, n)] = (a.astype(np.float64), b.astype(np.float64), (a @ b).astype(np.float64))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("knob", KNOBS)
def test_gemm_path_table(ex, operands, knob, shape):
    import torch
    L = ex.load_library()
    m, n = shape
    a, b, want = operands[shape]
    c0 = np.full((m, n + 2), PAD)
    c0[:, :n] = 1.5                           # beta = 0: the old body must not show through
    try:
        L.exblas_set_gemm_path(knob)
        for round_mode in (0, 1):
            L.exblas_set_round_mode(round_mode)
            for ta in "NT":
                for tb in "NT":
                    sa = np.ascontiguousarray(a.T if ta == "T" else a)
                    sb = np.ascontiguousarray(b.T if tb == "T" else b)
                    Ad, Bd = torch.from_numpy(sa).cuda(), torch.from_numpy(sb).cuda()
                    Cd = torch.from_numpy(c0.reshape(-1).copy()).cuda()
                    ex.exgemm_dev(ta, tb, m, n, K, 1.0, Ad, sa.shape[1], Bd, sb.shape[1], 0.0, Cd, n + 2)
                    info = (C.c_int * 8)()
                    assert L.exblas_last_gemm_info(info) == 0
                    what = (knob, shape, round_mode, ta + tb)
                    assert info[0] == expected_path(knob, m, n, round_mode), (what, list(info))
                    got = Cd.cpu().numpy().reshape(m, n + 2)
                    assert_bits(got[:, :n], want, what)
                    assert (bits(got[:, n:]) == bits(c0[:, n:])).all(), ("the padding of C was written", what)
    finally:
        L.exblas_set_gemm_path(0)
        L.exblas_set_round_mode(0)
