"""ExGEMV / ExGEMM on constructed ties and worst-case operands (tests/exact_cases.py), bit for bit.

Random 53-bit mantissas practically never put an exact dot product on a tie, one unit next to a tie, on a carry into
the next binade or at the largest magnitude a fixed-point path is sized for; these inputs do, on every internal path.
Expected bits: the Python-integer reference for ROUND_EXACT, the oracle for ROUND_REFERENCE.  No tolerance, no case
filtered at run time; the (path, case) pairs that must decline to the scalar kernel are written out below."""
import ctypes as C

import numpy as np
import pytest

import exact_cases as X
from test_gpu_blas23 import GEMM_VARIANTS, GEMV_VARIANTS

pytestmark = pytest.mark.gpu

TRANSPOSES = (("N", "N"), ("N", "T"), ("T", "N"), ("T", "T"))


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    return exblas_amd


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _info(lib):
    v = (C.c_int * 8)()
    assert lib.exblas_last_gemm_info(v) == 0
    return list(v)


def _expect_path(lib, path, case, k, mode):
    """What exblas_last_gemm_info must report for a forced path on an operand pair of case.bits_a / bits_b bits.
    Declines (scalar kernel, same bits), all of them: path 3 (21-bit fp64 slices, at most 4 per operand = 84 bits, exact
    rounding mode only) on more than 84 bits or in the reference rounding mode.  Everything else is inside the forced
    path's documented domain (finite normal entries, exponents within +-300, at most 126 bits per operand)."""
    info = _info(lib)
    assert max(case.bits_a, case.bits_b) <= 126
    if path == 1:
        assert info[0] == 0, info
    elif path == 2:
        da, db = (case.bits_a + 2 + 7) // 8, (case.bits_b + 2 + 7) // 8     # span + 2 bits in 8-bit digits, at most 16
        assert info[0] == 2 and da <= info[1] <= min(16, max(da, db) + 1) and db <= info[2] <= min(16, max(da, db) + 1), info
    elif path == 3:
        if max(case.bits_a, case.bits_b) > 84 or mode != 0:
            assert info[0] == 0, info
        else:
            slices = max(2, (max(case.bits_a, case.bits_b) + 20) // 21)
            assert info[:3] == [1, slices, slices], info
    else:
        assert info[0] == 4 and info[1:3] == [case.bits_a, case.bits_b], info
        assert info[3] == X.crt_moduli_needed(case.bits_a, case.bits_b, k), info
    return info


def _run_gemm(ex, lib, oracle, case, path, mode, ta, tb, fpe, ee, want):
    a, lda = X.gemm_operand(case.a, ta, 1)
    b, ldb = X.gemm_operand(case.b, tb, 2)
    ldc = case.n + 3
    c = np.full(case.m * ldc, -7.0)                         # beta = 0: the old C is ignored, its padding is kept
    ex.exgemm(ta, tb, case.m, case.n, case.k, 1.0, a, lda, b, ldb, 0.0, c, ldc, fpe, ee)
    info = _expect_path(lib, path, case, case.k, mode)
    got = c.reshape(case.m, ldc)
    assert (got[:, case.n:] == -7.0).all()
    bad = _bits(got[:, :case.n]) != _bits(want)
    assert not bad.any(), (path, mode, ta, tb, fpe, ee, info, int(bad.sum()),
                           sorted(set(case.classes[bad].tolist())), got[:, :case.n][bad][:3], want[bad][:3])


def _ref_mode_want(oracle, case):
    w = oracle.exgemm("N", "N", case.m, case.n, case.k, 1.0, case.a.reshape(-1), case.k, case.b.reshape(-1), case.n, 0.0,
                      np.zeros(case.m * case.n), case.n, 0, mode=oracle.ROUND_REFERENCE).reshape(case.m, case.n)
    assert not np.isnan(w).any()
    return w


@pytest.mark.parametrize("S", [54, 100, 118])
@pytest.mark.parametrize("path,m,n", [(1, 37, 50), (2, 37, 50), (3, 37, 50), (4, 37, 50), (4, 131, 67), (0, 197, 203)])
def test_exgemm_planted_ties(ex, oracle, path, m, n, S):
    """Every output is an exact tie (to even downwards, to even upwards, carrying into the next binade), one integer unit
    off a tie with the deciding bit S - 34 bits below the rounding position, a cancellation to zero or a short exact
    value: forced scalar kernel (1), digit slices (2), fp64 slices (3), residues (4) and the default dispatch at
    min(m, n) >= 192 (0: residues).  All four transposes with padded leading dimensions, every (fpe, early_exit), k below
    and above the 8192 of one contraction pass with H and the deciding unit in different passes, ragged m, n."""
    lib = ex.load_library()
    forced = 4 if path == 0 else path
    cases = [X.planted_gemm(m, n, 300, S, seed=3, layout="split"),
             X.planted_gemm(m if path else 40, n if path else 48, 9000, S, seed=4, layout="head"),
             X.planted_gemm(m if path else 40, n if path else 48, 8193, S, seed=5, layout="tail", ea=-40, eb=25)]
    try:
        for ci, case in enumerate(cases):
            X.planted_mix(case)
            if path == 0 and ci > 0:                       # small shapes: the default dispatch is the digit path there
                forced = 2
            lib.exblas_set_gemm_path(path)
            lib.exblas_set_round_mode(0)
            pairs = TRANSPOSES if ci == 0 else (TRANSPOSES[ci], TRANSPOSES[3 - ci])
            for ti, (ta, tb) in enumerate(pairs):
                variants = GEMM_VARIANTS if ci == 0 else [GEMM_VARIANTS[(ti + 3 * ci) % 7], GEMM_VARIANTS[(ti + 4) % 7]]
                for fpe, ee in variants:
                    _run_gemm(ex, lib, oracle, case, forced, 0, ta, tb, fpe, ee, case.want)
            lib.exblas_set_round_mode(1)
            want = _ref_mode_want(oracle, case)
            for ti, (ta, tb) in enumerate(pairs):
                fpe, ee = GEMM_VARIANTS[(2 * ti + ci) % 7]
                _run_gemm(ex, lib, oracle, case, forced, 1, ta, tb, fpe, ee, want)
    finally:
        lib.exblas_set_gemm_path(0)
        lib.exblas_set_round_mode(0)


def test_exgemm_worst_case_magnitudes(ex, oracle):
    """For every L from 2 to 36 an operand pair with bits(A) + bits(B) + ceil(log2 k) + 2 == bits[L] exactly and every
    entry at the largest magnitude those widths admit: the residue path must take exactly L moduli (the tight case of
    its |value| < M / 4 reconstruction: the largest sums reach 0.90 .. 0.97 of M_L / 4 for the L whose M_L is barely
    above 2^bits[L]), across the limb buckets of its finish kernel (L <= 18, <= 25, above) and the k-pass boundary.  The
    same operands through the digit slices (every base-256 digit 255: the largest int32 partial sums) and the scalar
    kernel.  Both rounding modes."""
    lib = ex.load_library()
    try:
        for L in range(2, 37):
            case = X.crt_worst_case(L)
            wants = {0: case.want, 1: _ref_mode_want(oracle, case)}
            for mode in (0, 1):
                lib.exblas_set_round_mode(mode)
                for path in (4, 2, 1):
                    lib.exblas_set_gemm_path(path)
                    c = np.full(case.m * case.n, -7.0)
                    ex.exgemm("N", "N", case.m, case.n, case.k, 1.0, case.a.reshape(-1), case.k, case.b.reshape(-1), case.n,
                              0.0, c, case.n, 8, True)
                    info = _expect_path(lib, path, case, case.k, mode)
                    if path == 4:
                        assert info[3] == L and info[1:3] == [case.na, case.nb], (L, info)
                    bad = _bits(c) != _bits(wants[mode].reshape(-1))
                    assert not bad.any(), (L, path, mode, info, (case.na, case.nb, case.k), int(bad.sum()),
                                           sorted(set(case.classes.reshape(-1)[bad].tolist())))
    finally:
        lib.exblas_set_gemm_path(0)
        lib.exblas_set_round_mode(0)


@pytest.mark.parametrize("k", [8192, 8193])
def test_exgemm_residue_128_wraps(ex, oracle, k):
    """Every entry = 128 (mod 256) in the path's integer units: the symmetric residue +128 of p = 256 is stored as the
    int8 -128, and at k = 8192 that modulus's int32 contraction reaches exactly 2^27; k = 8193 adds a second pass."""
    lib = ex.load_library()
    case = X.crt_wrap_case(k)
    try:
        for ta, tb in (("N", "N"), ("T", "T")):
            for path in (4, 2, 1):
                lib.exblas_set_gemm_path(path)
                _run_gemm(ex, lib, oracle, case, path, 0, ta, tb, 8, True, case.want)
    finally:
        lib.exblas_set_gemm_path(0)


# outputs, inner, S, layout, plant, beta, pad (lda = m + pad), offa, incx, offx, incy, offy
GEMV_PLANTED = [
    (40, 3001, 54, "split", None, 0, 2, 0, 1, 0, 1, 0),        # 'N': m, lda even, aligned: k_gemvN_fpe_sx; KS > 1
    (40, 3001, 118, "split", "H", 1, 2, 0, 1, 0, 1, 0),        # half a unit in y, leading part and deciding unit in different k segments
    (41, 2900, 100, "head", "d", 1, 2, 0, 1, 0, 1, 0),         # 'N': m odd: k_gemvN_fpe; the deciding unit in y
    (40, 3001, 100, "tail", "d", -0.75, 1, 0, 2, 1, 3, 2),     # 'N': lda odd; TwoProd(beta, y); strides and offsets
    (48, 3001, 54, "split", "H", -0.75, 0, 1, 1, 2, 2, 1),     # 'N': misaligned base
    (64, 300, 118, "head", None, 0, 2, 0, 1, 0, 1, 0),         # short rows
]


def _run_gemv(ex, oracle, g, x, y0, beta, want, want_ref, lay, variants, tag):
    lib = ex.load_library()
    pad, offa, incx, offx, incy, offy = lay
    for trans in ("N", "T"):
        m, n, a, lda, xs, ys = X.gemv_operands(g, x, y0, trans, pad=pad, offa=offa, incx=incx, offx=offx, incy=incy, offy=offy)
        for mode, expect in ((0, want), (1, want_ref)):
            if mode == 1 and expect is None:
                expect = oracle.exgemv(trans, m, n, 1.0, a, lda, xs, beta, ys, 0, incx=incx, incy=incy, offa=offa, offx=offx,
                                       offy=offy, mode=oracle.ROUND_REFERENCE)[offy::incy]
                assert not np.isnan(expect).any()
            lib.exblas_set_round_mode(mode)
            full = ys.copy()
            full[offy::incy] = expect
            for fpe, ee in (variants if mode == 0 else variants[::3]):
                y = ys.copy()
                ex.exgemv(trans, m, n, 1.0, a, lda, offa, xs, incx, offx, beta, y, incy, offy, fpe, ee)
                bad = _bits(y) != _bits(full)
                assert not bad.any(), (tag, trans, mode, fpe, ee, np.nonzero(bad)[0][:8], y[bad][:4], full[bad][:4])


@pytest.mark.parametrize("outputs,inner,S,layout,plant,beta,pad,offa,incx,offx,incy,offy", GEMV_PLANTED)
def test_exgemv_planted_ties(ex, oracle, outputs, inner, S, layout, plant, beta, pad, offa, incx, offx, incy, offy):
    """The planted classes per output of ExGEMV 'N' (each of its three kernels, the row split over KS > 1 workgroups with
    the high part, the half unit and the deciding unit in different k segments or in y) and 'T', every variant."""
    lib = ex.load_library()
    case = X.planted_gemv(outputs, inner, S, seed=6, layout=layout, plant=plant, beta=beta)
    X.planted_mix(case)
    if inner >= 2900 and layout != "tail":                 # the planted columns are further apart than any k segment
        p = sorted(case.pos[name] for name in ("lead", "H", "d"))
        assert min(p[1] - p[0], p[2] - p[1]) > 1000
    try:
        _run_gemv(ex, oracle, case.g, case.x, case.y0, case.beta, case.want, None, (pad, offa, incx, offx, incy, offy),
                  GEMV_VARIANTS, (outputs, inner, S, layout, plant, beta))
    finally:
        lib.exblas_set_round_mode(0)


@pytest.mark.parametrize("inner", [12, 3000])
def test_exgemv_result_range_rows(ex, oracle, inner):
    """Rows whose exact sum is a subnormal, the largest subnormal, the smallest normal, DBL_MAX, the tie at the overflow
    threshold (+-inf) or finite although partial sums leave the double range -- every product exact for TwoProd."""
    lib = ex.load_library()
    r = X.range_rows_gemv(inner)
    try:
        for beta, want in ((0.0, r.want), (1.0, r.want_with_y)):
            for lay in ((0, 0, 1, 0, 1, 0), (1, 1, 2, 1, 3, 2)):
                _run_gemv(ex, oracle, r.g, r.x, r.y0, beta, want, None, lay, GEMV_VARIANTS, ("range", inner, beta, r.names))
    finally:
        lib.exblas_set_round_mode(0)


def test_exgemv_planted_ties_on_a_context(ex, oracle):
    """the same through exblas_exgemv_ctx on device tensors (its own workspace and stream)"""
    import torch
    case = X.planted_gemv(40, 3001, 100, seed=7, layout="split", plant="H", beta=1)
    X.planted_mix(case)
    ctx = ex.Context()
    try:
        for trans in ("N", "T"):
            m, n, a, lda, xs, ys = X.gemv_operands(case.g, case.x, case.y0, trans, pad=2)
            A, Xd = torch.from_numpy(a).cuda(), torch.from_numpy(xs).cuda()
            for fpe, ee in ((8, True), (0, False), (3, False)):
                Y = torch.from_numpy(ys).cuda()
                ctx.exgemv(trans, m, n, 1.0, A, lda, Xd, 1.0, Y, fpe, ee)
                torch.cuda.synchronize()
                assert (_bits(Y.cpu().numpy()) == _bits(case.want)).all(), (trans, fpe, ee)
                Y = torch.from_numpy(ys).cuda()
                ex.exgemv_dev(trans, m, n, 1.0, A, lda, Xd, 1.0, Y, fpe, ee)
                torch.cuda.synchronize()
                assert (_bits(Y.cpu().numpy()) == _bits(case.want)).all(), (trans, fpe, ee)
    finally:
        ctx.destroy()
