"""ExTRSM on the GPU: every column bit for bit against exact_cases.trsv_exact, and against ExTRSV on that column.

The planted systems of the ExTRSV tests run with blocks of right-hand sides (tests/sptrsm_cases.py: the planted b and its
control under exact scalings, and random columns), so that ties, carries and near-ties sit in many columns of one wave at
once, next to columns the register test certifies, in all four (uplo, transa) with NaN in everything that must not be
read.  The counters keep the file from passing by luck: a tie decided in registers fails even where round-to-even
happens to give the right bits.  Then the slice, tile and panel boundaries in k and the row-group boundaries in n against
ExTRSV itself (non-finite columns included), the empty sizes, the padding of a wider block, the ends of the double range
as blocks, the reference rounding mode against the oracle, a row-major A, and the plumbing (context, stream, host
arrays, graph capture, workspace).  Expected bits never come from the code under test.  After every solve the watchdog
flag is read: it is never set."""
import ctypes
import functools

import numpy as np
import pytest

import exact_cases as X
import sptrsm_cases as M
import sptrsv_cases as S
from helpers import assert_bits as _same, bits as _bits
from sptrsm_cases import planted_block as _block   # the blocks of the planted systems, built once per session

pytestmark = pytest.mark.gpu

CASE_IDS = [f"n{n}-W{W}-m{mb}{'-filler' if fl else ''}" for n, W, mb, fl in X.TRSV_CASES]
ORIENT = (("L", "N"), ("U", "N"), ("L", "T"), ("U", "T"))
VARIANTS = ((8, True), (3, True), (0, False))
KS = (3, 8, 33, 65)
# (uplo, transa, path, (fpe, early_exit)): every orientation, every path and every variant class occur
COMBOS = (("L", "N", 0, (8, True)), ("U", "N", 0, (3, True)), ("L", "T", 1, (8, True)), ("U", "T", 2, (0, False)),
          ("L", "N", 3, (8, True)), ("U", "T", 3, (3, True)), ("L", "T", 0, (0, False)), ("U", "N", 2, (8, True)))
MAILBOX_BYTES = 64 << 20


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_trsm_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _clear(ex):
    """the watchdog of the last ExTRSM is clear (the C entry returns 0, the Python one does not raise); the counters"""
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_trsm_info(out) == 0, "the watchdog was raised"
    info = tuple(int(v) for v in out)
    assert ex.last_trsm_info() == info and info[2] == 0 and info[3] == 0
    return info


def _matrix(L, uplo, trans, diag="N", lda_pad=0):
    """the device operand of the logical lower system L: a column-major view (strides (1, lda)) of ExTRSV's storage, with
    NaN in the other triangle, in the lda padding and on the diagonal under 'U'; idx: logical row i is physical idx[i]"""
    import torch
    n = L.shape[0]
    a, lda, _, idx = X.trsv_operands(L, np.zeros(n), uplo, trans, diag, lda_pad=lda_pad)
    flat = torch.from_numpy(a).cuda()
    return torch.as_strided(flat, (n, n), (1, lda)), flat, lda, idx


def _solve(ex, A, B, idx, uplo, trans, diag="N", fpe=8, ee=True, entry=None, pad=0, sentinel=-7.25):
    """logical B (n x k) in, logical X out, and the counters; pad: X is the view [:, :k] of a block pad columns wider"""
    call = entry or ex.extrsm_dev
    return M.solve_block(lambda x: call(A, x, uplo, trans, diag, fpe, ee), lambda: _clear(ex), B, idx, pad, sentinel)


# ---------------------------------------------------------------------------------------------
# planted systems
# ---------------------------------------------------------------------------------------------
def _planted(ex, case, unit, k, kmax, combos):
    n, W, mbits, filler = X.TRSV_CASES[case]
    c, blk = _block(case, unit, kmax)
    B, want = blk.B[:, :k], blk.want[:, :k]
    from_b = sum(kd == "b" for kd in blk.kinds[:k])
    diag = "U" if unit else "N"
    ties = int(((c.classes == "tie") | (c.classes == "carry")).sum())
    seen = []
    try:
        for uplo, trans, path, (fpe, ee) in combos:
            A, _, _, idx = _matrix(c.L, uplo, trans, diag, lda_pad=case % 3)
            ex.set_trsm_path(path)
            got, info = _solve(ex, A, B, idx, uplo, trans, diag, fpe, ee)
            what = (n, W, k, unit, uplo, trans, path, fpe, ee, info)
            _same(got, want, what)
            assert info[0] + info[1] == n * k, what
            if path == 1 or fpe == 0:
                assert info[0] == 0, what
            else:
                assert info[1] >= ties * from_b, ("a tie was decided in registers", what)
            seen.append(info[1])
    finally:
        ex.set_trsm_path(0)
    print(f"planted {CASE_IDS[case]} unit={unit} k={k}: ties {ties} x {from_b} columns, accumulator outputs "
          f"{min(seen)}..{max(seen)} of {n * k}")


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", range(5), ids=CASE_IDS[:5])
def test_planted_blocks_every_path_width_and_orientation(ex, case, k, unit):
    _planted(ex, case, unit, k, max(KS), COMBOS)


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("case", [5, 6], ids=[CASE_IDS[5], CASE_IDS[6]])
def test_planted_blocks_many_row_groups(ex, case, unit):
    _planted(ex, case, unit, 5, 5, COMBOS)


@pytest.mark.parametrize("case", range(5), ids=CASE_IDS[:5])
def test_control_columns_are_decided_in_registers(ex, case):
    """a block of control columns only (every planted b_ij a quarter unit off its tie): the counter discriminates"""
    n = X.TRSV_CASES[case][0]
    for unit in (False, True):
        c, blk = _block(case, unit, max(KS))
        cols = [j for j, kd in enumerate(blk.kinds) if kd == "control"][:9]
        B, want = np.ascontiguousarray(blk.B[:, cols]), blk.want[:, cols]
        diag = "U" if unit else "N"
        try:
            for t, (uplo, trans) in enumerate(ORIENT):
                A, _, _, idx = _matrix(c.L, uplo, trans, diag)
                for path in (0, 2, 3):
                    ex.set_trsm_path(path)
                    got, info = _solve(ex, A, B, idx, uplo, trans, diag, *VARIANTS[(t + path) % 2])
                    _same(got, want, ("control", n, uplo, trans, unit, path, info))
                    assert info[0] > 0 and info[0] + info[1] == n * len(cols), ("control", n, uplo, trans, unit, path, info)
        finally:
            ex.set_trsm_path(0)


# ---------------------------------------------------------------------------------------------
# bit identity with ExTRSV, column by column, at the slice, tile, panel and row-group boundaries
# ---------------------------------------------------------------------------------------------
K_BOUNDS = (1, 2, 3, 5, 8, 17, 32, 33, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def _dense(n):
    rng = np.random.default_rng([n, 77])
    s = S._system(n, rng, lambda i: np.arange(i))                # dense lower: every dependency there is
    s.B = S.rand53(rng, (n, max(K_BOUNDS))) * rng.choice((-1.0, 1.0), (n, max(K_BOUNDS)))
    return s


def _extrsv_columns(ex, A_flat, lda, B, idx, uplo, trans, diag="N"):
    """ExTRSV on every column of the block in place (x = X + j, incx = ldx): the reference of the contract"""
    import torch
    n, k = B.shape
    phys = np.empty_like(B)
    phys[idx] = B
    Xr = torch.from_numpy(phys).cuda()
    for j in range(k):
        assert ex.extrsv_dev(uplo, trans, diag, n, A_flat, lda, Xr[:, j], 8, True, incx=Xr.stride(0)) == 0
    torch.cuda.synchronize()
    return Xr.cpu().numpy()[idx]


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 130])
def test_every_column_equals_extrsv(ex, n):
    s = _dense(n)
    try:
        for t, (uplo, trans) in enumerate(ORIENT):
            A, flat, lda, idx = _matrix(s.L, uplo, trans, lda_pad=3)
            assert lda == n + 3
            ref = _extrsv_columns(ex, flat, lda, s.B, idx, uplo, trans)
            assert np.isfinite(ref).all()
            for i, k in enumerate(K_BOUNDS):
                for path in ((0, 2, 3, 1)[(i + t) % 4], 0):
                    ex.set_trsm_path(path)
                    got, info = _solve(ex, A, s.B[:, :k], idx, uplo, trans, "N", *VARIANTS[(i + path) % 3])
                    _same(got, ref[:, :k], ("dense", n, uplo, trans, k, path, info))
                    assert info[0] + info[1] == n * k
    finally:
        ex.set_trsm_path(0)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 130])
def test_non_finite_columns_follow_extrsv_and_stay_in_their_column(ex, n):
    """one column holds an Inf in one row, one column is all NaN: where the results are not finite, and with which sign,
    is ExTRSV's (a zero entry times an infinite x counts), and every other column keeps the bits of the clean run"""
    s = _dense(n)
    try:
        for t, (uplo, trans) in enumerate(ORIENT):
            A, flat, lda, idx = _matrix(s.L, uplo, trans, lda_pad=3)
            clean = _extrsv_columns(ex, flat, lda, s.B[:, :9], idx, uplo, trans)
            for k, path in ((9, (0, 3)[t % 2]), (65, (2, 0)[t % 2]), (33, 1)):
                B = s.B[:, :k].copy()
                B[:, 2] = np.nan
                B[n // 3, 5] = -np.inf if t % 2 else np.inf
                ref = _extrsv_columns(ex, flat, lda, B[:, :9], idx, uplo, trans)
                assert np.isnan(ref[:, 2]).all() and not np.isfinite(ref[n // 3:, 5]).all()
                keep = np.ones(9, dtype=bool)
                keep[[2, 5]] = False
                assert (_bits(ref[:, keep]) == _bits(clean[:, keep])).all()
                ex.set_trsm_path(path)
                got, info = _solve(ex, A, B, idx, uplo, trans)
                _same(got[:, :9], ref, ("non-finite", n, uplo, trans, k, path))
                assert info[0] + info[1] == n * k
                if k > 9:                                        # the columns beyond: untouched by the two
                    ex.set_trsm_path(0)
                    plain, _ = _solve(ex, A, s.B[:, :k], idx, uplo, trans)
                    _same(got[:, 9:], plain[:, 9:], ("independent", n, uplo, trans, k, path))
    finally:
        ex.set_trsm_path(0)


# ---------------------------------------------------------------------------------------------
# empty sizes, padding
# ---------------------------------------------------------------------------------------------
def test_empty_sizes_launch_nothing(ex):
    import torch
    A0 = torch.zeros(0, 0, dtype=torch.float64).cuda()
    for k in (0, 1, 5, 65):
        x = torch.zeros(0, k, dtype=torch.float64).cuda()
        assert ex.extrsm_dev(A0, x) is x and _clear(ex) == (0, 0, 0, 0)
    s = _dense(9)
    A, _, _, idx = _matrix(s.L, "L", "N")
    _solve(ex, A, s.B[:, :3], idx, "L", "N")                     # a call that counts, then one that launches nothing
    x = torch.zeros(9, 0, dtype=torch.float64).cuda()
    assert ex.extrsm_dev(A, x, "L", "N") is x and _clear(ex) == (0, 0, 0, 0)
    lib = ex.load_library()
    assert lib.exblas_extrsm_dev(b"L", b"N", b"N", 0, 0, None, 1, None, 0, 8, 1, None) == 0
    assert ex.extrsm(np.zeros((0, 0)), np.zeros((0, 5))).shape == (0, 5)
    assert ex.extrsm(np.tril(s.L), np.zeros((9, 0)), "L").shape == (9, 0)


@pytest.mark.parametrize("k", [1, 5, 64, 67])
def test_padding_of_a_wider_block_keeps_its_bits(ex, k):
    """X is the view [:, :k] of an (n, k + 3) block: the three columns beyond it are neither read (NaN there changes
    nothing) nor written; path 3 puts panel seams inside the block"""
    c, blk = _block(2, False, max(KS))
    B, want = blk.B[:, :min(k, 65)], blk.want[:, :min(k, 65)]
    if k > 65:
        B, want = np.hstack([B, blk.B[:, :k - 65]]), np.hstack([want, blk.want[:, :k - 65]])
    try:
        for uplo, trans, path in (("L", "N", 0), ("U", "T", 3), ("L", "T", 1), ("U", "N", 2)):
            A, _, _, idx = _matrix(c.L, uplo, trans, lda_pad=2)
            ex.set_trsm_path(path)
            for sentinel in (-7.25, np.nan):
                got, _ = _solve(ex, A, B, idx, uplo, trans, pad=3, sentinel=sentinel)
                _same(got, want, ("ldx > k", k, uplo, trans, path, sentinel))
    finally:
        ex.set_trsm_path(0)


# ---------------------------------------------------------------------------------------------
# the ends of the double range, as blocks of 3 columns
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 58, 70])
def test_range_rows(ex, lead):
    """overflow ties, totals either side of 2^1000, subnormal totals and quotients, the sign of a zero by cancellation:
    the column itself, its negation (expected from trsv_exact: a zero total keeps its + sign) and the column again"""
    r = X.range_rows_trsv(lead)
    B = np.stack([r.b, -r.b, r.b], axis=1)
    want = np.stack([r.want, X.trsv_exact(r.L, -r.b)[0], r.want], axis=1)
    try:
        for uplo, trans in ORIENT:
            A, _, _, idx = _matrix(r.L, uplo, trans, lda_pad=lead % 4)
            for path in (0, 1, 2, 3):
                ex.set_trsm_path(path)
                for fpe, ee in VARIANTS:
                    got, _ = _solve(ex, A, B, idx, uplo, trans, "N", fpe, ee)
                    bad = (_bits(got) != _bits(want)).any(axis=1)
                    assert not bad.any(), (lead, uplo, trans, path, fpe, ee, [nm for nm in r.names if bad[r.rows[nm]]],
                                           got[bad], want[bad])
    finally:
        ex.set_trsm_path(0)


# ---------------------------------------------------------------------------------------------
# rounding mode, layouts, plumbing, graphs, the plain solve, the unsupported variants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 2], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_planted_reference_rounding_mode(ex, oracle, case):
    """ties are where the two rounding modes differ: every column follows the oracle's reference-mode substitution"""
    n = X.TRSV_CASES[case][0]
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        differs = 0
        for unit in (False, True):
            c, blk = _block(case, unit, max(KS))
            k, diag = 6, "U" if unit else "N"
            want = np.empty((n, k))
            for j in range(k):
                a, lda, xs, idx = X.trsv_operands(c.L, blk.B[:, j], "L", "N", diag)
                rc, w = oracle.extrsv("L", "N", diag, n, a, lda, xs, 0, mode=oracle.ROUND_REFERENCE)
                assert rc == 0
                want[:, j] = w[idx]
            differs += int((_bits(want) != _bits(blk.want[:, :k])).sum())
            for t, (uplo, trans) in enumerate(ORIENT):
                A, _, _, idx = _matrix(c.L, uplo, trans, diag)
                for path in (0, 2, 3):
                    ex.set_trsm_path(path)
                    fpe, ee = VARIANTS[(t + path) % 3]
                    got, info = _solve(ex, A, blk.B[:, :k], idx, uplo, trans, diag, fpe, ee)
                    _same(got, want, ("reference mode", n, uplo, trans, unit, path, fpe, ee))
                    assert info[0] == 0 and info[1] == n * k
        assert differs >= 1, "the reference rounding mode never differed from the exact one on these ties"
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_trsm_path(0)


def test_row_major_and_column_major_tensors_give_the_same_bits(ex):
    """the same logical system as a C-contiguous tensor and as its column-major copy, for both uplo and both trans"""
    c, blk = _block(2, False, max(KS))
    B, want = blk.B[:, :8], blk.want[:, :8]
    for uplo, trans in ORIENT:
        A, _, _, idx = _matrix(c.L, uplo, trans, lda_pad=1)      # strides (1, n + 1): column-major
        R = A.contiguous()                                       # strides (n, 1): the same A[i, j], row-major
        assert A.stride(0) == 1 and R.stride(1) == 1 and R.stride(0) == c.n
        got_c, _ = _solve(ex, A, B, idx, uplo, trans)
        got_r, _ = _solve(ex, R, B, idx, uplo, trans)
        _same(got_c, want, ("column-major", uplo, trans))
        assert (_bits(got_r) == _bits(got_c)).all(), ("row-major", uplo, trans)


def test_runs_contexts_streams_host_arrays_and_workspace_agree(ex):
    import torch
    c, blk = _block(3, False, max(KS))
    n = c.n
    B, want = blk.B[:, :8], blk.want[:, :8]
    for uplo, trans in (("L", "N"), ("U", "T")):
        A, _, lda, idx = _matrix(c.L, uplo, trans)
        first, _ = _solve(ex, A, B, idx, uplo, trans)
        again, _ = _solve(ex, A, B, idx, uplo, trans)
        _same(first, want, ("dev", uplo, trans))
        assert (_bits(first) == _bits(again)).all()
        assert ex.load_library().exblas_workspace_bytes() >= 256 + 8 * n * 8
        ctx, side = ex.Context(), torch.cuda.Stream()
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                got, _ = _solve(ex, A, B, idx, uplo, trans, entry=ctx.extrsm)
            side.synchronize()
            assert (_bits(got) == _bits(first)).all(), ("context on a side stream", uplo, trans)
            assert ctx.workspace_bytes() >= 256 + 8 * n * 8
        finally:
            torch.cuda.synchronize()
            ctx.destroy()
        # host arrays: the Python-indexed matrix (NaN where it must not be read), C order and Fortran order
        host_a = A.cpu().numpy()
        Xs = np.empty((n, 8))
        Xs[idx] = B
        keep = Xs.copy()
        for arr in (np.ascontiguousarray(host_a), np.asfortranarray(host_a)):
            host = ex.extrsm(arr, Xs, uplo, trans)
            assert (_bits(Xs) == _bits(keep)).all() and host is not Xs
            assert (_bits(host[idx]) == _bits(first)).all(), ("host arrays", uplo, trans)
            _clear(ex)
    # a panel narrower than k: the workspace holds one panel
    panel = max(64, MAILBOX_BYTES // (8 * n) // 64 * 64)
    assert ex.load_library().exblas_workspace_bytes() >= 256 + 8 * n * min(8, panel)


def test_host_entry_keeps_the_padding_of_x(ex):
    """the C host entry with ldx > k: the padding comes back as it went"""
    s = _dense(9)
    a, lda, _, idx = X.trsv_operands(s.L, np.zeros(9), "U", "N", lda_pad=2)
    ref = np.stack([X.trsv_exact(s.L, s.B[:, j])[0] for j in range(5)], axis=1)
    wide = np.full((9, 8), -7.25)
    wide[idx, :5] = s.B[:, :5]
    lib = ex.load_library()
    rc = lib.exblas_extrsm(b"U", b"N", b"N", 9, 5, ctypes.c_void_p(a.ctypes.data), lda, ctypes.c_void_p(wide.ctypes.data), 8,
                           8, 1)
    assert rc == 0
    _same(wide[idx, :5], ref, "host entry, ldx = 8")
    assert (wide[:, 5:] == -7.25).all()


def test_graph_capture_after_one_warm_call(ex):
    """(Four replays on a changing triangle, several panels and a dirty workspace between replays:
    tests/test_gpu_graph_replay_solves.py.)"""
    import torch
    c, blk = _block(4, False, max(KS))
    n, k = c.n, 65
    A, _, _, idx = _matrix(c.L, "L", "T", lda_pad=1)
    assert (idx == np.arange(n)[::-1]).all()
    rhs = (blk.B[:, :k], np.ascontiguousarray(blk.B[:, k - 1::-1]))
    wants = (blk.want[:, :k], blk.want[:, k - 1::-1])
    for b, want in zip(rhs, wants):                              # (also the warm call that sizes the workspace)
        _same(_solve(ex, A, b, idx, "L", "T")[0], want, "eager")
    x = torch.zeros(n, k, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.extrsm_dev(A, x, "L", "T")
    for b, want in zip(rhs, wants):
        phys = np.empty((n, k))
        phys[idx] = b
        x.copy_(torch.from_numpy(phys))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (_bits(x.cpu().numpy()[idx]) == _bits(want)).all()
        assert _clear(ex)[0] + _clear(ex)[1] == n * k


@functools.lru_cache(maxsize=None)
def _well_conditioned(n=40):
    """dense lower, off-diagonal entries +-[1, 2) / 256 against a diagonal in [1, 2) and b in +-[1, 2): the row sums stay
    below |b_i|, so no solution entry comes out of a cancellation"""
    rng = np.random.default_rng([n, 1234])
    s = S._system(n, rng, lambda i: np.arange(i))
    s.L = np.where(np.eye(n, dtype=bool), s.L, s.L * 2.0 ** -4)  # (exact: a power of two)
    s.B = S.rand53(rng, (n, 5)) * rng.choice((-1.0, 1.0), (n, 5))
    s.want = np.stack([X.trsv_exact(s.L, s.B[:, j])[0] for j in range(5)], axis=1)
    return s


def test_plain_solve_is_close_and_deterministic(ex):
    s = _well_conditioned()
    for uplo, trans in (("L", "N"), ("U", "T")):
        A, _, _, idx = _matrix(s.L, uplo, trans)
        got, info = _solve(ex, A, s.B, idx, uplo, trans, "N", 1, False)
        again, _ = _solve(ex, A, s.B, idx, uplo, trans, "N", 1, False)
        assert np.isfinite(got).all() and (_bits(got) == _bits(again)).all() and info[0] == info[1] == 0
        assert (np.abs(got - s.want) <= 1e-10 * np.abs(s.want)).all()


def test_fpe_9_is_unsupported_and_touches_nothing(ex):
    import torch
    s = _dense(9)
    A, flat, lda, idx = _matrix(s.L, "L", "N")
    x = torch.from_numpy(s.B[:, :5].copy()).cuda()
    keep = x.clone()
    lib = ex.load_library()
    for fpe in (9, 12):
        rc = lib.exblas_extrsm_dev(b"L", b"N", b"N", 9, 5, ctypes.c_void_p(flat.data_ptr()), lda,
                                   ctypes.c_void_p(x.data_ptr()), 5, fpe, 1, None)
        torch.cuda.synchronize()
        assert rc == -1 and torch.equal(x, keep)
    # the argument errors of the C entry
    bad = 1                                                      # hipErrorInvalidValue
    args = dict(uplo=b"L", trans=b"N", diag=b"N", n=9, k=5, lda=lda, ldx=5, fpe=8)
    for change in (dict(n=-1), dict(k=-1), dict(lda=8), dict(ldx=4), dict(uplo=b"X"), dict(trans=b"C"), dict(diag=b"T"),
                   dict(fpe=-1)):
        q = dict(args, **change)
        rc = lib.exblas_extrsm_dev(q["uplo"], q["trans"], q["diag"], q["n"], q["k"], ctypes.c_void_p(flat.data_ptr()),
                                   q["lda"], ctypes.c_void_p(x.data_ptr()), q["ldx"], q["fpe"], 1, None)
        assert rc == bad, change
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
