"""ExBTRSM on the GPU: every row bit for bit against the planted expectations and btrsm_cases.btrsm_exact, against ExTRSV on
that row and against ExTRSM on the transposed block.

The planted systems of the ExTRSV tests run as blocks of rows (tests/btrsm_cases.py), so that ties, carries and near-ties
sit in many lanes of one wave at once, next to rows the register test certifies, in all four (uplo, transt) with NaN in
everything that must not be read.  The counters keep the file from passing by luck: a tie decided in registers fails even
where round-to-even happens to give the right bits.  Then the seams in p (register block, slices, staged triangle, chunks)
and in n (rows per wave, rows per workgroup) against ExTRSV and ExTRSM themselves, non-finite rows included, alpha, the
padding of a wider block, the empty sizes, the ends of the double range, the reference rounding mode against the oracle, a
row-major T, and the plumbing (context, stream, host arrays, graph capture, workspace).  Expected bits never come from
the code under test."""
import ctypes
import functools

import numpy as np
import pytest

import btrsm_cases as R
import exact_cases as X
import sptrsv_cases as S
from helpers import assert_bits as _same, bits as _bits

pytestmark = pytest.mark.gpu

CASE_IDS = [f"p{n}-W{W}-m{mb}{'-filler' if fl else ''}" for n, W, mb, fl in X.TRSV_CASES]
ORIENT = R.ORIENT
VARIANTS = ((8, True), (3, True), (0, False))
NS = (3, 8, 33, 65, 300)
# (uplo, transt, path, (fpe, early_exit)): every orientation, every path and every variant class occur
COMBOS = (("L", "N", 0, (8, True)), ("U", "N", 0, (3, True)), ("L", "T", 1, (8, True)), ("U", "T", 2, (0, False)),
          ("L", "N", 3, (8, True)), ("U", "T", 3, (3, True)), ("L", "T", 0, (0, False)), ("U", "N", 2, (8, True)))


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_btrsm_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _info(ex):
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_btrsm_info(out) == 0
    info = tuple(int(v) for v in out)
    assert ex.last_btrsm_info() == info and info[2] == 0 and info[3] == 0
    return info


def _matrix(L, uplo, transt, diag="N", ldt_pad=0):
    """the device triangle of the logical lower system L (logical upper M = L^T): a column-major view (strides (1, ldt))
    with NaN in the other triangle, in the ldt padding and on the diagonal under 'U'; logical column j is physical idx[j]"""
    import torch
    p = L.shape[0]
    t, ldt, idx = R.operands(L, uplo, transt, diag, ldt_pad)
    flat = torch.from_numpy(t).cuda()
    return torch.as_strided(flat, (p, p), (1, ldt)), flat, ldt, idx


def _solve(ex, T, B, idx, uplo, transt, diag="N", alpha=1.0, fpe=8, ee=True, entry=None, pad=0, sentinel=-7.25):
    """logical B (n x p) in, logical X out, and the counters; pad: X is the view [:, :p] of a block pad columns wider"""
    call = entry or ex.exbtrsm_dev
    return R.solve_rows(lambda x: call(T, x, uplo, transt, diag, alpha, fpe, ee), lambda: _info(ex), B, idx, pad, sentinel)


# ---------------------------------------------------------------------------------------------
# planted systems
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("case", range(5), ids=CASE_IDS[:5])
def test_planted_rows_every_path_height_and_orientation(ex, case, n, unit):
    c, blk = R.row_block(case, unit, n)
    p, diag = c.n, "U" if unit else "N"
    ties = int(((c.classes == "tie") | (c.classes == "carry")).sum())
    seen = []
    try:
        for uplo, transt, path, (fpe, ee) in COMBOS:
            T, _, _, idx = _matrix(c.L, uplo, transt, diag, ldt_pad=case % 3)
            ex.set_btrsm_path(path)
            got, info = _solve(ex, T, blk.B, idx, uplo, transt, diag, 1.0, fpe, ee)
            what = (p, n, unit, uplo, transt, path, fpe, ee, info)
            _same(got, blk.want, what)
            assert info[0] + info[1] == n * p, what
            if path == 1 or fpe == 0:
                assert info[0] == 0, what
            else:
                assert info[1] >= ties * blk.from_b, ("a tie was decided in registers", what)
            seen.append(info[1])
    finally:
        ex.set_btrsm_path(0)
    print(f"planted {CASE_IDS[case]} unit={unit} n={n}: ties {ties} x {blk.from_b} rows, accumulator outputs "
          f"{min(seen)}..{max(seen)} of {n * p}")


@pytest.mark.parametrize("case", range(5), ids=CASE_IDS[:5])
def test_control_rows_are_decided_in_registers(ex, case):
    """a block of control rows only (every planted b a quarter unit off its tie): the counter discriminates"""
    for unit in (False, True):
        c, full = R.row_block(case, unit, R.KMAX)
        rows = [r for r, kd in enumerate(full.kinds) if kd == "control"][:9]
        B, want = np.ascontiguousarray(full.B[rows]), full.want[rows]
        diag = "U" if unit else "N"
        try:
            for t, (uplo, transt) in enumerate(ORIENT):
                T, _, _, idx = _matrix(c.L, uplo, transt, diag)
                for path in (0, 2, 3):
                    ex.set_btrsm_path(path)
                    got, info = _solve(ex, T, B, idx, uplo, transt, diag, 1.0, *VARIANTS[(t + path) % 2])
                    what = ("control", c.n, uplo, transt, unit, path, info)
                    _same(got, want, what)
                    assert info[0] > 0 and info[0] + info[1] == len(rows) * c.n, what
        finally:
            ex.set_btrsm_path(0)


# ---------------------------------------------------------------------------------------------
# bit identity with ExTRSV row by row and with ExTRSM on the transposed block, at every seam in p and n
# ---------------------------------------------------------------------------------------------
P_BOUNDS = (1, 2, 3, 4, 5, 8, 17, 32, 33, 63, 64, 65, 130)
N_BOUNDS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000)


@functools.lru_cache(maxsize=None)
def _dense(p, rows=max(N_BOUNDS), damp=0):
    rng = np.random.default_rng([p, 78])
    s = S._system(p, rng, lambda i: np.arange(i))                # dense lower: every dependency there is
    if damp:
        s.L = np.where(np.eye(p, dtype=bool), s.L, s.L * 2.0 ** -damp)   # (exact: a power of two)
    s.B = S.rand53(rng, (rows, p)) * rng.choice((-1.0, 1.0), (rows, p))
    return s


def _extrsv_rows(ex, flat, ldt, B, idx, uplo, transt, diag="N"):
    """ExTRSV with the other trans on every row of the block in place (x = X + r ldx, incx = 1): the contract"""
    import torch
    n, p = B.shape
    phys = np.empty_like(B)
    phys[:, idx] = B
    Xr = torch.from_numpy(phys).cuda()
    for r in range(n):
        assert ex.extrsv_dev(uplo, R.flip(transt), diag, p, flat, ldt, Xr[r], 8, True) == 0
    torch.cuda.synchronize()
    return Xr.cpu().numpy()[:, idx]


def _extrsm_transposed(ex, T, B, idx, uplo, transt, diag="N"):
    """ExTRSM with the other trans on the transposed block (p x n): column r is row r here"""
    import torch
    phys = np.empty_like(B)
    phys[:, idx] = B
    Xt = torch.from_numpy(np.array(phys.T, order="C", copy=True)).cuda()    # (a fresh array: strides (n, 1) also for p = 1)
    ex.extrsm_dev(T, Xt, uplo, R.flip(transt), diag)
    assert ex.last_trsm_info()[2] == 0
    return np.ascontiguousarray(Xt.cpu().numpy().T)[:, idx]


@pytest.mark.parametrize("p", P_BOUNDS)
def test_every_row_equals_extrsv_and_extrsm(ex, p):
    """finite rows, one row with an Inf and one all NaN: where the results are not finite, and with which sign, is
    ExTRSV's, and every other row keeps the bits of the clean run"""
    s = _dense(p)
    nmax = max(N_BOUNDS)
    try:
        for t, (uplo, transt) in enumerate(ORIENT):
            T, flat, ldt, idx = _matrix(s.L, uplo, transt, ldt_pad=3)
            assert ldt == p + 3
            clean = _extrsm_transposed(ex, T, s.B, idx, uplo, transt)
            assert np.isfinite(clean).all()
            some = np.unique(np.concatenate([np.arange(min(4, nmax)), [62, 63, 64, 65, 255, 256, 999]]))
            _same(_extrsv_rows(ex, flat, ldt, s.B[some], idx, uplo, transt), clean[some], ("ExTRSV = ExTRSM", p, uplo, transt))
            for i, n in enumerate(N_BOUNDS):
                if i % 4 != t:
                    continue
                B, ref = s.B[:n].copy(), clean[:n].copy()
                if n >= 3:
                    hot = [n // 3, (2 * n) // 3]
                    B[hot[0], min(1, p - 1)] = -np.inf if i % 2 else np.inf
                    B[hot[1]] = np.nan
                    ref[hot] = _extrsv_rows(ex, flat, ldt, B[hot], idx, uplo, transt)
                    assert np.isnan(ref[hot[1]]).all() and not np.isfinite(ref[hot[0]]).all()
                for path in (0, 1, 2, 3):
                    ex.set_btrsm_path(path)
                    got, info = _solve(ex, T, B, idx, uplo, transt, "N", 1.0, *VARIANTS[(i + path) % 3])
                    _same(got, ref, ("dense", p, n, uplo, transt, path, info))
                    assert info[0] + info[1] == n * p
                ex.set_btrsm_path(0)
                plain, _ = _solve(ex, T, s.B[:n], idx, uplo, transt)
                _same(plain, clean[:n], ("clean", p, n, uplo, transt))
    finally:
        ex.set_btrsm_path(0)


def test_the_widest_triangle_equals_extrsv(ex):
    p = ex.BTRSM_MAX_P
    assert p == 512
    s = _dense(p, 3, 10)
    try:
        for t, (uplo, transt) in enumerate(ORIENT):
            T, flat, ldt, idx = _matrix(s.L, uplo, transt, ldt_pad=1)
            ref = _extrsv_rows(ex, flat, ldt, s.B, idx, uplo, transt)
            assert np.isfinite(ref).all()
            for path in (0, (1, 2, 3, 2)[t]):
                ex.set_btrsm_path(path)
                got, info = _solve(ex, T, s.B, idx, uplo, transt)
                _same(got, ref, ("p = 512", uplo, transt, path, info))
                assert info[0] + info[1] == 3 * p
    finally:
        ex.set_btrsm_path(0)


# ---------------------------------------------------------------------------------------------
# alpha
# ---------------------------------------------------------------------------------------------
def test_alpha_powers_of_two_scale_exactly(ex):
    """alpha = s 2^e is the run on the exactly scaled B: every planted tie stays a tie"""
    c, blk = R.row_block(2, False, 70)
    try:
        for t, (uplo, transt) in enumerate(ORIENT):
            T, _, _, idx = _matrix(c.L, uplo, transt)
            for alpha in (2.0, -0.5, 2.0 ** 40, -2.0 ** -100):
                ex.set_btrsm_path((0, 2, 3, 1)[t])
                got, info = _solve(ex, T, blk.B, idx, uplo, transt, "N", alpha)
                _same(got, blk.want * alpha, ("alpha", alpha, uplo, transt))
                scaled, _ = _solve(ex, T, blk.B * alpha, idx, uplo, transt)
                _same(scaled, blk.want * alpha, ("scaled B", alpha, uplo, transt))
    finally:
        ex.set_btrsm_path(0)


@pytest.mark.parametrize("alpha", [-1.0, 0.1, -3.7])
def test_alpha_against_the_exact_substitution(ex, alpha):
    rng = np.random.default_rng(5)
    for p, n in ((17, 9), (66, 5)):
        s = S._system(p, rng, lambda i: np.arange(i))
        B = S.rand53(rng, (n, p)) * rng.choice((-1.0, 1.0), (n, p))
        for unit in (False, True):
            want = R.btrsm_exact(s.L.T, B, alpha, unit)
            diag = "U" if unit else "N"
            try:
                for t, (uplo, transt) in enumerate(ORIENT):
                    T, _, _, idx = _matrix(s.L, uplo, transt, diag)
                    for path in (t, 0):
                        ex.set_btrsm_path(path)
                        got, _ = _solve(ex, T, B, idx, uplo, transt, diag, alpha, *VARIANTS[(t + path) % 3])
                        _same(got, want, ("alpha", alpha, p, unit, uplo, transt, path))
            finally:
                ex.set_btrsm_path(0)


def test_alpha_zero_ignores_a_b_full_of_nan(ex):
    rng = np.random.default_rng(6)
    s = S._system(21, rng, lambda i: np.arange(i))
    s.L[7, 7] = -s.L[7, 7]
    B = np.full((70, 21), np.nan)
    want = R.btrsm_exact(s.L.T, B, 0.0)
    assert (want == 0.0).all() and np.signbit(want[:, 7]).all() and not np.signbit(want[:, 8]).any()
    try:
        for t, (uplo, transt) in enumerate(ORIENT):
            T, _, _, idx = _matrix(s.L, uplo, transt)
            ex.set_btrsm_path(t)
            got, _ = _solve(ex, T, B, idx, uplo, transt, "N", 0.0, *VARIANTS[t % 3])
            _same(got, want, ("alpha = 0", uplo, transt, t))
    finally:
        ex.set_btrsm_path(0)


def test_the_error_term_of_alpha_b_is_summed(ex):
    """a routine that rounds alpha * b before it sums gives x_1 = 0 instead of 1: 70 identical rows, every path; then the
    same construction across the 64-column seam of a p = 70 triangle"""
    try:
        M70, b70, want70 = R.embedded_error_term()
        for L, b, want in ((R.ERR_M.T, R.ERR_B, R.ERR_WANT), (M70.T, b70, want70)):
            B, W = np.tile(b, (70, 1)), np.tile(want, (70, 1))
            for t, (uplo, transt) in enumerate(ORIENT):
                T, _, _, idx = _matrix(L, uplo, transt, "U")
                for path in (0, 1, 2, 3):
                    ex.set_btrsm_path(path)
                    got, _ = _solve(ex, T, B, idx, uplo, transt, "U", R.ERR_ALPHA, *VARIANTS[(t + path) % 3])
                    _same(got, W, ("error term", L.shape[0], uplo, transt, path))
    finally:
        ex.set_btrsm_path(0)


# ---------------------------------------------------------------------------------------------
# padding, empty sizes, the ends of the double range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 2])
def test_padding_of_a_wider_block_keeps_its_bits(ex, case):
    """X is the view [:, :p] of an (n, p + 3) block: the three columns beyond it are neither read (NaN there changes
    nothing) nor written"""
    c, blk = R.row_block(case, False, 67)
    try:
        for uplo, transt, path in (("L", "N", 0), ("U", "T", 3), ("L", "T", 1), ("U", "N", 2)):
            T, _, _, idx = _matrix(c.L, uplo, transt, ldt_pad=2)
            ex.set_btrsm_path(path)
            for sentinel in (-7.25, np.nan):
                got, _ = _solve(ex, T, blk.B, idx, uplo, transt, pad=3, sentinel=sentinel)
                _same(got, blk.want, ("ldx > p", c.n, uplo, transt, path, sentinel))
    finally:
        ex.set_btrsm_path(0)


def test_empty_sizes_launch_nothing(ex):
    import torch
    T0 = torch.zeros(0, 0, dtype=torch.float64).cuda()
    for n in (0, 1, 5):
        x = torch.zeros(n, 0, dtype=torch.float64).cuda()
        assert ex.exbtrsm_dev(T0, x) is x and _info(ex) == (0, 0, 0, 0)
    s = _dense(8)
    T, _, _, idx = _matrix(s.L, "U", "N")
    _, info = _solve(ex, T, s.B[:3], idx, "U", "N")              # a call that counts, then one that launches nothing
    assert info[0] + info[1] == 24
    x = torch.zeros(0, 8, dtype=torch.float64).cuda()
    assert ex.exbtrsm_dev(T, x) is x and _info(ex) == (0, 0, 0, 0)
    lib = ex.load_library()
    assert lib.exblas_exbtrsm_dev(b"U", b"N", b"N", 0, 0, 1.0, None, 1, None, 0, 8, 1, None) == 0
    assert lib.exblas_exbtrsm_dev(b"U", b"N", b"N", 5, 0, 1.0, None, 1, None, 0, 8, 1, None) == 0
    assert ex.exbtrsm(np.zeros((0, 0)), np.zeros((5, 0))).shape == (5, 0)
    assert ex.exbtrsm(np.triu(s.L.T), np.zeros((0, 8))).shape == (0, 8)


@pytest.mark.parametrize("lead", [0, 58, 70])
def test_range_rows(ex, lead):
    """overflow ties, totals either side of 2^1000, subnormal totals and quotients, the sign of a zero by cancellation:
    the system's b as a row, its negation (expected from trsv_exact: a zero total keeps its + sign) and b again"""
    r = X.range_rows_trsv(lead)
    B = np.stack([r.b, -r.b, r.b] * 2)[:5]
    neg = X.trsv_exact(r.L, -r.b)[0]
    want = np.stack([r.want, neg, r.want, r.want, neg])
    try:
        for uplo, transt in ORIENT:
            T, _, _, idx = _matrix(r.L, uplo, transt, ldt_pad=lead % 4)
            for path in (0, 1, 2, 3):
                ex.set_btrsm_path(path)
                for fpe, ee in VARIANTS:
                    got, _ = _solve(ex, T, B, idx, uplo, transt, "N", 1.0, fpe, ee)
                    bad = (_bits(got) != _bits(want)).any(axis=0)
                    assert not bad.any(), (lead, uplo, transt, path, fpe, ee, [nm for nm in r.names if bad[r.rows[nm]]],
                                           got[:, bad], want[:, bad])
    finally:
        ex.set_btrsm_path(0)


# ---------------------------------------------------------------------------------------------
# rounding mode, layouts, plumbing, graphs, the plain solve, the unsupported variants
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 2], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_planted_reference_rounding_mode(ex, oracle, case):
    """ties are where the two rounding modes differ: every row follows the oracle's reference-mode substitution"""
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        differs = 0
        for unit in (False, True):
            c, blk = R.row_block(case, unit, 6)
            p, diag = c.n, "U" if unit else "N"
            want = np.empty((6, p))
            for r in range(6):
                a, lda, xs, idx = X.trsv_operands(c.L, blk.B[r], "L", "N", diag)
                rc, w = oracle.extrsv("L", "N", diag, p, a, lda, xs, 0, mode=oracle.ROUND_REFERENCE)
                assert rc == 0
                want[r] = w[idx]
            differs += int((_bits(want) != _bits(blk.want)).sum())
            for t, (uplo, transt) in enumerate(ORIENT):
                T, _, _, idx = _matrix(c.L, uplo, transt, diag)
                for path in (0, 2, 3):
                    ex.set_btrsm_path(path)
                    fpe, ee = VARIANTS[(t + path) % 3]
                    got, info = _solve(ex, T, blk.B, idx, uplo, transt, diag, 1.0, fpe, ee)
                    _same(got, want, ("reference mode", p, uplo, transt, unit, path, fpe, ee))
                    assert info[0] == 0 and info[1] == 6 * p
        assert differs >= 1, "the reference rounding mode never differed from the exact one on these ties"
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_btrsm_path(0)


def test_row_major_and_column_major_tensors_give_the_same_bits(ex):
    """the same logical triangle as a C-contiguous tensor and as its column-major copy, for both uplo and both trans"""
    c, blk = R.row_block(2, False, 8)
    for uplo, transt in ORIENT:
        T, _, _, idx = _matrix(c.L, uplo, transt, ldt_pad=1)     # strides (1, p + 1): column-major
        Rm = T.contiguous()                                      # strides (p, 1): the same T[i, j], row-major
        assert T.stride(0) == 1 and Rm.stride(1) == 1 and Rm.stride(0) == c.n
        got_c, _ = _solve(ex, T, blk.B, idx, uplo, transt)
        got_r, _ = _solve(ex, Rm, blk.B, idx, uplo, transt)
        _same(got_c, blk.want, ("column-major", uplo, transt))
        assert (_bits(got_r) == _bits(got_c)).all(), ("row-major", uplo, transt)


def test_runs_contexts_streams_and_host_arrays_agree(ex):
    import torch
    c, blk = R.row_block(3, False, 9)
    p = c.n
    for uplo, transt in (("U", "N"), ("L", "N")):
        T, _, ldt, idx = _matrix(c.L, uplo, transt)
        first, _ = _solve(ex, T, blk.B, idx, uplo, transt)
        again, _ = _solve(ex, T, blk.B, idx, uplo, transt)
        _same(first, blk.want, ("dev", uplo, transt))
        assert (_bits(first) == _bits(again)).all()
        ctx, side = ex.Context(), torch.cuda.Stream()
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                got, _ = _solve(ex, T, blk.B, idx, uplo, transt, entry=ctx.exbtrsm)
            side.synchronize()
            assert (_bits(got) == _bits(first)).all(), ("context on a side stream", uplo, transt)
            assert 0 < ctx.workspace_bytes() <= 1 << 16          # the counter slots, and nothing like a mailbox
        finally:
            torch.cuda.synchronize()
            ctx.destroy()
        # host arrays: the Python-indexed triangle (NaN where it must not be read), C order and Fortran order
        host_t = T.cpu().numpy()
        Xs = np.empty((9, p))
        Xs[:, idx] = blk.B
        keep = Xs.copy()
        for arr in (np.ascontiguousarray(host_t), np.asfortranarray(host_t)):
            host = ex.exbtrsm(arr, Xs, uplo, transt)
            assert (_bits(Xs) == _bits(keep)).all() and host is not Xs
            assert (_bits(host[:, idx]) == _bits(first)).all(), ("host arrays", uplo, transt)


def test_host_entry_keeps_the_padding_of_x(ex):
    """the C host entry with ldx > p: the padding comes back as it went"""
    s = _dense(8)
    t, ldt, idx = R.operands(s.L, "L", "N", ldt_pad=2)
    ref = R.btrsm_exact(s.L.T, s.B[:5], -3.7)
    wide = np.full((5, 11), -7.25)
    wide[:, idx] = s.B[:5]
    rc = ex.load_library().exblas_exbtrsm(b"L", b"N", b"N", 5, 8, -3.7, ctypes.c_void_p(t.ctypes.data), ldt,
                                          ctypes.c_void_p(wide.ctypes.data), 11, 8, 1)
    assert rc == 0
    _same(wide[:, idx], ref, "host entry, ldx = 11")
    assert (wide[:, 8:] == -7.25).all()


def test_graph_capture_after_one_warm_call(ex):
    """One warm call, then a capture replayed three times on new data, the counters read after each replay.  The
    captured work is a single kernel node."""
    import torch
    c, blk = R.row_block(4, False, 70)
    n, p = 70, c.n
    T, _, _, idx = _matrix(c.L, "L", "N", ldt_pad=1)
    rhs = (blk.B, np.ascontiguousarray(blk.B[::-1]), blk.B)
    wants = (blk.want, blk.want[::-1], blk.want)
    _same(_solve(ex, T, blk.B, idx, "L", "N")[0], blk.want, "eager")      # (also the warm call that sizes the workspace)
    x = torch.zeros(n, p, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exbtrsm_dev(T, x, "L", "N")
    ties = int(((c.classes == "tie") | (c.classes == "carry")).sum())
    for b, want in zip(rhs, wants):
        phys = np.empty((n, p))
        phys[:, idx] = b
        x.copy_(torch.from_numpy(phys))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (_bits(x.cpu().numpy()[:, idx]) == _bits(want)).all()
        info = _info(ex)
        assert info[0] + info[1] == n * p and info[1] >= ties * blk.from_b and info[0] > 0
    del g


def test_workspace_growth_during_capture_is_refused(ex):
    """a context that has no workspace yet must not allocate one under a capture: reserve, or call once, first"""
    import torch
    ctx = ex.Context()
    try:
        assert ctx.workspace_bytes() == 0
        T = torch.eye(4, dtype=torch.float64, device="cuda") * 2.0
        x = torch.ones(8, 4, dtype=torch.float64, device="cuda")
        ex.exbtrsm_dev(T, x.clone())                             # the one call of the process that a capture needs
        torch.cuda.synchronize()
        s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError):
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    ctx.exbtrsm(T, x)
        torch.cuda.synchronize()
        assert ctx.workspace_bytes() == 0 and (x.cpu().numpy() == 1.0).all()
        assert ex.load_library().exblas_reserve_workspace_ctx(ctx.handle, 256) == 0
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g2, stream=s):
                ctx.exbtrsm(T, x)
        g2.replay()
        torch.cuda.synchronize()
        assert (x.cpu().numpy() == 0.5).all()
        del g2
    finally:
        torch.cuda.synchronize()
        ctx.destroy()


def test_plain_solve_is_close_and_deterministic(ex):
    rng = np.random.default_rng([40, 1234])
    s = S._system(40, rng, lambda i: np.arange(i))
    s.L = np.where(np.eye(40, dtype=bool), s.L, s.L * 2.0 ** -4)          # (exact: a power of two)
    B = S.rand53(rng, (70, 40)) * rng.choice((-1.0, 1.0), (70, 40))
    want = R.btrsm_exact(s.L.T, B[:6])
    for uplo, transt in (("U", "N"), ("L", "N")):
        T, _, _, idx = _matrix(s.L, uplo, transt)
        got, info = _solve(ex, T, B, idx, uplo, transt, "N", 1.0, 1, False)
        again, _ = _solve(ex, T, B, idx, uplo, transt, "N", 1.0, 1, False)
        assert np.isfinite(got).all() and (_bits(got) == _bits(again)).all() and info[0] == info[1] == 0
        assert (np.abs(got[:6] - want) <= 1e-10 * np.abs(want)).all()


def test_fpe_9_and_bad_arguments_touch_nothing(ex):
    import torch
    s = _dense(8)
    T, flat, ldt, idx = _matrix(s.L, "U", "N")
    x = torch.from_numpy(s.B[:5].copy()).cuda()
    keep = x.clone()
    lib = ex.load_library()
    tp, xp = ctypes.c_void_p(flat.data_ptr()), ctypes.c_void_p(x.data_ptr())
    for fpe in (9, 12):
        assert lib.exblas_exbtrsm_dev(b"U", b"N", b"N", 5, 8, 1.0, tp, ldt, xp, 8, fpe, 1, None) == -1
    args = dict(uplo=b"U", trans=b"N", diag=b"N", n=5, p=8, ldt=ldt, ldx=8, fpe=8)
    for change in (dict(n=-1), dict(p=-1), dict(ldt=7), dict(ldx=7), dict(uplo=b"X"), dict(trans=b"C"), dict(diag=b"T"),
                   dict(fpe=-1), dict(p=513, ldt=513, ldx=513)):
        q = dict(args, **change)
        rc = lib.exblas_exbtrsm_dev(q["uplo"], q["trans"], q["diag"], q["n"], q["p"], 1.0, tp, q["ldt"], xp, q["ldx"],
                                    q["fpe"], 1, None)
        assert rc == 1, change                                   # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert torch.equal(x, keep)
