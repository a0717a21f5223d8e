"""GPU suite for the batched ExPOTRS: every output against the Fraction substitution of exact_cases (sweep 2 on the
index-reversed system; never against the code under test), for every block size, at the seams of the blocks a wave carries
and of the column tiles, with a short last block, on every sweep, path and variant, both triangles, both layouts and padded
ldr / stride / ldx; planted ties with the counters; 'B' against '1' then '2'; non-finite columns and blocks; ExTRSM as a
second witness; the plain variant, the reference rounding mode, refusals, contexts and host arrays.  The blocks of a call
cycle seven distinct factors, its columns five patterns (bjacobi_cases).  The ends of the double range (totals at the
overflow threshold, around 2^1000, among the subnormals, zeros by cancellation) are in test_gpu_bjacobi_range.py."""
import ctypes

import numpy as np
import pytest

import bjacobi_cases as J

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 4, 5, 16, 63, 64, 65, 130)
SWEEPS = ("1", "2", "B")


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_potrs_batched_path(0)
    exblas_amd.set_trsm_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _counters(ex):
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_potrs_batched_info(out) == 0
    info = tuple(int(v) for v in out)
    assert ex.last_potrs_batched_info() == info and info[2] == 0 and info[3] == 0
    return info


def _apply(ex, factors, X0, uplo, layout, pad, gap, padx, sweep, fpe=8, ee=True, entry=None):
    """the logical [nb, p, p] factors (NaN wherever nothing must be read) in the layout and X0 in a wider NaN block on the
    device; returns (X, counters) after checking that R and everything around R and X still hold what they held"""
    import torch
    nb, p = factors.shape[0], factors.shape[1]
    n, k = X0.shape
    buf, ld, stride, strides = J.pack(factors, layout, pad, gap)
    rdev = torch.from_numpy(buf).cuda()
    Rd = rdev.as_strided((nb, p, p), strides)
    wide = np.full((n, k + padx), np.nan)
    wide[:, :k] = X0
    xdev = torch.from_numpy(wide).cuda()
    Xd = xdev[:, :k]
    out = (entry or ex.expotrs_batched_dev)(Rd, Xd, uplo, sweep, fpe, ee)
    assert out is Xd
    counters = _counters(ex)
    back = xdev.cpu().numpy()
    assert (back[:, k:].view(np.int64) == J.NAN_BITS).all(), "the padding of X was written"
    after = rdev.cpu().numpy()
    assert ((after.view(np.int64) == buf.view(np.int64))).all(), "R was written"
    return back[:, :k], counters


def _nblocks(k, t):
    """block counts around what a wave (64 / kc blocks) and a workgroup item (four waves) carry"""
    kc = min(J.pw_of(k), 64)
    per = max(64 // kc, 1)
    return (per + 1, 4 * per + 1, 9)[t % 3]


def _rows(p, nb, t):
    """n: a multiple of p, or with a last block of 1 or of p - 1 rows"""
    tail = (0, 1, p - 1)[t % 3] if p > 1 else 0
    return nb * p if tail == 0 else (nb - 1) * p + tail


def _check(ex, p, n, k, sweep, path, t):
    uplo, layout, pad, gap = J.LAYOUTS[t % len(J.LAYOUTS)]
    fpe, ee = J.VARIANTS[t % 3]
    X0, want, ties = J.solve_case(p, n, k, sweep)
    ex.set_potrs_batched_path(path)
    got, cnt = _apply(ex, J.solve_factors(p, n, uplo, sweep), X0, uplo, layout, pad, gap, (0, 3, 1)[t % 3], sweep, fpe, ee)
    what = (p, n, k, sweep, path, uplo, layout, pad, gap, fpe)
    J.same_bits(got, want, np.ones_like(got, dtype=bool), what)
    assert cnt[0] + cnt[1] == n * k * (2 if sweep == "B" else 1), (what, cnt)
    assert cnt[1] >= ties, (what, cnt, ties)                        # no tie is ever decided in registers
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return cnt, ties


@pytest.mark.parametrize("p", J.SIZES)
def test_every_width_sweep_and_path(ex, p):
    try:
        t = p
        for k in KS:
            for rep in range(2):
                sweep, path = SWEEPS[t % 3], (0, 1, 2, 3)[(t // 3) % 4]
                n = _rows(p, _nblocks(k, t // 2), t // 4)
                cnt, ties = _check(ex, p, n, k, sweep, path, t)
                t += 1
        print("batched potrs", p, "last", (n, k, sweep, path), cnt, "ties", ties)
    finally:
        ex.set_potrs_batched_path(0)


@pytest.mark.parametrize("sweep", SWEEPS)
@pytest.mark.parametrize("p", [2, 16, 32, 40, 64])
def test_planted_triangles_on_each_sweep(ex, p, sweep):
    """blocks 5 and 6 of the seven carry the planted ties: their number is the least the accumulator must have settled"""
    try:
        t = 0
        for path in (0, 1, 2, 3):
            for k, nb in ((1, 15), (5, 14), (64, 8)):
                n = nb * p
                cnt, ties = _check(ex, p, n, k, sweep, path, t)
                assert ties >= (2 if sweep == "B" else 1), (p, sweep, ties)
                t += 1
    finally:
        ex.set_potrs_batched_path(0)


@pytest.mark.parametrize("p", [1, 3, 8, 17, 64])
def test_both_sweeps_in_one_launch_equal_one_after_the_other(ex, p):
    import torch
    try:
        for path, k, (uplo, layout, pad, gap) in zip((0, 1, 2, 3), (1, 4, 65, 7), J.LAYOUTS):
            ex.set_potrs_batched_path(path)
            n = 11 * p + (p - 1 if p > 1 else 0)
            X0, want, _ = J.solve_case(p, n, k, "B")
            F = J.solve_factors(p, n, uplo, "B")
            both, _ = _apply(ex, F, X0, uplo, layout, pad, gap, 2, "B")
            one, c1 = _apply(ex, F, X0, uplo, layout, pad, gap, 2, "1")
            two, c2 = _apply(ex, F, one, uplo, layout, pad, gap, 0, "2")
            assert c1[0] + c1[1] == n * k == c2[0] + c2[1]
            J.same_bits(two, both, np.ones_like(both, dtype=bool), ("1 then 2", p, path))
            J.same_bits(both, want, np.ones_like(both, dtype=bool), ("B", p, path))
    finally:
        ex.set_potrs_batched_path(0)
        torch.cuda.synchronize()


def _trsm_block(ex, F, Xb, sweep, uplo="U"):
    """extrsm_dev on one block: F upper (row-major tensor, NaN below), Xb [rows, k]"""
    import torch
    rows = Xb.shape[0]
    Fd = torch.from_numpy(np.where(J.tri_mask(rows, "U"), F[:rows, :rows], np.nan)).cuda()
    Xd = torch.from_numpy(np.ascontiguousarray(Xb)).cuda()
    if sweep in ("1", "B"):
        ex.extrsm_dev(Fd, Xd, "U", "T")
    if sweep in ("2", "B"):
        ex.extrsm_dev(Fd, Xd, "U", "N")
    return Xd.cpu().numpy()


@pytest.mark.parametrize("p", [4, 15, 33, 64])
def test_every_block_is_what_extrsm_gives(ex, p):
    for sweep in SWEEPS:
        k, n = 6, 8 * p - 1
        X0, want, _ = J.solve_case(p, n, k, sweep)
        got, _ = _apply(ex, J.solve_factors(p, n, "U", sweep), X0, "U", "col", 1, 2, 1, sweep)
        for b in range(8):
            rows = min(p, n - b * p)
            one = _trsm_block(ex, J.solve_seven(p, sweep)[b % 7].F, X0[b * p:b * p + rows], sweep)
            J.same_bits(got[b * p:b * p + rows], one, np.ones((rows, k), dtype=bool), ("extrsm", p, sweep, b))


@pytest.mark.parametrize("p", [3, 16, 33])
def test_non_finite_columns_and_blocks_change_nothing_else(ex, p):
    """a NaN column, an Inf entry, a NaN in a factor, and NaN in the unused part of the short last block's triangle (which
    solve_factors always plants): every other output keeps its bits, and the touched blocks follow ExTRSM"""
    try:
        for path, sweep in zip((0, 1, 2, 3), ("B", "1", "2", "B")):
            ex.set_potrs_batched_path(path)
            k, nb = 9, 19
            n = nb * p - 1
            X0, want, _ = J.solve_case(p, n, k, sweep)
            F = J.solve_factors(p, n, "U", sweep)
            X0 = X0.copy()
            X0[:, 4] = np.nan                       # a whole column
            X0[5 * p + 1, 2] = np.inf               # one entry: block 5, column 2
            F[8, 0, p - 1] = np.nan                 # one factor entry: block 8
            F[11, 1, 1] = 0.0                       # a zero pivot: the caller's concern, and block 11's alone
            got, _ = _apply(ex, F, X0, "U", "row", 2, 1, 2, sweep)
            clean = np.ones_like(got, dtype=bool)
            clean[:, 4] = False
            clean[5 * p:6 * p, 2] = False
            clean[8 * p:9 * p] = False
            clean[11 * p:12 * p] = False
            J.same_bits(got, want, clean, ("neighbours", p, path, sweep))
            assert np.isnan(got[:, 4]).all()
            for b in (5, 8, 11):
                one = _trsm_block(ex, F[b], X0[b * p:(b + 1) * p], sweep)
                J.same_bits(got[b * p:(b + 1) * p], one, np.ones((p, k), dtype=bool), ("extrsm", p, sweep, b))
    finally:
        ex.set_potrs_batched_path(0)


@pytest.mark.parametrize("p", [1, 5, 16, 33])
def test_plain_variant_equals_its_fp64_restatement(ex, p):
    try:
        for path, sweep in zip((0, 2, 3), SWEEPS):
            ex.set_potrs_batched_path(path)
            k, n = 7, 10 * p - (1 if p > 1 else 0)
            X0, _, _ = J.solve_case(p, n, k, sweep)
            a, cnt = _apply(ex, J.solve_factors(p, n, "L", sweep), X0, "L", "col", 1, 0, 1, sweep, 1, False)
            b, _ = _apply(ex, J.solve_factors(p, n, "L", sweep), X0, "L", "col", 1, 0, 1, sweep, 1, True)
            assert cnt == (0, 0, 0, 0)
            want = np.zeros_like(X0)
            for blk in range(10):
                rows = min(p, n - blk * p)
                F = J.solve_seven(p, sweep)[blk % 7].F[:rows, :rows]
                for j in range(k):
                    want[blk * p:blk * p + rows, j] = J.plain_solve(F, X0[blk * p:blk * p + rows, j], sweep)
            J.same_bits(a, want, np.ones_like(a, dtype=bool), ("plain", p, path, sweep))
            J.same_bits(b, a, np.ones_like(a, dtype=bool), ("plain, again", p, path, sweep))
    finally:
        ex.set_potrs_batched_path(0)


@pytest.mark.parametrize("p", [16, 40])
def test_reference_rounding_mode(ex, p):
    """every output goes through the accumulator and is rounded the reference's way: ExTRSM under the same mode is the
    witness (held to the oracle by its own tests), and the planted ties tell the modes apart"""
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        differ = False
        for path, sweep in zip((0, 1, 2, 3), ("1", "2", "B", "1")):
            ex.set_potrs_batched_path(path)
            k, n = 5, 8 * p
            X0, nearest, _ = J.solve_case(p, n, k, sweep)
            got, cnt = _apply(ex, J.solve_factors(p, n, "U", sweep), X0, "U", "col", 0, 0, 0, sweep)
            assert cnt == (0, n * k * (2 if sweep == "B" else 1), 0, 0)
            for b in range(8):
                one = _trsm_block(ex, J.solve_seven(p, sweep)[b % 7].F, X0[b * p:(b + 1) * p], sweep)
                J.same_bits(got[b * p:(b + 1) * p], one, np.ones((p, k), dtype=bool), ("reference mode", p, sweep, b))
            differ |= bool((got.view(np.int64) != nearest.view(np.int64)).any())
        assert differ, "the modes never differed on these ties"
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_potrs_batched_path(0)


def test_refusals_write_nothing_and_empty_sizes_launch_nothing(ex):
    import torch
    lib = ex.load_library()
    r = torch.full((3, 70, 70), 2.5, dtype=torch.float64, device="cuda")
    x = torch.full((200, 8), 1.5, dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p

    def call(uplo=b"U", sweep=b"B", p=4, n=10, k=2, ldr=70, stride=4900, ldx=8, fpe=8, rp=True, xp=True):
        return lib.exblas_expotrs_batched_dev(uplo, sweep, p, n, k, vp(r.data_ptr()) if rp else None, ldr, stride,
                                              vp(x.data_ptr()) if xp else None, ldx, fpe, 1, None)
    for change in (dict(uplo=b"X"), dict(sweep=b"3"), dict(p=65, n=130), dict(p=0), dict(n=-1), dict(k=-1), dict(ldr=3),
                   dict(stride=279), dict(ldx=1), dict(fpe=-1), dict(rp=False), dict(xp=False)):
        assert call(**change) == 1, change
    assert call(fpe=9) == -1
    with pytest.raises(ValueError):
        ex.expotrs_batched_dev(r[:, :4, :4], x[:13, :2])
    assert call(n=0) == 0 and _counters(ex) == (0, 0, 0, 0)
    assert call(k=0) == 0 and _counters(ex) == (0, 0, 0, 0)
    out = ex.expotrs_batched_dev(r[:0, :4, :4], x[:0, :2])
    assert out.shape[0] == 0 and _counters(ex) == (0, 0, 0, 0)
    torch.cuda.synchronize()
    assert (r == 2.5).all() and (x == 1.5).all()


def test_contexts_streams_and_host_arrays(ex):
    import torch
    p, k = 9, 6
    n = 12 * p - 1
    ctx, side = ex.Context(), torch.cuda.Stream()
    X0, want, _ = J.solve_case(p, n, k, "B")
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got, _ = _apply(ex, J.solve_factors(p, n, "L", "B"), X0, "L", "row", 2, 3, 1, "B", entry=ctx.expotrs_batched)
        side.synchronize()
        J.same_bits(got, want, np.ones_like(got, dtype=bool), "a private context on a side stream")
        assert 0 < ctx.workspace_bytes() <= 1 << 16              # the counters, and nothing like a mailbox
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
    # host arrays: C order and Fortran order per factor, both triangles; the inputs are not changed
    for uplo in ("U", "L"):
        F = np.nan_to_num(J.solve_factors(p, n, uplo, "B"), nan=0.5)      # (what is not read: any number)
        for arr in (F.copy(), np.ascontiguousarray(F.transpose(0, 2, 1)).transpose(0, 2, 1)):
            keepf, keepx = arr.copy(), X0.copy()
            X = ex.expotrs_batched(arr, X0, uplo)
            assert X is not X0 and (arr == keepf).all() and (X0 == keepx).all()
            J.same_bits(X, want, np.ones_like(X, dtype=bool), ("host", uplo))
    for sweep in ("1", 2):
        Xs = ex.expotrs_batched(np.nan_to_num(J.solve_factors(p, n, "U", str(sweep)), nan=0.5), J.solve_case(p, n, k, str(sweep))[0],
                                "U", sweep)
        J.same_bits(Xs, J.solve_case(p, n, k, str(sweep))[1], np.ones_like(Xs, dtype=bool), ("host", sweep))
    # the C host entry with padded ldr, stride and ldx: the padding of X comes back as it went
    buf, ld, stride, strides = J.pack(J.solve_factors(p, n, "U", "B"), "col", 2, 4)
    wide = np.full((n, k + 3), -7.25)
    wide[:, :k] = X0
    rc = ex.load_library().exblas_expotrs_batched(b"U", b"B", p, n, k, ctypes.c_void_p(buf.ctypes.data), ld, stride,
                                                 ctypes.c_void_p(wide.ctypes.data), k + 3, 8, 1)
    assert rc == 0 and (wide[:, k:] == -7.25).all()
    J.same_bits(wide[:, :k], want, np.ones((n, k), dtype=bool), "C host entry")
    assert ex.expotrs_batched(np.zeros((0, 4, 4)), np.zeros((0, 3))).shape == (0, 3)
