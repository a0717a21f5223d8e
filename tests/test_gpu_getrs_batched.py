"""GPU suite for the batched ExGETRS: every output against getrf_cases.getrs_model (the interchanges, then the Fraction
substitution of exact_cases twice; never against the code under test), for every block size, at the seams of the blocks a wave
carries and of the column tiles, with a short last block, on every path and variant, both orders and padded ldlu / stride /
ldx; the counters; pivots out of range; ExTRSV as a second witness; the plain variant, refusals, contexts and host arrays.
The blocks of a call cycle seven distinct factored blocks, its columns five patterns.  The ends of the double range (totals at the
overflow threshold, around 2^1000, among the subnormals, zeros by cancellation) are in test_gpu_bjacobi_range.py."""
import ctypes

import numpy as np
import pytest

import bjacobi_cases as J
import getrf_cases as G

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 64, 65, 130)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_getrs_batched_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _counters(ex):
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_getrs_batched_info(out) == 0
    info = tuple(int(v) for v in out)
    assert ex.last_getrs_batched_info() == info and info[2] == 0 and info[3] == 0
    return info


def _apply(ex, LU, ipiv, X0, layout, pad, gap, padx, fpe=8, ee=True, entry=None):
    """the logical [nb, p, p] factors (NaN wherever nothing must be read) in the layout, their pivots, and X0 in a wider NaN
    block on the device; returns (X, counters) after checking that LU, ipiv and everything around LU and X still hold what
    they held"""
    import torch
    nb, p = LU.shape[0], LU.shape[1]
    n, k = X0.shape
    buf, ld, stride, strides = J.pack(LU, layout, pad, gap)
    ldev = torch.from_numpy(buf).cuda()
    Ld = ldev.as_strided((nb, p, p), strides)
    pdev = torch.from_numpy(np.ascontiguousarray(ipiv, dtype=np.int32)).cuda()
    wide = np.full((n, k + padx), np.nan)
    wide[:, :k] = X0
    xdev = torch.from_numpy(wide).cuda()
    Xd = xdev[:, :k]
    out = (entry or ex.exgetrs_batched_dev)(Ld, pdev, Xd, fpe, ee)
    assert out is Xd
    counters = _counters(ex)
    back = xdev.cpu().numpy()
    assert (back[:, k:].view(np.int64) == J.NAN_BITS).all(), "the padding of X was written"
    assert (ldev.cpu().numpy().view(np.int64) == buf.view(np.int64)).all(), "LU was written"
    assert (pdev.cpu().numpy() == ipiv).all(), "ipiv was written"
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


def _check(ex, p, n, k, path, t):
    layout, pad, gap = G.LAYOUTS[t % len(G.LAYOUTS)]
    fpe, ee = G.VARIANTS[t % 3]
    LU, ipiv, X0, want, ties = G.solve_case(p, n, k)
    ex.set_getrs_batched_path(path)
    got, cnt = _apply(ex, LU, ipiv, X0, layout, pad, gap, (0, 3, 1)[t % 3], fpe, ee)
    what = (p, n, k, path, layout, pad, gap, fpe)
    J.same_bits(got, want, np.ones_like(got, dtype=bool), what)
    assert cnt[0] + cnt[1] == 2 * n * k, (what, cnt)
    assert cnt[1] >= ties, (what, cnt, ties)                        # no tie is ever decided in registers
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return cnt, ties


@pytest.mark.parametrize("p", G.SIZES)
def test_every_width_and_path(ex, p):
    try:
        t = p
        for k in KS:
            for rep in range(2):
                path = (0, 1, 2, 3)[t % 4]
                n = _rows(p, _nblocks(k, t // 2), t // 4)
                cnt, ties = _check(ex, p, n, k, path, t)
                t += 1
        print("batched getrs", p, "last", (n, k, path), cnt, "ties", ties)
    finally:
        ex.set_getrs_batched_path(0)


@pytest.mark.parametrize("p", [2, 16, 33, 64])
def test_the_hand_made_tie_on_every_path(ex, p):
    """block 5 of the seven meets a tie in the forward sweep of column pattern 0: the accumulator must have settled it"""
    try:
        t = 0
        for path in (0, 1, 2, 3):
            for k, nb in ((1, 15), (5, 14), (64, 8)):
                cnt, ties = _check(ex, p, nb * p, k, path, t)
                assert ties >= 1, (p, ties)
                t += 1
    finally:
        ex.set_getrs_batched_path(0)


@pytest.mark.parametrize("p", [1, 4, 17, 64])
def test_pivots_out_of_range_leave_the_rows_unswapped(ex, p):
    """garbage pivots (0, negative, beyond the block, INT_MAX / INT_MIN) are skipped: the block is solved as if its rows
    stayed where they were, nothing faults and nothing outside X is written"""
    try:
        for path, k in zip((0, 1, 2, 3), (1, 4, 65, 7)):
            ex.set_getrs_batched_path(path)
            n = 9 * p + (p - 1 if p > 1 else 0)
            LU, ipiv, X0, _, _ = G.solve_case(p, n, k)
            bad = np.array([0, -1, p + 1, 2 ** 31 - 1, -(2 ** 31), 65, 1 << 20, -p], dtype=np.int64)
            ipiv = ipiv.copy()
            for b in (1, 4, 9 if p > 1 else 8):
                ipiv[b] = bad[(np.arange(p) + b) % len(bad)].astype(np.int32)
            ipiv[2, ::2] = 0                       # half of them: the others still swap
            want = np.zeros_like(X0)
            for b in range(ipiv.shape[0]):
                rows = min(p, n - b * p)
                for j in range(min(k, G.NPAT)):            # the columns cycle NPAT patterns
                    want[b * p:b * p + rows, j::G.NPAT] = G.getrs_model(LU[b], ipiv[b], X0[b * p:b * p + rows, j])[0][:, None]
            got, cnt = _apply(ex, LU, ipiv, X0, ("col", "row")[path % 2], 1, 2, 2)
            J.same_bits(got, want, np.ones_like(got, dtype=bool), ("garbage pivots", p, path))
            assert cnt[0] + cnt[1] == 2 * n * k
    finally:
        ex.set_getrs_batched_path(0)


def _trsv_twice(ex, LUb, ipivb, col):
    """the interchanges on the host, then extrsv_dev ('L', 'N', 'U') and ('U', 'N', 'N') on the column-major block"""
    import torch
    rows = len(col)
    x = np.array(col, copy=True)
    for j in range(rows):
        pv = int(ipivb[j]) - 1
        if 0 <= pv < rows and pv != j:
            x[j], x[pv] = x[pv], x[j]
    a = torch.from_numpy(np.ascontiguousarray(LUb[:rows, :rows].T)).cuda()      # (i, j) at i + j * rows
    xd = torch.from_numpy(x).cuda()
    assert ex.extrsv_dev("L", "N", "U", rows, a, rows, xd, 8, True) == 0
    assert ex.extrsv_dev("U", "N", "N", rows, a, rows, xd, 8, True) == 0
    return xd.cpu().numpy()


@pytest.mark.parametrize("p", [4, 15, 33, 64])
def test_every_column_is_what_extrsv_gives_twice(ex, p):
    k, n = 3, 8 * p - 1
    LU, ipiv, X0, want, _ = G.solve_case(p, n, k)
    got, _ = _apply(ex, LU, ipiv, X0, "col", 1, 2, 1)
    for b in range(8):
        rows = min(p, n - b * p)
        for j in range(k):
            one = _trsv_twice(ex, LU[b], ipiv[b], X0[b * p:b * p + rows, j])
            J.same_bits(got[b * p:b * p + rows, j], one, np.ones(rows, dtype=bool), ("extrsv", p, b, j))


@pytest.mark.parametrize("p", [3, 16, 33])
def test_non_finite_columns_change_nothing_else(ex, p):
    """a NaN column and an Inf entry: every other output keeps its bits"""
    try:
        for path in (0, 1, 2, 3):
            ex.set_getrs_batched_path(path)
            k, nb = 9, 19
            n = nb * p - 1
            LU, ipiv, X0, want, _ = G.solve_case(p, n, k)
            X0 = X0.copy()
            X0[:, 4] = np.nan                       # a whole column
            X0[5 * p + 1, 2] = np.inf               # one entry: block 5, column 2
            got, _ = _apply(ex, LU, ipiv, X0, "row", 2, 1, 2)
            clean = np.ones_like(got, dtype=bool)
            clean[:, 4] = False
            clean[5 * p:6 * p, 2] = False
            J.same_bits(got, want, clean, ("neighbours", p, path))
            assert np.isnan(got[:, 4]).all() and not np.isfinite(got[5 * p:6 * p, 2]).all()
    finally:
        ex.set_getrs_batched_path(0)


@pytest.mark.parametrize("p", [1, 5, 16, 33])
def test_plain_variant_equals_its_fp64_restatement(ex, p):
    try:
        for path, k in zip((0, 2, 3), (3, 65, 6)):
            ex.set_getrs_batched_path(path)
            n = 6 * p + (p - 1 if p > 1 else 0)
            LU, ipiv, X0, _, _ = G.solve_case(p, n, k)
            want = np.zeros_like(X0)
            for b in range(ipiv.shape[0]):
                rows = min(p, n - b * p)
                for j in range(k):
                    want[b * p:b * p + rows, j] = G.plain_getrs(LU[b], ipiv[b], X0[b * p:b * p + rows, j])
            a, cnt = _apply(ex, LU, ipiv, X0, "col", 1, 0, 1, 1, False)
            b2, _ = _apply(ex, LU, ipiv, X0, "row", 0, 3, 0, 1, True)
            assert cnt == (0, 0, 0, 0)
            J.same_bits(a, want, np.ones_like(a, dtype=bool), ("plain", p, path))
            J.same_bits(b2, a, np.ones_like(a, dtype=bool), ("plain, again", p, path))
    finally:
        ex.set_getrs_batched_path(0)


def test_reference_rounding_mode_paths_agree(ex):
    lib = ex.load_library()
    p, k = 16, 5
    n = 14 * p - 3
    LU, ipiv, X0, want, ties = G.solve_case(p, n, k)
    lib.exblas_set_round_mode(1)
    try:
        first = None
        for path in (0, 1, 2, 3):
            ex.set_getrs_batched_path(path)
            got, cnt = _apply(ex, LU, ipiv, X0, "row", 1, 1, 1, (8, 0, 4, 8)[path])
            assert cnt == (0, 2 * n * k, 0, 0)
            first = got if first is None else first
            J.same_bits(got, first, np.ones_like(got, dtype=bool), ("reference mode", path))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_getrs_batched_path(0)


def test_refusals_write_nothing(ex):
    import torch
    lib = ex.load_library()
    lu = torch.full((3, 70, 70), 2.5, dtype=torch.float64, device="cuda")
    ipiv = torch.full((3, 70), 1, dtype=torch.int32, device="cuda")
    x = torch.full((12, 5), 1.5, dtype=torch.float64, device="cuda")
    vp = ctypes.c_void_p
    pl, pp, px = vp(lu.data_ptr()), vp(ipiv.data_ptr()), vp(x.data_ptr())
    for args in ((b"X", 4, 12, 5, 70, 4900, 5), (b"C", 65, 12, 5, 70, 4900, 5), (b"C", 0, 12, 5, 70, 4900, 5),
                 (b"R", 4, -1, 5, 70, 4900, 5), (b"R", 4, 12, -1, 70, 4900, 5), (b"C", 4, 12, 5, 3, 4900, 5),
                 (b"C", 4, 12, 5, 70, 279, 5), (b"C", 4, 12, 5, 70, 4900, 4)):
        order, p, n, k, ldlu, stride, ldx = args
        assert lib.exblas_exgetrs_batched_dev(order, p, n, k, pl, ldlu, stride, pp, px, ldx, 8, 1, None) == 1, args
    assert lib.exblas_exgetrs_batched_dev(b"C", 4, 12, 5, pl, 70, 4900, pp, px, 5, 9, 1, None) == -1
    assert lib.exblas_exgetrs_batched_dev(b"C", 4, 12, 5, pl, 70, 4900, pp, px, 5, -1, 1, None) == 1
    assert lib.exblas_exgetrs_batched_dev(b"C", 4, 12, 5, None, 70, 4900, pp, px, 5, 8, 1, None) == 1
    assert lib.exblas_exgetrs_batched_dev(b"C", 4, 12, 5, pl, 70, 4900, None, px, 5, 8, 1, None) == 1
    assert lib.exblas_exgetrs_batched_dev(b"C", 4, 12, 5, pl, 70, 4900, pp, None, 5, 8, 1, None) == 1
    assert lib.exblas_exgetrs_batched_dev(b"C", 4, 0, 5, pl, 70, 4900, pp, px, 5, 8, 1, None) == 0
    assert lib.exblas_exgetrs_batched_dev(b"C", 4, 12, 0, pl, 70, 4900, pp, px, 5, 8, 1, None) == 0
    assert _counters(ex) == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        ex.exgetrs_batched_dev(lu[:, :4, :4], ipiv[:, :4].contiguous(), x[:8])      # three blocks for two blocks of rows
    torch.cuda.synchronize()
    assert (lu == 2.5).all() and (x == 1.5).all() and (ipiv == 1).all()


def test_contexts_streams_and_host_arrays(ex):
    import torch
    p, k = 17, 6
    n = 11 * p + 5
    LU, ipiv, X0, want, _ = G.solve_case(p, n, k)
    ctx, side = ex.Context(), torch.cuda.Stream()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got, _ = _apply(ex, LU, ipiv, X0, "row", 2, 3, 1, entry=ctx.exgetrs_batched)
        side.synchronize()
        J.same_bits(got, want, np.ones_like(got, dtype=bool), "a private context on a side stream")
        assert 0 < ctx.workspace_bytes() <= 1 << 16
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
    # host arrays: whole blocks only (the host form sends every entry of LU; NaN outside the leading part is still not read)
    keepB = X0.copy()
    for arr in (LU.copy(), np.ascontiguousarray(LU.transpose(0, 2, 1)).transpose(0, 2, 1)):
        X = ex.exgetrs_batched(arr, ipiv, X0)
        assert X is not X0 and (X0 == keepB).all()
        J.same_bits(X, want, np.ones_like(X, dtype=bool), "host")
    # the C host entry with padded ldlu, a gap and padded ldx: the padding of X comes back as it went
    for order, layout in ((b"C", "col"), (b"R", "row")):
        buf, ld, stride, strides = J.pack(LU, layout, 2, 4)
        wide = np.full((n, k + 2), np.nan)
        wide[:, :k] = X0
        ip = np.ascontiguousarray(ipiv, dtype=np.int32)
        rc = ex.load_library().exblas_exgetrs_batched(order, p, n, k, ctypes.c_void_p(buf.ctypes.data), ld, stride,
                                                      ctypes.c_void_p(ip.ctypes.data), ctypes.c_void_p(wide.ctypes.data), k + 2,
                                                      8, 1)
        assert rc == 0 and (wide[:, k:].view(np.int64) == J.NAN_BITS).all()
        J.same_bits(wide[:, :k], want, np.ones((n, k), dtype=bool), "C host entry")
    X = ex.exgetrs_batched(np.zeros((0, 4, 4)), np.zeros((0, 4), dtype=np.int32), np.zeros((0, 3)))
    assert X.shape == (0, 3)
