"""GPU suite for the batched ExPOTRF: every triangle and every info word of every batch against the Fraction factorisation
of potrf_cases (never against the code under test), at the seams of the packing, on every path and variant, both
triangles, both layouts, padded leading dimensions and gaps between the matrices; the counters; breakdowns and NaN matrices
beside healthy ones; the plain variant, the reference rounding mode, the single routine as a second witness, refusals,
contexts and host arrays.  A batch cycles seven distinct matrices (bjacobi_cases).  The ends of the double range (totals at the
overflow threshold, around 2^1000, among the subnormals, zeros by cancellation) are in test_gpu_bjacobi_range.py."""
import ctypes

import numpy as np
import pytest

import bjacobi_cases as J
import potrf_cases as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_potrf_batched_path(0)
    exblas_amd.set_potrf_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _counters(ex):
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_potrf_batched_info(out) == 0
    info = tuple(int(v) for v in out)
    assert ex.last_potrf_batched_info() == info and info[2] == 0 and info[3] == 0
    return info


def _factor(ex, full, uplo, layout, pad, gap, fpe=8, ee=True, entry=None, info=None):
    """the logical [batch, p, p] matrices (NaN in the other triangle) on the device in the layout, NaN in the padding and
    the gaps; returns (the [batch, p, p] result, the info words, the counters) after checking that nothing else was written"""
    import torch
    batch, p = full.shape[0], full.shape[1]
    buf, ld, stride, strides = J.pack(full, layout, pad, gap)
    dev = torch.from_numpy(buf).cuda()
    Gd = dev.as_strided((batch, p, p), strides)
    out, inf = (entry or ex.expotrf_batched_dev)(Gd, uplo, info, fpe, ee)
    assert out is Gd and inf.dtype == torch.int32 and tuple(inf.shape) == (batch,) and (info is None or inf is info)
    counters = _counters(ex)
    got = J.unpack(dev.cpu().numpy(), batch, p, strides, J.tri_mask(p, uplo))
    return got, inf.cpu().numpy(), counters


def _check(ex, p, batch, path, t, seven=None):
    """one call: rotation t picks the layout and the variant"""
    uplo, layout, pad, gap = J.LAYOUTS[t % len(J.LAYOUTS)]
    fpe, ee = J.VARIANTS[t % 3]
    full, want, infos, entries = J.factor_batch(p, batch, uplo, seven)
    ex.set_potrf_batched_path(path)
    got, inf, cnt = _factor(ex, full, uplo, layout, pad, gap, fpe, ee)
    what = (p, batch, path, uplo, layout, pad, gap, fpe)
    assert (inf == infos).all(), (what, inf[:16], infos[:16])
    J.same_bits(got, want, J.tri_mask(p, uplo), what)
    assert cnt[0] + cnt[1] == sum(e.fixed for e in entries), (what, cnt)
    assert cnt[1] >= sum(e.ties for e in entries), (what, cnt)        # no tie is ever decided in registers
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return cnt


@pytest.mark.parametrize("p", J.SIZES)
def test_every_batch_at_the_seams_of_the_packing_on_every_path(ex, p):
    """breakdowns and a NaN matrix sit among the seven: every neighbour of theirs is held to its own model"""
    try:
        t = p
        for batch in J.batches(p):
            for path in (0, 1, 2, 3):
                cnt = _check(ex, p, batch, path, t)
                t += 1
        print("batched potrf", p, J.batches(p), "last counters", cnt)
    finally:
        ex.set_potrf_batched_path(0)


@pytest.mark.parametrize("p", [9, 17, 32, 40, 64])
def test_planted_leading_parts_fill_a_batch(ex, p):
    """every matrix of the batch carries the planted ties, in every lane group of a wave"""
    G, R, ties, _ = J.planted_lead(p)
    e = J._entry("planted", G, R, 0, ties)
    try:
        t = 0
        for path in (0, 1, 2, 3):
            for batch in (64 // J.pw_of(p) + 1, 23):
                cnt = _check(ex, p, batch, path, t, seven=(e,) * 7)
                assert cnt[1] >= batch * ties
                t += 1
    finally:
        ex.set_potrf_batched_path(0)


@pytest.mark.parametrize("what", ["zero", "neg", "nan"])
def test_breakdown_at_the_first_an_inner_and_the_last_pivot(ex, what):
    """LAPACK's rule per matrix: the radicand at its pivot, the rest of that matrix as it was, info = j + 1; the healthy
    matrices around it (and in its own wave) are factored as ever"""
    try:
        t = 0
        for p in (1, 3, 8, 16, 33, 64):
            base = J.factor_seven(p)
            for j in sorted({0, p // 2, p - 1}):
                G = P.breakdown(p, j, what)
                R, info = P.potrf_exact(G, "U")
                assert info == j + 1
                e = J._entry("breakdown", G, R, info, 0)
                seven = (base[0], e, base[2], base[3], e, base[5], base[1])
                _check(ex, p, 2 * (64 // J.pw_of(p)) + 3, (0, 2, 3, 1)[t % 4], t, seven=seven)
                t += 1
    finally:
        ex.set_potrf_batched_path(0)


@pytest.mark.parametrize("p", [1, 4, 7, 16, 33, 64])
def test_plain_variant_equals_its_fp64_restatement(ex, p):
    seven = tuple(J._entry(e.name, e.G, *J.plain_factor(e.G), 0) for e in J.factor_seven(p))
    try:
        for path, (uplo, layout, pad, gap) in zip((0, 2, 3), J.LAYOUTS):
            ex.set_potrf_batched_path(path)
            batch = 4 * (64 // J.pw_of(p)) + 1
            full, want, infos, _ = J.factor_batch(p, batch, uplo, seven)
            a, ia, cnt = _factor(ex, full, uplo, layout, pad, gap, 1, False)
            b, ib, _ = _factor(ex, full, uplo, layout, pad, gap, 1, True)
            assert cnt == (0, 0, 0, 0) and (ia == infos).all() and (ib == infos).all()
            J.same_bits(a, want, J.tri_mask(p, uplo), ("plain", p, path))
            J.same_bits(b, a, J.tri_mask(p, uplo), ("plain, again", p, path))
    finally:
        ex.set_potrf_batched_path(0)


def _single(ex, e, uplo="U"):
    """expotrf_dev on one matrix, column-major: (the p x p result, info)"""
    import torch
    p = e.G.shape[0]
    m = J.tri_mask(p, uplo)
    dev = torch.from_numpy(np.where(m, e.G, np.nan).T.copy()).cuda()
    _, inf = ex.expotrf_dev(dev.t(), uplo)
    return dev.cpu().numpy().T, int(inf.item())


@pytest.mark.parametrize("p", [3, 16, 40, 64])
def test_every_matrix_is_what_the_single_routine_gives(ex, p):
    seven = J.factor_seven(p)
    full, want, infos, _ = J.factor_batch(p, 7, "U")
    got, inf, _ = _factor(ex, full, "U", "col", 1, 2)
    for b, e in enumerate(seven):
        one, info = _single(ex, e)
        assert info == inf[b] == e.info
        J.same_bits(got[b], one, J.tri_mask(p, "U"), ("single", p, e.name))


@pytest.mark.parametrize("p", [9, 40])
def test_reference_rounding_mode(ex, p):
    """every output goes through the accumulator and is rounded the reference's way: the single routine under the same mode
    is the witness (held to the oracle by its own tests), the paths agree, and the planted ties tell the modes apart"""
    lib = ex.load_library()
    seven = J.factor_seven(p)
    lib.exblas_set_round_mode(1)
    try:
        ref = tuple(J._entry(e.name, e.G, *_single(ex, e), 0) for e in seven)
        assert [e.info for e in ref] == [e.info for e in seven]
        if p == 40:
            assert (np.triu(ref[1].R).view(np.int64) != np.triu(seven[1].R).view(np.int64)).any(), "the modes never differed"
        for path, (uplo, layout, pad, gap) in zip((0, 1, 2, 3), J.LAYOUTS):
            ex.set_potrf_batched_path(path)
            batch = 64 // J.pw_of(p) + 6
            full, want, infos, entries = J.factor_batch(p, batch, uplo, ref)
            got, inf, cnt = _factor(ex, full, uplo, layout, pad, gap, (8, 0, 4, 8)[path], True)
            assert (inf == infos).all() and cnt == (0, sum(e.fixed for e in entries), 0, 0)
            J.same_bits(got, want, J.tri_mask(p, uplo), ("reference mode", p, path))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_potrf_batched_path(0)


def test_refusals_write_nothing_and_an_empty_batch_leaves_info_alone(ex):
    import torch
    lib = ex.load_library()
    g = torch.full((3, 70, 70), 2.5, dtype=torch.float64, device="cuda")
    info = torch.full((3,), 7, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p
    for args in ((b"U", 65, 3, 70, 4900), (b"X", 4, 3, 70, 4900), (b"U", -1, 3, 70, 4900), (b"U", 4, -1, 70, 4900),
                 (b"U", 4, 3, 3, 4900), (b"U", 4, 3, 70, 279), (b"L", 8, 2, 8, 63)):
        uplo, p, batch, ldg, stride = args
        rc = lib.exblas_expotrf_batched_dev(uplo, p, batch, vp(g.data_ptr()), ldg, stride, vp(info.data_ptr()), 8, 1, None)
        assert rc == 1, args
    assert lib.exblas_expotrf_batched_dev(b"U", 4, 3, vp(g.data_ptr()), 70, 4900, vp(info.data_ptr()), -1, 1, None) == 1
    assert lib.exblas_expotrf_batched_dev(b"U", 4, 3, vp(g.data_ptr()), 70, 4900, vp(info.data_ptr()), 9, 1, None) == -1
    assert lib.exblas_expotrf_batched_dev(b"U", 4, 3, vp(g.data_ptr()), 70, 4900, None, 8, 1, None) == 1
    assert lib.exblas_expotrf_batched_dev(b"U", 4, 3, None, 70, 4900, vp(info.data_ptr()), 8, 1, None) == 1
    with pytest.raises(ValueError):
        ex.expotrf_batched_dev(g[:, :65, :65], "U", info)
    # p == 0 or batch == 0: success, nothing launched, info not written
    out, inf = ex.expotrf_batched_dev(g[:0, :4, :4], "U", info[:0])
    assert out.shape[0] == 0 and _counters(ex) == (0, 0, 0, 0)
    assert lib.exblas_expotrf_batched_dev(b"U", 4, 0, vp(g.data_ptr()), 70, 4900, vp(info.data_ptr()), 8, 1, None) == 0
    assert lib.exblas_expotrf_batched_dev(b"U", 0, 3, vp(g.data_ptr()), 70, 4900, vp(info.data_ptr()), 8, 1, None) == 0
    out, inf = ex.expotrf_batched_dev(g[:, :0, :0], "U", info)
    assert inf is info and _counters(ex) == (0, 0, 0, 0)
    torch.cuda.synchronize()
    assert (g == 2.5).all() and (info == 7).all()


def test_contexts_streams_and_host_arrays(ex):
    import torch
    p, batch = 17, 12
    seven = J.factor_seven(p)
    ctx, side = ex.Context(), torch.cuda.Stream()
    try:
        torch.cuda.synchronize()
        full, want, infos, _ = J.factor_batch(p, batch, "L")
        words = torch.full((batch,), -3, dtype=torch.int32, device="cuda")
        with torch.cuda.stream(side):
            got, inf, _ = _factor(ex, full, "L", "row", 2, 3, entry=ctx.expotrf_batched, info=words)
        side.synchronize()
        assert (inf == infos).all()
        J.same_bits(got, want, J.tri_mask(p, "L"), "a private context on a side stream")
        assert 0 < ctx.workspace_bytes() <= 1 << 16              # the counters, and nothing like a mailbox
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
    # host arrays: C order and Fortran order per matrix, both triangles; the input is not changed
    sym = np.stack([seven[b % 7].G for b in range(batch)])
    for uplo in ("U", "L"):
        _, want, infos, _ = J.factor_batch(p, batch, uplo)
        m = J.tri_mask(p, uplo)
        for arr in (sym.copy(), np.ascontiguousarray(sym.transpose(0, 2, 1)).transpose(0, 2, 1)):
            keep = arr.copy()
            R, info = ex.expotrf_batched(arr, uplo)
            assert info.dtype == np.int32 and (info == infos).all() and R is not arr
            assert ((arr == keep) | np.isnan(keep)).all()
            J.same_bits(R, want, m, ("host", uplo))
            J.same_bits(R, sym, ~m, ("host, the other triangle", uplo))
    # the C host entry with a padded leading dimension and a gap: both come back as they went, info may be NULL
    full, want, infos, _ = J.factor_batch(p, 3, "U")
    buf, ld, stride, strides = J.pack(full, "col", 2, 4)
    rc = ex.load_library().exblas_expotrf_batched(b"U", p, 3, ctypes.c_void_p(buf.ctypes.data), ld, stride, None, 8, 1)
    assert rc == 0
    J.same_bits(J.unpack(buf, 3, p, strides, J.tri_mask(p, "U")), want, J.tri_mask(p, "U"), "C host entry")
    R, info = ex.expotrf_batched(np.zeros((0, 4, 4)))
    assert R.shape == (0, 4, 4) and info.shape == (0,)
