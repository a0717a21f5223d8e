"""GPU suite for the batched ExGETRF: every entry, every pivot and every info word of every batch against the exact
factorisation of getrf_cases (never against the code under test), at the seams of the packing, on every path and variant,
both orders, padded leading dimensions and gaps between the matrices; the counters; planted ties, breakdowns and NaN
matrices beside healthy ones; pivot ties and signed zeros; the plain variant, the reference rounding mode, refusals, contexts
and host arrays.  A batch cycles seven distinct matrices.  The ends of the double range (totals at the
overflow threshold, around 2^1000, among the subnormals, zeros by cancellation) are in test_gpu_bjacobi_range.py."""
import ctypes

import numpy as np
import pytest

import bjacobi_cases as J
import getrf_cases as G

pytestmark = pytest.mark.gpu
ALL = np.ones((1, 1), dtype=bool)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_getrf_batched_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _counters(ex):
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_getrf_batched_info(out) == 0
    info = tuple(int(v) for v in out)
    assert ex.last_getrf_batched_info() == info and info[2] == 0 and info[3] == 0
    return info


def _factor(ex, A, layout, pad, gap, fpe=8, ee=True, entry=None, ipiv=None, info=None):
    """the logical [batch, p, p] matrices on the device in the layout, NaN in the padding and the gaps; returns (the
    [batch, p, p] result, the pivots, the info words, the counters) after checking that nothing else was written"""
    import torch
    batch, p = A.shape[0], A.shape[1]
    buf, ld, stride, strides = J.pack(A, layout, pad, gap)
    dev = torch.from_numpy(buf).cuda()
    Ad = dev.as_strided((batch, p, p), strides)
    out, piv, inf = (entry or ex.exgetrf_batched_dev)(Ad, ipiv, info, fpe, ee)
    assert out is Ad and inf.dtype == torch.int32 and tuple(inf.shape) == (batch,) and (info is None or inf is info)
    assert piv.dtype == torch.int32 and tuple(piv.shape) == (batch, p) and (ipiv is None or piv is ipiv)
    counters = _counters(ex)
    got = J.unpack(dev.cpu().numpy(), batch, p, strides, np.ones((p, p), dtype=bool))
    return got, piv.cpu().numpy(), inf.cpu().numpy(), counters


def _check(ex, p, batch, path, t, seven=None):
    """one call: rotation t picks the layout and the variant"""
    layout, pad, gap = G.LAYOUTS[t % len(G.LAYOUTS)]
    fpe, ee = G.VARIANTS[t % 3]
    A, want, pivots, infos, entries = G.factor_batch(p, batch, seven)
    ex.set_getrf_batched_path(path)
    got, piv, inf, cnt = _factor(ex, A, layout, pad, gap, fpe, ee)
    what = (p, batch, path, layout, pad, gap, fpe)
    assert (inf == infos).all(), (what, inf[:16], infos[:16])
    assert (piv == pivots).all(), (what, np.argwhere(piv != pivots)[:4].tolist())
    J.same_bits(got, want, ALL, what)
    assert cnt[0] + cnt[1] == sum(e.roundings for e in entries), (what, cnt)
    assert cnt[1] >= sum(e.ties for e in entries), (what, cnt)        # no tie is ever decided in registers
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return cnt


@pytest.mark.parametrize("p", G.SIZES)
def test_every_batch_at_the_seams_of_the_packing_on_every_path(ex, p):
    """breakdowns and a NaN matrix sit among the seven: every neighbour of theirs is held to its own model"""
    try:
        t = p
        for batch in J.batches(p):
            for path in (0, 1, 2, 3):
                cnt = _check(ex, p, batch, path, t)
                t += 1
        print("batched getrf", p, J.batches(p), "last counters", cnt)
    finally:
        ex.set_getrf_batched_path(0)


@pytest.mark.parametrize("p", [9, 17, 32, 40, 64])
def test_planted_matrices_fill_a_batch(ex, p):
    """every matrix of the batch carries the planted ties (as candidates and in the row of U), in every lane group of a
    wave; the row-shuffled copies give the same factors with other pivots"""
    c = G.planted(p)
    a, b = G._entry("planted", c.A), G._entry("planted, shuffled", c.shuffled)
    assert a.ties == b.ties == c.ties and (a.ipiv != b.ipiv).any()
    try:
        t = 0
        for path in (0, 1, 2, 3):
            for batch in (64 // J.pw_of(p) + 1, 23):
                cnt = _check(ex, p, batch, path, t, seven=(a, b, b, a, b, a, a))
                assert cnt[1] >= batch * c.ties
                t += 1
    finally:
        ex.set_getrf_batched_path(0)


@pytest.mark.parametrize("what", ["zero", "nan"])
def test_breakdown_at_the_first_an_inner_and_the_last_step(ex, what):
    """the rule per matrix: the candidates in column j, no swap, the identity pivots from j on, the rest of that matrix as it
    was, info = j + 1; the healthy matrices around it (and in its own wave) are factored as ever"""
    try:
        t = 0
        for p in (1, 3, 8, 16, 33, 64):
            base = G.factor_seven(p)
            for j in sorted({0, p // 2, p - 1}):
                e = G._entry("breakdown", G.zero_pivot(p, j) if what == "zero" else G.nan_pivot(p, j))
                assert e.info == j + 1
                seven = (base[0], e, base[2], base[3], e, base[1], base[1])
                _check(ex, p, 2 * (64 // J.pw_of(p)) + 3, (0, 2, 3, 1)[t % 4], t, seven=seven)
                t += 1
    finally:
        ex.set_getrf_batched_path(0)


@pytest.mark.parametrize("p", [2, 5, 16, 33])
def test_pivot_ties_signed_zeros_and_infinite_pivots(ex, p):
    """equal |c|: the first index wins, whatever the signs; a zero candidate under a negative pivot gives l = -0; an
    infinite pivot is no breakdown"""
    tie = G.pivot_tie(p)
    allt = G.random_matrix(p, 50)
    allt[:, 0] = np.sign(allt[:, 0]) * 0.5                                     # every candidate of column 0 ties
    neg = G.dominant(p, 6)
    neg[np.diag_indices(p)] = -np.abs(np.diag(neg))
    neg[1:, 0] = 0.0
    neg[p - 1, 0] = -0.0
    inf = G.dominant(p, 7)
    inf[0, 0] = np.inf
    inf2 = inf.copy()
    inf2[1, 0] = -np.inf
    ents = [G._entry(n, M) for n, M in (("tie", tie), ("all tie", allt), ("negative pivots", neg), ("inf", inf),
                                        ("two inf", inf2), ("tie, negated", -tie), ("tie, transposed", tie.T.copy()))]
    assert ents[0].ipiv[0] == (1 if p == 2 else p // 2 + 1) and ents[1].ipiv[0] == 1
    assert (ents[2].W[1:, 0] == 0).all() and np.signbit(ents[2].W[1:, 0]).all()
    assert ents[3].info == 0 and ents[4].info == 2
    try:
        for t, path in enumerate((0, 1, 2, 3)):
            _check(ex, p, 64 // J.pw_of(p) + 8, path, t, seven=tuple(ents))
    finally:
        ex.set_getrf_batched_path(0)


@pytest.mark.parametrize("p", [1, 4, 7, 16, 33, 64])
def test_plain_variant_equals_its_fp64_restatement(ex, p):
    from types import SimpleNamespace
    mats = [e.A for e in G.factor_seven(p)]
    mats[1] = mats[1].copy()
    mats[1][:, 0] = -0.0                 # a column of negative zeros: the plain candidate keeps its sign, a breakdown
    seven = []
    for A in mats:
        W, ipiv, info = G.plain_getrf(A)
        seven.append(SimpleNamespace(name="plain", A=A, W=W, ipiv=ipiv, info=info, ties=0, roundings=0))
    assert seven[1].info == 1 and np.signbit(seven[1].W[:, 0]).all()
    try:
        for path, (layout, pad, gap) in zip((0, 2, 3), G.LAYOUTS):
            ex.set_getrf_batched_path(path)
            batch = 4 * (64 // J.pw_of(p)) + 1
            A, want, pivots, infos, _ = G.factor_batch(p, batch, tuple(seven))
            a, pa, ia, cnt = _factor(ex, A, layout, pad, gap, 1, False)
            b, pb, ib, _ = _factor(ex, A, layout, pad, gap, 1, True)
            assert cnt == (0, 0, 0, 0) and (ia == infos).all() and (ib == infos).all()
            assert (pa == pivots).all() and (pb == pivots).all()
            J.same_bits(a, want, ALL, ("plain", p, path))
            J.same_bits(b, a, ALL, ("plain, again", p, path))
    finally:
        ex.set_getrf_batched_path(0)


@pytest.mark.parametrize("p", [9, 40])
def test_reference_rounding_mode(ex, p):
    """every output goes through the accumulator and is rounded the reference's way: the paths agree bit for bit, nothing is
    rounded in registers, and the planted ties tell the modes apart"""
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        first = None
        for path, (layout, pad, gap) in zip((0, 1, 2, 3), G.LAYOUTS):
            ex.set_getrf_batched_path(path)
            batch = 64 // J.pw_of(p) + 6
            A, want, pivots, infos, entries = G.factor_batch(p, batch)
            got, piv, inf, cnt = _factor(ex, A, layout, pad, gap, (8, 0, 4, 8)[path], True)
            assert cnt == (0, sum(e.roundings for e in entries), 0, 0), (path, cnt)
            assert (inf == infos).all()
            if first is None:
                first = (got, piv)
            J.same_bits(got, first[0], ALL, ("reference mode", p, path))
            assert (piv == first[1]).all()
        # matrix 0 is the planted one: its ties round the other way somewhere
        assert entries[0].name == "planted"
        assert (first[0][0].view(np.int64) != want[0].view(np.int64)).any(), "the modes never differed"
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_getrf_batched_path(0)


def test_refusals_write_nothing_and_an_empty_batch_leaves_ipiv_and_info_alone(ex):
    import torch
    lib = ex.load_library()
    a = torch.full((3, 70, 70), 2.5, dtype=torch.float64, device="cuda")
    ipiv = torch.full((3, 70), 9, dtype=torch.int32, device="cuda")
    info = torch.full((3,), 7, dtype=torch.int32, device="cuda")
    vp = ctypes.c_void_p
    pa, pp, pi = vp(a.data_ptr()), vp(ipiv.data_ptr()), vp(info.data_ptr())
    for args in ((b"C", 65, 3, 70, 4900), (b"X", 4, 3, 70, 4900), (b"U", 4, 3, 70, 4900), (b"R", -1, 3, 70, 4900),
                 (b"R", 4, -1, 70, 4900), (b"C", 4, 3, 3, 4900), (b"C", 4, 3, 70, 279), (b"R", 8, 2, 8, 63)):
        order, p, batch, lda, stride = args
        assert lib.exblas_exgetrf_batched_dev(order, p, batch, pa, lda, stride, pp, pi, 8, 1, None) == 1, args
    assert lib.exblas_exgetrf_batched_dev(b"C", 4, 3, pa, 70, 4900, pp, pi, -1, 1, None) == 1
    assert lib.exblas_exgetrf_batched_dev(b"C", 4, 3, pa, 70, 4900, pp, pi, 9, 1, None) == -1
    assert lib.exblas_exgetrf_batched_dev(b"C", 4, 3, pa, 70, 4900, pp, None, 8, 1, None) == 1
    assert lib.exblas_exgetrf_batched_dev(b"C", 4, 3, pa, 70, 4900, None, pi, 8, 1, None) == 1
    assert lib.exblas_exgetrf_batched_dev(b"C", 4, 3, None, 70, 4900, pp, pi, 8, 1, None) == 1
    with pytest.raises(ValueError):
        ex.exgetrf_batched_dev(a[:, :65, :65], None, info)
    # p == 0 or batch == 0: success, nothing launched, nothing written
    out, piv, inf = ex.exgetrf_batched_dev(a[:0, :4, :4], ipiv[:0, :4].contiguous(), info[:0])
    assert out.shape[0] == 0 and _counters(ex) == (0, 0, 0, 0)
    assert lib.exblas_exgetrf_batched_dev(b"C", 4, 0, pa, 70, 4900, pp, pi, 8, 1, None) == 0
    assert lib.exblas_exgetrf_batched_dev(b"R", 0, 3, pa, 70, 4900, pp, pi, 8, 1, None) == 0
    out, piv, inf = ex.exgetrf_batched_dev(a[:, :0, :0], None, info)
    assert inf is info and tuple(piv.shape) == (3, 0) and _counters(ex) == (0, 0, 0, 0)
    torch.cuda.synchronize()
    assert (a == 2.5).all() and (info == 7).all() and (ipiv == 9).all()


def test_contexts_streams_and_host_arrays(ex):
    import torch
    p, batch = 17, 12
    ctx, side = ex.Context(), torch.cuda.Stream()
    A, want, pivots, infos, _ = G.factor_batch(p, batch)
    try:
        torch.cuda.synchronize()
        words = torch.full((batch,), -3, dtype=torch.int32, device="cuda")
        pv = torch.full((batch, p), -3, dtype=torch.int32, device="cuda")
        with torch.cuda.stream(side):
            got, piv, inf, _ = _factor(ex, A, "row", 2, 3, entry=ctx.exgetrf_batched, ipiv=pv, info=words)
        side.synchronize()
        assert (inf == infos).all() and (piv == pivots).all()
        J.same_bits(got, want, ALL, "a private context on a side stream")
        assert 0 < ctx.workspace_bytes() <= 1 << 16              # the counters, and nothing like a mailbox
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
    # host arrays: C order and Fortran order per matrix; the input is not changed
    for arr in (A.copy(), np.ascontiguousarray(A.transpose(0, 2, 1)).transpose(0, 2, 1)):
        keep = arr.copy()
        LU, piv, info = ex.exgetrf_batched(arr)
        assert info.dtype == np.int32 and (info == infos).all() and LU is not arr
        assert piv.dtype == np.int32 and (piv == pivots).all()
        assert ((arr == keep) | np.isnan(keep)).all()
        J.same_bits(LU, want, ALL, "host")
    # the C host entry with a padded leading dimension and a gap: both come back as they went; ipiv and info may be NULL
    A3, want3, piv3, info3, _ = G.factor_batch(p, 3)
    for order, layout in ((b"C", "col"), (b"R", "row")):
        buf, ld, stride, strides = J.pack(A3, layout, 2, 4)
        rc = ex.load_library().exblas_exgetrf_batched(order, p, 3, ctypes.c_void_p(buf.ctypes.data), ld, stride, None, None, 8, 1)
        assert rc == 0
        J.same_bits(J.unpack(buf, 3, p, strides, np.ones((p, p), dtype=bool)), want3, ALL, "C host entry")
        buf, ld, stride, strides = J.pack(A3, layout, 2, 4)
        ip, inf = np.zeros((3, p), dtype=np.int32), np.full(3, -1, dtype=np.int32)
        rc = ex.load_library().exblas_exgetrf_batched(order, p, 3, ctypes.c_void_p(buf.ctypes.data), ld, stride,
                                                      ctypes.c_void_p(ip.ctypes.data), ctypes.c_void_p(inf.ctypes.data), 0, 0)
        assert rc == 0 and (ip == piv3).all() and (inf == info3).all()
    LU, piv, info = ex.exgetrf_batched(np.zeros((0, 4, 4)))
    assert LU.shape == (0, 4, 4) and piv.shape == (0, 4) and info.shape == (0,)
