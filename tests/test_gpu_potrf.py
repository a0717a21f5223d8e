"""GPU suite for ExPOTRF: every output bit against the Fraction factorisation of potrf_cases (never against the code under
test), on planted ties, carries and near-ties, at the seams of the row block, the column tile and the staging, on both
triangles and both layouts, with the counters; the square root and the division; the range; LAPACK's breakdown rule; the
plumbing (plain variant, reference rounding, contexts, host arrays, graphs) and the CholQR chain."""
import ctypes
import functools
import math

import numpy as np
import pytest

import potrf_cases as P

pytestmark = pytest.mark.gpu

VARIANTS = ((0, False), (4, True), (8, True))
LAYOUTS = (("U", "col", 0), ("L", "row", 3), ("L", "col", 2), ("U", "row", 0), ("U", "col", 5), ("L", "row", 0),
           ("L", "col", 0), ("U", "row", 1))            # (uplo, layout, padding of the leading dimension)
NAN_BITS = np.array(np.nan).view(np.int64)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_potrf_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _counters(ex):
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_potrf_info(out) == 0
    info = tuple(int(v) for v in out)
    assert ex.last_potrf_info() == info and info[2] == 0 and info[3] == 0
    return info


def _mask(p, uplo):
    return np.triu(np.ones((p, p), dtype=bool)) if uplo == "U" else np.tril(np.ones((p, p), dtype=bool))


def _same(got, want, mask, what):
    """bit for bit on the triangle; a NaN is a NaN"""
    g, w = np.asarray(got)[mask], np.asarray(want)[mask]
    ok = (g.view(np.int64) == w.view(np.int64)) | (np.isnan(g) & np.isnan(w))
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:4].tolist(), g[~ok][:4], w[~ok][:4])


def _factor(ex, G, uplo="U", layout="col", pad=0, fpe=8, ee=True, entry=None, info=None):
    """G's `uplo` triangle (as Python indexes it) on the device in the layout, NaN in the other triangle and in the
    padding; returns (the p x p result, info, counters) after checking that neither was written"""
    import torch
    G = np.asarray(G, dtype=np.float64)
    p = G.shape[0]
    mask = _mask(p, uplo)
    full = np.where(mask, G, np.nan)
    buf = np.full((p, p + pad), np.nan)
    buf[:, :p] = full.T if layout == "col" else full
    dev = torch.from_numpy(buf).cuda()
    Gd = dev[:, :p].t() if layout == "col" else dev[:, :p]
    out, inf = (entry or ex.expotrf_dev)(Gd, uplo, info, fpe, ee)
    assert out is Gd and inf.dtype == torch.int32 and inf.numel() == 1 and (info is None or inf is info)
    counters = _counters(ex)
    back = dev.cpu().numpy()
    got = back[:, :p].T if layout == "col" else back[:, :p]
    assert (back[:, p:].view(np.int64) == NAN_BITS).all(), "the padding was written"
    assert (got[~mask].view(np.int64) == NAN_BITS).all(), "the other triangle was written"
    return got, int(inf.item()), counters


def _want(G, uplo):
    """the model on the triangle the call was given"""
    R, info = P.potrf_exact(G, "U")
    return (R if uplo == "U" else R.T), info


# ---------------------------------------------------------------------------------------------
# planted systems
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pure", [False, True], ids=["mixed", "pure"])
@pytest.mark.parametrize("p", tuple(P.BLOCKS))
def test_planted_systems_every_path_and_variant(ex, p, pure):
    c = P.planted(p, pure)
    total, ties, clear = p * (p + 1) // 2, int((c.kind == P.TIE).sum()), int((c.kind == P.CLEAR).sum())
    try:
        t = 0
        for path in (0, 1, 2, 3):
            ex.set_potrf_path(path)
            for fpe, ee in VARIANTS:
                uplo, layout, pad = LAYOUTS[t % len(LAYOUTS)]
                t += 1
                got, info, cnt = _factor(ex, c.G, uplo, layout, pad, fpe, ee)
                print("planted", p, pure, path, fpe, uplo, layout, pad, cnt, "ties", ties, "clear", clear)
                assert info == 0
                _same(got, c.R if uplo == "U" else c.R.T, _mask(p, uplo), (p, pure, path, fpe, ee, uplo, layout, pad))
                assert cnt[0] + cnt[1] == total
                assert cnt[1] >= ties                              # no tie or carry is ever decided in registers
                if fpe == 0 or path == 1:
                    assert cnt[0] == 0
                elif path == 0 and pure:
                    # nothing of a pure system is left to either side: the ties, carries and out-of-range totals go to
                    # the accumulator, the quarter-unit controls and everything else are decided in registers
                    assert cnt == (clear, ties, 0, 0)
    finally:
        ex.set_potrf_path(0)


# ---------------------------------------------------------------------------------------------
# seams
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gram130():
    G = P.gram(130)
    R, info = P.potrf_exact(G)
    assert info == 0
    return G, R


SEAMS = ((1, 2, 3, 4, 5, 6, 7, 8, 9), (15, 16, 17, 31, 32, 33), (63, 64, 65, 66), (127, 128, 129, 130))


@pytest.mark.parametrize("sizes", SEAMS, ids=["1-9", "15-33", "63-66", "127-130"])
def test_random_gram_matrices_at_the_seams(ex, sizes):
    """the factor of a leading submatrix is the leading part of the factor: one Fraction factorisation serves them all"""
    G, R = _gram130()
    try:
        t = 0
        for q in sizes:
            for path in (0, 1, 2, 3):
                ex.set_potrf_path(path)
                uplo, layout, pad = LAYOUTS[t % len(LAYOUTS)]
                fpe, ee = VARIANTS[(t // 3) % 3]
                t += 1
                got, info, cnt = _factor(ex, G[:q, :q], uplo, layout, pad, fpe, ee)
                assert info == 0 and cnt[0] + cnt[1] == q * (q + 1) // 2
                _same(got, R[:q, :q] if uplo == "U" else R[:q, :q].T, _mask(q, uplo), (q, path, uplo, layout, pad, fpe))
    finally:
        ex.set_potrf_path(0)


def _identities(ex, G, got, cols, diags, what):
    """the strict part of column i is ExTRSV's solve with the leading factor; the radicand is ExBGEMM's rounded update"""
    import torch
    p = G.shape[0]
    Rd = torch.from_numpy(np.asfortranarray(np.triu(got)).T.copy()).cuda().t()      # column-major, ld p
    assert Rd.stride(0) == 1
    for i in cols:
        x = torch.from_numpy(np.ascontiguousarray(G[:i, i])).cuda()
        assert ex.extrsv_dev("U", "T", "N", i, Rd, p, x, 8, True) == 0
        assert (x.cpu().numpy().view(np.int64) == got[:i, i].view(np.int64)).all(), (what, "column", i)
    for i in diags:
        r = torch.from_numpy(np.ascontiguousarray(got[:i, i])).cuda()
        y = torch.tensor([[G[i, i]]], dtype=torch.float64, device="cuda")
        ex.exbgemm_dev(r.reshape(1, i), r.reshape(i, 1), -1.0, 1.0, y)
        assert math.sqrt(float(y.item())) == got[i, i], (what, "diagonal", i)


@pytest.mark.parametrize("p", [200, 512])
def test_banded_matrices_beyond_the_tile(ex, p):
    """bandwidth 5: the kernel still counts the zeros, the Fraction side skips them"""
    G = P.banded(p)
    R, info = P.potrf_exact(G)
    assert info == 0
    try:
        for path, uplo, layout, pad, fpe in ((0, "U", "col", 0, 8), (1 if p == 512 else 3, "L", "row", 1, 8),
                                             (2, "L", "col", 3, 0 if p == 200 else 4)):
            ex.set_potrf_path(path)
            got, info, cnt = _factor(ex, G, uplo, layout, pad, fpe, True)
            assert info == 0 and cnt[0] + cnt[1] == p * (p + 1) // 2
            _same(got, R if uplo == "U" else R.T, _mask(p, uplo), (p, path, uplo, layout))
            if path == 0:
                _identities(ex, G, got, (p - 1, 321 % p, 65), (p - 1, 64, 3), ("banded", p))
    finally:
        ex.set_potrf_path(0)


def test_dense_factor_at_200_through_the_identities(ex):
    rng = np.random.default_rng(200)
    Xm = rng.standard_normal((403, 200))
    G = Xm.T @ Xm
    got, info, cnt = _factor(ex, G, "U", "col", 0)
    assert info == 0 and cnt[0] + cnt[1] == 200 * 201 // 2
    assert np.allclose(np.triu(got), np.linalg.cholesky(G).T, rtol=1e-9, atol=1e-9)
    _identities(ex, G, got, (199, 130, 64), (199, 65, 4), "dense 200")
    again, _, _ = _factor(ex, G, "L", "row", 2, 0, False)
    _same(again, got.T, _mask(200, "L"), "dense 200, the other triangle, accumulators only")


def test_embedded_two_by_two_case_across_4_and_64(ex):
    try:
        t = 0
        for at in ((2, 3), (3, 4), (3, 5), (62, 63), (63, 64), (64, 65), (60, 69)):
            for g2, rad in ((P.G2, 3.0), (P.G7, 7.0)):
                G = P.embedded(70, at, g2)
                want, winfo = _want(G, "U")
                assert winfo == 0 and want[at[1], at[1]] == math.sqrt(rad)
                for path in (0, 1, 2, 3):
                    ex.set_potrf_path(path)
                    uplo, layout, pad = LAYOUTS[t % len(LAYOUTS)]
                    t += 1
                    got, info, _ = _factor(ex, G, uplo, layout, pad, *VARIANTS[t % 3])
                    assert info == 0
                    _same(got, want if uplo == "U" else want.T, _mask(70, uplo), (at, rad, path, uplo, layout))
    finally:
        ex.set_potrf_path(0)


# ---------------------------------------------------------------------------------------------
# square root, division, range
# ---------------------------------------------------------------------------------------------
def test_square_roots_bit_for_bit(ex):
    """a diagonal G: one call takes 512 roots"""
    v = P.root_values()
    want = np.array([math.sqrt(x) for x in v])
    try:
        for path, uplo, fpe in ((0, "U", 8), (2, "L", 0), (1, "U", 4)):
            ex.set_potrf_path(path)
            got, info, cnt = _factor(ex, np.diag(v), uplo, "col", 1, fpe, True)
            assert info == 0 and cnt[0] + cnt[1] == 512 * 513 // 2
            assert (np.diag(got).view(np.int64) == want.view(np.int64)).all(), (path, uplo)
        for path in (0, 1, 2, 3):
            ex.set_potrf_path(path)
            got, info, _ = _factor(ex, np.diag(v[100:170]), "U", "row", 0)
            assert info == 0 and (np.diag(got).view(np.int64) == want[100:170].view(np.int64)).all(), path
    finally:
        ex.set_potrf_path(0)


def test_totals_and_radicands_at_the_ends_of_the_range(ex):
    try:
        t = 0
        for name, G in P.range_cases():
            want, winfo = _want(G, "U")
            o = 66 if "@" in name else 0
            if name.startswith("subnormal total"):
                assert winfo == 0 and want[o + 1, o + 2] == -2.0 ** -1071
            if name.startswith("subnormal radicand"):
                assert winfo == 0 and want[o + 1, o + 1] == math.sqrt((2 ** 27 - 1) * 2.0 ** -1072)
            if name.startswith("overflow"):
                assert winfo == o + 3 and want[o + 1, o + 2] == np.inf and want[o + 2, o + 2] == -np.inf
            if name.startswith("inf"):
                assert winfo == 0 and np.isinf(want).sum() == 1
            for path in (0, 1, 2, 3):
                ex.set_potrf_path(path)
                uplo, layout, pad = LAYOUTS[t % len(LAYOUTS)]
                t += 1
                p = G.shape[0]
                got, info, cnt = _factor(ex, G, uplo, layout, pad, *VARIANTS[t % 3])
                assert info == winfo and cnt[0] + cnt[1] == P.fixed_entries(p, winfo), (name, path, info, cnt)
                _same(got, want if uplo == "U" else want.T, _mask(p, uplo), (name, path, uplo, layout))
    finally:
        ex.set_potrf_path(0)


# ---------------------------------------------------------------------------------------------
# breakdown
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["zero", "neg", "nan"])
def test_breakdown_follows_lapacks_rule(ex, what):
    import torch
    try:
        t = 0
        info_t = torch.full((1,), -5, dtype=torch.int32, device="cuda")
        for p in (66, 70):
            for j in P.breakdown_pivots(p):
                G = P.breakdown(p, j, what)
                want, winfo = _want(G, "U")
                assert winfo == j + 1
                for path in ((0, 3) if t % 2 else (1, 2)):
                    ex.set_potrf_path(path)
                    uplo, layout, pad = LAYOUTS[t % len(LAYOUTS)]
                    fpe, ee = VARIANTS[t % 3]
                    t += 1
                    got, info, cnt = _factor(ex, G, uplo, layout, pad, fpe, ee, info=info_t)
                    assert info == j + 1, (p, j, path, info)
                    # the stored pivot, the fixed rows, and every entry that must be unchanged: the model left them as G
                    _same(got, want if uplo == "U" else want.T, _mask(p, uplo), (what, p, j, path, uplo, layout))
                    v = got[j, j]
                    assert (v == 0.0) if what == "zero" else (v == -1.0) if what == "neg" else math.isnan(v)
                    assert cnt[0] + cnt[1] == P.fixed_entries(p, j + 1), (p, j, path, cnt)
        # a successful call on the same info tensor afterwards writes 0
        assert int(info_t.item()) != 0
        got, info, cnt = _factor(ex, P.G7, "U", "col", 0, info=info_t)
        assert info == 0 and int(info_t.item()) == 0 and got[1, 1] == math.sqrt(7.0) and cnt[0] + cnt[1] == 3
    finally:
        ex.set_potrf_path(0)


# ---------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------
def test_plain_variant_is_deterministic_and_close(ex):
    G, R = _gram130()
    for q, uplo, layout in ((40, "U", "col"), (130, "L", "row")):
        a, info, cnt = _factor(ex, G[:q, :q], uplo, layout, 1, 1, False)
        b, _, _ = _factor(ex, G[:q, :q], uplo, layout, 1, 1, False)
        assert info == 0 and cnt == (0, 0, 0, 0)
        m = _mask(q, uplo)
        assert (a[m].view(np.int64) == b[m].view(np.int64)).all()
        assert np.allclose(a[m], (R[:q, :q] if uplo == "U" else R[:q, :q].T)[m], rtol=1e-9, atol=0.0)
    G = P.breakdown(66, 64, "neg")
    got, info, cnt = _factor(ex, G, "U", "col", 0, 1, False)
    assert info == 65 and got[64, 64] == -1.0 and (got[64, 65:] == G[64, 65:]).all() and cnt == (0, 0, 0, 0)


@pytest.mark.parametrize("p", [40, 65])
def test_reference_rounding_mode(ex, oracle, p):
    """ties are where the two modes differ: column by column the factor follows the oracle's reference-mode ExTRSV on the
    leading factor, and the radicands ExBGEMM under the same mode"""
    import torch
    lib = ex.load_library()
    c = P.planted(p)
    lib.exblas_set_round_mode(1)
    try:
        first = None
        for path, (uplo, layout, pad) in zip((0, 3, 2), LAYOUTS):
            ex.set_potrf_path(path)
            got, info, cnt = _factor(ex, c.G, uplo, layout, pad, (8, 0, 4)[path % 3], True)
            got = got if uplo == "U" else got.T
            assert info == 0 and cnt == (0, p * (p + 1) // 2, 0, 0)
            if first is None:
                first = np.triu(got)
                a = np.asfortranarray(first).ravel(order="F")
                for i in range(1, p):
                    rc, w = oracle.extrsv("U", "T", "N", i, a, p, c.G[:i, i], 0, mode=oracle.ROUND_REFERENCE)
                    assert rc == 0 and (w.view(np.int64) == first[:i, i].view(np.int64)).all(), ("column", i)
                    r = torch.from_numpy(np.ascontiguousarray(first[:i, i])).cuda()
                    y = torch.tensor([[c.G[i, i]]], dtype=torch.float64, device="cuda")
                    ex.exbgemm_dev(r.reshape(1, i), r.reshape(i, 1), -1.0, 1.0, y)
                    assert math.sqrt(float(y.item())) == first[i, i], ("diagonal", i)
                assert (first.view(np.int64) != np.triu(c.R).view(np.int64)).any(), "the modes never differed on these ties"
            else:
                assert (np.triu(got).view(np.int64) == first.view(np.int64)).all(), (path, uplo, layout)
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_potrf_path(0)


def test_contexts_streams_host_arrays_and_empty(ex):
    import torch
    c = P.planted(65)
    ctx, side = ex.Context(), torch.cuda.Stream()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got, info, _ = _factor(ex, c.G, "L", "row", 2, entry=ctx.expotrf)
        side.synchronize()
        assert info == 0
        _same(got, c.R.T, _mask(65, "L"), "a private context on a side stream")
        assert 0 < ctx.workspace_bytes() <= 1 << 16              # the counters, and nothing like a mailbox
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
    # host arrays: C order and Fortran order, both triangles; the input is not changed
    for uplo in ("U", "L"):
        for arr in (np.ascontiguousarray(c.G), np.asfortranarray(c.G)):
            keep = arr.copy()
            R, info = ex.expotrf(arr, uplo)
            assert isinstance(info, int) and info == 0 and R is not arr and (arr == keep).all()
            _same(R, c.R if uplo == "U" else c.R.T, _mask(65, uplo), ("host", uplo))
            assert (R[~_mask(65, uplo)] == c.G[~_mask(65, uplo)]).all()
    R, info = ex.expotrf(P.breakdown(9, 4, "zero"), "U", 0, False)
    assert info == 5 and R[4, 4] == 0.0
    # the C host entry with a padded leading dimension: the padding comes back as it went
    g = np.full((2, 7), -7.25)                                   # g[column, row], ldg = 7
    g[:, :2] = P.G2.T
    word = ctypes.c_int(9)
    assert ex.load_library().exblas_expotrf(b"U", 2, ctypes.c_void_p(g.ctypes.data), 7, ctypes.byref(word), 8, 1) == 0
    assert word.value == 0 and g[1, 1] == math.sqrt(3.0) and g[1, 0] == P.A2 and g[0, 1] == P.A2
    assert (g[:, 2:] == -7.25).all()
    # p == 0: success, nothing launched, info not written
    empty = torch.zeros(0, 0, dtype=torch.float64, device="cuda")
    word = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    out, inf = ex.expotrf_dev(empty, "U", word)
    assert out is empty and inf is word and int(word.item()) == 7 and _counters(ex) == (0, 0, 0, 0)
    R, info = ex.expotrf(np.zeros((0, 0)))
    assert R.shape == (0, 0) and info == 0


def test_graph_restores_g_and_factors_it(ex):
    """A captured copy and factorisation, replayed three times, info, counters and bits read after each replay; the second
    replay meets a breakdown swapped into the source buffer."""
    import torch
    p = 65
    c = P.planted(p)
    Gb = P.breakdown(p, 64, "neg")
    wb, ib = P.potrf_exact(Gb)
    src = torch.from_numpy(c.G.copy()).cuda()
    work = torch.empty_like(src)
    info = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    work.copy_(src)
    ex.expotrf_dev(work, "U", info)                               # the warm call that sizes the workspace
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            work.copy_(src)
            ex.expotrf_dev(work, "U", info)
    m = _mask(p, "U")
    for G, want, winfo in ((c.G, c.R, 0), (Gb, wb, ib), (c.G, c.R, 0)):
        src.copy_(torch.from_numpy(G))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        cnt = _counters(ex)
        assert int(info.item()) == winfo and cnt[0] + cnt[1] == P.fixed_entries(p, winfo)
        _same(work.cpu().numpy(), want, m, ("replay", winfo))
        assert (work.cpu().numpy()[~m] == G[~m]).all()
    del g


# ---------------------------------------------------------------------------------------------
# the chain
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,p", [(300, 5), (1000, 64)])
def test_excholqr_chain_eager_and_captured(ex, n, p):
    """bit for bit exbdot_dev, then potrf_exact on the host, then exbtrsm_dev"""
    import torch
    rng = np.random.default_rng([n, p])
    X0 = torch.from_numpy(rng.standard_normal((n, p))).cuda()
    G = ex.exbdot_dev(X0).cpu().numpy()
    R, winfo = P.potrf_exact(G, "U")
    assert winfo == 0
    Rd = torch.from_numpy(np.triu(R)).cuda()
    Q = ex.exbtrsm_dev(Rd, X0.clone(), "U", "N")
    want_q, m = Q.cpu().numpy(), _mask(p, "U")

    X = X0.clone()
    out, Rg, info = ex.excholqr_dev(X)
    assert out is X and int(info.item()) == 0
    _same(Rg.cpu().numpy(), R, m, "eager R")
    assert (X.cpu().numpy().view(np.int64) == want_q.view(np.int64)).all()
    assert np.allclose(want_q.T @ want_q, np.eye(p), atol=1e-8)

    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            X.copy_(X0)
            _, Rg, info = ex.excholqr_dev(X)
    for _ in range(2):
        X.zero_()
        Rg.zero_()
        info.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(info.item()) == 0
        _same(Rg.cpu().numpy(), R, m, "replayed R")
        assert (X.cpu().numpy().view(np.int64) == want_q.view(np.int64)).all()
    del g
