"""GPU tests of ExBGEMM (Y = alpha X C + beta Y, row-major blocks), bit for bit.

Expected bits never come from ExBGEMM: the Python-integer references of tests/exact_cases.py on planted ties, carries
and near-ties (every path, fpe variant and both rounding modes; the oracle's ExGEMV per output in the reference mode),
exblas_exspmm_csr_dev on X stored as a dense CSR matrix (the routine's contract) on random data, non-finite entries and
every size on both sides of a tile or chunk seam, ExGEMM where the two contracts meet (alpha = 1, beta = 0), and the
exact sums at the ends of the double range.  Every call runs with ldx > p, ldc > q and ldy > q: the padding of X and C
holds NaN, which must never be read, the padding of Y a sentinel whose bits must survive.

What is asserted of the counters (`last_bgemm_info`) is derived, not measured:
  accounting    registers + accumulator == n q
  forced        path 1, fpe = 0 and the reference rounding mode decide nothing in registers
  soundness     no tie passes the register test: accumulator >= ties + carries
  non-vacuity   a sum 2^-20 or 2^-29 of a half unit off a tie (S = 54, 63) is inside the acceptance rule of
                spmv_round_fast: on paths 0 and 2, rounding mode 0, with no term in Y, registers >= the near-ties
Each test prints the counters it saw (pytest -s)."""
import ctypes

import numpy as np
import pytest

import bgemm_cases as B
import exact_cases as X

pytestmark = pytest.mark.gpu

SENTINEL = -12345.678
FPE_PATH0 = ((8, True), (3, True), (0, False))
FPE_ROT = ((0, False), (2, False), (4, True), (8, True), (8, False), (11, True))


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_bgemm_path(0)
    exblas_amd.set_spmm_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _padded(a, pad, fill):
    """a host block as a view [:, :cols] of a wider device block whose padding holds `fill`"""
    import torch
    a = np.asarray(a, dtype=np.float64)
    wide = torch.full((a.shape[0], a.shape[1] + pad), fill, dtype=torch.float64, device="cuda")
    wide[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return wide, wide[:, :a.shape[1]]


def _dev(ex, xb, cb, alpha, beta, y0, fpe=8, ee=True, entry=None, pads=(3, 2, 5)):
    """ExBGEMM with ldx = p + pads[0], ldc = q + pads[1], ldy = q + pads[2]; returns (Y, the counters)"""
    q = np.asarray(cb).shape[1]
    _, xv = _padded(xb, pads[0], np.nan)
    _, cv = _padded(cb, pads[1], np.nan)
    yw, yv = _padded(y0, pads[2], SENTINEL)
    (entry or ex.exbgemm_dev)(xv, cv, alpha, beta, yv, fpe, ee)
    info = ex.last_bgemm_info()
    out = yw.cpu().numpy()
    assert (_bits(out[:, q:]) == _bits(np.array([SENTINEL]))[0]).all(), "the padding of Y was written"
    return np.ascontiguousarray(out[:, :q]), info


def _spmm_form(ex, xb, cb, alpha, beta, y0, itype=np.int64, fpe=8, ee=True):
    """The contract: ExSpMM on the CSR matrix that stores X densely, against C as its dense block"""
    import torch
    xb = np.ascontiguousarray(xb, dtype=np.float64)
    n, p = xb.shape
    crow, col = B.dense_csr(n, p, itype)
    A = (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(xb.reshape(-1)).cuda(), (n, p))
    Y = torch.from_numpy(np.array(y0, dtype=np.float64)).cuda()
    ex.exspmm_dev(A, torch.from_numpy(np.ascontiguousarray(cb, dtype=np.float64)).cuda(), alpha, beta, Y, fpe, ee)
    return Y.cpu().numpy()


def _oracle_ref(oracle, xb, cb, alpha, beta, y0):
    """Output (r, j) under the reference rounding: the oracle's ExGEMV 'N' on the 1 x p row r of X against column j of C"""
    n, p = xb.shape
    out = np.empty((n, cb.shape[1]))
    ct = np.ascontiguousarray(cb.T)
    for r in range(n):
        row = np.ascontiguousarray(xb[r])
        for j in range(cb.shape[1]):
            out[r, j] = oracle.exgemv("N", 1, p, alpha, row, 1, ct[j], beta, np.array([y0[r, j]]), 0,
                                      mode=oracle.ROUND_REFERENCE)[0]
    return out


def _same(got, want, classes, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), sorted(set(np.asarray(classes)[bad].tolist())), np.argwhere(bad)[:4].tolist(),
                           np.asarray(got)[bad][:3], np.asarray(want)[bad][:3])


def _counters(info, classes, path, mode, fpe, near_rule=False):
    """module docstring; `classes` is n x q"""
    assert info[0] + info[1] == classes.size and info[2] == 0 and info[3] == 0, (info, path)
    if path == 1 or fpe == 0 or mode == 1:
        assert info[0] == 0, (info, path, fpe, mode)
    ties = int(((classes == "tie") | (classes == "carry")).sum())
    assert info[1] >= ties, ("a tie was decided in registers", info, ties, path)
    if near_rule and path in (0, 2) and mode == 0 and fpe >= 2:
        near = int(((classes == "tie+1") | (classes == "tie-1")).sum())
        assert info[0] >= near, ("near-ties inside the acceptance rule fell back", info, near, path)
    return tuple(info[:2])


def _sweep(ex, oracle, xb, cs, want, classes, beta, y0, alpha, near_rule, tag, reference=True):
    """One case through the forced paths with alpha = 1, then with alpha (a power of two) and C divided by it --
    cs = fl(alpha * ca) exactly -- through the (fpe, early_exit) variants on path 0 and, with `reference`, the reference
    rounding mode on every path."""
    lib = ex.load_library()
    ca = cs / alpha
    assert (ca[~np.isnan(cs)] * alpha == cs[~np.isnan(cs)]).all()
    seen = {}
    try:
        for path in B.PATHS:
            ex.set_bgemm_path(path)
            got, info = _dev(ex, xb, cs, 1.0, beta, y0)
            seen[path] = _counters(info, classes, path, 0, 8, near_rule)
            _same(got, want, classes, tag + ("path", path))
        ex.set_bgemm_path(0)
        for fpe, ee in FPE_PATH0:
            got, info = _dev(ex, xb, ca, alpha, beta, y0, fpe, ee, pads=(0, 7, 1))
            _counters(info, classes, 0, 0, fpe, near_rule)
            _same(got, want, classes, tag + ("fpe", fpe, ee))
        if reference:
            want_ref = _oracle_ref(oracle, xb, ca, alpha, beta, y0)
            assert not np.isnan(want_ref).any()
            lib.exblas_set_round_mode(1)
            for path in B.PATHS:
                ex.set_bgemm_path(path)
                fpe, ee = FPE_ROT[(path + len(tag)) % len(FPE_ROT)]
                got, info = _dev(ex, xb, ca, alpha, beta, y0, fpe, ee, pads=(1, 0, 2))
                _counters(info, classes, path, 1, fpe)
                _same(got, want_ref, classes, tag + ("reference mode, path", path))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_bgemm_path(0)
    return seen


# ---------------------------------------------------------------------------------------------
# 1. planted classes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index", range(len(B.PLANTED_SHAPES)))
def test_planted_classes(ex, oracle, index):
    """planted_spmm with X = c.g, C = c.x, Y0 = c.y0: every output is a tie, a carry, one unit off a tie or (q >= 16) an
    exact zero or a short value.  Paths 0 .. 3, three (fpe, early_exit) on path 0, alpha a power of two with C divided
    by it, the reference rounding mode against the oracle."""
    rows, q, p = B.PLANTED_SHAPES[index]
    S, layout, (plant, beta) = B.planted_rotation(index)
    c = X.planted_spmm(rows, q, p, S, seed=21 + index, layout=layout, plant=plant, beta=beta)
    cls = c.classes
    assert set(cls.ravel().tolist()) <= {"tie", "carry", "tie+1", "tie-1", "zero", "exact"}
    assert 10 * ((cls == "tie") | (cls == "carry")).sum() >= 3 * cls.size
    assert c.g.shape == (rows, p) and c.x.shape == (p, q)
    near_rule = S in (54, 63) and plant is None
    seen = _sweep(ex, oracle, c.g, c.x, c.want, cls, c.beta, c.y0, B.ALPHAS[1 + index % 3], near_rule,
                  (rows, q, p, S, layout, plant, beta))
    print("\nexbgemm planted", (rows, q, p), S, layout, plant, beta, seen)


# ---------------------------------------------------------------------------------------------
# 2. products with a non-zero TwoProd error term
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0, -0.75])
@pytest.mark.parametrize("inner", [8, 19])
@pytest.mark.parametrize("outputs", [15, 70])
def test_inexact_products(ex, oracle, outputs, inner, beta):
    """planted_inexact: the class of a row depends on TwoProd error terms, with beta = -3/4 on that of beta * y as well.
    C is the column c.x repeated q times, column j (and y) scaled by 2^e_j, |e_j| <= 20: exact scalings."""
    rng = np.random.default_rng([outputs, inner, 5])
    report = {}
    for si, S in enumerate((54, 63)):
        c = X.planted_inexact(outputs, inner, S, seed=31, layout=X.LAYOUTS[(si + inner + outputs) % 3], beta=beta)
        for q in (1, 3, 20):
            scale = np.ldexp(1.0, rng.integers(-20, 21, q))
            cs = c.x[:, None] * scale[None, :]
            want = c.want[:, None] * scale[None, :]
            y0 = c.y0[:, None] * scale[None, :] if beta else np.full((outputs, q), np.nan)
            assert np.isfinite(want).all() and (np.abs(want) > 2.0 ** -900).all()
            classes = np.repeat(c.classes[:, None], q, axis=1)
            report[S, q] = _sweep(ex, oracle, c.g, cs, want, classes, c.beta, y0, B.ALPHAS[1 + (si + q) % 3], False,
                                  ("inexact", outputs, inner, S, beta, q), reference=False)
    print("\nexbgemm inexact", outputs, inner, beta, report)


# ---------------------------------------------------------------------------------------------
# 3. bit identity with ExSpMM on the densified CSR, and with ExGEMM
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
def test_bit_identity_with_exspmm_on_the_dense_csr(ex, part):
    """Random 53-bit mantissas over 2^-200 .. 2^200 in X, C and Y; a covering subset of the sizes (bgemm_cases.py), both
    index widths, both (alpha, beta) pairs, every path."""
    shapes = B.identity_shapes()[part::4]
    try:
        for si, (n, q, p) in enumerate(shapes):
            rng = np.random.default_rng([n, q, p])
            xb, cb, y0 = B.wide_block(rng, n, p), B.wide_block(rng, p, q), B.wide_block(rng, n, q)
            for ai, (alpha, beta) in enumerate(((0.3, 0.7), (-1.0, 1.0))):
                want = _spmm_form(ex, xb, cb, alpha, beta, y0, (np.int32, np.int64)[(si + ai + part) % 2])
                for path in B.PATHS:
                    ex.set_bgemm_path(path)
                    got, info = _dev(ex, xb, cb, alpha, beta, y0)
                    assert info[0] + info[1] == n * q and (path != 1 or info[0] == 0), (info, n, q, p, path)
                    bad = np.argwhere(_bits(got) != _bits(want))
                    assert bad.size == 0, ((n, q, p), alpha, beta, path, len(bad), bad[:5].tolist())
    finally:
        ex.set_bgemm_path(0)


@pytest.mark.parametrize("n,q,p", [(257, 33, 63), (65, 8, 129), (1031, 64, 5)])
def test_bit_identity_with_exgemm_where_the_contracts_meet(ex, n, q, p):
    """alpha = 1, beta = 0: ExGEMM's Round(sum) is ExBGEMM's value"""
    import torch
    rng = np.random.default_rng([n, q, p, 1])
    xb, cb = B.wide_block(rng, n, p), B.wide_block(rng, p, q)
    out = torch.full((n * q,), np.nan, dtype=torch.float64, device="cuda")
    ex.exgemm_dev("N", "N", n, q, p, 1.0, torch.from_numpy(xb.reshape(-1)).cuda(), p, torch.from_numpy(cb.reshape(-1)).cuda(),
                  q, 0.0, out, q, 8, True)
    want = out.cpu().numpy().reshape(n, q)
    assert (_bits(_spmm_form(ex, xb, cb, 1.0, 0.0, np.full((n, q), np.nan))) == _bits(want)).all()
    got, _ = _dev(ex, xb, cb, 1.0, 0.0, np.full((n, q), np.nan))
    assert (_bits(got) == _bits(want)).all()


# ---------------------------------------------------------------------------------------------
# 4. non-finite entries stay in their row and column
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,q,p", [(70, 9, 12), (37, 65, 70)])
@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_entries_stay_in_their_row_and_column(ex, value, n, q, p):
    rng = np.random.default_rng([n, q, p, 7])
    xb = rng.integers(-8, 9, (n, p)).astype(np.float64) + 0.5       # no zeros but the planted one
    cb = rng.integers(-8, 9, (p, q)).astype(np.float64) + 0.25
    y0 = rng.integers(-8, 9, (n, q)).astype(np.float64)
    r0, i0, i1, j0, r1 = n - 3, 2, p - 2, q - 2, 5
    xn, cn = xb.copy(), cb.copy()
    xn[r0, i0] = value                    # one row of X
    cn[i1, j0] = value                    # one column of C ...
    xn[r1, i1] = 0.0                      # ... and a zero in X against it
    try:
        for path in B.PATHS:
            ex.set_bgemm_path(path)
            for alpha, beta in ((1.0, 0.0), (0.3, 0.7)):
                clean, _ = _dev(ex, xb, cb, alpha, beta, y0)
                got, info = _dev(ex, xn, cn, alpha, beta, y0)
                assert info[0] + info[1] == n * q
                want = _spmm_form(ex, xn, cn, alpha, beta, y0)
                assert (_bits(got) == _bits(want)).all(), (value, path, alpha, beta)
                assert not np.isfinite(got[r0]).any() and not np.isfinite(got[:, j0]).any()
                assert np.isnan(got[r1, j0])                               # 0 * Inf, or NaN itself
                keep = np.ones((n, q), dtype=bool)
                keep[r0, :] = False
                keep[:, j0] = False
                keep[r1, :] = False                                        # (its X differs by the planted zero)
                assert (_bits(got)[keep] == _bits(clean)[keep]).all(), (value, path, alpha, beta)
                assert np.isfinite(got[r1, np.arange(q) != j0]).all()
    finally:
        ex.set_bgemm_path(0)


# ---------------------------------------------------------------------------------------------
# 5. results at the ends of the double range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [12, 70])
def test_result_range_rows(ex, oracle, inner):
    """range_rows_gemv's rows as X against its x as a one-column C and as five equal columns: subnormal sums, the
    smallest normal, DBL_MAX, the tie at the overflow threshold, huge products that cancel; beta in {0, 1}."""
    r = X.range_rows_gemv(inner)
    nr = len(r.names)
    for q in (1, 5):
        cs = np.repeat(r.x[:, None], q, axis=1)
        none = np.full((nr, q), "other", dtype=object)
        for beta, want in ((0.0, r.want), (1.0, r.want_with_y)):
            y0 = np.repeat(r.y0[:, None], q, axis=1) if beta else np.full((nr, q), np.nan)
            _sweep(ex, oracle, r.g, cs, np.repeat(want[:, None], q, axis=1), none, beta, y0, 1.0, False,
                   ("range", inner, q, beta))


# ---------------------------------------------------------------------------------------------
# 6. layout and empty sizes
# ---------------------------------------------------------------------------------------------
def test_beta_zero_ignores_a_y_full_of_nan(ex):
    rng = np.random.default_rng(8)
    n, q, p = 131, 7, 10
    xb, cb = rng.integers(-99, 100, (n, p)).astype(np.float64), rng.integers(-99, 100, (p, q)).astype(np.float64)
    try:
        for path in B.PATHS:
            ex.set_bgemm_path(path)
            got, _ = _dev(ex, xb, cb, 2.0, 0.0, np.full((n, q), np.nan), pads=(9, 1, 60))
            assert (_bits(got) == _bits(2.0 * (xb @ cb))).all(), path        # small integers: the product is exact
    finally:
        ex.set_bgemm_path(0)


def test_empty_sizes_launch_nothing_and_p_zero_rounds_beta_y(ex):
    import torch
    rng = np.random.default_rng(9)
    dev = dict(dtype=torch.float64, device="cuda")
    y4 = rng.integers(-50, 51, (77, 6)).astype(np.float64) * 4.0
    try:
        for path in B.PATHS:
            ex.set_bgemm_path(path)
            # p == 0: Round(0 (+) beta Y); 0.7 y is one rounded product, and an exact zero is +0.0 whatever the sign of beta
            for beta, want in ((1.0, y4), (-0.75, -0.75 * y4), (0.7, 0.7 * y4), (0.0, np.zeros_like(y4))):
                want = np.where(want == 0, 0.0, want)
                got, info = _dev(ex, np.zeros((77, 0)), np.zeros((0, 6)), 3.0, beta, y4 if beta else np.full_like(y4, np.nan))
                assert (_bits(got) == _bits(want)).all(), (path, beta)
                assert info[0] + info[1] == 77 * 6
                if path == 0:
                    assert (_bits(_spmm_form(ex, np.zeros((77, 0)), np.zeros((0, 6)), 3.0, beta, y4)) == _bits(want)).all()
            # n == 0 and q == 0 after a call that counted: nothing is launched, the counters read zero
            for shape in ((0, 5, 6), (9, 5, 0), (0, 0, 0)):
                ex.exbgemm_dev(torch.ones(4, 3, **dev), torch.ones(3, 2, **dev))
                assert sum(ex.last_bgemm_info()) == 8
                n, p, q = shape
                y = torch.full((n, q + 2), SENTINEL, **dev)
                out = ex.exbgemm_dev(torch.ones(n, p, **dev), torch.ones(p, q, **dev), 1.0, 1.0, y[:, :q])
                assert tuple(out.shape) == (n, q) and ex.last_bgemm_info() == (0, 0, 0, 0), (shape, path)
                assert (y.cpu().numpy() == SENTINEL).all()
    finally:
        ex.set_bgemm_path(0)
    # the C entry: argument errors
    lib = ex.load_library()
    x, c, y = torch.ones(4, 3, **dev), torch.ones(3, 2, **dev), torch.ones(4, 2, **dev)
    px, pc, py = (ctypes.c_void_p(t.data_ptr()) for t in (x, c, y))
    ok = dict(n=4, p=3, q=2, ldx=3, ldc=2, ldy=2, fpe=8)
    for change in (dict(n=-1), dict(p=-1), dict(q=-1), dict(n=2 ** 31), dict(ldx=2), dict(ldc=1), dict(ldy=1), dict(fpe=-1)):
        a = dict(ok, **change)
        rc = lib.exblas_exbgemm_dev(a["n"], a["p"], a["q"], 1.0, px, a["ldx"], pc, a["ldc"], 0.0, py, a["ldy"], a["fpe"], 1, None)
        assert rc == 1, (change, rc)                                        # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert (y.cpu().numpy() == 1.0).all()


# ---------------------------------------------------------------------------------------------
# 7. plumbing
# ---------------------------------------------------------------------------------------------
def _small_case(index=1):
    rows, q, p = B.PLANTED_SHAPES[index]
    S, layout, (plant, beta) = B.planted_rotation(index)
    return X.planted_spmm(rows, q, p, S, seed=21 + index, layout=layout, plant=plant, beta=beta)


def test_contexts_streams_and_host_arrays_agree(ex):
    import torch
    c = _small_case(2)
    first, info = _dev(ex, c.g, c.x, 1.0, c.beta, c.y0)
    _same(first, c.want, c.classes, "device entry")
    ctx, side = ex.Context(), torch.cuda.Stream()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got, info2 = _dev(ex, c.g, c.x, 1.0, c.beta, c.y0, entry=ctx.exbgemm)
        side.synchronize()
        assert (_bits(got) == _bits(first)).all() and info2 == info
        assert ctx.workspace_bytes() >= 16
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
    keep = c.y0.copy()
    host = ex.exbgemm(c.g, c.x, 1.0, c.beta, c.y0)
    assert host is not c.y0 and (_bits(c.y0) == _bits(keep)).all()
    assert (_bits(host) == _bits(first)).all()
    # the C host entry with ldy > q: the padding comes back as it went
    rows, q = c.want.shape
    wide = np.full((rows, q + 3), -7.25)
    wide[:, :q] = c.y0
    g, xs = np.ascontiguousarray(c.g), np.ascontiguousarray(c.x)
    rc = ex.load_library().exblas_exbgemm(rows, g.shape[1], q, 1.0, ctypes.c_void_p(g.ctypes.data), g.shape[1],
                                          ctypes.c_void_p(xs.ctypes.data), q, c.beta, ctypes.c_void_p(wide.ctypes.data), q + 3,
                                          8, 1)
    assert rc == 0 and (_bits(wide[:, :q]) == _bits(first)).all() and (wide[:, q:] == -7.25).all()


def test_graph_capture_after_one_warm_call(ex):
    """One warm call, then a capture replayed twice on new data, the counters read after each replay.  The captured work
    is a single kernel node: a chain with no parallel branches, and no memset node."""
    import torch
    cases = (_small_case(1), _small_case(1))
    rows, q = cases[0].want.shape
    flipped = (cases[1].g[::-1].copy(), cases[1].y0[::-1].copy(), cases[1].want[::-1].copy())
    data = ((cases[0].g, cases[0].y0, cases[0].want), flipped)
    beta = cases[0].beta
    xd = torch.zeros(rows, cases[0].g.shape[1], dtype=torch.float64, device="cuda")
    cd = torch.from_numpy(np.ascontiguousarray(cases[0].x)).cuda()
    yd = torch.zeros(rows, q, dtype=torch.float64, device="cuda")
    ex.exbgemm_dev(xd, cd, 1.0, beta, yd)                                  # the warm call
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exbgemm_dev(xd, cd, 1.0, beta, yd)
    for gx, gy, want in data:
        xd.copy_(torch.from_numpy(np.ascontiguousarray(gx)))
        yd.copy_(torch.from_numpy(np.ascontiguousarray(gy)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (_bits(yd.cpu().numpy()) == _bits(want)).all()
        info = ex.last_bgemm_info()
        assert info[0] + info[1] == rows * q
    del g


def test_workspace_growth_during_capture_is_refused(ex):
    """a context that has no workspace yet must not allocate one under a capture: reserve, or call once, first"""
    import torch
    ctx = ex.Context()
    try:
        assert ctx.workspace_bytes() == 0
        x = torch.ones(8, 4, dtype=torch.float64, device="cuda")
        c = torch.ones(4, 3, dtype=torch.float64, device="cuda")
        y = torch.zeros(8, 3, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError):
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    ctx.exbgemm(x, c, 1.0, 0.0, y)
        torch.cuda.synchronize()
        assert ctx.workspace_bytes() == 0
        assert ex.load_library().exblas_reserve_workspace_ctx(ctx.handle, 256) == 0
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.stream(s):
            with torch.cuda.graph(g2, stream=s):
                ctx.exbgemm(x, c, 1.0, 0.0, y)
        g2.replay()
        torch.cuda.synchronize()
        assert (y.cpu().numpy() == 4.0).all()
        del g2
    finally:
        torch.cuda.synchronize()
        ctx.destroy()


def test_plain_product_is_close_and_deterministic(ex):
    """fpe == 1: plain fp64 sums in the order of i.  |got - exact| <= (p + 2) u (|alpha X| |C| + |beta Y|) + u |want|: p
    products and additions, alpha folded into C, the beta term; the reference is the exact result rounded."""
    rng = np.random.default_rng(10)
    n, q, p = 300, 20, 33
    xb, cb, y0 = rng.standard_normal((n, p)), rng.standard_normal((p, q)), rng.standard_normal((n, q))
    want = _spmm_form(ex, xb, cb, 0.3, 0.7, y0)
    got, info = _dev(ex, xb, cb, 0.3, 0.7, y0, 1, False)
    again, _ = _dev(ex, xb, cb, 0.3, 0.7, y0, 1, False)
    assert info == (0, 0, 0, 0) and (_bits(got) == _bits(again)).all()
    u = 2.0 ** -53
    bound = (p + 2) * u * (np.abs(0.3 * xb) @ np.abs(cb) + np.abs(0.7 * y0)) + u * np.abs(want)
    assert (np.abs(got - want) <= bound).all()
