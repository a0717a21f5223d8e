"""GPU tests of ExSpMM: bit-exact against the per-output ExGEMV oracle and against the ExSpMV column loop; invariance,
capture, contexts, full size.  Every comparison is on the bits; the only tolerance is the derived one of fpe == 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = [("fpuniform", 10, 0), ("fpuniform_signed", 60, 30), ("lognormal", 0.0, 50.0), ("ill_cond", 1e32, 0),
         ("cancel", 0, 0)]
AB = [(1.0, 0.0), (1.0, 1.0), (-0.7, 3.3), (2.0 ** -3, 0.0)]
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_spmm_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _random_csr(rng, m, n, lengths, itype=np.int64, p=None):
    lens = rng.choice(lengths, size=m, p=p)
    crow = np.zeros(m + 1, dtype=np.int64)
    crow[1:] = np.cumsum(lens)
    col = rng.integers(0, max(n, 1), size=int(crow[-1])) if n > 0 else np.zeros(int(crow[-1]), dtype=np.int64)
    return crow.astype(itype), col.astype(itype)


def _oracle_outputs(oracle, crow, col, val, X, alpha, beta, Y0, rows=None, cols=None, mode=0):
    """Output (i, j) = oracle.exgemv('N') on the 1 x len_i matrix of row i's values against the gathered X[:, j]."""
    out = np.array(Y0, dtype=np.float64, copy=True)
    rows = range(len(crow) - 1) if rows is None else rows
    cols = range(X.shape[1]) if cols is None else cols
    Xt = np.ascontiguousarray(X.T)
    for i in rows:
        a, b = int(crow[i]), int(crow[i + 1])
        for j in cols:
            if b <= a:
                v, xs = np.zeros(1), np.zeros(1)
            else:
                v, xs = val[a:b], Xt[j, col[a:b]]
            y0 = np.array([Y0[i, j]])
            out[i, j] = oracle.exgemv("N", 1, len(v), alpha, v, 1, xs, beta, y0, 0, mode=mode)[0]
    return out


def _cuda_csr(crow, col, val, m, n):
    import torch
    return (torch.from_numpy(np.asarray(crow)).cuda(), torch.from_numpy(np.asarray(col)).cuda(),
            torch.from_numpy(np.asarray(val)).cuda(), (m, n))


def _dev(ex, crow, col, val, X, m, n, alpha, beta, Y0, fpe=8, ee=True, ctx=None, xpad=3, ypad=5):
    """ExSpMM with ldx = k + xpad and ldy = k + ypad; the padding of Y holds a sentinel whose bits must survive."""
    import torch
    X = np.asarray(X)
    k = X.shape[1]
    A = _cuda_csr(crow, col, val, m, n)
    Xb = torch.full((X.shape[0], k + xpad), SENTINEL, dtype=torch.float64, device="cuda")
    Xb[:, :k] = torch.from_numpy(X).cuda()
    Yb = torch.full((m, k + ypad), SENTINEL, dtype=torch.float64, device="cuda")
    Yb[:, :k] = torch.from_numpy(np.array(Y0, dtype=np.float64)).cuda()
    f = ctx.exspmm if ctx is not None else ex.exspmm_dev
    f(A, Xb[:, :k], alpha, beta, Yb[:, :k], fpe, ee)
    out = Yb.cpu().numpy()
    assert (_bits(out[:, k:]) == _bits(np.array([SENTINEL]))[0]).all(), "the padding of Y was written"
    return np.ascontiguousarray(out[:, :k])


def _gen(oracle, kind, p0, p1, count, seed):
    return oracle.gen(kind, max(count, 1), seed, p0, p1)[:count].copy()


def _assert_bits(got, want, what, rows=None):
    g, w = _bits(got), _bits(want)
    if rows is not None:
        g, w = g[rows], w[rows]
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


# kind index -> the k values it is run with; a kind with two k values splits the four (alpha, beta) pairs between them
K_OF_KIND = [(1, 64), (2, 65), (3, 130), (8,), (17,)]


@pytest.mark.parametrize("mode", [0, 1])
def test_random_csr_vs_oracle(ex, oracle, mode):
    lib = ex.load_library()
    rng = np.random.default_rng(1 + mode)
    lengths = [0, 1, 2, 31, 63, 64, 65, 1000]
    try:
        lib.exblas_set_round_mode(mode)
        for t, (kind, p0, p1) in enumerate(KINDS):
            for s, k in enumerate(K_OF_KIND[t]):
                m, n = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
                m = max(1, min(m, 40000 // k))   # the oracle is called once per output
                crow, col = _random_csr(rng, m, n, lengths)
                if t == 0 and s == 0:   # one row of 70 000 entries (split across workgroups)
                    lens = np.diff(crow)
                    lens[m // 2] = 70000
                    crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                    col = rng.integers(0, n, size=int(crow[-1]))
                nnz = int(crow[-1])
                val = _gen(oracle, kind, p0, p1, nnz, 11 + t)
                X = _gen(oracle, kind, p0, p1, n * k, 12 + t).reshape(n, k)
                Y0 = _gen(oracle, kind, p0, p1, m * k, 13 + t).reshape(m, k)
                pairs = AB if len(K_OF_KIND[t]) == 1 else AB[2 * s:2 * s + 2]
                for alpha, beta in pairs:
                    want = _oracle_outputs(oracle, crow, col, val, X, alpha, beta, Y0, mode=mode)
                    got = _dev(ex, crow, col, val, X, m, n, alpha, beta, Y0)
                    _assert_bits(got, want, (kind, k, alpha, beta, mode))
    finally:
        lib.exblas_set_round_mode(0)


@pytest.mark.parametrize("itype", [np.int32, np.int64])
def test_against_the_exspmv_column_loop(ex, oracle, itype):
    import torch
    rng = np.random.default_rng(2)
    m, n, k = 20011, 19997, 48
    crow, col = _random_csr(rng, m, n, [0, 1, 2, 27, 63, 64, 65, 700, 20000], itype,
                            p=[0.1, 0.1, 0.1, 0.3, 0.1, 0.1, 0.1, 0.099, 0.001])
    nnz = int(crow[-1])
    assert np.diff(crow).max() == 20000
    val = _gen(oracle, "fpuniform_signed", 60, 30, nnz, 21)
    X = torch.from_numpy(_gen(oracle, "fpuniform_signed", 60, 30, n * k, 22).reshape(n, k)).cuda()
    Y0 = torch.from_numpy(_gen(oracle, "fpuniform_signed", 60, 30, m * k, 23).reshape(m, k)).cuda()
    A = _cuda_csr(crow, col, val, m, n)
    for alpha, beta in ((1.0, 0.0), (-0.7, 3.3)):
        got = ex.exspmm_dev(A, X, alpha, beta, Y0.clone()).cpu().numpy()
        want = np.empty((m, k))
        for j in range(k):
            want[:, j] = ex.exspmv_dev(A, X[:, j].contiguous(), alpha, beta, Y0[:, j].clone()).cpu().numpy()
        _assert_bits(got, want, (itype.__name__, alpha, beta))


def test_random_csr_vs_mpfr(ex, oracle):
    if oracle.mpfr() is None:
        pytest.skip("MPFR oracle not built")
    rng = np.random.default_rng(7)
    m, n, k = 300, 400, 5
    crow, col = _random_csr(rng, m, n, [1, 2, 31, 64, 65, 300])
    val = _gen(oracle, "fpuniform_signed", 60, 30, int(crow[-1]), 21)
    X = _gen(oracle, "fpuniform_signed", 60, 30, n * k, 22).reshape(n, k)
    Y0 = _gen(oracle, "fpuniform_signed", 60, 30, m * k, 23).reshape(m, k)
    got = _dev(ex, crow, col, val, X, m, n, 1.0, 1.0, Y0)
    for i in range(m):
        a, b = int(crow[i]), int(crow[i + 1])
        for j in range(k):
            xs = np.ascontiguousarray(X[col[a:b], j])
            want = oracle.mpfr_exgemv("N", 1, b - a, 1.0, val[a:b], 1, xs, 1.0, np.array([Y0[i, j]]))[0]
            assert _bits(got[i, j:j + 1])[0] == _bits(np.array([want]))[0], (i, j)


def _edge_rows():
    """(values, x) rows built on the fast path's boundaries (those of the ExSpMV test)."""
    ulp1 = 2.0 ** -52
    rows = []
    # exact sums halfway between two doubles: 1 + ulp/2 (tie to even -> 1), 1 + 3ulp/2 (tie -> 1 + 2ulp)
    rows.append(([1.0, ulp1 / 2], [1.0, 1.0]))
    rows.append(([1.0 + ulp1, ulp1 / 2], [1.0, 1.0]))
    # halfway +- 2^-1074
    rows.append(([1.0, ulp1 / 2, 2.0 ** -1074], [1.0, 1.0, 1.0]))
    rows.append(([1.0, ulp1 / 2, -(2.0 ** -1074)], [1.0, 1.0, 1.0]))
    # just below / above a power of two
    rows.append(([2.0, -(2.0 ** -60)], [1.0, 1.0]))
    rows.append(([2.0, 2.0 ** -60], [1.0, 1.0]))
    rows.append(([1.0, 1.0, -(2.0 ** -54), 2.0 ** -110], [1.0, 1.0, 1.0, 1.0]))
    # total cancellation
    rows.append(([1e300, 3.0, -1e300, -3.0], [1.0, 1.0, 1.0, 1.0]))
    rows.append(([0.1, 0.2, -0.3], [3.0, 3.0, 3.0]))
    # subnormal results
    rows.append(([2.0 ** -1070, -(2.0 ** -1071)], [1.0, 1.0]))
    rows.append(([1e-300, 1.0], [1e-10, 1e-300]))
    # round to +-inf
    rows.append(([1.7e308, 1.7e308], [1.0, 1.0]))
    rows.append(([-1.7e308, -1.7e308], [1.0, 1.0]))
    rows.append(([1e200], [1e200]))
    # NaN and Inf entries
    rows.append(([1.0, np.inf], [1.0, 1.0]))
    rows.append(([1.0, np.inf, -np.inf], [1.0, 1.0, 1.0]))
    rows.append(([np.nan, 1.0], [1.0, 1.0]))
    rows.append(([0.0, 1.0], [np.inf, 1.0]))
    return rows


@pytest.mark.parametrize("mode", [0, 1])
def test_rounding_edge_rows(ex, oracle, mode):
    import torch
    lib = ex.load_library()
    rows = _edge_rows()
    val, xs, crow = [], [], [0]
    for v, x in rows:
        val += v
        xs += x
        crow.append(len(val))
    n = len(xs)
    crow, col = np.array(crow, dtype=np.int64), np.arange(n, dtype=np.int64)
    val, x = np.array(val), np.array(xs)
    m = len(rows)
    # column 0 is the ExSpMV edge test; x times 8 and x times -1 are exact: ties stay ties, signs flip
    with np.errstate(over="ignore", invalid="ignore"):
        X = np.stack([x, x * 8.0, x * -1.0], axis=1)
        k = X.shape[1]
        Y0 = np.zeros((m, k))
        finite = [(i, j) for i in range(m) for j in range(k)
                  if np.isfinite(val[crow[i]:crow[i + 1]] * X[crow[i]:crow[i + 1], j]).all()]
    assert (0, 1) in finite and (11, 1) not in finite   # 1.7e308 * 8 overflows: joins the non-finite set
    try:
        lib.exblas_set_round_mode(mode)
        got = _dev(ex, crow, col, val, X, m, n, 1.0, 0.0, Y0)
        info = ex.last_spmm_info()   # (before the ExGEMV calls below reuse the workspace)
        for i in range(m):
            v = val[crow[i]:crow[i + 1]]
            for j in range(k):
                xj = np.ascontiguousarray(X[crow[i]:crow[i + 1], j])
                if (i, j) in finite:
                    want = oracle.exgemv("N", 1, len(v), 1.0, v, 1, xj, 0.0, np.zeros(1), 0, mode=mode)[0]
                else:
                    # non-finite products: the oracle's exgemv drops them, the library's ExGEMV follows IEEE (DESIGN
                    # section 3); ExSpMM is what GPU ExGEMV 'N' computes for the row as a 1 x len matrix
                    Y = torch.zeros(1, dtype=torch.float64, device="cuda")
                    ex.exgemv_dev("N", 1, len(v), 1.0, torch.from_numpy(v.copy()).cuda(), 1,
                                  torch.from_numpy(xj).cuda(), 0.0, Y, 8, True)
                    want = Y.cpu().numpy()[0]
                assert _bits(got[i, j:j + 1])[0] == _bits(np.array([want]))[0], (i, j, got[i, j], want)
        if mode == 0:
            # ties, near-ties, subnormal, infinite and non-finite outputs cannot be certified in registers
            assert info[1] >= 12 * k and info[0] + info[1] == m * k, info
    finally:
        lib.exblas_set_round_mode(0)
    if mode == 0:   # ties to even
        assert got[0, 0] == 1.0 and got[1, 0] == 1.0 + 2 * 2.0 ** -52
        assert got[0, 1] == 8.0 and got[0, 2] == -1.0 and got[1, 2] == -(1.0 + 2 * 2.0 ** -52)
    assert np.isnan(got[-3]).all() and np.isnan(got[-2]).all()
    assert got[-4, 0] == np.inf and got[-4, 2] == -np.inf and got[-6, 0] == -np.inf and got[-6, 2] == np.inf


def _stencil(k):
    """27-point stencil on a k^3 grid, int64 CSR."""
    idx = np.arange(k ** 3).reshape(k, k, k)
    cols = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                sh = np.full((k, k, k), -1, dtype=np.int64)
                src = idx[max(0, dz):k + min(0, dz), max(0, dy):k + min(0, dy), max(0, dx):k + min(0, dx)]
                sh[max(0, -dz):k - max(0, dz), max(0, -dy):k - max(0, dy), max(0, -dx):k - max(0, dx)] = src
                cols.append(sh.reshape(-1))
    c = np.stack(cols, axis=1)
    mask = c >= 0
    crow = np.zeros(k ** 3 + 1, dtype=np.int64)
    crow[1:] = np.cumsum(mask.sum(axis=1))
    return crow, c[mask]


def _invariance_case(oracle, rng):
    m, n, k = 600, 500, 70
    crow, col = _random_csr(rng, m, n, [0, 1, 2, 27, 63, 64, 65, 700, 5000])
    val = _gen(oracle, "lognormal", 0.0, 50.0, int(crow[-1]), 51)
    X = _gen(oracle, "lognormal", 0.0, 50.0, n * k, 52).reshape(n, k)
    Y0 = _gen(oracle, "lognormal", 0.0, 50.0, m * k, 53).reshape(m, k)
    return m, n, k, crow, col, val, X, Y0


def test_invariance_paths_fpe_width(ex, oracle):
    rng = np.random.default_rng(9)
    m, n, k, crow, col, val, X, Y0 = _invariance_case(oracle, rng)
    ref = _dev(ex, crow, col, val, X, m, n, -0.7, 3.3, Y0)
    # a second, tame data set so that path 2 / path 0 really round in registers somewhere
    val_t = _gen(oracle, "fpuniform", 10, 0, len(val), 54)
    X_t = _gen(oracle, "fpuniform", 10, 0, n * k, 55).reshape(n, k)
    ref_t = _dev(ex, crow, col, val_t, X_t, m, n, 1.0, 0.0, Y0)
    assert ex.last_spmm_info()[0] > 0
    try:
        for path in (0, 1, 2, 3):
            ex.set_spmm_path(path)
            got = _dev(ex, crow, col, val, X, m, n, -0.7, 3.3, Y0)
            info = ex.last_spmm_info()
            _assert_bits(got, ref, ("path", path))
            if path == 1:   # (the outputs of split rows are rounded from their global accumulators: not in info[1])
                assert info[0] == 0 and info[1] + info[2] * k == m * k, info
            if path == 2:
                assert info[2] == 0, info
            if path == 3:
                assert info[2] == m, info
            _assert_bits(_dev(ex, crow, col, val_t, X_t, m, n, 1.0, 0.0, Y0), ref_t, ("tame, path", path))
    finally:
        ex.set_spmm_path(0)
    for fpe in (0, 2, 4, 8):
        for ee in (False, True):
            _assert_bits(_dev(ex, crow, col, val, X, m, n, -0.7, 3.3, Y0, fpe, ee), ref, (fpe, ee))
            _assert_bits(_dev(ex, crow, col, val_t, X_t, m, n, 1.0, 0.0, Y0, fpe, ee), ref_t, ("tame", fpe, ee))
    got = _dev(ex, crow.astype(np.int32), col.astype(np.int32), val, X, m, n, -0.7, 3.3, Y0)
    _assert_bits(got, ref, "int32")
    # other leading dimensions (none: ldx = ldy = k)
    _assert_bits(_dev(ex, crow, col, val, X, m, n, -0.7, 3.3, Y0, xpad=0, ypad=0), ref, "ld = k")
    _assert_bits(_dev(ex, crow, col, val, X, m, n, -0.7, 3.3, Y0, xpad=58, ypad=1), ref, "ld = k + 58 / k + 1")


def test_invariance_orderings_and_column_tiling(ex, oracle):
    rng = np.random.default_rng(10)
    m, n, k, crow, col, val, X, Y0 = _invariance_case(oracle, rng)
    ref = _dev(ex, crow, col, val, X, m, n, -0.7, 3.3, Y0)
    # entries shuffled within rows
    col2, val2 = col.copy(), val.copy()
    for i in range(m):
        a, b = int(crow[i]), int(crow[i + 1])
        p = rng.permutation(b - a) + a
        col2[a:b], val2[a:b] = col[p], val[p]
    _assert_bits(_dev(ex, crow, col2, val2, X, m, n, -0.7, 3.3, Y0), ref, "entries shuffled")
    # permuted rows
    perm = rng.permutation(m)
    lens = np.diff(crow)[perm]
    crow3 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col3 = np.concatenate([col[crow[i]:crow[i + 1]] for i in perm])
    val3 = np.concatenate([val[crow[i]:crow[i + 1]] for i in perm])
    _assert_bits(_dev(ex, crow3, col3, val3, X, m, n, -0.7, 3.3, Y0[perm]), ref[perm], "rows permuted")
    # permuted columns of X: the columns of Y permute with them
    cp = rng.permutation(k)
    _assert_bits(_dev(ex, crow, col, val, X[:, cp], m, n, -0.7, 3.3, Y0[:, cp]), ref[:, cp], "columns permuted")
    # the first k1 columns do not depend on how many columns follow (both sides of every tile boundary)
    for k1 in (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65):
        got = _dev(ex, crow, col, val, X[:, :k1], m, n, -0.7, 3.3, Y0[:, :k1])
        _assert_bits(got, ref[:, :k1], ("k1", k1))


def test_out_of_range_column_gives_nan_rows(ex, oracle):
    import torch
    rng = np.random.default_rng(3)
    m, n, k = 200, 100, 6
    crow, col = _random_csr(rng, m, n, [1, 5, 40, 100, 6000])
    val = _gen(oracle, "fpuniform", 10, 0, int(crow[-1]), 61)
    Xfull = _gen(oracle, "fpuniform", 10, 0, (n + 64) * k, 62).reshape(n + 64, k)   # 64 rows more than the call's n
    bad_rows = [3, 77, int(np.argmax(np.diff(crow)))]
    col = col.copy()
    for r in bad_rows:
        col[int(crow[r])] = -1 if r == 77 else n + 5
    good = [i for i in range(m) if i not in bad_rows]
    want = _oracle_outputs(oracle, crow, col, val, Xfull[:n], 1.0, 0.0, np.zeros((m, k)), rows=good)
    A = _cuda_csr(crow, col, val, m, n)
    X = torch.from_numpy(Xfull).cuda()
    for path in (0, 1, 3):
        ex.set_spmm_path(path)
        try:
            for fpe in (8, 1):
                y = ex.exspmm_dev(A, X, 1.0, 0.0, None, fpe).cpu().numpy()
                assert np.isnan(y[bad_rows]).all(), (path, fpe)
                if fpe == 8:
                    _assert_bits(y, want, (path, fpe), rows=good)
                else:
                    assert not np.isnan(y[good]).any()
        finally:
            ex.set_spmm_path(0)


def test_graph_capture(ex, oracle):
    import torch
    rng = np.random.default_rng(4)
    m, n, k = 2000, 1800, 12
    crow, col = _random_csr(rng, m, n, [3, 27, 60])
    nnz = int(crow[-1])
    val = _gen(oracle, "fpuniform", 10, 0, nnz, 71)
    Crow, Col, Val = (torch.from_numpy(a).cuda() for a in (crow, col, val))
    X = torch.from_numpy(_gen(oracle, "fpuniform", 10, 0, n * k, 72).reshape(n, k)).cuda()
    Y = torch.zeros((m, k), dtype=torch.float64, device="cuda")
    A = (Crow, Col, Val, (m, n))
    ex.exspmm_dev(A, X, 1.0, 0.0, Y)   # warm-up: sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exspmm_dev(A, X, 1.0, 0.0, Y)
    # new X, then a matrix of the same shape and nnz whose rows change class (one long row, many medium and empty)
    lens = np.zeros(m, dtype=np.int64)
    lens[5] = nnz - 90 * 100
    lens[100:190] = 100
    crow2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col2 = rng.integers(0, n, size=nnz)
    for step, (cr, co) in enumerate(((crow, col), (crow2, col2))):
        X.copy_(torch.from_numpy(_gen(oracle, "lognormal", 0.0, 5.0, n * k, 80 + step).reshape(n, k)))
        Crow.copy_(torch.from_numpy(cr))
        Col.copy_(torch.from_numpy(co))
        Y.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        eager = ex.exspmm_dev(A, X, 1.0, 0.0).cpu().numpy()
        _assert_bits(Y.cpu().numpy(), eager, ("replay", step))
        if step == 1:
            assert ex.last_spmm_info()[2] == 1
        want = _oracle_outputs(oracle, cr, co, val, X.cpu().numpy(), 1.0, 0.0, np.zeros((m, k)))
        _assert_bits(eager, want, ("oracle", step))
    del g


def test_contexts_streams_and_host_entry(ex, oracle):
    import torch
    rng = np.random.default_rng(6)
    m, n, k = 1000, 900, 9
    crow, col = _random_csr(rng, m, n, [0, 5, 30, 70, 500, 17000])
    val = _gen(oracle, "ill_cond", 1e32, 0, int(crow[-1]), 91)
    X = _gen(oracle, "ill_cond", 1e32, 0, n * k, 92).reshape(n, k)
    Y0 = _gen(oracle, "ill_cond", 1e32, 0, m * k, 93).reshape(m, k)
    ref = _dev(ex, crow, col, val, X, m, n, 1.0, 1.0, Y0)
    c1, c2 = ex.Context(), ex.Context()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    A = _cuda_csr(crow, col, val, m, n)
    Xd = torch.from_numpy(X).cuda()
    Y1, Y2 = torch.from_numpy(Y0.copy()).cuda(), torch.from_numpy(Y0.copy()).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c1.exspmm(A, Xd, 1.0, 1.0, Y1)
    with torch.cuda.stream(s2):
        c2.exspmm(A, Xd, 1.0, 1.0, Y2)
    torch.cuda.synchronize()
    _assert_bits(Y1.cpu().numpy(), ref, "context 1")
    _assert_bits(Y2.cpu().numpy(), ref, "context 2")
    host = ex.exspmm((crow, col, val, (m, n)), X, 1.0, 1.0, Y0)
    _assert_bits(host, ref, "host arrays")
    # a column-major X is copied, not misread
    Xf = torch.from_numpy(np.asfortranarray(X)).cuda()
    assert Xf.stride(1) != 1
    _assert_bits(ex.exspmm_dev(A, Xf, 1.0, 1.0, torch.from_numpy(Y0.copy()).cuda()).cpu().numpy(), ref, "X strided")
    c1.destroy()
    c2.destroy()


def test_stencil_takes_the_register_path(ex, oracle):
    crow, col = _stencil(12)
    m = n = 12 ** 3
    k = 8
    val = oracle.gen("fpuniform", int(crow[-1]), 31, 10, 0)
    X = oracle.gen("fpuniform", n * 8, 32, 10, 0).reshape(n, 8)
    got = _dev(ex, crow.astype(np.int32), col.astype(np.int32), val, X, m, n, 1.0, 0.0, np.zeros((m, k)))
    info = ex.last_spmm_info()
    assert info[2] == 0 and info[1] <= 5 * k and info[0] + info[1] == m * k, info
    want = _oracle_outputs(oracle, crow, col, val, X, 1.0, 0.0, np.zeros((m, k)))
    _assert_bits(got, want, "stencil")


def test_full_size_stencil_and_long_row(ex, oracle):
    import torch
    g, k = 64, 16
    crow, col = _stencil(g)
    m0 = g ** 3
    n = m0
    long_len = 2 ** 22
    crow = np.concatenate([crow, [crow[-1] + long_len]]).astype(np.int64)
    rng = np.random.default_rng(8)
    col = np.concatenate([col, rng.integers(0, n, size=long_len)]).astype(np.int32)
    crow = crow.astype(np.int32)
    m = m0 + 1
    nnz = int(crow[-1])
    val = ex.gen_dev("fpuniform_signed", nnz, 101, 40, 20)
    X = ex.gen_dev("fpuniform_signed", n * k, 102, 40, 20).view(n, k)
    A = (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), val, (m, n))
    y = ex.exspmm_dev(A, X, 1.0, 0.0).cpu().numpy()
    info = ex.last_spmm_info()
    assert info[2] == 1 and info[0] + info[1] == (m - 1) * k, info
    valh, xh = val.cpu().numpy(), X.cpu().numpy()
    sample = sorted(set(rng.choice(m0, size=2000, replace=False).tolist()) | {m - 1})
    want = _oracle_outputs(oracle, crow, col, valh, xh, 1.0, 0.0, np.zeros((m, k)), rows=sample)
    _assert_bits(y, want, "sample", rows=sample)
    ex.set_spmm_path(1)
    try:
        y1 = ex.exspmm_dev(A, X, 1.0, 0.0).cpu().numpy()
    finally:
        ex.set_spmm_path(0)
    _assert_bits(y1, y, "path 1")


def test_plain_fpe1_within_the_summation_bound(ex, oracle):
    """fpe == 1 is a plain fp64 sum in some order.  For any order, |computed - exact| <= gamma(len + 1) S with
    S = sum |val alpha X|: one rounding of alpha X, one of the product, at most len - 1 additions; the addition of
    the beta term adds one more u S and the term's own product and addition 2 u |beta Y|.  The reference is the
    exact result rounded (half an ulp of it more).  u = 2^-53, gamma(t) ~ t u: (len + 2) u S + 2 u |beta Y| + u |want|."""
    rng = np.random.default_rng(12)
    m, n, k = 400, 300, 8
    crow, col = _random_csr(rng, m, n, [0, 1, 2, 31, 64, 65, 1000, 9000])
    val = _gen(oracle, "fpuniform_signed", 40, 20, int(crow[-1]), 111)
    X = _gen(oracle, "fpuniform_signed", 40, 20, n * k, 112).reshape(n, k)
    Y0 = _gen(oracle, "fpuniform_signed", 40, 20, m * k, 113).reshape(m, k)
    u = 2.0 ** -53
    for alpha, beta in ((1.0, 0.0), (-0.7, 3.3)):
        got = _dev(ex, crow, col, val, X, m, n, alpha, beta, Y0, fpe=1)
        assert not np.isnan(got).any()
        want = _oracle_outputs(oracle, crow, col, val, X, alpha, beta, Y0)
        lens = np.diff(crow)
        S = np.zeros((m, k))
        for i in range(m):
            a, b = int(crow[i]), int(crow[i + 1])
            S[i] = np.abs(val[a:b, None] * (alpha * X[col[a:b]])).sum(axis=0)
        bound = (lens[:, None] + 2) * u * S + 2 * u * np.abs(beta * Y0) + u * np.abs(want)
        err = np.abs(got - want)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print("fpe=1: max err / bound =", float(np.max(err / np.maximum(bound, 1e-300))))
        assert (err <= bound).all(), (alpha, beta, worst, err[worst], bound[worst])
