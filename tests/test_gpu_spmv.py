"""GPU tests of ExSpMV: bit-exact against the per-row ExGEMV oracle, invariance, capture, contexts, full size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = [("fpuniform", 10, 0), ("fpuniform_signed", 60, 30), ("lognormal", 0.0, 50.0), ("ill_cond", 1e32, 0),
         ("cancel", 0, 0)]
AB = [(1.0, 0.0), (1.0, 1.0), (-0.7, 3.3), (2.0 ** -3, 0.0)]


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_spmv_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _random_csr(rng, m, n, lengths, itype=np.int64):
    lens = rng.choice(lengths, size=m)
    crow = np.zeros(m + 1, dtype=np.int64)
    crow[1:] = np.cumsum(lens)
    col = rng.integers(0, max(n, 1), size=int(crow[-1])) if n > 0 else np.zeros(int(crow[-1]), dtype=np.int64)
    return crow.astype(itype), col.astype(itype)


def _oracle_rows(oracle, crow, col, val, x, alpha, beta, y0, rows=None, mode=0):
    """Row i = oracle.exgemv('N') on the 1 x k_i matrix of row i's values against the gathered x."""
    out = np.array(y0, dtype=np.float64, copy=True)
    rows = range(len(crow) - 1) if rows is None else rows
    for i in rows:
        a, b = int(crow[i]), int(crow[i + 1])
        if b <= a:
            v, xs = np.zeros(1), np.zeros(1)
        else:
            v, xs = val[a:b], x[col[a:b]]
        out[i] = oracle.exgemv("N", 1, len(v), alpha, v, 1, xs, beta, y0[i:i + 1], 0, mode=mode)[0]
    return out


def _dev(ex, crow, col, val, x, m, n, alpha, beta, y0, fpe=8, ee=True, ctx=None):
    import torch
    A = (torch.from_numpy(np.asarray(crow)).cuda(), torch.from_numpy(np.asarray(col)).cuda(),
         torch.from_numpy(np.asarray(val)).cuda(), (m, n))
    X = torch.from_numpy(np.asarray(x)).cuda()
    Y = torch.from_numpy(np.array(y0, dtype=np.float64)).cuda()
    f = ctx.exspmv if ctx is not None else ex.exspmv_dev
    f(A, X, alpha, beta, Y, fpe, ee)
    return Y.cpu().numpy()


def _gen(oracle, kind, p0, p1, count, seed):
    return oracle.gen(kind, max(count, 1), seed, p0, p1)[:count].copy()


@pytest.mark.parametrize("mode", [0, 1])
def test_random_csr_vs_oracle(ex, oracle, mode):
    lib = ex.load_library()
    rng = np.random.default_rng(1 + mode)
    lengths = [0, 1, 2, 31, 63, 64, 65, 1000]
    try:
        lib.exblas_set_round_mode(mode)
        for t, (kind, p0, p1) in enumerate(KINDS):
            m, n = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
            crow, col = _random_csr(rng, m, n, lengths)
            if t == 0:   # one row of 70 000 entries (split across workgroups)
                lens = np.diff(crow)
                lens[m // 2] = 70000
                crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
                col = rng.integers(0, n, size=int(crow[-1]))
            nnz = int(crow[-1])
            val = _gen(oracle, kind, p0, p1, nnz, 11 + t)
            x = _gen(oracle, kind, p0, p1, n, 12 + t)
            y0 = _gen(oracle, kind, p0, p1, m, 13 + t)
            for alpha, beta in AB:
                want = _oracle_rows(oracle, crow, col, val, x, alpha, beta, y0, mode=mode)
                got = _dev(ex, crow, col, val, x, m, n, alpha, beta, y0)
                bad = np.nonzero(_bits(got) != _bits(want))[0]
                assert bad.size == 0, (kind, alpha, beta, mode, bad[:5], got[bad[:3]], want[bad[:3]])
    finally:
        lib.exblas_set_round_mode(0)


def test_random_csr_vs_mpfr(ex, oracle):
    if oracle.mpfr() is None:
        pytest.skip("MPFR oracle not built")
    rng = np.random.default_rng(7)
    m, n = 500, 700
    crow, col = _random_csr(rng, m, n, [1, 2, 31, 64, 65, 300])
    val = _gen(oracle, "fpuniform_signed", 60, 30, int(crow[-1]), 21)
    x = _gen(oracle, "fpuniform_signed", 60, 30, n, 22)
    y0 = _gen(oracle, "fpuniform_signed", 60, 30, m, 23)
    got = _dev(ex, crow, col, val, x, m, n, 1.0, 1.0, y0)
    for i in range(m):
        a, b = int(crow[i]), int(crow[i + 1])
        want = oracle.mpfr_exgemv("N", 1, b - a, 1.0, val[a:b], 1, x[col[a:b]], 1.0, y0[i:i + 1])[0]
        assert _bits(got[i:i + 1])[0] == _bits(np.array([want]))[0], i


def _edge_rows():
    """(values, x, expected rounding result or None) rows built on the fast path's boundaries."""
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
    y0 = np.zeros(m)
    with np.errstate(over="ignore", invalid="ignore"):
        finite = [i for i in range(m) if np.isfinite(np.array(rows[i][0]) * np.array(rows[i][1])).all()]
    try:
        lib.exblas_set_round_mode(mode)
        want = _oracle_rows(oracle, crow, col, val, x, 1.0, 0.0, y0, rows=finite, mode=mode)
        got = _dev(ex, crow, col, val, x, m, n, 1.0, 0.0, y0)
        info = ex.last_spmv_info()   # (before the ExGEMV calls below reuse the workspace)
        assert (_bits(got[finite]) == _bits(want[finite])).all(), np.nonzero(_bits(got) != _bits(want))[0]
        # non-finite products: the oracle's exgemv drops them, the library's ExGEMV follows IEEE;
        # ExSpMV is what GPU ExGEMV 'N' computes for the row as a 1 x k matrix
        for i in range(m):
            if i in finite:
                continue
            v, xs = np.array(rows[i][0]), np.array(rows[i][1])
            Y = torch.zeros(1, dtype=torch.float64, device="cuda")
            ex.exgemv_dev("N", 1, len(v), 1.0, torch.from_numpy(v).cuda(), 1, torch.from_numpy(xs).cuda(), 0.0, Y, 8, True)
            assert _bits(got[i:i + 1])[0] == _bits(Y.cpu().numpy())[0], (i, got[i], Y)
        if mode == 0:
            # ties, near-ties, subnormal, infinite and non-finite rows cannot be certified in registers
            assert info[1] >= 12 and info[0] + info[1] == m, info
    finally:
        lib.exblas_set_round_mode(0)
    if mode == 0:   # ties to even (the reference rounding mode rounds them its own way; checked against the oracle above)
        assert got[0] == 1.0 and got[1] == 1.0 + 2 * 2.0 ** -52
    assert np.isnan(got[-3]) and np.isnan(got[-2]) and got[-4] == np.inf and got[-6] == -np.inf


def _stencil(k):
    """27-point stencil on a k^3 grid, int32 CSR."""
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


def test_stencil_takes_the_fast_path(ex, oracle):
    crow, col = _stencil(12)
    m = n = 12 ** 3
    val = _gen(oracle, "fpuniform", 10, 0, int(crow[-1]), 31)
    x = _gen(oracle, "fpuniform", 10, 0, n, 32)
    got = _dev(ex, crow.astype(np.int32), col.astype(np.int32), val, x, m, n, 1.0, 0.0, np.zeros(m))
    info = ex.last_spmv_info()
    assert info[0] >= m - 5 and info[2] == 0, info
    want = _oracle_rows(oracle, crow, col, val, x, 1.0, 0.0, np.zeros(m))
    assert (_bits(got) == _bits(want)).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_dense_equivalence_with_exgemv(ex, oracle, mode):
    import torch
    lib = ex.load_library()
    rng = np.random.default_rng(5)
    m, n = 300, 257
    a = _gen(oracle, "fpuniform_signed", 40, 20, m * n, 41).reshape(m, n)
    a[rng.random((m, n)) < 0.3] = 0.0
    x = _gen(oracle, "fpuniform_signed", 40, 20, n, 42)
    y0 = _gen(oracle, "fpuniform_signed", 40, 20, m, 43)
    mask = a != 0.0
    crow = np.zeros(m + 1, dtype=np.int64)
    crow[1:] = np.cumsum(mask.sum(axis=1))
    col = np.nonzero(mask)[1].astype(np.int64)
    val = a[mask]
    try:
        lib.exblas_set_round_mode(mode)
        for alpha, beta in AB:
            A = torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).cuda()
            Y = torch.from_numpy(y0.copy()).cuda()
            ex.exgemv_dev("N", m, n, alpha, A, m, torch.from_numpy(x).cuda(), beta, Y, 8, True)
            got = _dev(ex, crow, col, val, x, m, n, alpha, beta, y0)
            assert (_bits(got) == _bits(Y.cpu().numpy())).all(), (alpha, beta, mode)
    finally:
        lib.exblas_set_round_mode(0)


def test_invariance(ex, oracle):
    rng = np.random.default_rng(9)
    m, n = 1500, 1200
    crow, col = _random_csr(rng, m, n, [0, 1, 2, 27, 63, 64, 65, 700, 20000])
    val = _gen(oracle, "lognormal", 0.0, 50.0, int(crow[-1]), 51)
    x = _gen(oracle, "lognormal", 0.0, 50.0, n, 52)
    y0 = _gen(oracle, "lognormal", 0.0, 50.0, m, 53)
    ref = _dev(ex, crow, col, val, x, m, n, -0.7, 3.3, y0)
    try:
        for path in (0, 1, 2, 3):
            ex.set_spmv_path(path)
            got = _dev(ex, crow, col, val, x, m, n, -0.7, 3.3, y0)
            assert (_bits(got) == _bits(ref)).all(), path
            info = ex.last_spmv_info()
            if path == 1:
                assert info[0] == 0, info
            if path == 3:
                assert info[2] == m, info
    finally:
        ex.set_spmv_path(0)
    for fpe in (0, 2, 4, 8):
        for ee in (False, True):
            assert (_bits(_dev(ex, crow, col, val, x, m, n, -0.7, 3.3, y0, fpe, ee)) == _bits(ref)).all(), (fpe, ee)
    got = _dev(ex, crow.astype(np.int32), col.astype(np.int32), val, x, m, n, -0.7, 3.3, y0)
    assert (_bits(got) == _bits(ref)).all()
    # columns shuffled within rows
    col2, val2 = col.copy(), val.copy()
    for i in range(m):
        a, b = int(crow[i]), int(crow[i + 1])
        p = rng.permutation(b - a) + a
        col2[a:b], val2[a:b] = col[p], val[p]
    assert (_bits(_dev(ex, crow, col2, val2, x, m, n, -0.7, 3.3, y0)) == _bits(ref)).all()
    # permuted rows
    perm = rng.permutation(m)
    lens = np.diff(crow)[perm]
    crow3 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col3 = np.concatenate([col[crow[i]:crow[i + 1]] for i in perm])
    val3 = np.concatenate([val[crow[i]:crow[i + 1]] for i in perm])
    got = _dev(ex, crow3, col3, val3, x, m, n, -0.7, 3.3, y0[perm])
    assert (_bits(got) == _bits(ref[perm])).all()


def test_out_of_range_column_gives_nan_row(ex, oracle):
    import torch
    rng = np.random.default_rng(3)
    m, n = 200, 100
    crow, col = _random_csr(rng, m, n, [1, 5, 40, 100, 3000])
    val = _gen(oracle, "fpuniform", 10, 0, int(crow[-1]), 61)
    xfull = _gen(oracle, "fpuniform", 10, 0, n + 64, 62)   # x has n + 64 entries, the call passes n
    bad_rows = [3, 77, int(np.argmax(np.diff(crow)))]
    col = col.copy()
    for r in bad_rows:
        col[int(crow[r])] = n + 5 if r != 77 else -1 if crow[r + 1] > crow[r] else col[int(crow[r])]
    A = (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), (m, n))
    X = torch.from_numpy(xfull).cuda()
    for path in (0, 1, 3):
        ex.set_spmv_path(path)
        try:
            for fpe in (8, 1):
                y = ex.exspmv_dev(A, X, 1.0, 0.0, None, fpe).cpu().numpy()
                good = [i for i in range(m) if i not in bad_rows]
                assert np.isnan(y[bad_rows]).all(), (path, fpe)
                if fpe == 8:
                    want = _oracle_rows(oracle, crow, col, val, xfull[:n], 1.0, 0.0, np.zeros(m), rows=good)
                    assert (_bits(y[good]) == _bits(want[good])).all()
                else:
                    assert not np.isnan(y[good]).any()
        finally:
            ex.set_spmv_path(0)


def test_graph_capture(ex, oracle):
    import torch
    rng = np.random.default_rng(4)
    m, n = 2000, 1800
    crow, col = _random_csr(rng, m, n, [3, 27, 60])
    nnz = int(crow[-1])
    val = _gen(oracle, "fpuniform", 10, 0, nnz, 71)
    Crow, Col, Val = (torch.from_numpy(a).cuda() for a in (crow, col, val))
    X = torch.from_numpy(_gen(oracle, "fpuniform", 10, 0, n, 72)).cuda()
    Y = torch.zeros(m, dtype=torch.float64, device="cuda")
    A = (Crow, Col, Val, (m, n))
    ex.exspmv_dev(A, X, 1.0, 0.0, Y)   # warm-up: sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exspmv_dev(A, X, 1.0, 0.0, Y)
    # new x, then a matrix of the same shape and nnz whose rows change class (one long row, many medium and empty)
    lens = np.zeros(m, dtype=np.int64)
    lens[5] = nnz - 90 * 100
    lens[100:190] = 100
    crow2 = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col2 = rng.integers(0, n, size=nnz)
    for step, (cr, co) in enumerate(((crow, col), (crow2, col2))):
        X.copy_(torch.from_numpy(_gen(oracle, "lognormal", 0.0, 5.0, n, 80 + step)))
        Crow.copy_(torch.from_numpy(cr))
        Col.copy_(torch.from_numpy(co))
        Y.fill_(-1.0)
        g.replay()
        torch.cuda.synchronize()
        eager = ex.exspmv_dev(A, X, 1.0, 0.0).cpu().numpy()
        assert (_bits(Y.cpu().numpy()) == _bits(eager)).all(), step
        want = _oracle_rows(oracle, cr, co, val, X.cpu().numpy(), 1.0, 0.0, np.zeros(m))
        assert (_bits(eager) == _bits(want)).all(), step
    del g


def test_contexts_streams_and_host_entry(ex, oracle):
    import torch
    rng = np.random.default_rng(6)
    m, n = 1000, 900
    crow, col = _random_csr(rng, m, n, [0, 5, 30, 70, 500, 17000])
    val = _gen(oracle, "ill_cond", 1e32, 0, int(crow[-1]), 91)
    x = _gen(oracle, "ill_cond", 1e32, 0, n, 92)
    y0 = _gen(oracle, "ill_cond", 1e32, 0, m, 93)
    ref = _dev(ex, crow, col, val, x, m, n, 1.0, 1.0, y0)
    c1, c2 = ex.Context(), ex.Context()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    A = (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), (m, n))
    X = torch.from_numpy(x).cuda()
    Y1, Y2 = torch.from_numpy(y0.copy()).cuda(), torch.from_numpy(y0.copy()).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        c1.exspmv(A, X, 1.0, 1.0, Y1)
    with torch.cuda.stream(s2):
        c2.exspmv(A, X, 1.0, 1.0, Y2)
    torch.cuda.synchronize()
    assert (_bits(Y1.cpu().numpy()) == _bits(ref)).all()
    assert (_bits(Y2.cpu().numpy()) == _bits(ref)).all()
    host = ex.exspmv((crow, col, val, (m, n)), x, 1.0, 1.0, y0)
    assert (_bits(host) == _bits(ref)).all()
    c1.destroy()
    c2.destroy()


def test_full_size_stencil_and_long_row(ex, oracle):
    import torch
    k = 64
    crow, col = _stencil(k)
    m0 = k ** 3
    n = m0
    long_len = 2 ** 22
    crow = np.concatenate([crow, [crow[-1] + long_len]]).astype(np.int64)
    rng = np.random.default_rng(8)
    col = np.concatenate([col, rng.integers(0, n, size=long_len)]).astype(np.int32)
    crow = crow.astype(np.int32)
    m = m0 + 1
    nnz = int(crow[-1])
    val = ex.gen_dev("fpuniform_signed", nnz, 101, 40, 20)
    X = ex.gen_dev("fpuniform_signed", n, 102, 40, 20)
    A = (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), val, (m, n))
    y = ex.exspmv_dev(A, X, 1.0, 0.0).cpu().numpy()
    info = ex.last_spmv_info()
    assert info[2] == 1 and info[0] + info[1] == m - 1, info
    valh, xh = val.cpu().numpy(), X.cpu().numpy()
    # fallen-back rows: every row of the path-1 run matches; the sample covers >= 20000 rows incl. the long one
    sample = sorted(set(rng.choice(m0, size=20000, replace=False).tolist()) | {m - 1})
    want = _oracle_rows(oracle, crow, col, valh, xh, 1.0, 0.0, np.zeros(m), rows=sample)
    assert (_bits(y[sample]) == _bits(want[sample])).all()
    ex.set_spmv_path(1)
    try:
        y1 = ex.exspmv_dev(A, X, 1.0, 0.0).cpu().numpy()
    finally:
        ex.set_spmv_path(0)
    assert (_bits(y1) == _bits(y)).all()
