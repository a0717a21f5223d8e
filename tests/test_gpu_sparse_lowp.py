"""Narrow ExSpMV / ExSpMM on the GPU, bit for bit.

Identity 1: with float64 vectors the result is what exspmv_dev / exspmm_dev give on val.double(), in both rounding modes.
Identity 2: with narrow vectors the result is the integer model's single rounding (tests/sparse_lowp_cases.py) of the exact
row total -- on every planted edge of the output format and on the traps where "round to double, then cast" is wrong --
and the counters show that near-ties went through the accumulator and well-separated rows were rounded in registers.
Identity 3: a row is exdot_to_dev of its values and gathered x.  Shapes: the row lengths and m that cross the lane-group,
batch and classifier seams, every k that changes the lane-group width or the column tile, odd leading dimensions, odd
element offsets, int32 and int64 indices, paths 0 to 3 (3 splits every row at 16 entries)."""
import numpy as np
import pytest

import lowp_cases as L
import sparse_lowp_cases as S

pytestmark = pytest.mark.gpu
LENS = [0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257, 600]
KS = [1, 2, 3, 4, 5, 8, 17, 32, 33, 64, 65, 70]
AB = [(1.0, 0.0), (0.3, 1.0), (-1.0, 0.3), (1.0, -1.0), (0.0, 0.3), (0.3, 0.0), (-1.0, 1.0), (0.0, 0.0)]


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.load_library().exblas_set_round_mode(0)
    exblas_amd.set_spmv_path(0)
    exblas_amd.set_spmm_path(0)


def tdt(name):
    import torch
    return getattr(torch, name)


def bits(t):
    """the bit patterns of a tensor's elements as a numpy array of unsigned ints"""
    import torch
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()]
    ut = {8: np.uint64, 4: np.uint32, 2: np.uint16}[t.element_size()]
    return t.detach().contiguous().view(it).cpu().numpy().view(ut)


def odd(src, off=1):
    """a CUDA copy of the CPU tensor src that starts `off` elements past a 16-byte boundary (1-D)"""
    import torch
    buf = torch.zeros(src.numel() + 8, dtype=src.dtype, device="cuda")
    v = buf[off:off + src.numel()]
    v.copy_(src)
    return v


def padded(src, pad, fill=0.0):
    """a CUDA copy of the 2-D CPU tensor src as the leading columns of a block whose leading dimension is odd and above k,
    starting one element past a 16-byte boundary; returns (view, whole buffer view of the rows)"""
    import torch
    r, k = src.shape
    ld = k + pad + ((k + pad + 1) % 2)
    buf = torch.full((r * ld + 9,), fill, dtype=src.dtype, device="cuda")
    whole = buf[1:1 + r * ld].view(r, ld)
    whole[:, :k].copy_(src)
    return whole[:, :k], whole


def csr_shape(rng, m, n, itype):
    lens = np.array([LENS[(i * 7 + 3) % len(LENS)] for i in range(m)])
    if m >= 2:
        lens[rng.integers(m)] = 0
    crow = np.concatenate([[0], np.cumsum(lens)]).astype(itype)
    col = rng.integers(0, n, size=int(crow[-1])).astype(itype)          # unsorted, duplicates included
    return crow, col


def narrow_random(rng, size, name, spread=8):
    import torch
    x = rng.standard_normal(size) * np.exp2(rng.integers(-spread, spread, size))
    return torch.from_numpy(x).to(tdt(name))


def with_subnormals(rng, t, name):
    """t (a CPU tensor of the narrow dtype) with about a tenth of its entries replaced by subnormals of the dtype, both signs"""
    prec = L.FORMATS[name][0]
    flat = t.reshape(-1)
    pick = np.nonzero(rng.random(flat.numel()) < 0.1)[0]
    if pick.size:
        pats = rng.integers(1, 1 << (prec - 1), size=pick.size) | (rng.integers(0, 2, size=pick.size) << (L.FORMATS[name][3] - 1))
        flat[pick] = L.as_torch(pats.tolist(), name)
    return t


def dev_csr(crow, col, val, shape):
    import torch
    return (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), odd(val), shape)


# ---------------------------------------------------------------------------------------------
# identity 1: float64 vectors
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vt", S.NARROW)
def test_identity1_spmv(ex, vt):
    import torch
    lib = ex.load_library()
    rng = np.random.default_rng([1, L.DT_CODE[vt]])
    for m in (1, 9, 70, 300):
        n = 2 * m + 5
        itype = np.int32 if m % 2 else np.int64
        crow, col = csr_shape(rng, m, n, itype)
        val = with_subnormals(rng, narrow_random(rng, int(crow[-1]), vt), vt)
        A = dev_csr(crow, col, val, (m, n))
        Ad = (A[0], A[1], A[2].double(), (m, n))
        assert m < 9 or ((A[2] != 0) & (A[2].double().abs() < 2.0 ** L.FORMATS[vt][1])).any()      # subnormal values are fed
        x = odd(torch.from_numpy(rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))))
        y0 = torch.from_numpy(rng.standard_normal(m)).cuda()
        if m == 300:    # every (path, fpe, mode) and every (path, alpha, beta), the third factor cycling on its own counter
            combos = [(p, f, md, AB[j % len(AB)]) for j, (p, f, md) in
                      enumerate((p, f, md) for p in range(4) for f in (0, 4, 8) for md in (0, 1))]
            combos += [(p, (0, 4, 8)[j % 3], (j // 3) % 2, ab) for j, (p, ab) in
                       enumerate((p, ab) for p in range(4) for ab in AB)]
        else:
            combos = [(p, 8, 0, AB[(p + m) % len(AB)]) for p in range(4)]
        for path, fpe, mode, (alpha, beta) in combos:
            try:
                lib.exblas_set_round_mode(mode)
                ex.set_spmv_path(path)
                got = ex.exspmv_lp_dev(A, x, alpha, beta, odd(y0.cpu()), fpe=fpe)
                want = ex.exspmv_dev(Ad, x, alpha, beta, y0.clone(), fpe=fpe)
            finally:
                lib.exblas_set_round_mode(0)
                ex.set_spmv_path(0)
            assert got.dtype == torch.float64
            assert (bits(got) == bits(want)).all(), (vt, m, path, fpe, mode, alpha, beta)
    # y = None allocates float64 zeros
    got = ex.exspmv_lp_dev(A, x)
    assert got.dtype == torch.float64 and (bits(got) == bits(ex.exspmv_dev(Ad, x))).all()


@pytest.mark.parametrize("vt", S.NARROW)
def test_identity1_spmm(ex, vt):
    import torch
    lib = ex.load_library()
    rng = np.random.default_rng([2, L.DT_CODE[vt]])
    for m, ks in ((70, KS), (300, [4, 65]), (9, [3]), (1, [5])):
        n = m + 11
        itype = np.int64 if m % 2 else np.int32
        crow, col = csr_shape(rng, m, n, itype)
        val = with_subnormals(rng, narrow_random(rng, int(crow[-1]), vt), vt)
        A = dev_csr(crow, col, val, (m, n))
        Ad = (A[0], A[1], A[2].double(), (m, n))
        cases = [(k, i % 4, (0, 4, 8)[i % 3], (i // 2) % 2, AB[(i + m) % len(AB)]) for i, k in enumerate(ks)]
        if m == 70:     # every (path, alpha, beta) and every (path, fpe, mode), at a k of one lane group and of a column tile
            cases += [((5, 65)[j % 2], p, (0, 4, 8)[j % 3], (j // 3) % 2, ab) for j, (p, ab) in
                      enumerate((p, ab) for p in range(4) for ab in AB)]
            cases += [((5, 65)[j % 2], p, f, md, AB[j % len(AB)]) for j, (p, f, md) in
                      enumerate((p, f, md) for p in range(4) for f in (0, 4, 8) for md in (0, 1))]
        for k, path, fpe, mode, (alpha, beta) in cases:
            X, _ = padded(torch.from_numpy(rng.standard_normal((n, k)) * np.exp2(rng.integers(-20, 20, (n, k)))), 2)
            Y0 = torch.from_numpy(rng.standard_normal((m, k)))
            Y, whole = padded(Y0, 4, fill=float("nan"))
            try:
                lib.exblas_set_round_mode(mode)
                ex.set_spmm_path(path)
                got = ex.exspmm_lp_dev(A, X, alpha, beta, Y, fpe=fpe)
                want = ex.exspmm_dev(Ad, X, alpha, beta, Y0.cuda(), fpe=fpe)
            finally:
                lib.exblas_set_round_mode(0)
                ex.set_spmm_path(0)
            assert (bits(got) == bits(want)).all(), (vt, m, k, path, fpe, mode)
            assert torch.isnan(whole[:, k:]).all()                      # the padding of Y is never written


# ---------------------------------------------------------------------------------------------
# identity 2: narrow vectors, the integer model
# ---------------------------------------------------------------------------------------------
def exact_want(val_pats, x_pats, dt):
    """round_fine of the exact total of one row (patterns as numpy arrays), all in Python integers"""
    mv, sv = L._split(np.asarray(val_pats), dt)
    mx, sx = L._split(np.asarray(x_pats), dt)
    tot = 0
    for a, b, s in zip(mv.tolist(), mx.tolist(), (sv + sx).tolist()):
        tot += (a * b) << s
    return S.round_fine(tot, dt)


class PlantedMatrix:
    """rows (S.Row or random) against x = [table | random tail]; every row's expected pattern from the integer model"""

    def __init__(self, dt, rows, n_random, seed, itype=np.int32, tail_only=False):
        rng = np.random.default_rng([seed, L.DT_CODE[dt]])
        tab = S.table(dt)
        lo = S.lo_exp(dt)
        tail = bits(narrow_random(rng, 97, dt, spread=6))
        self.x_pats = np.concatenate([np.array(tab, dtype=np.uint64), tail.astype(np.uint64)])
        n = self.x_pats.size
        vals, cols, crow, want, must = [], [], [0], [], []
        slots = list(rows) + [None] * n_random
        order = rng.permutation(len(slots)) if n_random else np.arange(len(slots))
        for i, idx in enumerate(order):
            r = slots[idx]
            if r is not None:
                v = [p for p, _ in r.entries]
                c = [b - lo for _, b in r.entries]
                perm = rng.permutation(len(v))
                v, c = [v[j] for j in perm], [c[j] for j in perm]
                w = r.want
            else:
                ln = LENS[(i * 5 + 1) % len(LENS)]
                v = bits(narrow_random(rng, ln, dt, spread=6)).astype(np.uint64).tolist()
                c = rng.integers(len(tab) if tail_only else 0, n, size=ln).tolist()
                w = exact_want(v, self.x_pats[c], dt) if ln else 0
            vals += v
            cols += c
            crow.append(len(vals))
            want.append(w)
            must.append(bool(r is not None and r.must_acc))
        self.m, self.n, self.dt = len(slots), n, dt
        self.crow, self.col = np.array(crow, dtype=itype), np.array(cols, dtype=itype)
        self.val_pats, self.want, self.must = vals, np.array(want, dtype=np.uint64), np.array(must)

    def device(self):
        import torch
        val = L.as_torch(self.val_pats, self.dt) if self.val_pats else torch.zeros(0, dtype=tdt(self.dt))
        A = dev_csr(self.crow, self.col, val, (self.m, self.n))
        return A, odd(L.as_torch(self.x_pats.tolist(), self.dt))


@pytest.mark.parametrize("dt", S.NARROW)
def test_identity2_planted_and_trap_rows(ex, dt):
    rows = S.all_rows(dt)
    alone = PlantedMatrix(dt, rows, 0, 5, np.int64)
    among = PlantedMatrix(dt, rows, 130, 6, np.int32)
    for pm in (alone, among):
        A, x = pm.device()
        for path in range(4):
            for fpe, mode in ((8, 0), (0, 0), (4, 1)):                  # narrow outputs: nearest even whatever the mode
                try:
                    ex.load_library().exblas_set_round_mode(mode)
                    ex.set_spmv_path(path)
                    y = ex.exspmv_lp_dev(A, x, fpe=fpe)
                    info = ex.last_spmv_info()
                finally:
                    ex.load_library().exblas_set_round_mode(0)
                    ex.set_spmv_path(0)
                assert y.dtype == tdt(dt)
                bad = np.nonzero(bits(y).astype(np.uint64) != pm.want)[0]
                assert bad.size == 0, (dt, path, fpe, mode, bad[:5], [hex(int(v)) for v in bits(y)[bad[:5]]],
                                       [hex(int(v)) for v in pm.want[bad[:5]]])
                if path == 3:
                    assert info[2] == pm.m and info[3] > 0              # every row split
    # the near-ties that no double holds cannot be certified: all of them are rounded from the accumulator
    hard = PlantedMatrix(dt, [r for r in rows if r.must_acc], 0, 7)
    assert hard.m >= 8
    A, x = hard.device()
    for path in (0, 2):
        ex.set_spmv_path(path)
        try:
            y = ex.exspmv_lp_dev(A, x)
            info = ex.last_spmv_info()
        finally:
            ex.set_spmv_path(0)
        assert (bits(y).astype(np.uint64) == hard.want).all()
        assert info[0] == 0 and info[1] == hard.m, (dt, path, info)


@pytest.mark.parametrize("dt", S.NARROW)
def test_identity2_random_rows_round_in_registers(ex, dt):
    """well-separated random rows: the integer model's bits, and on paths 0 and 2 most of them straight from registers"""
    pm = PlantedMatrix(dt, [], 300, 8, tail_only=True)      # (the table's range of exponents would spill the expansions)
    A, x = pm.device()
    for path in range(4):
        ex.set_spmv_path(path)
        try:
            y = ex.exspmv_lp_dev(A, x, fpe=(8, 0, 4, 6)[path])
            info = ex.last_spmv_info()
        finally:
            ex.set_spmv_path(0)
        assert (bits(y).astype(np.uint64) == pm.want).all(), (dt, path)
        if path in (0, 2):      # 0 is the path every caller runs: it must not send these rows through the accumulator
            assert info[0] > pm.m // 2 and info[0] + info[1] == pm.m, (path, info)
        if path == 1:
            assert info[0] == 0


@pytest.mark.parametrize("dt", S.NARROW)
def test_identity2_spmm_every_column_position(ex, dt):
    """X holds the table in every column, negated in the odd ones: each planted row sits in every column position (and every
    lane of its group), with the mirrored total next to it; column j is the narrow ExSpMV on column j"""
    import torch
    rows = S.all_rows(dt)
    pm = PlantedMatrix(dt, rows, 40, 9)
    A, x = pm.device()
    sign = S.sign_bit(dt)
    yv = bits(ex.exspmv_lp_dev(A, x)).astype(np.uint64)
    assert (yv == pm.want).all()
    yneg = bits(ex.exspmv_lp_dev(A, x, alpha=-1.0)).astype(np.uint64)      # fl64(-x) is exact: the mirrored totals
    zero = (yv & ~np.uint64(sign)) == 0
    assert ((yneg == (yv ^ np.uint64(sign))) | (zero & (yneg <= np.uint64(sign)))).all()
    for i, k in enumerate((3, 8, 33, 70)):
        X0 = x.cpu().unsqueeze(1).repeat(1, k)
        X0[:, 1::2] = -X0[:, 1::2]
        X, _ = padded(X0, 2)
        Y, whole = padded(torch.zeros((pm.m, k), dtype=tdt(dt)), 2, fill=float("nan"))
        ex.set_spmm_path(i % 4)
        try:
            got = ex.exspmm_lp_dev(A, X, 1.0, 0.0, Y, fpe=(8, 0, 4, 2)[i])
            info = ex.last_spmm_info()
        finally:
            ex.set_spmm_path(0)
        g = bits(got).astype(np.uint64)
        for j in range(k):
            ref = yv if j % 2 == 0 else yneg
            assert (g[:, j] == ref).all(), (dt, k, j)
        assert torch.isnan(whole[:, k:].float()).all()
        assert info[1] >= (pm.must.sum() * k if i % 4 != 3 else 0)        # near-ties were deferred to the accumulator


@pytest.mark.parametrize("dt", S.NARROW)
def test_spmm_columns_are_spmv_and_beta(ex, dt):
    """random narrow blocks: column j is bit for bit the narrow ExSpMV on (A, X[:, j], Y[:, j]), beta and alpha included"""
    import torch
    rng = np.random.default_rng([10, L.DT_CODE[dt]])
    m, n = 70, 90
    crow, col = csr_shape(rng, m, n, np.int32)
    A = dev_csr(crow, col, narrow_random(rng, int(crow[-1]), dt, 4), (m, n))
    for i, k in enumerate((2, 5, 17, 65)):
        X, _ = padded(narrow_random(rng, (n, k), dt, 4), 2)
        Y0 = narrow_random(rng, (m, k), dt, 4)
        alpha, beta = AB[(i + 1) % len(AB)]
        ex.set_spmm_path(i % 4)
        try:
            Y, whole = padded(Y0, 2, fill=float("nan"))
            got = ex.exspmm_lp_dev(A, X, alpha, beta, Y)
        finally:
            ex.set_spmm_path(0)
        for j in range(k):
            ref = ex.exspmv_lp_dev(A, X[:, j].contiguous(), alpha, beta, Y0[:, j].contiguous().cuda())
            assert (bits(got[:, j]) == bits(ref)).all(), (dt, k, j)
        assert torch.isnan(whole[:, k:].float()).all()


# ---------------------------------------------------------------------------------------------
# identity 3: a row is an ExDOT rounded once
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", S.NARROW)
def test_identity3_rows_are_exdot_to(ex, dt):
    rng = np.random.default_rng([11, L.DT_CODE[dt]])
    m, n = 45, 120
    crow, col = csr_shape(rng, m, n, np.int64)
    val = narrow_random(rng, int(crow[-1]), dt, 6)
    A = dev_csr(crow, col, val, (m, n))
    x = odd(narrow_random(rng, n, dt, 6))
    y = bits(ex.exspmv_lp_dev(A, x))
    for i in range(m):
        a, b = int(crow[i]), int(crow[i + 1])
        if b > a:
            d = ex.exdot_to_dev(A[2][a:b].contiguous(), x[A[1][a:b].long()].contiguous(), dtype=tdt(dt))
            assert int(bits(d.reshape(1))[0]) == int(y[i]), (dt, i, b - a)
        else:
            assert int(y[i]) == 0


# ---------------------------------------------------------------------------------------------
# non-finite values, columns out of range, y = None, the host entry
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vt,xt", S.PAIRS)
def test_nonfinite_and_out_of_range_columns(ex, vt, xt):
    import torch
    names = list(L.NONFINITE)
    tabs = [L.NONFINITE[k][1] for k in names] + [(L.NONFINITE[k][1][1], L.NONFINITE[k][1][0]) for k in names]
    flags = [L.NONFINITE[k][2] for k in names] * 2
    vals, xs, crow = [], [], [0]
    for a, b in tabs:
        vals += a
        xs += b
        crow.append(len(vals))
    # two finite rows, the second with a column outside [0, n)
    vals += [1.0, 2.0, 1.0, 2.0]
    crow += [len(vals) - 2, len(vals)]
    n = len(xs) + 2
    xs += [3.0, 4.0]
    m = len(crow) - 1
    for itype, out_col in ((np.int32, -1), (np.int64, n), (np.int64, 1 << 40)):
        col = np.arange(len(vals), dtype=itype)
        col[-4:] = [n - 2, n - 1, n - 2, out_col]
        A = dev_csr(np.array(crow, dtype=itype), col, torch.tensor(vals, dtype=tdt(vt)), (m, n))
        x = odd(torch.tensor(xs, dtype=tdt(xt)))
        for path in range(4):
            ex.set_spmv_path(path)
            ex.set_spmm_path(path)
            try:
                y = ex.exspmv_lp_dev(A, x).double().cpu().numpy()
                Y = ex.exspmm_lp_dev(A, torch.stack([x, x, x], dim=1)).double().cpu().numpy()
            finally:
                ex.set_spmv_path(0)
                ex.set_spmm_path(0)
            for out in (y, Y[:, 0], Y[:, 2]):
                for i, f in enumerate(flags):
                    if f == 1:
                        assert out[i] == np.inf, (i, path)
                    elif f == 2:
                        assert out[i] == -np.inf, (i, path)
                    else:
                        assert np.isnan(out[i]), (i, path)
                assert out[m - 2] == 11.0 and np.isnan(out[m - 1])


@pytest.mark.parametrize("dt", S.NARROW)
def test_host_entries_and_contexts(ex, dt):
    """the host forms (numpy; bfloat16: torch CPU tensors) and a Context give the bits of the default context's device form"""
    import torch
    rng = np.random.default_rng([12, L.DT_CODE[dt]])
    m, n, k = 9, 14, 3
    crow, col = csr_shape(rng, m, n, np.int32)
    val, x, X = narrow_random(rng, int(crow[-1]), dt), narrow_random(rng, n, dt), narrow_random(rng, (n, k), dt)
    A = dev_csr(crow, col, val, (m, n))
    want = ex.exspmv_lp_dev(A, x.cuda())
    wantM = ex.exspmm_lp_dev(A, X.cuda())
    wantd = ex.exspmv_lp_dev(A, x.double().cuda(), 0.3, 0.0)
    host = (lambda t: t) if dt == "bfloat16" else (lambda t: t.numpy())
    got = ex.exspmv_lp((crow, col, host(val), (m, n)), host(x))
    gotM = ex.exspmm_lp((crow, col, host(val), (m, n)), host(X))
    gotd = ex.exspmv_lp((crow, col, host(val), (m, n)), x.double().numpy(), alpha=0.3)
    as_t = (lambda a: a) if dt == "bfloat16" else torch.from_numpy
    assert (bits(as_t(got)) == bits(want)).all() and (bits(as_t(gotM)) == bits(wantM)).all()
    assert (bits(torch.from_numpy(gotd)) == bits(wantd)).all()
    ctx = ex.Context()
    try:
        assert (bits(ctx.exspmv_lp(A, x.cuda())) == bits(want)).all()
        assert (bits(ctx.exspmm_lp(A, X.cuda())) == bits(wantM)).all()
    finally:
        ctx.destroy()
    with pytest.raises(NotImplementedError):
        ex.exspmv_lp_dev(A, x.cuda(), fpe=1)


# ---------------------------------------------------------------------------------------------
# graph capture
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("routine", ["spmv", "spmm"])
def test_graph_replay_on_new_data(ex, routine):
    import torch
    dt = "bfloat16" if routine == "spmv" else "float16"
    rng = np.random.default_rng([13, len(routine)])
    m, n, k = 300, 310, 5
    crow, col = csr_shape(rng, m, n, np.int32)
    nnz = int(crow[-1])
    A = dev_csr(crow, col, narrow_random(rng, nnz, dt, 4), (m, n))
    shape = (n,) if routine == "spmv" else (n, k)
    x = narrow_random(rng, shape, dt, 4).cuda()
    y = torch.zeros((m,) if routine == "spmv" else (m, k), dtype=tdt(dt), device="cuda")
    call = ex.exspmv_lp_dev if routine == "spmv" else ex.exspmm_lp_dev
    call(A, x, 1.0, 0.0, y)            # the warm call sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            call(A, x, 1.0, 0.0, y)
    x.copy_(narrow_random(rng, shape, dt, 4))
    A[2].copy_(narrow_random(rng, nnz, dt, 4))
    A[1].copy_(torch.from_numpy(rng.integers(0, n, size=nnz).astype(np.int32)))
    y.fill_(-1.0)
    g.replay()
    torch.cuda.synchronize()
    eager = call(A, x)
    assert (bits(y) == bits(eager)).all()
    assert not (bits(y) == bits(torch.full_like(y, -1.0))).all()
    del g
