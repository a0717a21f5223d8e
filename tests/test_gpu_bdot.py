"""GPU tests of ExBDOT: bit-exact against the per-output ExDOT oracle and against exdot_dev on the strided columns;
invariance under variants, paths and entry points; constructed roundings; non-finite and degenerate inputs; capture.
Every comparison is on the bits; the only tolerance is the derived one of fpe == 1."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import bdot_cases as D
from helpers import FPE_VARIANTS_DOT

pytestmark = pytest.mark.gpu

KINDS = [("fpuniform", 10, 0), ("fpuniform_signed", 60, 30), ("lognormal", 0.0, 50.0), ("ill_cond", 1e32, 0),
         ("cancel", 0, 0)]
NS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4099]
D_KS = [1, 2, 3, 4, 5, 8, 16, 17, 33, 64, 65]
G_PQ = [(1, 1), (1, 7), (7, 1), (3, 5), (4, 4), (5, 4), (8, 8), (9, 17), (16, 16), (17, 3), (33, 2), (64, 1), (65, 2)]
SENTINEL = -12345.678
PRODUCT_FLAGS = 0x78   # bits 3..6 of a record's flag word: products outside the double-range accumulator's domain
SHIFTS = (0, 7, -13, 40)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_bdot_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_bits(got, want, what, keep=None):
    g, w = _bits(got), _bits(want)
    bad = np.argwhere((g != w) if keep is None else ((g != w) & keep))
    assert bad.size == 0, (what, len(bad), bad[:5].tolist())


def _gen(oracle, kind, p0, p1, count, seed):
    return oracle.gen(kind, max(count, 1), seed, p0, p1)[:count].copy()


def _padded(a, pad, off):
    """The block `a` on the device as a view [:, :k] of rows of k + pad doubles, NaN in the padding, the first entry
    `off` doubles into the allocation (off = 1 with an odd k + pad: rows alternate between 8- and 16-byte alignment)"""
    import torch
    n, k = a.shape
    ld = k + pad
    flat = torch.full((off + n * ld + 1,), float("nan"), dtype=torch.float64, device="cuda")
    view = flat[off:off + n * ld].view(n, ld)[:, :k]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    return view


def _run(ex, X, Y, mode, fpe=8, ee=True, ctx=None, xpad=3, ypad=1, off=0, cpad=2):
    """ExBDOT on padded blocks (Y None: Y = X); the padding of C holds a sentinel whose bits must survive"""
    import torch
    Xd = _padded(X, xpad, off)
    Yd = None if Y is None else _padded(Y, ypad, off)
    p, q = X.shape[1], (X if Y is None else Y).shape[1]
    f = ctx.exbdot if ctx is not None else ex.exbdot_dev
    if mode == "D":
        buf = torch.full((p + cpad,), SENTINEL, dtype=torch.float64, device="cuda")
        out = f(Xd, Yd, "D", buf[:p], fpe, ee)
        res = buf.cpu().numpy()
        assert (_bits(res[p:]) == _bits(np.array([SENTINEL]))[0]).all(), "the words behind c were written"
        assert out.data_ptr() == buf.data_ptr()
        return res[:p].copy()
    buf = torch.full((p, q + cpad), SENTINEL, dtype=torch.float64, device="cuda")
    out = f(Xd, Yd, "G", buf[:, :q], fpe, ee)
    res = buf.cpu().numpy()
    assert (_bits(res[:, q:]) == _bits(np.array([SENTINEL]))[0]).all(), "the padding of C was written"
    assert out.data_ptr() == buf.data_ptr()
    return np.ascontiguousarray(res[:, :q])


def _oracle(oracle, X, Y, mode, rmode=0):
    """one oracle ExDOT per output, on the strided columns of the contiguous blocks"""
    n, p = X.shape
    q = Y.shape[1]
    xf, yf = np.ascontiguousarray(X).ravel(), np.ascontiguousarray(Y).ravel()
    if n == 0:
        return np.zeros(p) if mode == "D" else np.zeros((p, q))
    if mode == "D":
        return np.array([oracle.exdot(xf, yf, inca=p, offa=j, incb=q, offb=j, n=n, mode=rmode) for j in range(p)])
    return np.array([[oracle.exdot(xf, yf, inca=p, offa=i, incb=q, offb=j, n=n, mode=rmode) for j in range(q)]
                     for i in range(p)])


def _blocks(oracle, t, n, p, q):
    kind, p0, p1 = KINDS[t % len(KINDS)]
    return (_gen(oracle, kind, p0, p1, n * p, 31 + t).reshape(n, p), _gen(oracle, kind, p0, p1, n * q, 57 + t).reshape(n, q))


@pytest.mark.parametrize("rmode", [0, 1])
def test_random_blocks_vs_oracle(ex, oracle, rmode):
    lib = ex.load_library()
    shapes = [("D", NS[t % len(NS)], k, k) for t, k in enumerate(D_KS)]
    shapes += [("G", NS[(t + 3) % len(NS)], p, q) for t, (p, q) in enumerate(G_PQ)]
    shapes += [("G", 70000, 2, 2), ("D", 70000, 2, 2)]   # the automatic path merges many workgroups per output
    assert {s[1] for s in shapes if s[0] == "D"} >= set(NS) and {s[1] for s in shapes if s[0] == "G"} >= set(NS)
    try:
        lib.exblas_set_round_mode(rmode)
        for t, (mode, n, p, q) in enumerate(shapes):
            X, Y = _blocks(oracle, t + rmode, n, p, q)
            want = _oracle(oracle, X, Y, mode, rmode)
            got = _run(ex, X, Y, mode, off=t % 2)
            _assert_bits(got, want, (mode, n, p, q, KINDS[(t + rmode) % len(KINDS)][0], rmode))
    finally:
        lib.exblas_set_round_mode(0)


def test_outputs_beyond_one_batch(ex, oracle):
    """more than 4096 outputs ('D'), more than 64 x 64 ('G'): batches that share the workspace"""
    X, Y = _blocks(oracle, 1, 5, 4100, 4100)
    _assert_bits(_run(ex, X, Y, "D"), _oracle(oracle, X, Y, "D"), "D 4100")
    X, Y = _blocks(oracle, 2, 4, 70, 66)
    _assert_bits(_run(ex, X, Y, "G"), _oracle(oracle, X, Y, "G"), "G 70 x 66")


@pytest.mark.parametrize("kind", [1, 2])
def test_same_bits_across_variants_paths_and_entries(ex, oracle, kind):
    import torch
    lib = ex.load_library()
    n, p, q = 3001, 7, 7
    X, Y = _blocks(oracle, kind, n, p, q)
    ctx = ex.Context()
    try:
        for rmode in (0, 1):
            lib.exblas_set_round_mode(rmode)
            # the yardstick: exdot_dev on the strided columns, records without product flags
            Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
            ref = np.empty((p, q))
            for i in range(p):
                for j in range(q):
                    rec = ex.read_record(ex.exdot_dev(Xd[:, i], Yd[:, j], incx=p, incy=q, n=n))
                    assert rec.flags & PRODUCT_FLAGS == 0, (i, j, rec.flags)
                    ref[i, j] = rec.refmode if rmode else rec.exact
            _assert_bits(ref, _oracle(oracle, X, Y, "G", rmode), ("exdot_dev vs oracle", rmode))
            for path in (0, 1, 2):
                ex.set_bdot_path(path)
                for fpe, ee in (FPE_VARIANTS_DOT if path == 0 or rmode == 0 else [(8, True)]):
                    what = (kind, rmode, path, fpe, ee)
                    g = _run(ex, X, Y, "G", fpe, ee)
                    _assert_bits(g, ref, ("G", what))
                    _assert_bits(_run(ex, X, Y, "D", fpe, ee), np.diag(ref), ("D vs the diagonal of G", what))
                _assert_bits(_run(ex, X, Y, "G", ctx=ctx), ref, ("ctx G", rmode, path))
                _assert_bits(_run(ex, X, Y, "D", ctx=ctx, off=1), np.diag(ref), ("ctx D", rmode, path))
                _assert_bits(ex.exbdot(X, Y, "G"), ref, ("host G", rmode, path))
                _assert_bits(ex.exbdot(X, Y, "D"), np.diag(ref), ("host D", rmode, path))
                gram = _run(ex, X, None, "G")
                _assert_bits(gram, _run(ex, X, X.copy(), "G"), ("Y=None vs a copy", rmode, path))
                _assert_bits(gram, gram.T, ("X is Y: C == C.T", rmode, path))
                _assert_bits(_run(ex, X, None, "D"), np.diag(gram), ("Y=None, D", rmode, path))
                _assert_bits(ex.exbdot(X), gram, ("host, Y=None", rmode, path))
    finally:
        ex.set_bdot_path(0)
        lib.exblas_set_round_mode(0)
        ctx.destroy()


def test_early_exit_beyond_fpe_8_is_a_silent_return(ex, oracle):
    X, Y = _blocks(oracle, 0, 100, 3, 3)
    got = _run(ex, X, Y, "G", 9, True)
    assert (_bits(got) == _bits(np.array([SENTINEL]))[0]).all()
    _assert_bits(_run(ex, X, Y, "G", 9, False), _oracle(oracle, X, Y, "G"), "fpe 9 without early exit")


@pytest.fixture(scope="module")
def planted_d_blocks():
    cases = D.sample(2048)
    return [D.planted_d(cases[i:i + 64]) for i in range(0, len(cases), 64)]


@pytest.mark.parametrize("path", [0, 1, 2])
def test_planted_roundings_d(ex, planted_d_blocks, path):
    try:
        ex.set_bdot_path(path)
        for b, d in enumerate(planted_d_blocks):
            _assert_bits(_run(ex, d.X, d.Y, "D", off=b % 2), d.want, ("planted_d", b, path))
    finally:
        ex.set_bdot_path(0)


@pytest.mark.parametrize("path", [0, 1, 2])
def test_planted_roundings_g(ex, path):
    cases = D.sample(256)
    kept = 0
    try:
        ex.set_bdot_path(path)
        for b in range(0, len(cases), 64):
            g = D.planted_g(cases[b:b + 64], SHIFTS)
            _assert_bits(_run(ex, g.X, g.Y, "G"), g.want, ("planted_g", b, path), keep=g.keep)
            kept += int(g.keep.sum())
        c = D.integer_blocks(np.random.default_rng(7), 200, 9, 9)
        got = _run(ex, c.X, c.Y, "G")
        _assert_bits(got, c.want, ("integer_blocks", path))
        assert all(_bits(got)[i, j] == 0 for i, j in c.zeros)   # +0.0
        _assert_bits(_run(ex, c.X, c.Y, "D"), np.diag(c.want), ("integer_blocks D", path))
    finally:
        ex.set_bdot_path(0)
    assert kept >= 600


def test_non_finite_values_stay_in_their_column(ex, oracle):
    import torch
    n, p, q = 300, 5, 4
    X0, Y0 = _blocks(oracle, 0, n, p, q)   # fpuniform: positive, so that an infinity keeps its sign in every product
    assert (X0 > 0).all() and (Y0 > 0).all()
    base_g = _run(ex, X0, Y0, "G")
    base_d = _run(ex, X0[:, :q], Y0, "D")

    def exdot_bits(X, Y, i, j):
        Xd, Yd = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
        return ex.read_record(ex.exdot_dev(Xd[:, i], Yd[:, j], incx=X.shape[1], incy=Y.shape[1], n=n)).exact

    for plant in ([np.nan], [np.inf], [-np.inf], [np.inf, -np.inf], [np.inf, np.inf]):
        for side in ("X", "Y"):
            X, Y = X0.copy(), Y0.copy()
            for t, v in enumerate(plant):
                (X if side == "X" else Y)[17 + 150 * t, 2] = v
            g = _run(ex, X, Y, "G")
            touched = np.zeros((p, q), dtype=bool)
            if side == "X":
                touched[2, :] = True
            else:
                touched[:, 2] = True
            _assert_bits(g, base_g, ("untouched outputs", plant, side), keep=~touched)
            want = np.array([[exdot_bits(X, Y, i, j) if touched[i, j] else 0.0 for j in range(q)] for i in range(p)])
            _assert_bits(g, want, ("touched outputs vs exdot_dev", plant, side), keep=touched)
            assert not np.isfinite(g[touched]).any()
            if len(plant) == 2:
                assert np.isnan(g[touched]).all() == (plant[0] != plant[1])
            d = _run(ex, X[:, :q], Y, "D")
            _assert_bits(np.delete(d, 2), np.delete(base_d, 2), ("D untouched", plant, side))
            assert _bits(d)[2] == _bits(np.array([g[2, 2]]))[0]
    # 0 * Inf is NaN, in that output alone
    X, Y = X0.copy(), Y0.copy()
    X[40, 1], Y[40, 3] = 0.0, np.inf
    g = _run(ex, X, Y, "G")
    assert np.isnan(g[1, 3]) and np.isinf(g[[0, 2, 3, 4], 3]).all() and np.isfinite(np.delete(g, 3, axis=1)).all()
    Y[40, 1] = -np.inf
    d = _run(ex, X[:, :q], Y, "D")
    assert np.isnan(d[1]) and np.isposinf(d[3]) and np.isfinite(d[[0, 2]]).all()


def test_degenerate_sizes(ex):
    import torch
    lib = ex.load_library()
    for mode, p, q in (("G", 3, 5), ("D", 70, 70), ("G", 1, 1)):
        got = _run(ex, np.zeros((0, p)), np.zeros((0, q)), mode)
        assert got.shape == ((p, q) if mode == "G" else (p,)) and (_bits(got) == 0).all(), (mode, p, q)   # +0.0
    # p == 0 or q == 0: success, and nothing is written anywhere
    buf = torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda")
    x = torch.ones(64, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.exblas_exbdot_dev(b"G", 8, 0, 3, ptr(x), 0, ptr(x), 3, ptr(buf), 3, 8, 1, st) == 0
    assert lib.exblas_exbdot_dev(b"G", 8, 3, 0, ptr(x), 3, ptr(x), 0, ptr(buf), 0, 8, 1, st) == 0
    assert lib.exblas_exbdot_dev(b"D", 8, 0, 0, ptr(x), 0, ptr(x), 0, ptr(buf), 0, 8, 1, st) == 0
    torch.cuda.synchronize()
    assert (_bits(buf.cpu().numpy()) == _bits(np.array([SENTINEL]))[0]).all()
    assert tuple(ex.exbdot_dev(x.view(8, 8)[:, :0], x.view(8, 8)[:, :3]).shape) == (0, 3)
    assert tuple(ex.exbdot_dev(x.view(8, 8)[:, :0], None, "D").shape) == (0,)


@pytest.mark.parametrize("mode,n,p,q", [("D", 4099, 17, 17), ("G", 1000, 9, 5), ("G", 70000, 2, 2)])
def test_fpe1_error_bound(ex, oracle, mode, n, p, q):
    """plain fp64 on the same structure: |c - exact| <= g sum |x y|, g = (n + 2) u / (1 - (n + 2) u), the bound of any
    summation order with or without FMA"""
    X, Y = _blocks(oracle, 1, n, p, q)
    got = _run(ex, X, Y, mode, 1, False)
    u = Fraction(1, 2 ** 53)
    gam = (n + 2) * u / (1 - (n + 2) * u)
    pairs = [(j, j) for j in range(p)] if mode == "D" else [(i, j) for i in range(p) for j in range(q)]
    if n > 10000:
        pairs = pairs[:2]
    for i, j in pairs:
        prods = [Fraction(float(a)) * Fraction(float(b)) for a, b in zip(X[:, i], Y[:, j])]
        c = got[j] if mode == "D" else got[i, j]
        assert abs(Fraction(float(c)) - sum(prods)) <= gam * sum(abs(v) for v in prods), (mode, i, j)


def test_graph_capture(ex, oracle):
    """(Four replays on new data, several batches and ExGEMV's sums over the same bytes between replays:
    tests/test_gpu_graph_replay_solves.py.)"""
    import torch
    n, p, q = 5000, 6, 5
    X, Y = _blocks(oracle, 1, n, p, q)
    Xd, Yd = _padded(X, 3, 1), _padded(Y, 1, 0)
    out = torch.zeros((p, q), dtype=torch.float64, device="cuda")
    dout = torch.zeros(q, dtype=torch.float64, device="cuda")
    ex.exbdot_dev(Xd, Yd, "G", out)   # warm-up: sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exbdot_dev(Xd, Yd, "G", out)
            ex.exbdot_dev(Xd[:, :q], Yd, "D", dout)
    other = ex.Context()
    X2, Y2 = _blocks(oracle, 2, n, p, q)
    try:
        for rep, (Xn, Yn) in enumerate(((X2, Y2), (Y2[:, [0, 1, 2, 3, 4, 0]] * 0.5, X2[:, :q]))):
            Xd.copy_(torch.from_numpy(np.ascontiguousarray(Xn)).cuda())
            Yd.copy_(torch.from_numpy(np.ascontiguousarray(Yn)).cuda())
            out.fill_(SENTINEL)
            torch.cuda.synchronize()
            g.replay()
            # a second context's call between the replays uses its own workspace
            side = other.exbdot(torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda(), "G")
            torch.cuda.synchronize()
            _assert_bits(out.cpu().numpy(), _oracle(oracle, Xn, Yn, "G"), ("replay G", rep))
            _assert_bits(dout.cpu().numpy(), _oracle(oracle, Xn[:, :q], Yn, "D"), ("replay D", rep))
            _assert_bits(side.cpu().numpy(), _oracle(oracle, X, Y, "G"), ("the other context", rep))
    finally:
        other.destroy()
