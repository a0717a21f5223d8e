"""Captured graphs replayed four times on new data, at the sizes at which a captured clear has been lost before, and a
census of what every device routine puts into a graph.

The replays.  `replay_four` makes one warm call, captures on a side stream and replays four times.  Before a replay new
inputs are copied into the captured buffers; after it the output is compared, bit for bit, with values that never come
from the library: the CPU oracle, or the Python integers of tests/blas1_cases.py.  Between the replays the context is
used in ways that leave its workspace dirty, so that a clear which did not happen cannot pass by luck:

    replay 0 | eager call, default context, same shape, other data, fpe = 0 | replay 1 | call on a second Context |
    replay 2 | replay 3

A routine that updates its output in place (y of ExGEMV with beta = 1, x of ExTRSV) is handed its input there, which
no result equals; every other output is filled with -1.

The census.  `test_node_census` captures every device routine once with the HIP runtime's own capture calls, counts
the nodes of the graph by kind and holds them to CENSUS: no routine puts a memset node into a graph, and none may start
to (on this stack graphs with memset nodes lost the clear, or faulted, on a replay).

The mailbox solves with several right-hand sides (ExTRSM, ExSpTRSV, ExSpTRSM) and ExBDOT have the same protocol in
tests/test_gpu_graph_replay_solves.py."""
import ctypes as C
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

from helpers import assert_bits, bits, digits_from_int, exact_int_from_canon, exact_int_from_digits, same_double

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    return exblas_amd


def _oracle():
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def replay_four(warm, body, load, check, eager=None, other=None):
    """warm(): the call that sizes the workspace; body(): the captured calls; load(r): new inputs for replay r;
    check(r): its outputs; eager(): the default context's call after replay 0; other(): a second context's after 1"""
    import torch
    warm()
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            body()
    for r in range(4):
        load(r)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        check(r)
        if r == 0 and eager is not None:
            eager()
        if r == 1 and other is not None:
            other()
        torch.cuda.synchronize()
    del g


# ---------------------------------------------------------------------------------------------
# ExGEMV: 'N' clears 576 m bytes (and the tickets) before it adds to them (k_gemv_zero; a memset node until this file
# found a replay of it ending in a memory access fault); 'T' clears nothing
# ---------------------------------------------------------------------------------------------
GEMV_SHAPES = [(4096, 130, 4096), (4097, 70, 4099), (32768, 64, 32768)]   # 2.25 MiB, odd (no vector kernel), 18 MiB
GEMV_VARIANTS = [(0, False, "narrow"), (3, False, "wide"), (8, True, "narrow")]
WIDE = (("fpuniform_signed", 600, 300), ("lognormal", 0.0, 50.0))          # the small expansions spill on these


@functools.lru_cache(maxsize=None)
def _gemv_sets(trans, m, n, lda, family):
    """six (a, x, y0, want): the four replays, the eager call, the second context's call -- all data differ"""
    O = _oracle()
    rows, inner = (n, m) if trans == "T" else (m, n)
    out = []
    for r in range(6):
        kind, p0, p1 = WIDE[r % 2] if family == "wide" else ("fpuniform_signed", 10, 0)
        seed = 7000 + 10 * r + m % 97
        a = O.gen(kind, lda * n, seed, p0, p1)
        x = O.gen("fpuniform_signed", inner, seed + 1, 20, 10)
        y0 = O.gen("fpuniform_signed", rows, seed + 2, 20, 10)
        want = O.exgemv(trans, m, n, 1.0, a, lda, x, 1.0, y0, 0)
        assert np.isfinite(want).all() and (bits(want) != bits(y0)).any()
        out.append((a, x, y0, want))
    return out


def _gemv_replays(ex, trans, m, n, lda, fpe, ee, family):
    import torch
    sets = _gemv_sets(trans, m, n, lda, family)
    rows, inner = (n, m) if trans == "T" else (m, n)
    new = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")  # noqa: E731
    cap, side = (new(lda * n), new(inner), new(rows)), (new(lda * n), new(inner), new(rows))
    ctx2 = ex.Context()

    def put(i, bufs):
        for t, h in zip(bufs, sets[i][:3]):
            t.copy_(torch.from_numpy(h))

    def call(f, bufs, fpe, ee):
        f(trans, m, n, 1.0, bufs[0], lda, bufs[1], 1.0, bufs[2], fpe, ee)

    def aside(i, f, fpe, ee):
        put(i, side)
        call(f, side, fpe, ee)
        assert_bits(side[2].cpu().numpy(), sets[i][3], (trans, m, n, fpe, ee, "beside the graph", i))

    put(0, cap)
    try:
        replay_four(lambda: call(ex.exgemv_dev, cap, fpe, ee), lambda: call(ex.exgemv_dev, cap, fpe, ee),
                    lambda r: put(r, cap),
                    lambda r: assert_bits(cap[2].cpu().numpy(), sets[r][3], (trans, m, n, fpe, ee, "replay", r)),
                    lambda: aside(4, ex.exgemv_dev, 0, False), lambda: aside(5, ctx2.exgemv, fpe, ee))
    finally:
        ctx2.destroy()


@pytest.mark.parametrize("fpe,ee,family", GEMV_VARIANTS, ids=lambda v: str(v))
@pytest.mark.parametrize("m,n,lda", GEMV_SHAPES)
def test_exgemv_n_replays(ex, m, n, lda, fpe, ee, family):
    """(0, False): every product passes through the cleared accumulators, a stale set doubles the row; (3, False) on
    wide-range data: tiles spill into them; (8, True): the shipped default."""
    _gemv_replays(ex, "N", m, n, lda, fpe, ee, family)


@pytest.mark.parametrize("fpe,ee,family", GEMV_VARIANTS, ids=lambda v: str(v))
def test_exgemv_t_replays(ex, fpe, ee, family):
    """the control: 'T' has nothing to clear"""
    _gemv_replays(ex, "T", 4096, 130, 4096, fpe, ee, family)


# ---------------------------------------------------------------------------------------------
# two graphs on one context whose clears cover the same 2.25 MiB of its workspace
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gram_sets(n, p):
    O = _oracle()
    out = []
    for r in range(2):
        X = O.gen("fpuniform_signed", n * p, 7300 + r, 20, 10).reshape(n, p)
        Xt = np.ascontiguousarray(X.T)
        G = np.empty((p, p))
        for i in range(p):
            for j in range(i, p):
                G[i, j] = G[j, i] = O.exdot(Xt[i], Xt[j], 0)
        out.append((X, G))
    return out


def test_two_graphs_alternate_on_one_context(ex):
    """A: ExGEMV 'N' fpe = 0 at m = 4096 (k_gemv_zero over the workspace's first 2.25 MiB); B: ExBDOT 'G' at p = 64,
    n = 1000 (k_bdot_zero over the same bytes).  A, B, A, B: each finds what the other left."""
    import torch
    m, n, lda = GEMV_SHAPES[0]
    gv, gr = _gemv_sets("N", m, n, lda, "narrow"), _gram_sets(1000, 64)
    a, x, y = (torch.empty(k, dtype=torch.float64, device="cuda") for k in (lda * n, n, m))
    X = torch.empty((1000, 64), dtype=torch.float64, device="cuda")
    G = torch.empty((64, 64), dtype=torch.float64, device="cuda")

    def put(r):
        for t, h in zip((a, x, y), gv[r][:3]):
            t.copy_(torch.from_numpy(h))
        X.copy_(torch.from_numpy(gr[r][0]))
        G.fill_(-1.0)

    put(0)
    ex.exgemv_dev("N", m, n, 1.0, a, lda, x, 1.0, y, 0, False)
    ex.exbdot_dev(X, out=G)
    torch.cuda.synchronize()
    s, ga, gb = torch.cuda.Stream(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(ga, stream=s):
            ex.exgemv_dev("N", m, n, 1.0, a, lda, x, 1.0, y, 0, False)
        with torch.cuda.graph(gb, stream=s):
            ex.exbdot_dev(X, out=G)
    for r in range(2):
        put(r)
        torch.cuda.synchronize()
        ga.replay()
        torch.cuda.synchronize()
        assert_bits(y.cpu().numpy(), gv[r][3], ("A", r))
        gb.replay()
        torch.cuda.synchronize()
        assert_bits(G.cpu().numpy(), gr[r][1], ("B", r))
    del ga, gb


# ---------------------------------------------------------------------------------------------
# ExTRSV: the ticket word to zero and the mailbox (8 n bytes) to all-ones before every solve (k_trsv_preset)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _trsv_sets(uplo, trans, n):
    """two triangles and six right-hand sides: replays 0, 1 on triangle 0, replays 2, 3 on triangle 1, the eager call on
    triangle 1 and the second context's on triangle 0; (triangles, [(triangle index, b, want)])"""
    from test_gpu_trsv import tri_system
    O = _oracle()
    tris = [tri_system(O, uplo, n, 7500 + 3 * t, dominant=True)[0] for t in range(2)]
    out = []
    for r, t in enumerate((0, 0, 1, 1, 1, 0)):
        b = O.gen("fpuniform_signed", n, 7520 + r, 10, 0)
        rc, want = O.extrsv(uplo, trans, "N", n, tris[t], n, b, 0)
        assert rc == 0 and np.isfinite(want).all() and (bits(want) != bits(b)).any()
        out.append((t, b, want))
    return tris, out


@pytest.mark.parametrize("fpe,ee", [(0, False), (8, True)])
@pytest.mark.parametrize("n", [700, 2048])
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("U", "T")])
def test_extrsv_replays(ex, uplo, trans, n, fpe, ee):
    """With changed data a mailbox that was not reset to all-ones hands a consumer the previous solve's x: the eager
    solve between replays 0 and 1 is on the other triangle, and the triangle changes again at replay 2."""
    import torch
    tris, sets = _trsv_sets(uplo, trans, n)
    dt = [_cuda(t) for t in tris]
    a = dt[0].clone()
    x, xs = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
    ctx2 = ex.Context()

    def put(r):
        a.copy_(dt[sets[r][0]])
        x.copy_(torch.from_numpy(sets[r][1]))

    def aside(i, f, fpe, ee):
        xs.copy_(torch.from_numpy(sets[i][1]))
        assert f(uplo, trans, "N", n, dt[sets[i][0]], n, xs, fpe, ee) == 0
        assert_bits(xs.cpu().numpy(), sets[i][2], (uplo, trans, n, fpe, ee, "beside the graph", i))

    put(0)
    try:
        replay_four(lambda: ex.extrsv_dev(uplo, trans, "N", n, a, n, x, fpe, ee),
                    lambda: ex.extrsv_dev(uplo, trans, "N", n, a, n, x, fpe, ee), put,
                    lambda r: assert_bits(x.cpu().numpy(), sets[r][2], (uplo, trans, n, fpe, ee, "replay", r)),
                    lambda: aside(4, ex.extrsv_dev, 0, False), lambda: aside(5, ctx2.extrsv, fpe, ee))
    finally:
        ctx2.destroy()


# ---------------------------------------------------------------------------------------------
# ExSUM + ExDOT in one graph: the finalize leaves the sets, the flags and the low / high accumulators zeroed
# ---------------------------------------------------------------------------------------------
SUMDOT_N = (1 << 16) + 2


def _embed(case_vals, at, even, odd):
    """a vector of SUMDOT_N entries: the case's values, in order, at the even position `at`, among pairs (even[i],
    odd[i]) and a trailing zero -- pairs (v, -v) cancel exactly, alone or against pairs (w, w) of the other operand"""
    k = SUMDOT_N - len(case_vals)
    rest = np.zeros(k)
    rest[0:2 * (k // 2):2] = even[:k // 2]
    rest[1:2 * (k // 2):2] = odd[:k // 2]
    assert at % 2 == 0
    return np.concatenate([rest[:at], case_vals, rest[at:]])


@functools.lru_cache(maxsize=None)
def _sumdot_sets():
    """six (xs, xd, yd, expected of the sum, expected of the dot); an expected record is a dict of the fields that are
    compared.  Index 1: a Family D sum (the running total passes 2^1024 and comes back) and a Family F dot whose
    products leave the double range on both sides (all four product flags), among terms that cancel exactly; the rest
    plain."""
    import blas1_cases as B
    O = _oracle()
    n = SUMDOT_N
    out = []
    for r in range(6):
        if r == 1:
            d = next(c for c in B.family_d() if c.kind == "16385 x DBL_MAX, 16384 back, A tie" and c.want > 0)
            f = next(c for c in B.family_f_high() if c.kind == "cancel onto A:tie+1 p=2096" and c.want > 0)
            assert f.flags == 120 and f.exact * B.ONE == int(f.exact * B.ONE)
            pad = O.gen("fpuniform_signed", n, 7600, 10, 0)
            w = O.gen("fpuniform_signed", n, 7601, 10, 0)
            xs = _embed(np.array(d.terms), 1000, pad, -pad)
            xd, yd = _embed(f.a, 2000, pad, -pad), _embed(f.b, 2000, w, w)
            assert sum(Fraction(v) for v in xs) == Fraction(d.T, B.ONE)
            assert sum(Fraction(u) * Fraction(v) for u, v in zip(xd, yd)) == f.exact
            canon = B.canon_from_int(d.T)
            es = dict(exact=d.want, refmode=O.round_limbs(canon, O.ROUND_REFERENCE), canon=canon,
                      digits=digits_from_int(d.T), flags=0)
            ed = dict(exact=f.want, flags=f.flags)
        else:
            xs = O.gen("ill_cond", n, 7610 + r, 1e32)
            xd, yd = O.gen("lognormal", n, 7620 + r, 0.0, 2.0), O.gen("lognormal", n, 7630 + r, 0.0, 2.0)
            v, l = O.exsum_omp(xs, 8, True, 4, limbs=True)
            es = dict(exact=v, refmode=O.round_limbs(l, O.ROUND_REFERENCE), canon=l, flags=0)
            v, l = O.exdot_omp(xd, yd, 8, True, 4, limbs=True)
            ed = dict(exact=v, refmode=O.round_limbs(l, O.ROUND_REFERENCE), canon=l, flags=0)
        out.append((xs, xd, yd, es, ed))
    return out


def _check_record(ex, rec_tensor, want, what):
    rec = ex.read_record(rec_tensor)
    assert same_double(rec.exact, want["exact"]), (what, rec.exact, want["exact"])
    assert rec.flags == want["flags"], (what, rec.flags, want["flags"])
    if "canon" in want:
        assert (rec.canon == want["canon"]).all(), (what, "canonical limbs",
                                                    np.nonzero(rec.canon != want["canon"])[0][:5])
        assert same_double(rec.refmode, want["refmode"]), (what, rec.refmode, want["refmode"])
        assert exact_int_from_digits(rec.digits) << 18 == exact_int_from_canon(rec.canon), (what, "digits")
    if "digits" in want:
        assert (rec.digits == want["digits"]).all(), (what, "digits")


@pytest.mark.parametrize("fpe,ee", [(0, False), (8, True)])
def test_exsum_exdot_replays(ex, fpe, ee):
    """plain data, data that leaves the double range (range flags, low / high accumulators), plain data again: the
    second and later finalizes under the graph find sets, flags and extension sets as clean as the first did"""
    import torch
    sets = _sumdot_sets()
    n = SUMDOT_N
    new = lambda: torch.empty(n, dtype=torch.float64, device="cuda")  # noqa: E731
    cap, side = (new(), new(), new()), (new(), new(), new())
    rs, rd, rs2, rd2 = (ex.new_record_buffer() for _ in range(4))
    ctx2, default = ex.Context(), SimpleNamespace(exsum=ex.exsum_dev, exdot=ex.exdot_dev)

    def put(i, bufs):
        for t, h in zip(bufs, sets[i][:3]):
            t.copy_(torch.from_numpy(h))

    def load(r):
        put(r, cap)
        rs.fill_(-1)
        rd.fill_(-1)

    def body():
        ex.exsum_dev(cap[0], fpe, ee, out=rs)
        ex.exdot_dev(cap[1], cap[2], fpe, ee, out=rd)

    def check(r):
        _check_record(ex, rs, sets[r][3], ("exsum", fpe, ee, "replay", r))
        _check_record(ex, rd, sets[r][4], ("exdot", fpe, ee, "replay", r))

    def aside(i, c, fpe, ee):
        put(i, side)
        c.exsum(side[0], fpe, ee, out=rs2)
        c.exdot(side[1], side[2], fpe, ee, out=rd2)
        _check_record(ex, rs2, sets[i][3], ("exsum", fpe, ee, "beside the graph", i))
        _check_record(ex, rd2, sets[i][4], ("exdot", fpe, ee, "beside the graph", i))

    put(0, cap)
    try:
        replay_four(body, body, load, check, lambda: aside(4, default, 0, False), lambda: aside(5, ctx2, fpe, ee))
    finally:
        ctx2.destroy()


# ---------------------------------------------------------------------------------------------
# segmented ExSUM, unsupported variant: the call only clears `out`
# ---------------------------------------------------------------------------------------------
def test_exsum_segmented_unsupported_variant_replays(ex):
    """nseg = 300000: 2.3 MiB to clear.  (fpe = 9 with early exit has no summing kernel: every segment reads 0.0.)"""
    import torch
    O = _oracle()
    nseg = 300000
    vals = O.gen("lognormal", nseg, 7700, 0.0, 2.0)
    dv, do = _cuda(vals), torch.arange(nseg + 1, dtype=torch.int64, device="cuda")
    out = torch.empty(nseg, dtype=torch.float64, device="cuda")
    out2 = torch.empty(nseg, dtype=torch.float64, device="cuda")

    def check(r):
        got = out.cpu().numpy()
        assert (bits(got) == 0).all(), (r, int((bits(got) != 0).sum()), got[bits(got) != 0][:5])

    def eager():   # one element per segment: the sum is the element
        ex.exsum_segmented_dev(dv, do, 0, False, out=out2)
        assert_bits(out2.cpu().numpy(), vals, "supported variant beside the graph")

    replay_four(lambda: ex.exsum_segmented_dev(dv, do, 9, True, out=out),
                lambda: ex.exsum_segmented_dev(dv, do, 9, True, out=out), lambda r: out.fill_(-1.0), check, eager)


# ---------------------------------------------------------------------------------------------
# ExSpMV / ExSpMM: the header is cleared before the first kernel counts into it; the two matrices of their own graph
# tests, alternated
# ---------------------------------------------------------------------------------------------
SP_M, SP_N, SP_K = 2000, 1800, 12


@functools.lru_cache(maxsize=None)
def _sparse_pair():
    """(nnz, [(crow, col)] x 2, val): short rows, then one long row with many medium and empty ones, same nnz"""
    rng = np.random.default_rng(4)
    lens = rng.choice([3, 27, 60], size=SP_M)
    crow = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(crow[-1])
    col = rng.integers(0, SP_N, size=nnz)
    lens2 = np.zeros(SP_M, dtype=np.int64)
    lens2[5] = nnz - 90 * 100
    lens2[100:190] = 100
    crow2 = np.concatenate([[0], np.cumsum(lens2)]).astype(np.int64)
    col2 = rng.integers(0, SP_N, size=nnz)
    return nnz, [(crow, col), (crow2, col2)], _oracle().gen("fpuniform", nnz, 71, 10, 0)


def _sparse_want(crow, col, val, X):
    """output (i, j) = the oracle's ExGEMV 'N' on the 1 x len_i matrix of row i against the gathered X[:, j]"""
    O = _oracle()
    Xt = np.ascontiguousarray(X.T)
    out = np.zeros((len(crow) - 1, X.shape[1]))
    zero = np.zeros(1)
    for i in range(len(crow) - 1):
        a, b = int(crow[i]), int(crow[i + 1])
        if b > a:
            for j in range(X.shape[1]):
                out[i, j] = O.exgemv("N", 1, b - a, 1.0, val[a:b], 1, Xt[j, col[a:b]], 0.0, zero, 0)[0]
    return out


@functools.lru_cache(maxsize=None)
def _sparse_sets(k):
    """six (matrix index, X [n, k], want or None): the four replays alternate the matrices; the two calls beside the
    graph take the other matrix of their neighbours and are not compared"""
    O = _oracle()
    _, mats, val = _sparse_pair()
    out = []
    for r, t in enumerate((0, 1, 0, 1, 1, 0)):
        X = O.gen("lognormal", SP_N * k, 7800 + r, 0.0, 5.0).reshape(SP_N, k)
        out.append((t, X, _sparse_want(*mats[t], val, X) if r < 4 else None))
    return out


def _sparse_replays(ex, k):
    import torch
    nnz, mats, val = _sparse_pair()
    sets = _sparse_sets(k or 1)
    dm = [(_cuda(cr), _cuda(co)) for cr, co in mats]
    crow, col, dval = dm[0][0].clone(), dm[0][1].clone(), _cuda(val)
    shape = (SP_N,) if k == 0 else (SP_N, k)
    oshape = (SP_M,) if k == 0 else (SP_M, k)
    X, Xs = (torch.empty(shape, dtype=torch.float64, device="cuda") for _ in range(2))
    Y, Ys = (torch.empty(oshape, dtype=torch.float64, device="cuda") for _ in range(2))
    A = (crow, col, dval, (SP_M, SP_N))
    ctx2 = ex.Context()
    dev, other = (ex.exspmv_dev, ctx2.exspmv) if k == 0 else (ex.exspmm_dev, ctx2.exspmm)

    def load(r):
        crow.copy_(dm[sets[r][0]][0])
        col.copy_(dm[sets[r][0]][1])
        X.copy_(torch.from_numpy(sets[r][1]).reshape(shape))
        Y.fill_(-1.0)

    def aside(i, f, fpe, ee):
        Xs.copy_(torch.from_numpy(sets[i][1]).reshape(shape))
        f((*dm[sets[i][0]], dval, (SP_M, SP_N)), Xs, 1.0, 0.0, Ys, fpe, ee)

    load(0)
    try:
        replay_four(lambda: dev(A, X, 1.0, 0.0, Y), lambda: dev(A, X, 1.0, 0.0, Y), load,
                    lambda r: assert_bits(Y.cpu().numpy().reshape(SP_M, -1), sets[r][2], ("k", k, "replay", r)),
                    lambda: aside(4, dev, 0, False), lambda: aside(5, other, 8, True))
    finally:
        ctx2.destroy()


def test_exspmv_replays(ex):
    _sparse_replays(ex, 0)


def test_exspmm_replays(ex):
    _sparse_replays(ex, SP_K)


# ---------------------------------------------------------------------------------------------
# the node census
# ---------------------------------------------------------------------------------------------
NODE_KINDS = {0: "kernel", 1: "memcpy", 2: "memset"}       # hipGraphNodeType; anything else is reported by number

# What one call of each routine puts into a graph: (kernel nodes, memset nodes), nothing else.  DESIGN.md 5c-2 holds
# the same table.  Every row is kernel nodes only and must stay that way: clear in a kernel (5f, 5m, 5c-2).
CENSUS = {
    "exsum_dev": (2, 0),
    "exdot_dev": (2, 0),
    "exsum_segmented_dev": (1, 0),
    "exsum_segmented_dev, unsupported variant": (1, 0),
    "exgemv_dev N, fpe 8, even m and lda": (4, 0),
    "exgemv_dev N, fpe 8, odd m": (3, 0),
    "exgemv_dev N, fpe 0": (3, 0),
    "exgemv_dev T": (2, 0),
    "extrsv_dev": (2, 0),
    "extrsm_dev": (2, 0),
    "extrsm_dev, path 3, k = 9": (6, 0),           # three panels of 4, 4, 1 columns: a preset and a solve kernel each
    "exgemm_dev, digit-slice shape": (19, 0),      # 130 x 75 x 200; the scan, the decision, slices, passes, the finish
    "exgemm_dev, residue shape": (11, 0),          # 200 x 260 x 96
    "exspmv_dev": (7, 0),
    "exspmm_dev": (8, 0),
    "exsptrsv_dev": (2, 0),
    "exsptrsm_dev": (2, 0),
    "exsptrsm_dev, path 3, k = 9": (6, 0),         # three panels
    "exbdot_dev": (3, 0),
    "exbdot_dev G, 65 x 65": (12, 0),              # batches of 64 x 64, 64 x 1, 1 x 64 and 1 x 1 outputs, three kernels each
    "exbdot_export_dev": (3, 0),
    "exbdot_round_dev": (1, 0),
    "exbgemm_dev": (1, 0),
    "exbtrsm_dev": (1, 0),
    "expotrf_dev": (1, 0),
    "excholqr_dev": (6, 0),          # ExBDOT 3, ExPOTRF 1, ExBTRSM 1, and torch's fill of the info word it allocates
}


def _hip_runtime():
    """the libamdhip64 this process has already loaded (torch's), not a second one"""
    with open("/proc/self/maps") as fh:
        paths = {line.split()[-1] for line in fh if "libamdhip64" in line}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    vp = C.c_void_p
    hip.hipStreamBeginCapture.argtypes = [vp, C.c_int]
    hip.hipStreamEndCapture.argtypes = [vp, C.POINTER(vp)]
    hip.hipGraphGetNodes.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [vp, C.POINTER(C.c_int)]
    hip.hipGraphDestroy.argtypes = [vp]
    return hip


def _count_nodes(hip, stream, fn):
    """captures fn() on `stream` (the current one), counts the graph's nodes by kind and destroys the graph"""
    graph = C.c_void_p()
    assert hip.hipStreamBeginCapture(stream.cuda_stream, 2) == 0          # hipStreamCaptureModeRelaxed
    try:
        fn()
    finally:
        rc = hip.hipStreamEndCapture(stream.cuda_stream, C.byref(graph))
    assert rc == 0 and graph.value, rc
    try:
        count = C.c_size_t(0)
        assert hip.hipGraphGetNodes(graph, None, C.byref(count)) == 0
        nodes = (C.c_void_p * max(count.value, 1))()
        assert hip.hipGraphGetNodes(graph, nodes, C.byref(count)) == 0
        kinds = {}
        for i in range(count.value):
            t = C.c_int(-1)
            assert hip.hipGraphNodeGetType(nodes[i], C.byref(t)) == 0
            name = NODE_KINDS.get(t.value, t.value)
            kinds[name] = kinds.get(name, 0) + 1
        return kinds
    finally:
        assert hip.hipGraphDestroy(graph) == 0


def _on_path_3(set_path, fn):
    """fn() with the routine's path knob at 3 (panels and tiles of 4 columns), the knob restored"""
    def call():
        set_path(3)
        try:
            fn()
        finally:
            set_path(0)
    return call


def _census_calls(ex):
    """{row of CENSUS: a call with every output preallocated}, small shapes, plain data"""
    import torch
    O = _oracle()
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    gen = lambda k, seed: _cuda(O.gen("fpuniform_signed", k, seed, 10, 0))  # noqa: E731
    calls = {}
    x, y, rec = gen(100003, 1), gen(100003, 2), ex.new_record_buffer()
    calls["exsum_dev"] = lambda: ex.exsum_dev(x, 8, True, out=rec)
    calls["exdot_dev"] = lambda: ex.exdot_dev(x, y, 8, True, out=rec)
    offs, seg = torch.arange(0, 100001, 100, dtype=torch.int64, device="cuda"), f64(1000)
    calls["exsum_segmented_dev"] = lambda: ex.exsum_segmented_dev(x, offs, 8, True, out=seg)
    calls["exsum_segmented_dev, unsupported variant"] = lambda: ex.exsum_segmented_dev(x, offs, 9, True, out=seg)
    a, v, w = gen(259 * 257, 3), gen(257, 4), gen(257, 5)
    calls["exgemv_dev N, fpe 8, even m and lda"] = lambda: ex.exgemv_dev("N", 256, 64, 1.0, a, 256, v, 1.0, w, 8, True)
    calls["exgemv_dev N, fpe 8, odd m"] = lambda: ex.exgemv_dev("N", 257, 64, 1.0, a, 259, v, 1.0, w, 8, True)
    calls["exgemv_dev N, fpe 0"] = lambda: ex.exgemv_dev("N", 256, 64, 1.0, a, 256, v, 1.0, w, 0, False)
    calls["exgemv_dev T"] = lambda: ex.exgemv_dev("T", 256, 64, 1.0, a, 256, v, 1.0, w, 8, True)
    # a lower triangle with a dominant diagonal, dense (n = 200) and as CSR
    n = 200
    L = np.tril(O.gen("fpuniform_signed", n * n, 6, 6, -9).reshape(n, n), -1) + np.diag(O.gen("fpuniform", n, 7, 1, 0))
    dl, b, B = _cuda(L), gen(n, 8), gen(n * 8, 9).reshape(n, 8)
    calls["extrsv_dev"] = lambda: ex.extrsv_dev("U", "T", "N", n, dl, n, b, 8, True)     # (row-major L: column-major U)
    calls["extrsm_dev"] = lambda: ex.extrsm_dev(dl, B, "L", "N")
    B9 = gen(n * 9, 15).reshape(n, 9)
    calls["extrsm_dev, path 3, k = 9"] = _on_path_3(ex.set_trsm_path, lambda: ex.extrsm_dev(dl, B9, "L", "N"))
    nz = np.nonzero(L)
    crow = np.concatenate([[0], np.cumsum(np.bincount(nz[0], minlength=n))]).astype(np.int64)
    S = (_cuda(crow), _cuda(nz[1].astype(np.int64)), _cuda(L[nz]), (n, n))
    sy, sY = f64(n), f64(n, 8)
    calls["exspmv_dev"] = lambda: ex.exspmv_dev(S, b, 1.0, 0.0, sy)
    calls["exspmm_dev"] = lambda: ex.exspmm_dev(S, B, 1.0, 0.0, sY)
    calls["exsptrsv_dev"] = lambda: ex.exsptrsv_dev(S, b, "L", "N")
    calls["exsptrsm_dev"] = lambda: ex.exsptrsm_dev(S, B, "L", "N")
    calls["exsptrsm_dev, path 3, k = 9"] = _on_path_3(ex.set_sptrsm_path, lambda: ex.exsptrsm_dev(S, B9, "L", "N"))
    # the two shapes of the smoke run: digit slices, and from 192 x 192 up the residue path
    for name, (m, k, q) in (("digit-slice", (130, 200, 75)), ("residue", (200, 96, 260))):
        ga, gb = _cuda(O.gen("fpuniform", m * k, 10, 10, 0)), _cuda(O.gen("fpuniform", k * q, 11, 10, 0))
        gc = f64(m * q)
        calls[f"exgemm_dev, {name} shape"] = (lambda m=m, k=k, q=q, ga=ga, gb=gb, gc=gc:
                                              ex.exgemm_dev("N", "N", m, q, k, 1.0, ga, k, gb, q, 0.0, gc, q, 8, True))
    X, Cm, Yb = gen(1000 * 8, 12).reshape(1000, 8), gen(64, 13).reshape(8, 8), f64(1000, 8)
    G, sets = f64(8, 8), torch.empty((64, 72), dtype=torch.int64, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    calls["exbdot_dev"] = lambda: ex.exbdot_dev(X, out=G)
    X65, G65 = gen(1000 * 65, 16).reshape(1000, 65), f64(65, 65)
    calls["exbdot_dev G, 65 x 65"] = lambda: ex.exbdot_dev(X65, out=G65)
    calls["exbdot_export_dev"] = lambda: ex.exbdot_export_dev(X, sets=sets)
    calls["exbdot_round_dev"] = lambda: ex.exbdot_round_dev(sets, "G", 8, 8, out=G)
    calls["exbgemm_dev"] = lambda: ex.exbgemm_dev(X, Cm, 1.0, 0.0, Yb)
    R = _cuda(np.triu(O.gen("fpuniform", 64, 14, 1, 0).reshape(8, 8)) + 8 * np.eye(8))
    P = _cuda(np.eye(8) * 4 + 0.25)                      # (factored again and again, in place: only the nodes count)
    Xq, Pq = X.clone(), P
    calls["exbtrsm_dev"] = lambda: ex.exbtrsm_dev(R, Xq, "U", "N")
    calls["expotrf_dev"] = lambda: ex.expotrf_dev(Pq, "U", info=info)
    Xc = X.clone()
    calls["excholqr_dev"] = lambda: ex.excholqr_dev(Xc)
    return calls


def test_node_census(ex):
    """Each routine captured once after a warm call; the counts by kind against CENSUS.  Nothing is replayed."""
    import torch
    hip = _hip_runtime()
    calls = _census_calls(ex)
    assert set(calls) == set(CENSUS)
    s = torch.cuda.Stream()
    got = {}
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for name, fn in calls.items():
            fn()                                   # sizes the workspace, and leaves torch's allocator what fn allocates
            s.synchronize()
            got[name] = _count_nodes(hip, s, fn)
            s.synchronize()
    torch.cuda.synchronize()
    want = {name: {k: c for k, c in (("kernel", kn), ("memset", ms)) if c} for name, (kn, ms) in CENSUS.items()}
    for name in CENSUS:
        print(f"{name:45s} {got[name]}")
    wrong = {name: (got[name], want[name]) for name in CENSUS if got[name] != want[name]}
    assert not wrong, wrong
