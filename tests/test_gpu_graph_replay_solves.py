"""Captured graphs of the routines that carry the most state between their kernels -- the mailbox solves ExTRSM, ExSpTRSV
and ExSpTRSM (sptrs_common.hip.h: per column panel a preset of the ticket, the mailbox and, in the first panel only, the
counters and the watchdog flag) and ExBDOT (per batch of 64 x 64 outputs a zeroing, an accumulate and a finalize kernel
over one workspace block) -- held to the protocol of tests/test_gpu_graph_replay.py:

    replay 0 | eager call, default context, same shape, other data, fpe = 0 | replay 1 | call on a second Context |
    replay 2 | replay 3

The solves change the TRIANGLE as well as the right-hand side: replays 0 and 1 run on triangle 0, replays 2 and 3 on
triangle 1 (for the sparse ones another sparsity pattern, copied over the captured crow / col / val), the eager call on
triangle 1 in the other orientation, the second context's call on triangle 0.  After every replay: every bit of X, the
padding of a wider X, and the counters of last_*_info, which must hold for that replay alone.  Then a graph that goes on
replaying after its context's workspace has grown (the block it was captured in is parked, not freed), and graphs
captured as the FIRST call of a context that only reserved the documented byte count.

Expected bits never come from the library: tests/graph_replay_cases.py (trsv_exact, the planted systems, the planted
ExBDOT pairs, the CPU oracle's ExDOT per output); tests/test_graph_replay_cases.py runs its builders without a GPU.
profiles/graph_replay_mutations.md, section 5: the one-line changes that lose a clear under capture only, and the test
of this file that fails on each."""
import numpy as np
import pytest

import exact_cases as X
import graph_replay_cases as G
from helpers import assert_bits, bits
from test_gpu_graph_replay import _cuda, _gemv_sets, replay_four

pytestmark = pytest.mark.gpu

VARIANTS = [(8, True), (0, False)]
SENTINEL, PAD = -7.25, 3
BLOCK_SHAPES = [(65, 0), (9, 3)]     # (k, path): two column tiles in one panel; on path 3 three panels of 4, 4, 1 columns
MAILBOX_BYTES = 64 << 20             # EXBLAS_TRSM_MAILBOX_BYTES, EXBLAS_SPTRSM_MAILBOX_BYTES
BDOT_WORKSPACE_BYTES = 4096 * 576    # EXBLAS_BDOT_WORKSPACE_BYTES


def documented_workspace_bytes(routine, n=0, k=1):
    """include/exblas_hip.h: 256 + 8 n for ExSpTRSV; 256 + 8 n min(k, P) for ExSpTRSM and ExTRSM, P the largest multiple
    of 64 with 8 n P within the mailbox budget, at least 64; EXBLAS_BDOT_WORKSPACE_BYTES for ExBDOT whatever the sizes"""
    if routine == "bdot":
        return BDOT_WORKSPACE_BYTES
    if routine == "sptrsv":
        return 256 + 8 * n
    return 256 + 8 * n * min(k, max(64, MAILBOX_BYTES // (8 * n) // 64 * 64))


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    for knob in (exblas_amd.set_trsm_path, exblas_amd.set_sptrsv_path, exblas_amd.set_sptrsm_path):
        knob(0)


def _entry(ex, ctx, name):
    """the routine `name` on a context, or on the default one"""
    return getattr(ctx, name) if ctx is not None else getattr(ex, name + "_dev")


# ---------------------------------------------------------------------------------------------
# the three mailbox solves behind one face: both triangles on the device in both orientations, and a captured copy
# ---------------------------------------------------------------------------------------------
class _Trsm:
    """ExTRSM on graph_replay_cases.dense_triangles; orient = (uplo, trans), the other one turns trans"""
    name, vector = "extrsm", False
    sets = staticmethod(G.dense_sets)

    def __init__(self, ex, orient):
        self.ex, self.orient = ex, orient
        self.other = (orient[0], "T" if orient[1] == "N" else "N")
        self.tris, self.n = G.dense_triangles(), G.DENSE_N
        self.dev, self.rows = {}, {}
        for o in (self.orient, self.other):
            for t in (0, 1):
                a, self.lda, _, self.rows[o] = X.trsv_operands(self.tris[t].L, np.zeros(self.n), *o, lda_pad=1)
                self.dev[o, t] = _cuda(a)          # (NaN in the other triangle and in the lda padding)
        self.cap = self.dev[self.orient, 0].clone()

    def put(self, t):
        self.cap.copy_(self.dev[self.orient, t])

    def solve(self, ctx, x, fpe, ee, t=None, o=None):
        """on the captured matrix, or (t, o given) on triangle t in orientation o"""
        import torch
        flat, o = (self.cap, self.orient) if t is None else (self.dev[o, t], o)
        A = torch.as_strided(flat, (self.n, self.n), (1, self.lda))
        assert _entry(self.ex, ctx, "extrsm")(A, x, o[0], o[1], "N", fpe, ee) is x

    def skipped(self, t):
        return 0

    def info(self):
        return self.ex.last_trsm_info()

    def set_path(self, path):
        self.ex.set_trsm_path(path)


class _Sptrs:
    """ExSpTRSV (vector) or ExSpTRSM on graph_replay_cases.sparse_triangles; orient = (uplo,), int64 indices under 'L' and
    int32 under 'U'; col and val are padded to one budget so that either pattern fits the captured buffers"""
    sets = staticmethod(G.sparse_sets)

    def __init__(self, ex, orient, vector):
        self.ex, self.orient, self.vector = ex, orient, vector
        self.name = "exsptrsv" if vector else "exsptrsm"
        self.other = ("U" if orient[0] == "L" else "L",)
        self.tris, self.n = G.sparse_triangles(), G.SPARSE_N
        self.dev, self.rows = {}, {}
        for o in (self.orient, self.other):
            for t in (0, 1):
                self.dev[o, t] = tuple(_cuda(a) for a in G.padded_csr(t, o[0]))
                self.rows[o] = G.sparse_csr(t, o[0])[3]
        self.cap = tuple(a.clone() for a in self.dev[self.orient, 0])

    def put(self, t):
        for dst, src in zip(self.cap, self.dev[self.orient, t]):
            dst.copy_(src)

    def solve(self, ctx, x, fpe, ee, t=None, o=None):
        arrays, o = (self.cap, self.orient) if t is None else (self.dev[o, t], o)
        assert _entry(self.ex, ctx, self.name)((*arrays, (self.n, self.n)), x, o[0], "N", fpe, ee) is x

    def skipped(self, t):
        """the stored entries of the other triangle (NaN, up to three per row), counted by the case builder: what ExSpTRSV
        and ExSpTRSM both have to report for this matrix, whatever k and the panels"""
        return G.sparse_csr(t, self.orient[0])[4]

    def info(self):
        return self.ex.last_sptrsv_info() if self.vector else self.ex.last_sptrsm_info()

    def set_path(self, path):
        (self.ex.set_sptrsv_path if self.vector else self.ex.set_sptrsm_path)(path)


class _Block:
    """a device block of right-hand sides: [n, k + PAD] with the solve's X the view [:, :k] (ExSpTRSV: a vector of n),
    logical row i at physical row rows[i]"""

    def __init__(self, R, k):
        import torch
        self.R, self.k = R, k
        self.full = torch.empty(R.n if R.vector else (R.n, k + PAD), dtype=torch.float64, device="cuda")
        self.x = self.full if R.vector else self.full[:, :k]

    def load(self, B, o):
        """the right-hand side into the output buffer (the solves work in place), the sentinel into the padding"""
        import torch
        wide = np.full((self.R.n, self.k + PAD), SENTINEL)
        wide[self.R.rows[o], :self.k] = B
        self.full.copy_(torch.from_numpy(np.ascontiguousarray(wide[:, 0]) if self.R.vector else wide))

    def check(self, want, o, what):
        back = self.full.cpu().numpy()
        if self.R.vector:
            assert_bits(back[self.R.rows[o]], want[:, 0], what)
        else:
            assert_bits(back[self.R.rows[o], :self.k], want, what)
            assert (bits(back[:, self.k:]) == bits(np.array(SENTINEL))).all(), (what, "the padding of X was written")


def _solve_replays(ex, R, k, path, fpe, ee):
    sets = R.sets(k)
    n, outputs = R.n, R.n * k
    cap, side = _Block(R, k), _Block(R, k)
    R.set_path(path)
    ctx2 = ex.Context()

    def load(r):
        R.put(sets[r][0])
        cap.load(sets[r][1], R.orient)

    def check(r):
        t, _, want, from_b = sets[r]
        what = (R.name, R.orient, k, path, fpe, ee, "replay", r)
        cap.check(want, R.orient, what)
        # The counters are the default context's record of its last call of this routine: a pointer to the header at the
        # start of its workspace.  The eager call between the replays has the same shape, so it records the same header,
        # and the second context's call does not touch the default context: what is read here is what THIS replay
        # counted.  (It raises if the watchdog flag is set.)
        info = R.info()
        assert info[0] + info[1] == outputs, (what, info, "the counters are not this replay's alone")
        assert info[2] == 0 and info[3] == R.skipped(t), (what, info)
        if fpe == 0:
            assert info[0] == 0, (what, info)
        elif R.tris[t].ties and from_b:
            assert info[1] >= R.tris[t].ties * from_b > 0, (what, info, "a tie was decided in registers")

    def aside(i, ctx, fpe, ee, o):
        side.load(sets[i][1], o)
        R.solve(ctx, side.x, fpe, ee, sets[i][0], o)
        side.check(sets[i][2], o, (R.name, o, k, path, fpe, ee, "beside the graph", i))

    load(0)
    try:
        replay_four(lambda: R.solve(None, cap.x, fpe, ee), lambda: R.solve(None, cap.x, fpe, ee), load, check,
                    lambda: aside(4, None, 0, False, R.other), lambda: aside(5, ctx2, fpe, ee, R.orient))
    finally:
        R.set_path(0)
        ctx2.destroy()


@pytest.mark.parametrize("fpe,ee", VARIANTS)
@pytest.mark.parametrize("k,path", BLOCK_SHAPES)
@pytest.mark.parametrize("uplo,trans", [("L", "N"), ("L", "T")])
def test_extrsm_replays(ex, uplo, trans, k, path, fpe, ee):
    """n = 203 (a partial item of TR_R = 4 rows, a partial staged tile of TR_CH = 64 columns of A), both triangles planted
    (ties: the accumulator rounding runs inside the graph); k = 65: two column tiles, the second of one column; k = 9 on
    path 3: three presets, of which only the first clears the counters"""
    _solve_replays(ex, _Trsm(ex, (uplo, trans)), k, path, fpe, ee)


@pytest.mark.parametrize("fpe,ee", VARIANTS)
@pytest.mark.parametrize("path", [0, 2])
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_exsptrsv_replays(ex, uplo, path, fpe, ee):
    """n = 700: triangle 0 planted (short rows, ties), triangle 1 with a row of 100 entries in every 50 (the 64-lane form
    of k_sptrsv among items of the 8-lane form); path 2: every row in the 64-lane form"""
    _solve_replays(ex, _Sptrs(ex, (uplo,), True), 1, path, fpe, ee)


@pytest.mark.parametrize("fpe,ee", VARIANTS)
@pytest.mark.parametrize("k,path", BLOCK_SHAPES)
@pytest.mark.parametrize("uplo", ["L", "U"])
def test_exsptrsm_replays(ex, uplo, k, path, fpe, ee):
    """the matrices of test_exsptrsv_replays; out[2] and out[3] are the structure's, counted once (by the first tile of
    the first panel): the same figures test_exsptrsv_replays holds ExSpTRSV to, on every replay"""
    _solve_replays(ex, _Sptrs(ex, (uplo,), False), k, path, fpe, ee)


# ---------------------------------------------------------------------------------------------
# ExBDOT: batches of zero / accumulate / finalize over one block, which ExGEMV 'N' at m = 4096 covers with its sums
# ---------------------------------------------------------------------------------------------
def _bdot_replays(ex, mode, body_of, sets=None):
    """body_of(X, Y, out) -> the captured calls; four data sets (G.bdot_sets: the planted one, ties, second); the eager
    call in between is ExGEMV 'N' fpe = 0 at m = 4096, which leaves its row sums in the bytes ExBDOT's sets live in; the
    second context runs the same ExBDOT on the data of replay 0"""
    import torch
    sets = sets or G.bdot_sets(mode)
    (n, p), q = sets[0][0].shape, sets[0][1].shape[1]
    m, gn, lda = 4096, 130, 4096
    gv = _gemv_sets("N", m, gn, lda, "narrow")[4]
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    Xd, Yd, X2, Y2 = new(n, p + 1)[:, :p], new(n, q + 2)[:, :q], new(n, p), new(n, q)
    oshape = (p, q) if mode == "G" else (p,)
    out, out2 = new(*oshape), new(*oshape)
    a, x, y = (_cuda(h) for h in gv[:3])
    ctx2 = ex.Context()

    def load(r):
        Xd.copy_(torch.from_numpy(sets[r][0]))
        Yd.copy_(torch.from_numpy(sets[r][1]))
        out.fill_(-1.0)

    def eager():
        y.copy_(torch.from_numpy(gv[2]))
        ex.exgemv_dev("N", m, gn, 1.0, a, lda, x, 1.0, y, 0, False)
        assert_bits(y.cpu().numpy(), gv[3], ("ExGEMV beside the graph", mode))

    def other():
        X2.copy_(torch.from_numpy(sets[0][0]))
        Y2.copy_(torch.from_numpy(sets[0][1]))
        out2.fill_(-1.0)
        ctx2.exbdot(X2, Y2, mode, out2)
        assert_bits(out2.cpu().numpy(), sets[0][2], ("the second context", mode))

    body = body_of(Xd, Yd, out)
    load(0)
    try:
        replay_four(body, body, load, lambda r: assert_bits(out.cpu().numpy(), sets[r][2], ("exbdot", mode, "replay", r)),
                    eager, other)
    finally:
        ctx2.destroy()


def test_exbdot_gram_replays(ex):
    """p = q = 65, n = 1000: batches of 64 x 64, 64 x 1, 1 x 64 and 1 x 1 outputs over the same block in one capture"""
    _bdot_replays(ex, "G", lambda Xd, Yd, out: lambda: ex.exbdot_dev(Xd, Yd, "G", out))


def test_exbdot_later_batch_uses_more_sets_replays(ex):
    """p = 67, q = 3: the batch of 64 x 3 outputs uses 192 sets (one group), the batch of 3 x 3 after it 252 (28 groups).
    Sets 192 .. 251 are neither cleared by the first batch nor left zero by its finalize: the only shape class in which
    the zeroing before a LATER batch is what stands between ExGEMV's sums and the outputs"""
    _bdot_replays(ex, "G", lambda Xd, Yd, out: lambda: ex.exbdot_dev(Xd, Yd, "G", out), G.bdot_uneven_sets())


def test_exbdot_diagonal_replays(ex):
    _bdot_replays(ex, "D", lambda Xd, Yd, out: lambda: ex.exbdot_dev(Xd, Yd, "D", out))


def test_exbdot_export_and_round_replays(ex):
    """exbdot_export_dev, then exbdot_round_dev on its sets, in one graph; the sets are filled with -1 before every
    replay ("every word of every set is written")"""
    import torch
    words = torch.empty((G.BDOT_G * G.BDOT_G, 72), dtype=torch.int64, device="cuda")

    def body_of(Xd, Yd, out):
        def body():
            words.fill_(-1)
            ex.exbdot_export_dev(Xd, Yd, "G", sets=words)
            ex.exbdot_round_dev(words, "G", G.BDOT_G, G.BDOT_G, out=out)
        return body

    _bdot_replays(ex, "G", body_of)


# ---------------------------------------------------------------------------------------------
# a graph outlives the growth of its context's workspace
# ---------------------------------------------------------------------------------------------
def _capture(fn):
    import torch
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn()
    return g


def _replay(g):
    import torch
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()


def _solve_outlives_growth(ex, R, small, big):
    """On a fresh Context (the default one only grows over a process, so it may not grow on demand): warm call and capture
    at k = small, replay, an eager call at k = big on the same context (the workspace at least doubles: the old block
    is parked), then two more replays on new data -- they run in the parked block while the context works in the new
    one.  After the growth last_*_info is not read for the replays: the context's record points into the new block
    (and a Context has no last_*_info anyway); the bits are what is held."""
    import torch
    ssets, bsets = R.sets(small), R.sets(big)
    cap, side = _Block(R, small), _Block(R, big)
    ctx, g = ex.Context(), None
    what = (R.name, R.orient, small, big)
    try:
        assert ctx.workspace_bytes() == 0
        R.put(ssets[0][0])
        cap.load(ssets[0][1], R.orient)
        R.solve(ctx, cap.x, 8, True)                                   # 1. the warm call
        cap.check(ssets[0][2], R.orient, (what, "warm"))
        before = ctx.workspace_bytes()
        assert before >= documented_workspace_bytes(R.name[2:], R.n, small)
        g = _capture(lambda: R.solve(ctx, cap.x, 8, True))             # 2.
        cap.load(ssets[0][1], R.orient)
        _replay(g)                                                     # 3.
        cap.check(ssets[0][2], R.orient, (what, "replay before the growth"))
        side.load(bsets[4][1], R.other)                                # 4. the other triangle, the other orientation
        R.solve(ctx, side.x, 0, False, bsets[4][0], R.other)
        torch.cuda.synchronize()
        assert ctx.workspace_bytes() >= 2 * before, (what, before, ctx.workspace_bytes())
        side.check(bsets[4][2], R.other, (what, "the call that grew the workspace"))
        for r in (1, 2):                                               # 5. (replay 2 changes the triangle)
            R.put(ssets[r][0])
            cap.load(ssets[r][1], R.orient)
            _replay(g)
            cap.check(ssets[r][2], R.orient, (what, "replay after the growth", r))
            side.load(bsets[r][1], R.orient)                           # and the context goes on working in the new block
            R.solve(ctx, side.x, 8, True, bsets[r][0], R.orient)
            side.check(bsets[r][2], R.orient, (what, "beside the parked graph", r))
    finally:
        del g                                                          # nothing is released while the graph exists
        torch.cuda.synchronize()
        ctx.destroy()


def test_extrsm_graph_outlives_workspace_growth(ex):
    _solve_outlives_growth(ex, _Trsm(ex, ("L", "N")), 9, 65)


def test_exsptrsm_graph_outlives_workspace_growth(ex):
    _solve_outlives_growth(ex, _Sptrs(ex, ("U",), False), 9, 65)


def test_exgemv_n_graph_outlives_workspace_growth(ex):
    """ExGEMV 'N' fpe = 0 (576 m bytes of row accumulators): captured at m = 1024, grown by a call at m = 4096"""
    import torch
    small, big = (1024, 70, 1024), (4096, 130, 4096)
    ss, bs = _gemv_sets("N", *small, "narrow"), _gemv_sets("N", *big, "narrow")
    new = lambda k: torch.empty(k, dtype=torch.float64, device="cuda")  # noqa: E731
    cap = tuple(new(k) for k in (small[2] * small[1], small[1], small[0]))
    side = tuple(new(k) for k in (big[2] * big[1], big[1], big[0]))
    ctx, g = ex.Context(), None

    def put(bufs, data):
        for t, h in zip(bufs, data[:3]):
            t.copy_(torch.from_numpy(h))

    def check(bufs, data, what):
        torch.cuda.synchronize()
        assert_bits(bufs[2].cpu().numpy(), data[3], what)

    def call(shape, bufs):
        ctx.exgemv("N", shape[0], shape[1], 1.0, bufs[0], shape[2], bufs[1], 1.0, bufs[2], 0, False)

    try:
        put(cap, ss[0])
        call(small, cap)                                               # 1. the warm call
        check(cap, ss[0], "warm")
        before = ctx.workspace_bytes()
        assert before >= 576 * small[0]
        g = _capture(lambda: call(small, cap))                         # 2.
        put(cap, ss[0])
        _replay(g)                                                     # 3.
        check(cap, ss[0], "replay before the growth")
        put(side, bs[4])
        call(big, side)                                                # 4.
        check(side, bs[4], "the call that grew the workspace")
        assert ctx.workspace_bytes() >= 2 * before, (before, ctx.workspace_bytes())
        for r in (1, 2):                                               # 5.
            put(cap, ss[r])
            _replay(g)
            check(cap, ss[r], ("replay after the growth", r))
            put(side, bs[r])
            call(big, side)
            check(side, bs[r], ("beside the parked graph", r))
    finally:
        del g
        torch.cuda.synchronize()
        ctx.destroy()


# ---------------------------------------------------------------------------------------------
# capturable after exblas_reserve_workspace alone: the first call of a context is made under capture
# ---------------------------------------------------------------------------------------------
def _reserved(ex, nbytes):
    ctx = ex.Context()
    assert ctx.workspace_bytes() == 0
    assert ex.load_library().exblas_reserve_workspace_ctx(ctx.handle, nbytes) == 0
    assert ctx.workspace_bytes() == nbytes       # a first reservation takes the byte count as it is: no slack hides a
    return ctx                                   # formula that is too small


@pytest.mark.parametrize("which,k", [("extrsm", 65), ("exsptrsv", 1), ("exsptrsm", 65)])
def test_solves_capture_after_a_reservation_alone(ex, which, k):
    import torch
    R = {"extrsm": lambda: _Trsm(ex, ("L", "T")), "exsptrsv": lambda: _Sptrs(ex, ("L",), True),
         "exsptrsm": lambda: _Sptrs(ex, ("L",), False)}[which]()
    sets = R.sets(k)
    cap = _Block(R, k)
    nbytes = documented_workspace_bytes(which[2:], R.n, k)
    ctx, g = _reserved(ex, nbytes), None
    try:
        R.put(0)
        cap.load(sets[0][1], R.orient)
        g = _capture(lambda: R.solve(ctx, cap.x, 8, True))
        for r in (0, 2):                                               # two data sets, one per triangle
            R.put(sets[r][0])
            cap.load(sets[r][1], R.orient)
            _replay(g)
            cap.check(sets[r][2], R.orient, (which, k, "captured as the first call, replay", r))
        assert ctx.workspace_bytes() == nbytes
    finally:
        del g
        torch.cuda.synchronize()
        ctx.destroy()


@pytest.mark.parametrize("mode", ["G", "D"])
def test_exbdot_captures_after_a_reservation_alone(ex, mode):
    import torch
    sets = G.bdot_sets(mode)
    n, p = sets[0][0].shape
    new = lambda *shape: torch.empty(shape, dtype=torch.float64, device="cuda")  # noqa: E731
    Xd, Yd, out = new(n, p), new(n, p), new(*((p, p) if mode == "G" else (p,)))
    ctx, g = _reserved(ex, documented_workspace_bytes("bdot")), None
    try:
        g = _capture(lambda: ctx.exbdot(Xd, Yd, mode, out))
        for r in (1, 0):                                               # the planted pair, then wide-range data
            Xd.copy_(torch.from_numpy(sets[r][0]))
            Yd.copy_(torch.from_numpy(sets[r][1]))
            out.fill_(-1.0)
            _replay(g)
            assert_bits(out.cpu().numpy(), sets[r][2], ("exbdot", mode, "captured as the first call, replay", r))
        assert ctx.workspace_bytes() == BDOT_WORKSPACE_BYTES
    finally:
        del g
        torch.cuda.synchronize()
        ctx.destroy()
