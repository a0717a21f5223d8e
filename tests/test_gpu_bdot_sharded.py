"""GPU tests of the row-sharded ExBDOT in one process, without a communicator: exbdot_export_dev per shard, the sets
stacked, exbdot_round_dev.  Every comparison is on the bits: against exbdot_dev on the whole block, against the digit sets
and doubles that tests/bdot_rank_cases.py derives from Python integers, and against raw limb sets of blas1_cases."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import bdot_rank_cases as S
import blas1_cases as B
import exact_cases as E
from helpers import exact_int_from_digits

pytestmark = pytest.mark.gpu

KINDS = [("fpuniform", 10, 0), ("fpuniform_signed", 60, 30), ("lognormal", 0.0, 50.0), ("ill_cond", 1e32, 0),
         ("cancel", 0, 0)]
NS = [1, 65, 257, 1000]
SHAPES = [("D", k, k) for k in (1, 5, 17, 64)] + [("G", 3, 5), ("G", 9, 17), ("G", 16, 16)]
VARIANTS = [(fpe, ee) for fpe in (0, 3, 8) for ee in (False, True)]
SENTINEL = -12345.678
SET_SENTINEL = -0x0123456789abcdef
INVALID = 1   # hipErrorInvalidValue
W = 72


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


def _dev(a, pad=0):
    """the block `a` on the device: contiguous, or a view [:, :k] of rows of k + pad doubles with NaN in the padding"""
    import torch
    a = np.ascontiguousarray(a, dtype=np.float64)
    if pad == 0:
        return torch.from_numpy(a).cuda()
    n, k = a.shape
    full = torch.full((n, k + pad), float("nan"), dtype=torch.float64, device="cuda")
    full[:, :k] = torch.from_numpy(a).cuda()
    return full[:, :k]


def _gen(oracle, kind, p0, p1, count, seed):
    return oracle.gen(kind, max(count, 1), seed, p0, p1)[:count].copy()


def _blocks(oracle, t, n, p, q):
    kind, p0, p1 = KINDS[t % len(KINDS)]
    return (_gen(oracle, kind, p0, p1, n * p, 131 + t).reshape(n, p), _gen(oracle, kind, p0, p1, n * q, 157 + t).reshape(n, q))


def _export_shards(ex, Xs, Ys, mode, outputs, salt=0, ctx=None):
    """[R, outputs, 72] on the device: shard r exported on path r % 3 with the variant (r + salt) % 6; Ys None: Y = X"""
    import torch
    R = len(Xs)
    sets = torch.full((R, outputs, W), SET_SENTINEL, dtype=torch.int64, device="cuda")
    try:
        for r in range(R):
            ex.set_bdot_path(r % 3)
            fpe, ee = VARIANTS[(r + salt) % len(VARIANTS)]
            f = ctx.exbdot_export if (ctx is not None and r % 2) else ex.exbdot_export_dev
            got = f(_dev(Xs[r], pad=r % 3), None if Ys is None else _dev(Ys[r], pad=(r + 1) % 2), mode, sets[r], fpe, ee)
            assert got.data_ptr() == sets[r].data_ptr()
    finally:
        ex.set_bdot_path(0)
    return sets


def _cuts(rng, n, R):
    """R shards of n rows, empty ones included"""
    c = np.sort(rng.integers(0, n + 1, size=R - 1)).tolist()
    return [0] + c + [n]


@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_random_blocks_equal_the_whole_block(ex, oracle, R):
    import torch
    lib = ex.load_library()
    rng = np.random.default_rng(100 + R)
    ctx = ex.Context()
    empty = 0
    try:
        for t, (mode, p, q) in enumerate(SHAPES):
            for n in NS:
                X, Y = _blocks(oracle, t + n, n, p, q)
                cut = _cuts(rng, n, R)
                empty += sum(a == b for a, b in zip(cut, cut[1:]))
                outputs = p if mode == "D" else p * q
                sets = _export_shards(ex, [X[a:b] for a, b in zip(cut, cut[1:])], [Y[a:b] for a, b in zip(cut, cut[1:])],
                                      mode, outputs, salt=t + n, ctx=ctx)
                assert not bool((sets == SET_SENTINEL).any()), "a word of a set was not written"
                assert bool((sets[:, :, 71] == 0).all()) and bool((sets[:, :, 68:71] == 0).all())
                assert bool(((sets[:, :, :67] >= 0) & (sets[:, :, :67] < 2 ** 32)).all()), "a digit is not normalised"
                Xd, Yd = _dev(X), _dev(Y)
                for rmode in (0, 1):
                    lib.exblas_set_round_mode(rmode)
                    want = ex.exbdot_dev(Xd, Yd, mode)
                    got = (ctx.exbdot_round if rmode else ex.exbdot_round_dev)(sets if (R > 1 or n % 2) else sets[0], mode, p, q)
                    assert got.shape == want.shape
                    _assert_bits(got.cpu().numpy(), want.cpu().numpy(), (mode, n, p, q, R, cut, rmode))
    finally:
        lib.exblas_set_round_mode(0)
        ctx.destroy()
    torch.cuda.synchronize()
    assert R == 1 or empty > 0


def test_export_of_the_whole_block_does_not_depend_on_path_or_variant(ex, oracle):
    import torch
    n, p, q = 3001, 7, 5
    X, Y = _blocks(oracle, 2, n, p, q)
    Xd, Yd = _dev(X, 3), _dev(Y, 1)
    ref = None
    try:
        for path in (0, 1, 2):
            ex.set_bdot_path(path)
            for fpe, ee in VARIANTS + [(9, False), (2, False)]:
                g, d = ex.exbdot_export_dev(Xd, Yd, "G", None, fpe, ee), ex.exbdot_export_dev(Xd[:, :q], Yd, "D", None, fpe, ee)
                if ref is None:
                    ref = (g.clone(), d.clone())
                assert torch.equal(g, ref[0]) and torch.equal(d, ref[1]), (path, fpe, ee)
                assert torch.equal(d, g.view(p, q, W)[torch.arange(q), torch.arange(q)]), "D is not the diagonal of G"
    finally:
        ex.set_bdot_path(0)


@pytest.mark.parametrize("R", S.RANKS)
def test_planted_cases_export_the_expected_digits_and_round_to_want(ex, R):
    import torch
    for sh in S.jobs(R):
        con = sh.con
        keep = con.keep
        sets = _export_shards(ex, sh.X, sh.Y, con.mode, con.outputs, salt=sh.index).cpu().numpy()
        for r in range(R):
            want_digits = sh.digits_r(r)
            bad = np.argwhere((sets[r, :, :B.NDIG] != want_digits).any(axis=1) & keep)
            assert bad.size == 0, (sh, r, "digits", bad[:5].tolist())
            assert (sets[r, :, B.NDIG:][keep] == 0).all(), (sh, r, "words 68..71")
        got = ex.exbdot_round_dev(torch.from_numpy(sets).cuda(), con.mode, con.p, con.q)
        _assert_bits(got.cpu().numpy().ravel(), con.want, (sh, "round"), keep=keep)
        # the same through exbdot_dev on the shards stacked in another order (ballast rows included)
        Xs, Ys = sh.stacked(order=[(r + 1) % R for r in range(R)])
        whole = ex.exbdot_dev(_dev(Xs), _dev(Ys), con.mode)
        _assert_bits(whole.cpu().numpy().ravel(), con.want, (sh, "exbdot_dev on the stack"), keep=keep)


def test_raw_limb_sets_into_the_round_alone(ex):
    import torch
    cases = B.family_e()
    by_nsets = {}
    for c in cases:
        by_nsets.setdefault(c.sets.shape[0], []).append(c)
    assert len(by_nsets) >= len(B.E_NSETS)
    for nsets, group in by_nsets.items():
        sets = np.ascontiguousarray(np.stack([c.sets for c in group], axis=1))      # [nsets, outputs, 72]
        assert sets.shape == (nsets, len(group), W)
        src = torch.from_numpy(sets).cuda()
        got = ex.exbdot_round_dev(src, "D", len(group), len(group))
        _assert_bits(got.cpu().numpy(), np.array([c.want for c in group]), ("family E", nsets))
        assert torch.equal(src.cpu(), torch.from_numpy(sets)), "the source sets were modified"
    # 64 copies of -1 (every digit 0xffffffff under a top digit of -1) and of its positive twin 2^2144 - 1: the borrow and
    # the carry run through 67 digits; a third output mixes them, 32 and 32 copies: 32 (2^2144 - 2)
    neg = np.array([B.DIGIT] * 67 + [-1] + [0] * 4, dtype=np.int64)
    pos = np.array([B.DIGIT] * 67 + [0] + [0] * 4, dtype=np.int64)
    nsets = 64
    sets = np.zeros((nsets, 3, W), dtype=np.int64)
    sets[:, 0], sets[:, 1] = neg, pos
    sets[::2, 2], sets[1::2, 2] = neg, pos
    want = []
    for o in range(3):
        T = sum(exact_int_from_digits(sets[k, o, :B.NDIG]) for k in range(nsets))
        want.append(E.round_nearest_even(Fraction(T, B.ONE)))
    assert want[0] == -64 * 2.0 ** -1074 and want[1] == float("inf") and want[2] == float("inf")
    # (the two finite-width twins overflow the double range; a pair scaled down to limb 30 stays finite)
    low = np.zeros((nsets, 2, W), dtype=np.int64)
    low[:, 0, :30], low[:, 0, 30:B.NDIG] = B.DIGIT, 0                # 2^960 - 1 units, 64 times: a 30-digit carry
    low[:, 1, :30], low[:, 1, 30:B.NDIG - 1], low[:, 1, B.NDIG - 1] = 1, B.DIGIT, -1
    want_low = [E.round_nearest_even(Fraction(sum(exact_int_from_digits(low[k, o, :B.NDIG]) for k in range(nsets)), B.ONE))
                for o in range(2)]
    got = ex.exbdot_round_dev(torch.from_numpy(sets).cuda(), "D", 3, 3).cpu().numpy()
    _assert_bits(got, np.array(want), "64 copies: borrow, carry, both")
    got = ex.exbdot_round_dev(torch.from_numpy(low).cuda(), "D", 2, 2).cpu().numpy()
    assert all(np.isfinite(want_low)) and want_low[0] > 0 > want_low[1]
    _assert_bits(got, np.array(want_low), "64 copies below the double range's top")


def test_non_finite_values_merge_across_shards(ex, oracle):
    import torch
    n, p, q = 300, 5, 4
    X0, Y0 = _blocks(oracle, 0, n, p, q)   # fpuniform: positive, so that an infinity keeps its sign in every product
    assert (X0 > 0).all() and (Y0 > 0).all()
    cut = [0, 100, 100, 200, 300]          # four shards, one of them empty
    inf, nan = np.inf, np.nan
    for plants, in_row2 in (([(17, inf)], "pinf"), ([(250, -inf)], "ninf"), ([(17, inf), (250, -inf)], "nan"),
                            ([(17, inf), (120, inf)], "pinf"), ([(120, nan)], "nan"), ([(17, nan), (250, inf)], "nan")):
        for side in ("X", "Y"):
            X, Y = X0.copy(), Y0.copy()
            for row, v in plants:
                (X if side == "X" else Y)[row, 2] = v
            touched = np.zeros((p, q), dtype=bool)
            if side == "X":
                touched[2, :] = True
            else:
                touched[:, 2] = True
            Xs, Ys = [X[a:b] for a, b in zip(cut, cut[1:])], [Y[a:b] for a, b in zip(cut, cut[1:])]
            sets = _export_shards(ex, Xs, Ys, "G", p * q, salt=len(plants))
            ind = sets[:, :, 68:].cpu().numpy().reshape(4, p, q, 4)
            assert ((ind == 0) | (ind == 1)).all() and (ind[..., 3] == 0).all(), "indicator words are 0 or 1, word 71 is 0"
            assert (ind[:, ~touched] == 0).all(), "an indicator outside the row / column of the non-finite value"
            for r, (a, b) in enumerate(zip(cut, cut[1:])):
                here = [v for row, v in plants if a <= row < b]
                want_ind = [int(any(v == inf for v in here)), int(any(v == -inf for v in here)), int(any(v != v for v in here))]
                assert (ind[r][touched][:, :3] == want_ind).all(), (plants, side, r, ind[r][touched][:, :3].tolist(), want_ind)
            got = ex.exbdot_round_dev(sets, "G", p, q).cpu().numpy()
            whole = ex.exbdot_dev(_dev(X), _dev(Y), "G").cpu().numpy()
            _assert_bits(got, whole, ("vs exbdot_dev", plants, side))
            assert np.isfinite(got[~touched]).all()
            t = got[touched]
            assert {"pinf": np.isposinf(t).all(), "ninf": np.isneginf(t).all(), "nan": np.isnan(t).all()}[in_row2], (plants, side, t)
            d = ex.exbdot_round_dev(_export_shards(ex, [x[:, :q] for x in Xs], Ys, "D", q), "D", q, q).cpu().numpy()
            assert _bits(d)[2] == _bits(got)[2, 2] and np.isfinite(np.delete(d, 2)).all()
            _assert_bits(np.delete(d, 2), np.delete(np.diag(got[:q, :q]), 2), ("D untouched", plants, side))


def _small_integers(rng, n, k):
    return rng.integers(-(1 << 20), 1 << 20, size=(n, k)).astype(np.float64)


@pytest.mark.parametrize("mode,n,p,q", [("G", 8, 65, 2), ("G", 5, 2, 65), ("D", 8, 4097, 4097)])
def test_batches_write_their_sets_at_their_own_offsets(ex, mode, n, p, q):
    """more than 64 x 64 ('G') or 4096 ('D') outputs: two batches; integer data, so that every set is known"""
    import torch
    rng = np.random.default_rng(p + q)
    X, Y = _small_integers(rng, n, p), _small_integers(rng, n, q)
    exact = (X.astype(np.int64) * Y.astype(np.int64)).sum(axis=0) if mode == "D" else X.astype(np.int64).T @ Y.astype(np.int64)
    outputs = p if mode == "D" else p * q
    digits = B.digits_matrix([int(v) << B.U for v in exact.ravel()])
    cut = [0, 3, n]
    buf = torch.full((2 * outputs * W + W,), SET_SENTINEL, dtype=torch.int64, device="cuda")
    sets = buf[:2 * outputs * W].view(2, outputs, W)
    part = []
    for r, (a, b) in enumerate(zip(cut, cut[1:])):
        ex.exbdot_export_dev(_dev(X[a:b]), _dev(Y[a:b]), mode, sets[r])
        part.append((X[a:b].astype(np.int64) * Y[a:b].astype(np.int64)).sum(axis=0) if mode == "D"
                    else X[a:b].astype(np.int64).T @ Y[a:b].astype(np.int64))
    host = buf.cpu().numpy()
    assert (host[2 * outputs * W:] == SET_SENTINEL).all(), "words behind the last set were written"
    for r in range(2):
        got = host[r * outputs * W:(r + 1) * outputs * W].reshape(outputs, W)
        want = B.digits_matrix([int(v) << B.U for v in part[r].ravel()])
        bad = np.argwhere((got[:, :B.NDIG] != want).any(axis=1))
        assert bad.size == 0, (mode, r, "set o is not at o * 72", bad[:5].tolist())
        assert (got[:, B.NDIG:] == 0).all()
    assert (digits == B.digits_matrix([int(a) + int(b) << B.U for a, b in zip(part[0].ravel(), part[1].ravel())])).all()
    before = sets.clone()
    if mode == "D":
        cbuf = torch.full((p + 2,), SENTINEL, dtype=torch.float64, device="cuda")
        out = ex.exbdot_round_dev(sets, "D", p, q, cbuf[:p])
        res = cbuf.cpu().numpy()
        assert (_bits(res[p:]) == _bits(np.array([SENTINEL]))[0]).all(), "the words behind c were written"
        got = res[:p]
    else:
        cbuf = torch.full((p, q + 2), SENTINEL, dtype=torch.float64, device="cuda")
        out = ex.exbdot_round_dev(sets, "G", p, q, cbuf[:, :q])
        res = cbuf.cpu().numpy()
        assert (_bits(res[:, q:]) == _bits(np.array([SENTINEL]))[0]).all(), "the padding of C was written"
        got = np.ascontiguousarray(res[:, :q])
    assert out.data_ptr() == cbuf.data_ptr()
    assert torch.equal(sets, before), "the round modified its source sets"
    _assert_bits(got, exact.astype(np.float64), (mode, p, q, "exact integers"))
    _assert_bits(got, ex.exbdot_dev(_dev(X), _dev(Y), mode).cpu().numpy(), (mode, p, q, "vs exbdot_dev"))


def test_degenerate_sizes_and_refusals(ex):
    import torch
    lib = ex.load_library()
    for mode, p, q in (("G", 3, 5), ("D", 70, 70), ("G", 1, 1)):
        outputs = p if mode == "D" else p * q
        sets = torch.full((outputs, W), SET_SENTINEL, dtype=torch.int64, device="cuda")
        ex.exbdot_export_dev(torch.zeros((0, p), dtype=torch.float64, device="cuda"),
                             torch.zeros((0, q), dtype=torch.float64, device="cuda"), mode, sets)
        assert bool((sets == 0).all()), (mode, p, q)
        got = ex.exbdot_round_dev(sets, mode, p, q).cpu().numpy()
        assert got.shape == ((p, q) if mode == "G" else (p,)) and (_bits(got) == 0).all(), (mode, p, q)   # +0.0
    # p == 0 or q == 0: success, and nothing is written anywhere
    sbuf = torch.full((2 * W,), SET_SENTINEL, dtype=torch.int64, device="cuda")
    cbuf = torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda")
    x = torch.ones(64, dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    assert lib.exblas_exbdot_export_dev(b"G", 8, 0, 3, ptr(x), 0, ptr(x), 3, ptr(sbuf), 8, 1, st) == 0
    assert lib.exblas_exbdot_export_dev(b"G", 8, 3, 0, ptr(x), 3, ptr(x), 0, ptr(sbuf), 8, 1, st) == 0
    assert lib.exblas_exbdot_export_dev(b"D", 8, 0, 0, ptr(x), 0, ptr(x), 0, ptr(sbuf), 8, 1, st) == 0
    assert lib.exblas_exbdot_round_dev(b"G", 0, 3, ptr(sbuf), 1, ptr(cbuf), 3, st) == 0
    assert lib.exblas_exbdot_round_dev(b"D", 0, 0, ptr(sbuf), 2, ptr(cbuf), 1, st) == 0
    # refused with valid device pointers: plain fp64 sums, the silent return, no sets to add
    assert lib.exblas_exbdot_export_dev(b"G", 8, 1, 2, ptr(x), 1, ptr(x), 2, ptr(sbuf), 1, 0, st) == INVALID
    assert lib.exblas_exbdot_export_dev(b"G", 8, 1, 2, ptr(x), 1, ptr(x), 2, ptr(sbuf), 9, 1, st) == INVALID
    assert lib.exblas_exbdot_round_dev(b"G", 1, 2, ptr(sbuf), 0, ptr(cbuf), 2, st) == INVALID
    torch.cuda.synchronize()
    assert bool((sbuf == SET_SENTINEL).all()) and (_bits(cbuf.cpu().numpy()) == _bits(np.array([SENTINEL]))[0]).all()
    blocks = x.view(8, 8)
    for fpe, ee in ((1, False), (1, True), (9, True)):
        with pytest.raises(ValueError, match="^exbdot:"):
            ex.exbdot_export_dev(blocks[:, :2], blocks[:, 2:5], "G", None, fpe, ee)
    assert tuple(ex.exbdot_export_dev(blocks[:, :0], blocks[:, :3]).shape) == (0, W)
    assert tuple(ex.exbdot_round_dev(torch.zeros((0, W), dtype=torch.int64, device="cuda"), "D", 0, 0).shape) == (0,)
    # fpe 9 without early exit exports like every other variant
    a = ex.exbdot_export_dev(blocks[:, :2], blocks[:, 2:5], "G", None, 9, False)
    assert torch.equal(a, ex.exbdot_export_dev(blocks[:, :2], blocks[:, 2:5], "G"))


def test_graph_capture_of_export_and_round(ex, oracle):
    """(Four replays on new data at 65 x 65 outputs, with a dirty workspace between replays:
    tests/test_gpu_graph_replay_solves.py.)"""
    import torch
    n, p, q = 5000, 6, 5
    X, Y = _blocks(oracle, 1, n, p, q)
    Xd, Yd = _dev(X, 3), _dev(Y, 1)
    sets = torch.zeros((2, p * q, W), dtype=torch.int64, device="cuda")
    out = torch.zeros((p, q), dtype=torch.float64, device="cuda")
    h = n // 3
    ex.exbdot_export_dev(Xd[:h], Yd[:h], "G", sets[0])   # warm-up: sizes the workspace
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exbdot_export_dev(Xd[:h], Yd[:h], "G", sets[0])
            ex.exbdot_export_dev(Xd[h:], Yd[h:], "G", sets[1])
            ex.exbdot_round_dev(sets, "G", p, q, out)
    X2, Y2 = _blocks(oracle, 2, n, p, q)
    Xd.copy_(torch.from_numpy(X2).cuda())
    Yd.copy_(torch.from_numpy(Y2).cuda())
    out.fill_(SENTINEL)
    sets.fill_(SET_SENTINEL)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    _assert_bits(out.cpu().numpy(), ex.exbdot_dev(Xd, Yd, "G").cpu().numpy(), "replay")
