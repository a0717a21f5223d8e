"""ExSpTRSM on the GPU: every column bit for bit against exact_cases.trsv_exact, and against ExSpTRSV on that column.

The planted systems of the ExTRSV / ExSpTRSV tests run with blocks of right-hand sides (tests/sptrsm_cases.py: the
planted b and its control under exact scalings, and random columns), so that ties, carries and near-ties sit in many
columns of one wave at once, next to columns the register test certifies.  The counters keep the file from passing by
luck: a tie decided in registers fails even where round-to-even happens to give the right bits.  Then the slice, tile
and panel boundaries in k against ExSpTRSV, the small sizes, the padding of a wider block, the independence of the
columns, the divisor rules and the ends of the double range as blocks, the reference rounding mode against the oracle,
and the plumbing (context, stream, host arrays, graph capture).  Expected bits never come from the code under test.
After every solve the watchdog flag is read: it is never set."""
import ctypes
import functools

import numpy as np
import pytest

import exact_cases as X
import sptrsm_cases as M
import sptrsv_cases as S
from helpers import assert_bits as _same, bits as _bits
from sptrsm_cases import planted_block as _block   # the blocks of the planted systems, built once per session
from sptrsv_cases import planted_csr as _csr, upload as _upload

pytestmark = pytest.mark.gpu

CASE_IDS = [f"n{n}-W{W}-m{mb}{'-filler' if fl else ''}" for n, W, mb, fl in X.TRSV_CASES]
TIE_ROWS = (15, 27, 30, 90, 63, 312, 348)      # rows of class tie or carry, non-unit cases (tests/test_sptrsv_api.py)
KS = (3, 8, 33, 65)
# (uplo, index type, shuffled rows + NaN junk in the other triangle, path, (fpe, early_exit)): every value of every
# factor occurs, every path with every variant class that matters for it
COMBOS = (("L", np.int32, False, 0, (8, True)), ("U", np.int64, True, 0, (3, True)), ("L", np.int64, True, 1, (8, True)),
          ("U", np.int32, False, 2, (0, False)), ("L", np.int32, True, 3, (8, True)), ("U", np.int64, False, 3, (3, True)),
          ("U", np.int32, True, 0, (0, False)), ("L", np.int64, False, 2, (8, True)))


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_sptrsm_path(0)
    exblas_amd.set_sptrsv_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _clear(ex):
    """the watchdog of the last ExSpTRSM is clear (the C entry returns 0, the Python one does not raise); the counters"""
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_sptrsm_info(out) == 0, "the watchdog was raised"
    info = tuple(int(v) for v in out)
    assert ex.last_sptrsm_info() == info
    return info


def _solve(ex, A, B, idx, uplo, diag="N", fpe=8, ee=True, entry=None, pad=0, sentinel=-7.25):
    """logical B (n x k) in, logical X out, and the counters; pad: X is the view [:, :k] of a block pad columns wider"""
    call = entry or ex.exsptrsm_dev
    return M.solve_block(lambda x: call(A, x, uplo, diag, fpe, ee), lambda: _clear(ex), B, idx, pad, sentinel)


def _sptrsv_skipped(ex, A, n, uplo, diag):
    """ExSpTRSV's own count of skipped entries for this A"""
    import torch
    ex.set_sptrsv_path(0)
    ex.exsptrsv_dev(A, torch.ones(n, dtype=torch.float64, device="cuda"), uplo, diag)
    return ex.last_sptrsv_info()[3]


# ---------------------------------------------------------------------------------------------
# planted systems
# ---------------------------------------------------------------------------------------------
def _planted(ex, case, unit, k, kmax, combos):
    n, W, mbits, filler = X.TRSV_CASES[case]
    c, blk = _block(case, unit, kmax)
    B, want = blk.B[:, :k], blk.want[:, :k]
    from_b = sum(kd == "b" for kd in blk.kinds[:k])
    diag = "U" if unit else "N"
    ties = int(((c.classes == "tie") | (c.classes == "carry")).sum())
    if not unit:
        assert ties == TIE_ROWS[case]
    used, seen = int(np.count_nonzero(np.tril(c.L, -1))), []
    try:
        for uplo, itype, messy, path, (fpe, ee) in combos:
            csr = _csr(n, W, mbits, filler, unit, uplo, itype, messy)
            A = _upload(csr, n)
            skipped = len(csr[1]) - used - (0 if unit else n)   # junk, and under 'U' the stored diagonal
            assert skipped == _sptrsv_skipped(ex, A, n, uplo, diag)
            ex.set_sptrsm_path(path)
            got, info = _solve(ex, A, B, csr[3], uplo, diag, fpe, ee)
            what = (n, W, k, unit, uplo, itype.__name__, messy, path, fpe, ee, info)
            _same(got, want, what)
            assert info[0] + info[1] == n * k and info[2] == 0, what
            assert info[3] == skipped, what
            if path == 1 or fpe == 0:
                assert info[0] == 0, what
            else:
                assert info[1] >= ties * from_b, ("a tie was decided in registers", what)
            seen.append(info[1])
    finally:
        ex.set_sptrsm_path(0)
    print(f"planted {CASE_IDS[case]} unit={unit} k={k}: ties {ties} x {from_b} columns, accumulator outputs "
          f"{min(seen)}..{max(seen)} of {n * k}")


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", range(5), ids=CASE_IDS[:5])
def test_planted_blocks_every_path_width_and_orientation(ex, case, k):
    _planted(ex, case, False, k, max(KS), COMBOS)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("case", range(5), ids=CASE_IDS[:5])
def test_planted_blocks_unit_diagonal(ex, case, k):
    """the same with diag = 'U' (NaN stored on the diagonal of the shuffled forms); the two large systems with the
    filler keep to the blocks of 3 and 8 columns on every combination and take half of them at 33 and 65"""
    small = case < 3 or k <= 8
    _planted(ex, case, True, k, max(KS), COMBOS if small else COMBOS[::2])


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("case", [5, 6], ids=[CASE_IDS[5], CASE_IDS[6]])
def test_planted_blocks_many_row_groups(ex, case, unit):
    _planted(ex, case, unit, 5, 5, COMBOS)


@pytest.mark.parametrize("case", range(5), ids=CASE_IDS[:5])
def test_control_columns_are_decided_in_registers(ex, case):
    """a block of control columns only (every planted b_ij a quarter unit off its tie): the counter discriminates"""
    n, W, mbits, filler = X.TRSV_CASES[case]
    for unit in (False, True):
        c, blk = _block(case, unit, max(KS))
        cols = [j for j, kd in enumerate(blk.kinds) if kd == "control"][:9]
        B, want = np.ascontiguousarray(blk.B[:, cols]), blk.want[:, cols]
        for uplo in ("L", "U"):
            csr = _csr(n, W, mbits, filler, unit, uplo, np.int32, True)
            A = _upload(csr, n)
            try:
                for path in (0, 2, 3):
                    ex.set_sptrsm_path(path)
                    got, info = _solve(ex, A, B, csr[3], uplo, "U" if unit else "N")
                    _same(got, want, ("control", n, uplo, unit, path, info))
                    assert info[0] > 0 and info[0] + info[1] == n * len(cols), ("control", n, uplo, unit, path, info)
            finally:
                ex.set_sptrsm_path(0)


# ---------------------------------------------------------------------------------------------
# bit identity with ExSpTRSV at the slice, tile and panel boundaries
# ---------------------------------------------------------------------------------------------
K_BOUNDS = (1, 2, 3, 5, 8, 17, 32, 33, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def _structure(name):
    s = {"chain": lambda: S.chain(600), "arrow": lambda: S.arrow(300), "random": lambda: S.random_earlier(300),
         "blocks": lambda: S.block_diagonal(64, 5), "diagonal": lambda: S.diagonal_only(64)}[name]()
    rng = np.random.default_rng([s.n, 5])
    s.B = S.rand53(rng, (s.n, max(K_BOUNDS))) * rng.choice((-1.0, 1.0), (s.n, max(K_BOUNDS)))
    s.B[:, 0] = s.b
    return s


@pytest.mark.parametrize("name", ["chain", "arrow", "random", "blocks", "diagonal"])
def test_every_column_equals_exsptrsv(ex, name):
    import torch
    s = _structure(name)
    assert name != "arrow" or np.count_nonzero(s.L[-1]) > 2 * 128
    try:
        for uplo, itype in (("L", np.int32), ("U", np.int64)):
            csr = S.csr_of_triangular(s.L, uplo, itype, shuffle=itype is np.int64)
            A, idx = _upload(csr, s.n), csr[3]
            ref = np.empty_like(s.B)                             # ExSpTRSV, column by column
            ex.set_sptrsv_path(0)
            for j in range(s.B.shape[1]):
                xs = np.empty(s.n)
                xs[idx] = s.B[:, j]
                x = ex.exsptrsv_dev(A, torch.from_numpy(xs).cuda(), uplo)
                ex.last_sptrsv_info()
                ref[:, j] = x.cpu().numpy()[idx]
            assert np.isfinite(ref).all()
            for i, k in enumerate(K_BOUNDS):
                for path in ((0, 2, 3, 1)[i % 4], 0):
                    ex.set_sptrsm_path(path)
                    got, info = _solve(ex, A, s.B[:, :k], idx, uplo)
                    _same(got, ref[:, :k], (name, uplo, k, path, info))
                    assert info[0] + info[1] == s.n * k and info[2] == 0 and info[3] == 0
            ex.set_sptrsm_path(0)
            got, info = _solve(ex, A, s.B[:, :5], idx, uplo, "U")
            assert info[3] == s.n and info[2] == 0               # the stored diagonal is skipped, counted once
            for j in range(5):
                want, _ = X.trsv_exact(s.L, s.B[:, j], True)
                _same(got[:, j], want, (name, uplo, "unit", j))
    finally:
        ex.set_sptrsm_path(0)


# ---------------------------------------------------------------------------------------------
# sizes, padding, independence
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dense_small(m):
    rng = np.random.default_rng(m)
    s = S._system(m, rng, lambda i: np.arange(i))                # dense lower: every dependency there is
    s.B = S.rand53(rng, (m, 65)) * rng.choice((-1.0, 1.0), (m, 65))
    s.want = np.stack([X.trsv_exact(s.L, s.B[:, j])[0] for j in range(65)], axis=1)
    return s


@pytest.mark.parametrize("m", [0, 1, 7, 8, 9, 63, 64, 65])
def test_small_sizes(ex, m):
    import torch
    if m == 0:
        for itype in (torch.int32, torch.int64):
            A = (torch.zeros(1, dtype=itype).cuda(), torch.zeros(0, dtype=itype).cuda(),
                 torch.zeros(0, dtype=torch.float64).cuda(), (0, 0))
            for k in (0, 1, 5, 64, 65):
                x = torch.zeros(0, k, dtype=torch.float64).cuda()
                assert ex.exsptrsm_dev(A, x) is x and _clear(ex) == (0, 0, 0, 0)
        host = ex.exsptrsm((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), (0, 0)), np.zeros((0, 5)))
        assert host.shape == (0, 5)
        return
    s = _dense_small(m)
    try:
        for uplo in ("L", "U"):
            csr = S.csr_of_triangular(s.L, uplo, np.int32, shuffle=True, junk=True)
            A = _upload(csr, m)
            x = torch.zeros(m, 0, dtype=torch.float64).cuda()
            assert ex.exsptrsm_dev(A, x, uplo) is x and _clear(ex) == (0, 0, 0, 0)   # k == 0: nothing is launched
            for k in (1, 5, 64, 65):
                for path in (0, 1, 2, 3):
                    ex.set_sptrsm_path(path)
                    got, info = _solve(ex, A, s.B[:, :k], csr[3], uplo)
                    _same(got, s.want[:, :k], (m, k, uplo, path))
                    assert info[0] + info[1] == m * k
        host = ex.exsptrsm((csr[0], csr[1], csr[2], (m, m)), np.zeros((m, 0)), "U")
        assert host.shape == (m, 0)
    finally:
        ex.set_sptrsm_path(0)


@pytest.mark.parametrize("k", [1, 5, 64, 67])
def test_padding_of_a_wider_block_keeps_its_bits(ex, k):
    """X is the view [:, :k] of an (m, k + 3) block: the three columns beyond it are neither read (NaN there changes
    nothing) nor written"""
    c, blk = _block(2, False, max(KS))
    n = c.n
    B, want = blk.B[:, :min(k, 65)], blk.want[:, :min(k, 65)]
    if k > 65:
        B, want = np.hstack([B, blk.B[:, :k - 65]]), np.hstack([want, blk.want[:, :k - 65]])
    try:
        for uplo, path in (("L", 0), ("U", 3), ("L", 1)):
            csr = _csr(*X.TRSV_CASES[2], False, uplo, np.int64, True)
            ex.set_sptrsm_path(path)
            for sentinel in (-7.25, np.nan):
                got, _ = _solve(ex, _upload(csr, n), B, csr[3], uplo, pad=3, sentinel=sentinel)
                _same(got, want, ("ldx > k", k, uplo, path, sentinel))
    finally:
        ex.set_sptrsm_path(0)


def test_columns_are_independent(ex):
    """one column of B all NaN, one holding an Inf: every other column keeps the bits of the run without them"""
    c, blk = _block(3, False, max(KS))
    n = c.n
    try:
        for k, path in ((8, 0), (65, 0), (8, 3), (33, 2)):
            B = blk.B[:, :k].copy()
            B[:, 2] = np.nan
            B[3, 5] = np.inf
            keep = np.ones(k, dtype=bool)
            keep[[2, 5]] = False
            for uplo in ("L", "U"):
                csr = _csr(*X.TRSV_CASES[3], False, uplo, np.int32, True)
                ex.set_sptrsm_path(path)
                got, info = _solve(ex, _upload(csr, n), B, csr[3], uplo)
                _same(got[:, keep], blk.want[:, :k][:, keep], ("independent", k, path, uplo))
                assert np.isnan(got[:, 2]).all() and not np.isfinite(got[3, 5]) and info[0] + info[1] == n * k
                assert (_bits(got[:3, 5]) == _bits(blk.want[:3, 5])).all()      # rows before the Inf do not see it
    finally:
        ex.set_sptrsm_path(0)


# ---------------------------------------------------------------------------------------------
# the edge cases of the single-vector tests, as blocks of 3 columns
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _three(name):
    s = {"random": lambda: S.random_earlier(300), "blocks": lambda: S.block_diagonal(64, 5)}[name]()
    rng = np.random.default_rng([s.n, 3])
    s.B = np.stack([s.b, -2.0 * s.b, S.rand53(rng, s.n) * rng.choice((-1.0, 1.0), s.n)], axis=1)
    s.want = np.stack([X.trsv_exact(s.L, s.B[:, j])[0] for j in range(3)], axis=1)
    s.want_unit = np.stack([X.trsv_exact(s.L, s.B[:, j], True)[0] for j in range(3)], axis=1)
    return s


def test_strictly_lower_matrix(ex):
    """no stored diagonal: fine under 'U'; under 'N' every row divides by +0.0 (Inf / NaN) and is counted once"""
    s = _three("random")
    strict = np.tril(s.L, -1)
    for uplo in ("L", "U"):
        csr = S.csr_of_triangular(strict, uplo, np.int32)
        A = _upload(csr, s.n)
        got, info = _solve(ex, A, s.B, csr[3], uplo, "U")
        _same(got, s.want_unit, ("strict, unit", uplo))
        assert info[2] == 0 and info[3] == 0
        got, info = _solve(ex, A, s.B, csr[3], uplo, "N")
        assert info[2] == s.n and not np.isfinite(got).any()
        assert (got[0] == np.copysign(np.inf, s.B[0])).all()


def test_duplicates_zeros_and_second_diagonal(ex):
    s = _three("random")
    crow, col, val, idx = S.csr_of_triangular(s.L, "L", np.int64, shuffle=True)
    n = s.n
    dup = S.with_duplicates(crow, col, val)
    assert dup[3] > 100
    got, info = _solve(ex, _upload(dup, n), s.B, idx, "L")
    _same(got, s.want, "duplicate off-diagonal columns are summed")
    assert info[3] == 0
    sec = S.with_second_diagonal(crow, col, val)                 # NaN as the later diagonal entry: never used
    got, info = _solve(ex, _upload(sec, n), s.B, idx, "L")
    _same(got, s.want, "the first stored diagonal entry is the divisor")
    assert info[3] == n and info[2] == 0
    got, info = _solve(ex, _upload(sec, n), s.B, idx, "L", "U")
    _same(got, s.want_unit, "unit: every stored diagonal entry is skipped")
    assert info[3] == 2 * n
    near = np.tri(n, dtype=bool) & (np.arange(n)[:, None] - np.arange(n)[None, :] <= 3)
    for uplo in ("L", "U"):
        z = S.csr_of_triangular(s.L, uplo, np.int32, keep=near | (s.L != 0), shuffle=True)
        assert (z[2] == 0).sum() > n
        got, info = _solve(ex, _upload(z, n), s.B, z[3], uplo)
        _same(got, s.want, ("explicit zeros", uplo))


def test_out_of_range_column_makes_the_row_nan_in_every_column(ex):
    s = _three("blocks")
    crow, col, val, idx = S.csr_of_triangular(s.L, "L", np.int64)
    try:
        for path in (0, 1):
            ex.set_sptrsm_path(path)
            for badcol in (-1, s.n, 2 ** 40):
                col2 = col.copy()
                col2[crow[7]] = badcol                           # row 7 = block 1, position 2: rows 8, 9 consume it
                got, _ = _solve(ex, _upload((crow, col2, val), s.n), s.B, idx, "L")
                nan = np.zeros(s.n, dtype=bool)
                nan[7:10] = True
                assert np.isnan(got[nan]).all(), badcol
                _same(got[~nan], s.want[~nan], ("rows that do not depend on it", badcol))
    finally:
        ex.set_sptrsm_path(0)


@pytest.mark.parametrize("lead", [0, 58, 70])
def test_range_rows(ex, lead):
    """overflow ties, totals either side of 2^1000, subnormal totals and quotients, the sign of a zero by cancellation:
    the column itself, its negation (expected from trsv_exact: a zero total keeps its + sign) and the column again"""
    r = X.range_rows_trsv(lead)
    B = np.stack([r.b, -r.b, r.b], axis=1)
    want = np.stack([r.want, X.trsv_exact(r.L, -r.b)[0], r.want], axis=1)
    try:
        for uplo in ("L", "U"):
            for itype in (np.int32, np.int64):
                csr = S.csr_of_triangular(r.L, uplo, itype, shuffle=True, junk=True)
                A = _upload(csr, r.n)
                for path in (0, 1, 2, 3):
                    ex.set_sptrsm_path(path)
                    for fpe, ee in ((0, False), (3, True), (8, True)):
                        got, _ = _solve(ex, A, B, csr[3], uplo, "N", fpe, ee)
                        bad = (_bits(got) != _bits(want)).any(axis=1)
                        assert not bad.any(), (lead, uplo, path, fpe, ee, [nm for nm in r.names if bad[r.rows[nm]]],
                                               got[bad], want[bad])
    finally:
        ex.set_sptrsm_path(0)


# ---------------------------------------------------------------------------------------------
# rounding mode, plumbing, graphs, the plain solve
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 2], ids=[CASE_IDS[0], CASE_IDS[2]])
def test_planted_reference_rounding_mode(ex, oracle, case):
    """ties are where the two rounding modes differ: every column follows the oracle's reference-mode substitution"""
    n, W, mbits, filler = X.TRSV_CASES[case]
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        differs = 0
        for unit in (False, True):
            c, blk = _block(case, unit, max(KS))
            k, diag = 6, "U" if unit else "N"
            want = np.empty((n, k))
            for j in range(k):
                a, lda, xs, idx = X.trsv_operands(c.L, blk.B[:, j], "L", "N", diag)
                rc, w = oracle.extrsv("L", "N", diag, n, a, lda, xs, 0, mode=oracle.ROUND_REFERENCE)
                assert rc == 0
                want[:, j] = w[idx]
            differs += int((_bits(want) != _bits(blk.want[:, :k])).sum())
            for uplo in ("L", "U"):
                csr = _csr(n, W, mbits, filler, unit, uplo, np.int32, True)
                A = _upload(csr, n)
                for path in (0, 2, 3):
                    ex.set_sptrsm_path(path)
                    for fpe, ee in ((0, False), (3, True), (8, True)):
                        got, info = _solve(ex, A, blk.B[:, :k], csr[3], uplo, diag, fpe, ee)
                        _same(got, want, ("reference mode", n, uplo, unit, path, fpe, ee))
                        assert info[0] == 0 and info[1] == n * k
        assert differs >= 1, "the reference rounding mode never differed from the exact one on these ties"
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_sptrsm_path(0)


def test_runs_contexts_streams_and_host_arrays_agree(ex):
    import torch
    n, W, mbits, filler = X.TRSV_CASES[3]
    c, blk = _block(3, False, max(KS))
    B, want = blk.B[:, :8], blk.want[:, :8]
    for uplo in ("L", "U"):
        csr = _csr(n, W, mbits, filler, False, uplo, np.int64, True)
        A = _upload(csr, n)
        first, _ = _solve(ex, A, B, csr[3], uplo)
        again, _ = _solve(ex, A, B, csr[3], uplo)
        _same(first, want, ("dev", uplo))
        assert (_bits(first) == _bits(again)).all()
        ctx, side = ex.Context(), torch.cuda.Stream()
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                got, _ = _solve(ex, A, B, csr[3], uplo, entry=ctx.exsptrsm)
            side.synchronize()
            assert (_bits(got) == _bits(first)).all(), ("context on a side stream", uplo)
        finally:
            torch.cuda.synchronize()
            ctx.destroy()
        Xs = np.empty((n, 8))
        Xs[csr[3]] = B
        keep = Xs.copy()
        host = ex.exsptrsm((csr[0], csr[1], csr[2], (n, n)), Xs, uplo, "N")
        assert (_bits(Xs) == _bits(keep)).all() and host is not Xs
        assert (_bits(host[csr[3]]) == _bits(first)).all(), ("host arrays", uplo)
        _clear(ex)


def test_graph_capture_after_one_warm_call(ex):
    """(Four replays on a changing triangle, several panels and a dirty workspace between replays:
    tests/test_gpu_graph_replay_solves.py.)"""
    import torch
    n, W, mbits, filler = X.TRSV_CASES[4]
    c, blk = _block(4, False, max(KS))
    csr = _csr(n, W, mbits, filler, False, "L", np.int32, False)
    A = _upload(csr, n)
    k = 65
    rhs = (blk.B[:, :k], np.ascontiguousarray(blk.B[:, k - 1::-1]))
    wants = (blk.want[:, :k], blk.want[:, k - 1::-1])
    for b, want in zip(rhs, wants):                              # (also the warm call that sizes the workspace)
        _same(_solve(ex, A, b, csr[3], "L")[0], want, "eager")
    x = torch.zeros(n, k, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exsptrsm_dev(A, x, "L", "N")
    for b, want in zip(rhs, wants):
        x.copy_(torch.from_numpy(np.ascontiguousarray(b)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (_bits(x.cpu().numpy()) == _bits(want)).all()
        _clear(ex)


def test_plain_solve_is_close_and_deterministic(ex):
    s = _three("random")
    csr = S.csr_of_triangular(s.L, "L", np.int64)
    A = _upload(csr, s.n)
    got, info = _solve(ex, A, s.B, csr[3], "L", "N", 1, False)
    again, _ = _solve(ex, A, s.B, csr[3], "L", "N", 1, False)
    assert np.isfinite(got).all() and (_bits(got) == _bits(again)).all() and info[0] == info[1] == 0
    assert (np.abs(got - s.want) <= 1e-10 * np.abs(s.want)).all()
