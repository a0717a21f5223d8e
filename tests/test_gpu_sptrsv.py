"""ExSpTRSV on the GPU, bit for bit against exact_cases.trsv_exact (Fraction substitution on the dense logical system).

The planted systems of the dense ExTRSV tests (ties, carries and near-ties on every planted row, 106-bit products,
hundreds of dependencies inside batches of 8 rows, with the filler rows of up to 157 entries) run as CSR in both
orientations, on every path, with both index widths, with the entries of each row shuffled and NaN junk in the other
triangle.  The counters keep the file from passing by luck: a tie decided in registers fails even where round-to-even
happens to give the right bits.  Then structures that exercise the hand-off (a chain, an arrow, random and independent
rows), the divisor rules, the ends of the double range, the reference rounding mode against the oracle, and the
plumbing (context, stream, host arrays, graph capture).  After every solve the watchdog flag is read: it is never set."""
import ctypes
import functools

import numpy as np
import pytest

import exact_cases as X
import sptrsv_cases as S
from exact_cases import planted_trsv_case as _case   # the planted systems, built once per session for every file
from helpers import assert_bits as _same, bits as _bits
from sptrsv_cases import planted_csr as _csr, upload as _upload

pytestmark = pytest.mark.gpu

CASE_IDS = [f"n{n}-W{W}-m{mb}{'-filler' if fl else ''}" for n, W, mb, fl in X.TRSV_CASES]
TIE_ROWS = (15, 27, 30, 90, 63, 312, 348)      # rows of class tie or carry, non-unit cases (tests/test_sptrsv_api.py)
VARIANTS = ((0, False), (3, True), (8, True))
PATHS = (0, 1, 2)
ITYPES = (np.int32, np.int64)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_sptrsv_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _clear(ex):
    """the watchdog of the last call is clear (the C entry returns 0); returns the counters"""
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_sptrsv_info(out) == 0, "the watchdog was raised"
    return tuple(int(v) for v in out)


def _solve(ex, A, b, idx, uplo, diag="N", fpe=8, ee=True, entry=None):
    """logical b in, logical x out, and the counters"""
    import torch
    xs = np.empty(len(b))
    xs[idx] = b
    x = torch.from_numpy(xs).cuda()
    out = (entry or ex.exsptrsv_dev)(A, x, uplo, diag, fpe, ee)
    assert out is x
    info = _clear(ex)
    return x.cpu().numpy()[idx], info


# ---------------------------------------------------------------------------------------------
# planted systems
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("case", range(len(X.TRSV_CASES)), ids=CASE_IDS)
def test_planted_every_path_width_and_orientation(ex, case, unit):
    n, W, mbits, filler = X.TRSV_CASES[case]
    c = _case(n, W, mbits, filler, unit)
    diag = "U" if unit else "N"
    ties = int(((c.classes == "tie") | (c.classes == "carry")).sum())
    if not unit:
        assert ties == TIE_ROWS[case]
    seen, used = [], int(np.count_nonzero(np.tril(c.L, -1)))
    try:
        for uplo in ("L", "U"):
            for itype in ITYPES:
                for messy in (False, True):
                    csr = _csr(n, W, mbits, filler, unit, uplo, itype, messy)
                    A = _upload(csr, n)
                    skipped = len(csr[1]) - used - (0 if unit else n)   # junk, and under 'U' the stored diagonal
                    assert skipped == (3 * n - 6 if messy else 0) + (n if unit else 0)
                    for path in PATHS:
                        ex.set_sptrsv_path(path)
                        for fpe, ee in VARIANTS:
                            got, info = _solve(ex, A, c.b, csr[3], uplo, diag, fpe, ee)
                            what = (n, W, uplo, itype.__name__, messy, path, fpe, ee, info)
                            _same(got, c.want, what)
                            assert info[0] + info[1] == n and info[2] == 0, what
                            if path == 1 or fpe == 0:
                                assert info[0] == 0, what
                            else:
                                assert info[1] >= ties, ("a tie was decided in registers", what)
                            assert info[3] == skipped, what
                            seen.append(info[1])
    finally:
        ex.set_sptrsv_path(0)
    print(f"planted {CASE_IDS[case]} unit={unit}: ties {ties}, accumulator rows {min(seen)}..{max(seen)} of {n}")


@pytest.mark.parametrize("case", range(len(X.TRSV_CASES)), ids=CASE_IDS)
def test_control_is_decided_in_registers(ex, case):
    """the same matrix, every planted b_i a quarter unit further from its tie: the counter discriminates"""
    n, W, mbits, filler = X.TRSV_CASES[case]
    for unit in (False, True):
        c = _case(n, W, mbits, filler, unit)
        want, _ = X.trsv_exact(c.L, c.b_control, unit)
        for uplo in ("L", "U"):
            csr = _csr(n, W, mbits, filler, unit, uplo, np.int32, True)
            A = _upload(csr, n)
            try:
                for path in (0, 2):
                    ex.set_sptrsv_path(path)
                    got, info = _solve(ex, A, c.b_control, csr[3], uplo, "U" if unit else "N")
                    _same(got, want, ("control", n, uplo, unit, path, info))
                    assert info[0] > 0, ("control", n, uplo, unit, path, info)
            finally:
                ex.set_sptrsv_path(0)


@pytest.mark.parametrize("case", [5, 6], ids=[CASE_IDS[5], CASE_IDS[6]])
def test_same_bits_as_dense_extrsv(ex, case):
    import torch
    n, W, mbits, filler = X.TRSV_CASES[case]
    for unit in (False, True):
        c = _case(n, W, mbits, filler, unit)
        diag = "U" if unit else "N"
        for uplo in ("L", "U"):
            a, lda, xs, idx = X.trsv_operands(c.L, c.b, uplo, "N", diag)
            dx = torch.from_numpy(xs).cuda()
            assert ex.extrsv_dev(uplo, "N", diag, n, torch.from_numpy(a).cuda(), lda, dx, 8, True) == 0
            dense = dx.cpu().numpy()[idx]
            csr = _csr(n, W, mbits, filler, unit, uplo, np.int64, False)
            got, _ = _solve(ex, _upload(csr, n), c.b, csr[3], uplo, diag)
            assert (_bits(got) == _bits(dense)).all(), (n, uplo, unit)


@pytest.mark.parametrize("case", range(len(X.TRSV_CASES)), ids=CASE_IDS)
def test_planted_reference_rounding_mode(ex, oracle, case):
    """ties are where the two rounding modes differ: the library follows the oracle's reference-mode substitution"""
    n, W, mbits, filler = X.TRSV_CASES[case]
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        differs = 0
        for unit in (False, True):
            c = _case(n, W, mbits, filler, unit)
            diag = "U" if unit else "N"
            a, lda, xs, idx = X.trsv_operands(c.L, c.b, "L", "N", diag)
            rc, want = oracle.extrsv("L", "N", diag, n, a, lda, xs, 0, mode=oracle.ROUND_REFERENCE)
            assert rc == 0
            want = want[idx]
            differs += int((_bits(want) != _bits(c.want)).sum())
            for uplo in ("L", "U"):
                csr = _csr(n, W, mbits, filler, unit, uplo, np.int32, True)
                A = _upload(csr, n)
                for path in (0, 2):
                    ex.set_sptrsv_path(path)
                    for fpe, ee in VARIANTS:
                        got, info = _solve(ex, A, c.b, csr[3], uplo, diag, fpe, ee)
                        _same(got, want, ("reference mode", n, uplo, unit, path, fpe, ee))
                        assert info[0] == 0
        assert differs >= 1, "the reference rounding mode never differed from the exact one on these ties"
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_sptrsv_path(0)


# ---------------------------------------------------------------------------------------------
# structures
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _structure(name):
    s = {"chain": lambda: S.chain(1000), "arrow": lambda: S.arrow(3000), "random": lambda: S.random_earlier(600),
         "blocks": lambda: S.block_diagonal(64, 5), "diagonal": lambda: S.diagonal_only(300)}[name]()
    s.want, _ = X.trsv_exact(s.L, s.b)
    s.want_unit, _ = X.trsv_exact(s.L, s.b, True)
    return s


@pytest.mark.parametrize("name", ["chain", "arrow", "random", "blocks", "diagonal"])
def test_structures(ex, name):
    s = _structure(name)
    try:
        for uplo in ("L", "U"):
            for itype in ITYPES:
                csr = S.csr_of_triangular(s.L, uplo, itype, shuffle=itype is np.int64)
                A = _upload(csr, s.n)
                for path in PATHS:
                    ex.set_sptrsv_path(path)
                    got, info = _solve(ex, A, s.b, csr[3], uplo)
                    _same(got, s.want, (name, uplo, itype.__name__, path, info))
                    assert info[0] + info[1] == s.n and info[2] == 0 and info[3] == 0
                ex.set_sptrsv_path(0)
                got, info = _solve(ex, A, s.b, csr[3], uplo, "U")
                _same(got, s.want_unit, (name, uplo, "unit"))
                assert info[3] == s.n and info[2] == 0           # the stored diagonal is skipped
    finally:
        ex.set_sptrsv_path(0)


def test_strictly_lower_matrix(ex):
    """no stored diagonal: fine under 'U'; under 'N' every row divides by +0.0 (Inf / NaN), is counted, and the run ends"""
    s = _structure("random")
    strict = np.tril(s.L, -1)
    for uplo in ("L", "U"):
        csr = S.csr_of_triangular(strict, uplo, np.int32)
        A = _upload(csr, s.n)
        got, info = _solve(ex, A, s.b, csr[3], uplo, "U")
        _same(got, s.want_unit, ("strict, unit", uplo))
        assert info[2] == 0 and info[3] == 0
        got, info = _solve(ex, A, s.b, csr[3], uplo, "N")
        assert info[2] == s.n and not np.isfinite(got).any()
        assert got[0] == np.copysign(np.inf, s.b[0])


def test_duplicates_zeros_and_second_diagonal(ex):
    s = _structure("random")
    crow, col, val, idx = S.csr_of_triangular(s.L, "L", np.int64, shuffle=True)
    n = s.n
    dup = S.with_duplicates(crow, col, val)
    assert dup[3] > 100
    got, info = _solve(ex, _upload(dup, n), s.b, idx, "L")
    _same(got, s.want, "duplicate off-diagonal columns are summed")
    assert info[3] == 0
    sec = S.with_second_diagonal(crow, col, val)                 # NaN as the later diagonal entry: never used
    got, info = _solve(ex, _upload(sec, n), s.b, idx, "L")
    _same(got, s.want, "the first stored diagonal entry is the divisor")
    assert info[3] == n and info[2] == 0
    got, info = _solve(ex, _upload(sec, n), s.b, idx, "L", "U")
    _same(got, s.want_unit, "unit: every stored diagonal entry is skipped")
    assert info[3] == 2 * n
    near = np.tri(n, dtype=bool) & (np.arange(n)[:, None] - np.arange(n)[None, :] <= 3)
    for uplo in ("L", "U"):
        z = S.csr_of_triangular(s.L, uplo, np.int32, keep=near | (s.L != 0), shuffle=True)
        assert (z[2] == 0).sum() > n
        got, info = _solve(ex, _upload(z, n), s.b, z[3], uplo)
        _same(got, s.want, ("explicit zeros", uplo))


def test_out_of_range_column_makes_the_row_nan(ex):
    s = _structure("blocks")
    crow, col, val, idx = S.csr_of_triangular(s.L, "L", np.int64)
    for badcol in (-1, s.n, 2 ** 40):
        col2 = col.copy()
        col2[crow[7]] = badcol                                   # row 7 = block 1, position 2: rows 8, 9 consume it
        got, _ = _solve(ex, _upload((crow, col2, val), s.n), s.b, idx, "L")
        nan = np.zeros(s.n, dtype=bool)
        nan[7:10] = True
        assert np.isnan(got[nan]).all(), badcol
        _same(got[~nan], s.want[~nan], ("rows that do not depend on it", badcol))


@pytest.mark.parametrize("m", [0, 1, 7, 8, 9, 63, 64, 65])
def test_small_sizes(ex, m):
    import torch
    if m == 0:
        for itype in (torch.int32, torch.int64):
            A = (torch.zeros(1, dtype=itype).cuda(), torch.zeros(0, dtype=itype).cuda(),
                 torch.zeros(0, dtype=torch.float64).cuda(), (0, 0))
            x = torch.zeros(0, dtype=torch.float64).cuda()
            assert ex.exsptrsv_dev(A, x) is x and _clear(ex) == (0, 0, 0, 0)
        assert ex.exsptrsv((np.zeros(1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0), (0, 0)), np.zeros(0)).size == 0
        return
    rng = np.random.default_rng(m)
    s = S._system(m, rng, lambda i: np.arange(i))                # dense lower: every dependency there is
    want, _ = X.trsv_exact(s.L, s.b)
    try:
        for uplo in ("L", "U"):
            csr = S.csr_of_triangular(s.L, uplo, np.int32, shuffle=True, junk=True)
            for path in PATHS:
                ex.set_sptrsv_path(path)
                got, info = _solve(ex, _upload(csr, m), s.b, csr[3], uplo)
                _same(got, want, (m, uplo, path))
                assert info[0] + info[1] == m
    finally:
        ex.set_sptrsv_path(0)


@pytest.mark.parametrize("lead", [0, 58, 70])
def test_range_rows(ex, lead):
    """overflow ties, totals either side of 2^1000, subnormal totals and quotients, the sign of a zero by cancellation"""
    r = X.range_rows_trsv(lead)
    try:
        for uplo in ("L", "U"):
            for itype in ITYPES:
                csr = S.csr_of_triangular(r.L, uplo, itype, shuffle=True, junk=True)
                A = _upload(csr, r.n)
                for path in PATHS:
                    ex.set_sptrsv_path(path)
                    for fpe, ee in VARIANTS:
                        got, _ = _solve(ex, A, r.b, csr[3], uplo, "N", fpe, ee)
                        bad = _bits(got) != _bits(r.want)
                        assert not bad.any(), (lead, uplo, path, fpe, ee, [nm for nm in r.names if bad[r.rows[nm]]],
                                               got[bad], r.want[bad])
    finally:
        ex.set_sptrsv_path(0)


# ---------------------------------------------------------------------------------------------
# invariance and plumbing
# ---------------------------------------------------------------------------------------------
def test_runs_contexts_streams_and_host_arrays_agree(ex):
    import torch
    n, W, mbits, filler = X.TRSV_CASES[3]
    c = _case(n, W, mbits, filler, False)
    for uplo in ("L", "U"):
        csr = _csr(n, W, mbits, filler, False, uplo, np.int64, True)
        A = _upload(csr, n)
        first, _ = _solve(ex, A, c.b, csr[3], uplo)
        again, _ = _solve(ex, A, c.b, csr[3], uplo)
        _same(first, c.want, ("dev", uplo))
        assert (_bits(first) == _bits(again)).all()
        ctx, side = ex.Context(), torch.cuda.Stream()
        try:
            torch.cuda.synchronize()
            with torch.cuda.stream(side):
                got, _ = _solve(ex, A, c.b, csr[3], uplo, entry=ctx.exsptrsv)
            side.synchronize()
            assert (_bits(got) == _bits(first)).all(), ("context on a side stream", uplo)
        finally:
            torch.cuda.synchronize()
            ctx.destroy()
        xs = np.empty(n)
        xs[csr[3]] = c.b
        keep = xs.copy()
        host = ex.exsptrsv((csr[0], csr[1], csr[2], (n, n)), xs, uplo, "N")
        assert (_bits(xs) == _bits(keep)).all() and host is not xs
        assert (_bits(host[csr[3]]) == _bits(first)).all(), ("host arrays", uplo)
        _clear(ex)


def test_graph_capture_after_one_warm_call(ex):
    """(Four replays on a changing triangle, several panels and a dirty workspace between replays:
    tests/test_gpu_graph_replay_solves.py.)"""
    import torch
    n, W, mbits, filler = X.TRSV_CASES[4]
    c = _case(n, W, mbits, filler, False)
    csr = _csr(n, W, mbits, filler, False, "L", np.int32, False)
    A = _upload(csr, n)
    rhs = (c.b, c.b_control)
    eager = [_solve(ex, A, b, csr[3], "L")[0] for b in rhs]      # (also the warm call that sizes the workspace)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exsptrsv_dev(A, x, "L", "N")
    for b, want in zip(rhs, eager):
        x.copy_(torch.from_numpy(np.ascontiguousarray(b)))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (_bits(x.cpu().numpy()) == _bits(want)).all()
        _clear(ex)


def test_plain_solve_is_close_and_deterministic(ex):
    s = _structure("random")
    csr = S.csr_of_triangular(s.L, "L", np.int64)
    A = _upload(csr, s.n)
    got, info = _solve(ex, A, s.b, csr[3], "L", "N", 1, False)
    again, _ = _solve(ex, A, s.b, csr[3], "L", "N", 1, False)
    assert np.isfinite(got).all() and (_bits(got) == _bits(again)).all() and info[0] == info[1] == 0
    assert (np.abs(got - s.want) <= 1e-10 * np.abs(s.want)).all()
