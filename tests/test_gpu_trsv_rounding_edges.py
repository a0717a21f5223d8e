"""ExTRSV on constructed ties along the substitution chain (tests/exact_cases.py: planted_trsv, range_rows_trsv), bit for bit.

The diagonal phase keeps each row as a three-level TwoSum expansion in registers plus an LDS remainder with a bound B,
and accepts the folded double only behind a certificate; a wrong certificate or a lost remainder changes one bit of
one row, on totals random data never produces.  These systems put an exact tie (to even, to odd, carrying into the
next binade) or a total one deciding unit off a tie (that unit 1, 30, 110 or 250 bits below the half unit: inside one
double, inside the three levels, below them) on every planted row, over a solution of full 53-bit doubles (106-bit
products, non-zero TwoProd error terms), with the closing terms consumed in the row's own block (diagonal phase) or in
earlier blocks (tile phase and its hand-over), followed by a division by an odd multiple of a power of two.
One planted row in seven also holds a pair of entries 2^120 or 2^150 times its total that cancels exactly: while the
pair is in an expansion the bits that decide the rounding can only live in the remainder, which the certificate knows
through B alone.

Expected bits: the Fraction substitution `trsv_exact` in the exact rounding mode (not the oracle, whose agreement
with it is a CPU test), the oracle in the reference rounding mode.  No tolerance.

The counter (`exblas_extrsv_last_slow_rows`) keeps the file from passing by luck: after every exact-mode solve of a
planted system it must be at least the number of ties, carries and near-ties with the deciding unit 30 or more bits
down (`trsv_must_round_as_integers`: derived from the certificate's 1.0000001 inflation, not measured) -- a tie
accepted in registers fails even where round-to-even happens to give the right bits -- and on the control system (the
same matrix, every planted b_i a quarter unit further from its tie) below a quarter of the rows, the bar
test_extrsv_scaled_rows_and_columns uses.  Each test prints the counts it saw (pytest -s)."""
import numpy as np
import pytest

import exact_cases as X
from exact_cases import TRSV_VARIANTS, planted_trsv_case as _case
from helpers import bits as _bits

pytestmark = pytest.mark.gpu

ORIENT = (("L", "N"), ("U", "N"), ("L", "T"), ("U", "T"))
FEW_VARIANTS = ((0, False), (3, False), (8, True))
CASE_IDS = [f"n{n}-W{W}-m{mb}{'-filler' if fl else ''}" for n, W, mb, fl in X.TRSV_CASES]


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.load_library().exblas_set_round_mode(0)


def _same(got, want, what, classes=None, gap=None):
    bad = _bits(got) != _bits(want)
    rows = np.nonzero(bad)[0][:6]
    assert not bad.any(), (what, int(bad.sum()), rows.tolist(), None if classes is None else classes[rows].tolist(),
                           None if gap is None else gap[rows].tolist(), np.asarray(got)[rows][:3], np.asarray(want)[rows][:3])


def _solve_twice(ex, L, b, uplo, trans, diag, fpe, ee, **layout):
    """through the host entry point, twice; returns the solution in logical order and the slow-row counter"""
    n = len(b)
    a, lda, xs, idx = X.trsv_operands(L, b, uplo, trans, diag, **layout)
    outs = []
    for _ in range(2):
        x = xs.copy()
        assert ex.extrsv(uplo, trans, diag, n, a, lda, layout.get("offa", 0), x, layout.get("incx", 1),
                         layout.get("offx", 0), fpe, ee) == 0
        outs.append(x)
    slow = ex.load_library().exblas_extrsv_last_slow_rows()
    assert (_bits(outs[0]) == _bits(outs[1])).all(), ("two runs differ", uplo, trans, diag, fpe, ee)
    gaps = np.ones(len(xs), dtype=bool)
    gaps[idx] = False
    assert np.isnan(outs[0][gaps]).all(), "the gaps of x were written"
    return outs[0][idx], slow


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("n,W,mbits,filler", X.TRSV_CASES, ids=CASE_IDS)
def test_planted_every_variant_and_orientation(ex, n, W, mbits, filler, unit):
    """bits, in every (fpe, early_exit) variant and all four orientations, each solve twice"""
    c = _case(n, W, mbits, filler, unit)
    diag = "U" if unit else "N"
    for uplo, trans in ORIENT:
        for fpe, ee in TRSV_VARIANTS:
            got, _ = _solve_twice(ex, c.L, c.b, uplo, trans, diag, fpe, ee)
            _same(got, c.want, (n, W, uplo, trans, diag, fpe, ee), c.classes, c.gap)


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("n,W,mbits,filler", X.TRSV_CASES, ids=CASE_IDS)
def test_planted_ties_are_never_decided_in_registers(ex, n, W, mbits, filler, unit):
    """the counter alone, whatever the bits are: a tie accepted in registers fails here even where round-to-even
    happens to give the right answer"""
    c = _case(n, W, mbits, filler, unit)
    must = X.trsv_must_round_as_integers(c)
    assert must >= int(c.planted.sum()) * 9 // 10 - 5
    diag = "U" if unit else "N"
    seen = []
    for uplo, trans in ORIENT:
        for fpe, ee in TRSV_VARIANTS:
            _, slow = _solve_twice(ex, c.L, c.b, uplo, trans, diag, fpe, ee)
            assert must <= slow <= n, ("a tie or near-tie was decided in registers", uplo, trans, fpe, ee, slow, must)
            seen.append(slow)
    print(f"planted n={n} W={W} mbits={mbits} filler={filler} unit={unit}: classes {c.counts}, "
          f"{int((c.cancel > 0).sum())} rows with a cancelling pair, must {must}, slow rows {min(seen)}..{max(seen)} of {n}")


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("n,W,mbits,filler", X.TRSV_CASES, ids=CASE_IDS)
def test_control_is_decided_in_registers(ex, n, W, mbits, filler, unit):
    """the same matrix, every planted b_i a quarter unit of its total further from the tie: the counter discriminates"""
    c = _case(n, W, mbits, filler, unit)
    want, _ = X.trsv_exact(c.L, c.b_control, unit)
    diag = "U" if unit else "N"
    seen = []
    for uplo, trans in ORIENT:
        for fpe, ee in TRSV_VARIANTS:
            got, slow = _solve_twice(ex, c.L, c.b_control, uplo, trans, diag, fpe, ee)
            _same(got, want, ("control", n, W, uplo, trans, diag, fpe, ee))
            assert 0 <= slow < max(n // 4, 1), ("control", uplo, trans, fpe, ee, slow)
            seen.append(slow)
    print(f"control n={n} W={W} mbits={mbits} filler={filler} unit={unit}: slow rows {min(seen)}..{max(seen)} of {n} "
          f"(planted system: at least {X.trsv_must_round_as_integers(c)})")


@pytest.mark.parametrize("n,W,mbits,filler", [X.TRSV_CASES[3], X.TRSV_CASES[6]], ids=[CASE_IDS[3], CASE_IDS[6]])
def test_planted_lda_incx_offsets(ex, n, W, mbits, filler):
    for unit in (False, True):
        c = _case(n, W, mbits, filler, unit)
        must = X.trsv_must_round_as_integers(c)
        for uplo, trans in ORIENT:
            for fpe, ee in FEW_VARIANTS:
                got, slow = _solve_twice(ex, c.L, c.b, uplo, trans, "U" if unit else "N", fpe, ee,
                                         lda_pad=5, offa=3, incx=3, offx=2)       # (asserts that the gaps still hold NaN)
                _same(got, c.want, ("strided", n, uplo, trans, unit, fpe, ee), c.classes, c.gap)
                assert slow >= must, (uplo, trans, unit, fpe, ee, slow, must)


@pytest.mark.parametrize("n,W,mbits,filler", [X.TRSV_CASES[2], X.TRSV_CASES[3], X.TRSV_CASES[5]],
                         ids=[CASE_IDS[2], CASE_IDS[3], CASE_IDS[5]])
def test_planted_device_pointer_and_context(ex, n, W, mbits, filler):
    import torch
    lib = ex.load_library()
    ctx = ex.Context()
    try:
        for unit in (False, True):
            c = _case(n, W, mbits, filler, unit)
            diag = "U" if unit else "N"
            must = X.trsv_must_round_as_integers(c)
            for uplo, trans in ORIENT:
                a, lda, xs, idx = X.trsv_operands(c.L, c.b, uplo, trans, diag, lda_pad=1, offa=4, incx=2, offx=6)
                da, dx0 = torch.from_numpy(a).cuda(), torch.from_numpy(xs).cuda()
                for fpe, ee in FEW_VARIANTS:
                    outs = []
                    for entry in (ex.extrsv_dev, ex.extrsv_dev, ctx.extrsv, ctx.extrsv):
                        dx = dx0.clone()
                        assert entry(uplo, trans, diag, n, da[4:], lda, dx[6:], fpe, ee, incx=2) == 0
                        torch.cuda.synchronize()
                        # (the counter reads the workspace of the library's own contexts: a Context's private
                        # workspace is not one of them, so after Context.extrsv it still shows the solve before)
                        if entry is ex.extrsv_dev:
                            assert lib.exblas_extrsv_last_slow_rows() >= must, (uplo, trans, unit, fpe, ee)
                        outs.append(dx.cpu().numpy())
                    for o in outs:
                        _same(o[idx], c.want, ("dev/ctx", n, uplo, trans, unit, fpe, ee), c.classes, c.gap)
                        assert (_bits(o) == _bits(outs[0])).all()
                    assert np.isnan(outs[0]).sum() == len(xs) - n
    finally:
        ctx.destroy()


@pytest.mark.parametrize("lead", [0, 58, 70])
def test_range_rows(ex, lead):
    """totals at both ends of the double range: inf, DBL_MAX, either side of 2^1000, subnormal totals and quotients, and
    the sign of a zero that comes out of cancelling 106-bit products.  lead = 58 puts the support rows at the end of
    the first block and the range rows at the start of the second, so that the huge and tiny products are formed in
    the tile phase and handed over; with 0 and 70 they are formed in the diagonal phase (first / second block)."""
    r = X.range_rows_trsv(lead)
    for uplo, trans in ORIENT:
        for fpe, ee in TRSV_VARIANTS:
            got, slow = _solve_twice(ex, r.L, r.b, uplo, trans, "N", fpe, ee, lda_pad=lead % 4)
            bad = _bits(got) != _bits(r.want)
            assert not bad.any(), (lead, uplo, trans, fpe, ee, [nm for nm in r.names if bad[r.rows[nm]]], got[bad], r.want[bad])
            assert slow >= 0


@pytest.mark.parametrize("n,W,mbits,filler", X.TRSV_CASES, ids=CASE_IDS)
def test_planted_reference_rounding_mode(ex, oracle, n, W, mbits, filler):
    """ties are exactly where the two rounding modes can differ: the oracle's reference-mode solution is not the
    exact-mode expectation, and the library follows the oracle"""
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        for unit in (False, True):
            c = _case(n, W, mbits, filler, unit)
            diag = "U" if unit else "N"
            differs = 0
            for uplo, trans in ORIENT:
                a, lda, xs, idx = X.trsv_operands(c.L, c.b, uplo, trans, diag)
                rc, want = oracle.extrsv(uplo, trans, diag, n, a, lda, xs, 0, mode=oracle.ROUND_REFERENCE)
                assert rc == 0
                differs += int((_bits(want[idx]) != _bits(c.want)).sum())
                for fpe, ee in FEW_VARIANTS + ((4, False), (6, True)):
                    got, _ = _solve_twice(ex, c.L, c.b, uplo, trans, diag, fpe, ee)
                    _same(got, want[idx], ("reference mode", n, uplo, trans, unit, fpe, ee), c.classes, c.gap)
            assert differs >= 1, "the reference rounding mode never differed from the exact one on these ties"
    finally:
        lib.exblas_set_round_mode(0)
