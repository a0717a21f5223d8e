"""ExSpIC0 on the GPU at its edges, bit for bit against spic0_cases.ic0_exact / plain_ic0 / apply_exact on the cases of
spic0_edge_cases.py (never the code under test): totals at the ends of the double range off the diagonal, in carriers of
every row class (8 to 512 owned entries, alone and behind a healthy block) and through source rows of 64 and more
entries; the square root on its own over the whole range; dense range cases, breakdowns and planted ties in long rows;
the reference rounding mode where it differs; the plain variant in its several-entries form; the small structures; a
captured graph of factor and apply replayed after a breakdown.  After every call the watchdog flag is read.

The counters hold the kernel to its certificate.  On paths 0 and 2 with fpe >= 2 the accumulator must have rounded at
least `settle` entries: the model's ties (potrf_cases._kind classes every entry outside the certificate's range a tie) and
the range entry where range_block_cases.settles() holds; for the planted systems the ties and the near-ties, as for
ExSpILU0 (test_gpu_spic0.py allows no more than that on the healthy cases, so there it is met with equality)."""
import numpy as np
import pytest

import spic0_cases as C
import spic0_edge_cases as X
from helpers import assert_bits as _same, bits as _bits
from test_gpu_spic0 import ITYPES, PATHS, _counters, _factor, _upload, ex  # noqa: F401  (ex: the module's fixture)

pytestmark = pytest.mark.gpu

FPES = (0, 2, 8)
VARIANTS = X.variants()


def _sweep(ex, csr, model, what, settle=None, registers=False, thin=False):
    """every path, width, fpe and place on one matrix: bits, info and the counters; returns cnt[1] - settle of the calls on
    paths 0 and 2 with fpe >= 2.  thin: without the int64 x in-place corner"""
    want, i0, i1, d = model
    assert i0 == 0
    m = len(csr[0]) - 1
    settle = d.ties if settle is None else settle
    above = []
    try:
        for itype in ITYPES:
            A = _upload(csr, itype)
            for path in PATHS:
                ex.set_spic0_path(path)
                for fpe in FPES:
                    for inplace in (False, True):
                        if thin and inplace and itype is np.int64:
                            continue
                        got, info, cnt = _factor(ex, A, fpe, True, inplace)
                        tag = (what, len(want), itype.__name__, path, fpe, inplace, cnt)
                        assert info == (0, i1), (tag, info)
                        _same(got, want, tag)
                        assert cnt[0] + cnt[1] == d.owned and cnt[2] == d.terms, tag
                        assert cnt[3] == (m if path == 2 else d.wide), tag
                        if path == 1 or fpe == 0:
                            assert cnt[0] == 0, tag
                        else:
                            assert cnt[1] >= settle, ("a total outside the certificate's range or a tie was decided in registers", tag)
                            assert cnt[0] > 0 or not registers, ("nothing was rounded in registers", tag)
                            above.append(cnt[1] - settle)
    finally:
        ex.set_spic0_path(0)
    return above


def _detail(csr):
    return C.ic0_exact(*csr, detail=True)


# ---------------------------------------------------------------------------------------------
# 1. the range cases in every row class, alone and behind a healthy block
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length,wide,reader", VARIANTS)
def test_range_totals_in_every_row_class_alone_and_behind_a_healthy_block(ex, length, wide, reader):
    cases = X.range_cases(length, wide, reader)
    assert len(cases) == 15
    lead = C.tridiagonal(X.LEAD)
    low = []
    for c in cases:
        low += _sweep(ex, c.csr, X.model(c), c.name, X.model(c)[3].settle, registers=True, thin=True)
        behind = X.behind_model(c)
        low += _sweep(ex, X.behind(lead, c.csr), behind, c.name + " behind", behind[3].settle, registers=True, thin=True)
    print(f"length {length} wide {wide} reader {reader}: accumulator entries above the model's least {min(low)}..{max(low)}")


# ---------------------------------------------------------------------------------------------
# 2. radicands and roots
# ---------------------------------------------------------------------------------------------
def test_every_root_value_is_the_correctly_rounded_root(ex):
    import math
    csr = X.root_diagonal()
    want = np.array([math.sqrt(float(v)) for v in csr[2]])
    try:
        for itype in ITYPES:
            A = _upload(csr, itype)
            for path in PATHS:
                ex.set_spic0_path(path)
                for fpe in (0, 1, 2, 8):
                    got, info, cnt = _factor(ex, A, fpe, fpe != 1)
                    assert info == (0, 0), (path, fpe, info)
                    _same(got, want, ("roots", itype.__name__, path, fpe))
                    assert cnt[2] == 0 and cnt[0] + cnt[1] == (0 if fpe == 1 else 512), (path, fpe, cnt)
    finally:
        ex.set_spic0_path(0)


@pytest.mark.parametrize("pad", X.DENSE_PADS)
def test_dense_range_cases_behind_idle_rows(ex, pad):
    low = []
    for name in X.DENSE_NAMES:
        c = X.dense_case(name, pad)
        model = X.dense_model(name, pad)
        assert (model[2] > 0) == (name in X.DENSE_STOPPED)
        low += _sweep(ex, c.csr, model, c.name)
    print(f"dense cases, pad {pad}: accumulator entries above the model's ties {min(low)}..{max(low)}")


@pytest.mark.parametrize("what", ["zero", "neg"])
@pytest.mark.parametrize("owned", [65, C.MAX_ROW])
def test_breakdowns_at_the_end_of_long_rows(ex, what, owned):
    c = X.long_breakdown(what, owned)
    model = _detail(c.csr)
    assert model[2] == c.row + 1
    _sweep(ex, c.csr, model, c.name)


# ---------------------------------------------------------------------------------------------
# 3. planted ties and near-ties in long rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", list(X.PLANTED_ALL))
def test_planted_ties_in_long_rows_are_never_decided_in_registers(ex, length):
    for spec in X.PLANTED_ALL[length]:
        model = X.planted_model(spec)
        d = model[3]
        assert model[1:3] == (0, 0)
        settle = d.ties + d.nears
        assert d.ties >= 16 and d.nears >= 9
        above = _sweep(ex, X.planted(*spec), model, ("planted", length, spec), settle, registers=True)
        print(f"planted {length} {spec}: ties {d.ties}, nears {d.nears}, accumulator entries above their sum "
              f"{min(above)}..{max(above)}")


# ---------------------------------------------------------------------------------------------
# 4. the reference rounding mode, where it differs from nearest-even
# ---------------------------------------------------------------------------------------------
def _in_reference_mode(ex, csr, model, owned, what):
    want, i0, i1, _ = model
    lib = ex.load_library()
    try:
        for path in (0, 2):
            ex.set_spic0_path(path)
            lib.exblas_set_round_mode(1)
            got, info, cnt = _factor(ex, _upload(csr, np.int32))
            assert info == (i0, i1) and cnt[0] == 0 and cnt[1] == owned, (what, path, info, cnt)
            _same(got, want, (what, path, "reference mode"))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_spic0_path(0)


@pytest.mark.parametrize("length", list(X.PLANTED))
def test_reference_rounding_mode_on_the_planted_variants(ex, length):
    for spec in X.PLANTED[length]:
        ref, even = X.planted_model(spec, True), X.planted_model(spec)
        assert (_bits(ref[0]) != _bits(even[0])).sum() >= 30, "the two rounding modes cannot be told apart"
        _in_reference_mode(ex, X.planted(*spec), ref, even[3].owned, spec)


def test_reference_rounding_mode_on_the_range_cases(ex):
    """the model with the reference rounding exists where the oracle's limbs hold every total (spic0_edge_cases.py: not in
    the subnormal classes and not where a square of the carrier overflows); every entry of the factor is rounded in that
    mode, and in the wide-range cancellation and the 2^1000 products it moves bits"""
    moved = ran = 0
    for length in (0, 65):
        for c in X.range_cases(length):
            ref = X.model(c, True)
            if ref is None:
                continue
            even = X.model(c)
            ran += 1
            moved += int((_bits(ref[0]) != _bits(even[0])).any())
            _in_reference_mode(ex, c.csr, ref, even[3].owned, c.name)
    assert ran >= 10 and moved >= 2, (ran, moved)


# ---------------------------------------------------------------------------------------------
# 5. the plain variant in its several-entries form
# ---------------------------------------------------------------------------------------------
def _plain_cases():
    return {"range, wide-range cancellation, 129": lambda: X.range_cases(129)[14].csr,
            "range, zero by cancellation, 65": lambda: X.range_cases(65)[9].csr,
            "range, wide source with reader": lambda: X.range_cases(0, X.WIDES[-1], True)[14].csr,
            "dense, partial sums, pad 64": lambda: X.dense_case("partial sums", 64).csr,
            "dense, subnormal total, pad 508": lambda: X.dense_case("subnormal total", 508).csr,
            "planted 130": lambda: X.planted(*X.PLANTED[130][0]),
            "planted 512": lambda: X.planted(*X.PLANTED[C.MAX_ROW][0]),
            "negative zero": X.negative_zero}


@pytest.mark.parametrize("name", list(_plain_cases()))
def test_plain_variant_in_the_several_entries_form(ex, name):
    csr = _plain_cases()[name]()
    want = C.plain_ic0(*csr)
    m = len(csr[0]) - 1
    rows = np.repeat(np.arange(m), np.diff(csr[0]))
    on = csr[1] == rows
    wide = int((np.bincount(rows[csr[1] <= rows], minlength=m) > 64).sum())      # rows that own more than 64 entries
    assert wide or name in ("negative zero", "range, wide source with reader")      # (there the SOURCE rows are wide)
    # info[1] of the plain form: its own first radicand that is not > 0, i.e. the first root that is not > 0 (the subnormal
    # radicand behind the planted systems is lost to fp64's rounding of the square)
    bad = np.nonzero(~(want[on] > 0))[0]
    info1 = int(bad[0]) + 1 if len(bad) else 0
    assert info1 == {"negative zero": 3, "planted 130": m, "planted 512": m}.get(name, 0)
    try:
        for path in (0, 2):
            ex.set_spic0_path(path)
            for itype in ITYPES:
                got, info, cnt = _factor(ex, _upload(csr, itype), fpe=1, ee=False)
                assert info == (0, info1) and cnt[0] == cnt[1] == 0, (name, path, info, cnt)
                assert cnt[3] == (m if path == 2 else wide), (name, path, cnt)
                _same(got, want, ("plain", name, path))          # (bit for bit: the sign of a zero as well)
    finally:
        ex.set_spic0_path(0)


# ---------------------------------------------------------------------------------------------
# 6. the small structures
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.SMALL))
def test_small_structures(ex, name):
    """negative zero: the exact paths give +0.0 for the stored -0.0 at (1, 0) and for the radicand -0.0 of row 2, which
    info[1] = 3 reports (spic0_edge_cases.negative_zero; the plain form, which keeps the signs, is held above)"""
    csr = X.SMALL[name]()
    model = _detail(csr)
    assert model[1:3] == (0, X.SMALL_INFO[name])
    _sweep(ex, csr, model, name)


def test_an_empty_matrix_is_factored_into_nothing(ex):
    import torch
    for itype in (torch.int32, torch.int64):
        A = (torch.zeros(1, dtype=itype, device="cuda"), torch.zeros(0, dtype=itype, device="cuda"),
             torch.zeros(0, dtype=torch.float64, device="cuda"), (0, 0))
        info = torch.full((2,), 7, dtype=torch.int64, device="cuda")
        LL, got = ex.exspic0_dev(A, info=info)
        assert got is info and tuple(info.cpu().tolist()) == (0, 0) and LL[2].numel() == 0
        assert _counters(ex) == (0, 0, 0, 0)


# ---------------------------------------------------------------------------------------------
# 7. capture: factor and apply replayed after a breakdown
# ---------------------------------------------------------------------------------------------
def test_captured_factor_and_apply_start_fresh_after_a_breakdown(ex):
    """one graph of factor + apply, replayed on healthy values, on a zero radicand, on other healthy values and on two range
    value sets.  The factor and info are compared on every replay; the applied vector where the factor is healthy (with the
    range values the sweeps form products below 2^-968 that are not exact, outside the solves' product domain, and a
    non-finite factor leaves the exact model of the solve)."""
    import torch
    crow, col = X.replay_pattern()
    sets = X.replay_sets()
    m = len(crow) - 1
    b = np.random.default_rng(16).integers(-8, 9, m).astype(np.float64)
    A = _upload((crow, col, sets[0][1]), np.int32)
    LL, info = ex.exspic0_dev(A)                       # the warm calls that size the workspaces
    _counters(ex)
    x = torch.from_numpy(b.copy()).cuda()
    ex.exspic0_apply_dev(LL, x)
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exspic0_dev(A, out=LL[2], info=info)
            ex.exspic0_apply_dev(LL, x)
    assert [n for n, _ in sets[:3]] == ["healthy", "zero radicand", "healthy again"] and len(sets) == 5
    for turn, (name, v) in enumerate(sets):
        want, i0, i1 = C.ic0_exact(crow, col, v)
        assert i0 == 0 and (i1 == 2) == (name == "zero radicand")
        A[2].copy_(torch.from_numpy(v))
        x.copy_(torch.from_numpy(b))
        LL[2].copy_(torch.from_numpy(np.random.default_rng(turn).random(len(v)) * 1e9))
        info.fill_(77 + turn)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        _counters(ex)
        assert tuple(info.cpu().tolist()) == (0, i1), (name, info)
        _same(LL[2].cpu().numpy(), want, ("replayed factor", name))
        if name.startswith("healthy"):
            _same(x.cpu().numpy(), C.apply_exact(crow, col, want, b.copy()), ("replayed apply", name))
