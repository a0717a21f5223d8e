"""ExSpILU0 on the GPU at its edges, bit for bit against spilu0_cases.ilu0_exact / plain_ilu0 / apply_exact on the cases
of spilu0_edge_cases.py (never the code under test): totals at the ends of the double range in rows of every class (8 to
512 entries, alone and behind a healthy block), planted ties in long rows, source rows of 64 and more entries, the
reference rounding mode where it differs, the plain variant in its several-entries form, the small structures, the
mailbox's reserved NaN, and captured graphs replayed after a breakdown and beyond their capacity.  The counters hold the
kernel to its certificate: what settles() names and the model's ties never come from the registers.  After every call the
watchdog flag is read."""
import numpy as np
import pytest

import spilu0_cases as S
import spilu0_edge_cases as X
from helpers import assert_bits as _same, bits as _bits
from test_gpu_spilu0 import ITYPES, PATHS, _counters, _factor, _upload, ex  # noqa: F401  (ex: the module's fixture)

pytestmark = pytest.mark.gpu

FPES = (0, 2, 8)
VARIANTS = X.variants()


def _wide_rows(csr, path):
    return len(csr[0]) - 1 if path == 2 else int((np.diff(csr[0]) > 64).sum())


# ---------------------------------------------------------------------------------------------
# 1. the range cases in every row class, alone and behind a healthy block
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,length,wide,reader", VARIANTS)
def test_range_totals_in_every_row_class_alone_and_behind_a_healthy_block(ex, form, length, wide, reader):
    cases = X.range_cases(form, length, wide, reader)
    assert len(cases) == 15
    lead = S.tridiagonal(X.LEAD)
    low = []
    try:
        for c in cases:
            for csr, (want, i0, i1, d) in ((c.csr, X.model(c)), (X.behind(lead, c.csr), X.behind_model(c))):
                assert i0 == 0
                nnz = len(want)
                for itype in ITYPES:
                    A = _upload(csr, itype)
                    for path in PATHS:
                        ex.set_spilu0_path(path)
                        for fpe in FPES:
                            for inplace in (False, True):
                                got, info, cnt = _factor(ex, A, fpe, True, inplace)
                                what = (c.name, nnz, itype.__name__, path, fpe, inplace, cnt)
                                assert info == (0, i1), what
                                _same(got, want, what)
                                assert cnt[0] + cnt[1] == nnz and cnt[2] == d.terms, what
                                assert cnt[3] == _wide_rows(csr, path), what
                                if path == 1 or fpe == 0:
                                    assert cnt[0] == 0, what
                                else:
                                    assert cnt[1] >= d.settle, ("a total outside the certificate's range or a tie was decided in registers", what)
                                    assert cnt[0] > 0, ("nothing was rounded in registers", what)
                                    low.append(cnt[1] - d.settle)
    finally:
        ex.set_spilu0_path(0)
    print(f"{form} length {length} wide {wide} reader {reader}: accumulator entries above the model's least {min(low)}..{max(low)}")


def test_a_later_row_meets_the_inf_of_the_overflow_tie_with_a_zero_multiplier(ex):
    c = X.inf_meets_zero()
    want, i0, i1, d = X.model(c)
    try:
        for path in PATHS:
            ex.set_spilu0_path(path)
            for fpe in FPES:
                got, info, cnt = _factor(ex, _upload(c.csr, np.int32), fpe)
                assert info == (0, i1), (path, fpe, info)
                _same(got, want, (c.name, path, fpe))
                assert cnt[0] + cnt[1] == len(want) and cnt[2] == d.terms and (path == 1 or fpe == 0 or cnt[1] >= d.settle), cnt
    finally:
        ex.set_spilu0_path(0)


# ---------------------------------------------------------------------------------------------
# 2. planted ties and near-ties in long rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", X.PLANTED_LENGTHS)
def test_planted_ties_in_long_rows_are_never_decided_in_registers(ex, length):
    csr = X.planted(X.planted_pad(length))
    want, i0, i1, d = X.planted_model(X.planted_pad(length))
    assert (i0, i1) == (0, 0) and min(d.ties_l, d.ties_u, d.nears_l, d.nears_u) >= 16
    try:
        for itype in ITYPES:
            A = _upload(csr, itype)
            for path in PATHS:
                ex.set_spilu0_path(path)
                for fpe in FPES:
                    for inplace in (False, True):
                        got, info, cnt = _factor(ex, A, fpe, True, inplace)
                        what = (length, itype.__name__, path, fpe, inplace, cnt)
                        assert info == (0, 0), what
                        _same(got, want, what)
                        assert cnt[0] + cnt[1] == len(want) and cnt[2] == d.terms, what
                        assert cnt[3] == _wide_rows(csr, path), what
                        if path == 1 or fpe == 0:
                            assert cnt[0] == 0, what
                        else:
                            assert cnt[1] >= d.ties + d.nears, ("a tie or a near-tie inside the margin was decided in registers", what)
                            assert cnt[0] > 0, ("nothing was rounded in registers", what)
    finally:
        ex.set_spilu0_path(0)


# ---------------------------------------------------------------------------------------------
# 3. the reference rounding mode, where it differs from nearest-even
# ---------------------------------------------------------------------------------------------
def _in_reference_mode(ex, csr, want, info1, what):
    lib = ex.load_library()
    try:
        for path in (0, 2):
            ex.set_spilu0_path(path)
            lib.exblas_set_round_mode(1)
            got, info, cnt = _factor(ex, _upload(csr, np.int32))
            assert info == (0, info1) and cnt[0] == 0 and cnt[1] == len(want), (what, path, info, cnt)
            _same(got, want, (what, path, "reference mode"))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_spilu0_path(0)


@pytest.mark.parametrize("length", X.PLANTED_LENGTHS)
def test_reference_rounding_mode_on_the_planted_variants(ex, length):
    csr = X.planted(X.planted_pad(length))
    want, i0, i1 = X.planted_model(X.planted_pad(length), True)
    even = X.planted_model(X.planted_pad(length))[0]
    assert i0 == 0 and (_bits(want) != _bits(even)).sum() == 30, "the two rounding modes cannot be told apart"
    _in_reference_mode(ex, csr, want, i1, length)


@pytest.mark.parametrize("form", X.FORMS)
def test_reference_rounding_mode_on_the_range_cases(ex, form):
    """the reference rounding agrees with nearest-even on each of the 15 totals of rows() (test_spilu0_edge_cases.py), but
    every entry of the factor is rounded in that mode, the multipliers in front of the total as well: the model with the
    reference rounding decides (in the wide-range cancellation it moves the multiplier -fl(v w) / 4 by one unit, and the
    total with it)"""
    moved = 0
    for length in (0, 65):
        for c in X.range_cases(form, length):
            want, i0, i1, _ = X.model(c, True)
            assert i0 == 0
            moved += int(_bits(want)[c.at] != _bits(X.model(c)[0])[c.at])
            _in_reference_mode(ex, c.csr, want, i1, c.name)
    assert moved == 2, moved


# ---------------------------------------------------------------------------------------------
# 4. the plain variant in its several-entries form
# ---------------------------------------------------------------------------------------------
def _plain_cases():
    out = {"arrow_band": S.arrow_band, "negative zero": X.negative_zero,
           "wide source": lambda: X.range_cases("U", 0, X.WIDES[-1], True)[-1].csr,
           "wide source, two passes": lambda: X.range_cases("L", 0, 64)[14].csr}
    for length in (130, S.MAX_ROW):
        out[f"planted {length}"] = (lambda n: lambda: X.planted(X.planted_pad(n)))(length)
    return out


@pytest.mark.parametrize("name", list(_plain_cases()))
def test_plain_variant_in_the_several_entries_form(ex, name):
    csr = _plain_cases()[name]()
    want = S.plain_ilu0(*csr)
    exact = S.ilu0_exact(*csr)[0]
    diag = want[csr[1] == np.repeat(np.arange(len(csr[0]) - 1), np.diff(csr[0]))]
    assert np.isfinite(diag).all() and (diag != 0).all()
    assert (_bits(want) != _bits(exact)).any(), "the plain and the exact form cannot be told apart here"
    try:
        for path in (0, 2):
            ex.set_spilu0_path(path)
            for itype in ITYPES:
                got, info, cnt = _factor(ex, _upload(csr, itype), fpe=1, ee=False)
                assert info == (0, 0) and cnt[0] == cnt[1] == 0 and cnt[3] == _wide_rows(csr, path), (name, path, info, cnt)
                _same(got, want, ("plain", name, path))          # (bit for bit: the sign of a zero as well)
    finally:
        ex.set_spilu0_path(0)


# ---------------------------------------------------------------------------------------------
# 5. wide sources through the chain, the small structures, the reserved NaN
# ---------------------------------------------------------------------------------------------
def test_factor_then_apply_on_a_wide_source_case(ex):
    import torch
    c = X.range_cases("U", 0, 64, False)[14]           # the wide-range cancellation: every support row is read
    assert c.cls == 5 and min(c.nu) == 65
    crow, col, val = c.csr
    lu_want = X.model(c)[0]
    assert np.isfinite(lu_want).all()
    b = np.random.default_rng(14).integers(-8, 9, c.m).astype(np.float64)
    b[:X.NSUP] = 0.0                                   # (the huge and tiny support values stay out of the sweeps' products)
    b[c.carrier:] = 0.0
    want = S.apply_exact(crow, col, lu_want, b.copy())
    assert np.isfinite(want).all() and (want != 0).sum() > 32
    for itype in ITYPES:
        A = _upload(c.csr, itype)
        LU, info = ex.exspilu0_dev(A)
        _counters(ex)
        assert tuple(info.cpu().tolist()) == (0, 0)
        _same(LU[2].cpu().numpy(), lu_want, "factor")
        x = torch.from_numpy(b.copy()).cuda()
        assert ex.exspilu0_apply_dev(LU, x) is x
        _same(x.cpu().numpy(), want, "apply")


@pytest.mark.parametrize("name", list(X.SMALL))
def test_small_structures(ex, name):
    csr = X.SMALL[name]()
    want, i0, i1, d = S.ilu0_exact(*csr, detail=True)
    assert (i0, i1) == (0, 0)
    try:
        for itype in ITYPES:
            for path in PATHS:
                ex.set_spilu0_path(path)
                for fpe in FPES:
                    for inplace in (False, True):
                        got, info, cnt = _factor(ex, _upload(csr, itype), fpe, True, inplace)
                        what = (name, itype.__name__, path, fpe, inplace, cnt)
                        assert info == (0, 0), what
                        _same(got, want, what)          # (bit for bit: the sign of a zero as well)
                        assert cnt[0] + cnt[1] == len(want) and cnt[2] == d.terms, what
    finally:
        ex.set_spilu0_path(0)


def test_an_empty_row_is_a_structural_defect(ex):
    csr = X.empty_row()
    blank = np.full(len(csr[2]), S.NAN_BITS, dtype=np.uint64).view(np.float64)
    try:
        for itype in ITYPES:
            for path in PATHS:
                ex.set_spilu0_path(path)
                for inplace in (False, True):
                    got, info, cnt = _factor(ex, _upload(csr, itype), inplace=inplace)
                    assert info == (7, 0) and cnt == (0, 0, 0, 0), (itype.__name__, path, info, cnt)
                    assert (_bits(got) == _bits(csr[2] if inplace else blank)).all(), ("lu was written", path)
    finally:
        ex.set_spilu0_path(0)


@pytest.mark.parametrize("where", ["pivot", "upper"])
def test_the_all_ones_nan_is_posted_and_fetched(ex, where):
    """ST_EMPTY is the all-ones NaN: a stored value with that pattern must reach the rows behind it as a NaN, not keep them
    waiting (the watchdog flag stays clear: _factor reads it)"""
    csr = X.empty_pattern_nan(where)
    exact, i0, i1 = S.ilu0_exact(*csr)
    assert i0 == 0 and i1 > 0
    for fpe in (8, 1):
        want = exact if fpe == 8 else S.plain_ilu0(*csr)
        got, info, cnt = _factor(ex, _upload(csr, np.int32), fpe, fpe != 1)
        assert info == (0, i1), (where, fpe, info)
        assert (np.isnan(got) == np.isnan(want)).all(), (where, fpe, got)
        _same(got, want, (where, fpe))           # (the finite entries; a NaN matches a NaN)


# ---------------------------------------------------------------------------------------------
# 6. capture: replays after a breakdown, and beyond the captured capacity
# ---------------------------------------------------------------------------------------------
def _junk(t, k):
    import torch
    t.copy_(torch.from_numpy(np.random.default_rng(k).random(t.numel()) * 1e9))


def test_captured_factor_starts_fresh_after_a_breakdown(ex):
    import torch
    crow, col, val = S.zero_pivot()
    sets = X.zero_pivot_sets()
    A = _upload((crow, col, sets[0][1]), np.int32)
    LU, info = ex.exspilu0_dev(A)                      # the warm call that sizes the workspace
    _counters(ex)
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exspilu0_dev(A, out=LU[2], info=info)
    assert [n for n, _ in sets[:3]] == ["healthy", "zero pivot", "healthy again"] and len(sets) == 5
    for turn, (name, v) in enumerate(sets):
        want, i0, i1 = S.ilu0_exact(crow, col, v)
        assert i0 == 0 and (i1 > 0) == (name == "zero pivot")
        A[2].copy_(torch.from_numpy(v))
        _junk(LU[2], turn)
        info.fill_(77 + turn)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        cnt = _counters(ex)
        assert tuple(info.cpu().tolist()) == (0, i1), (name, info)
        _same(LU[2].cpu().numpy(), want, ("replay", name))
        assert cnt[0] + cnt[1] == len(want), (name, cnt)


def test_captured_factor_refuses_a_row_beyond_its_capacity(ex):
    """the documented rule: a captured call takes the mailbox of the warm call before it, and a row that ends beyond those
    nnz_1 entries is a structural defect of the replay: info[0] names the first such row and lu is not written"""
    import torch
    m = 12
    first = S.tridiagonal(m)
    rng = np.random.default_rng(15)
    rows = [{c: -float(rng.random()) for c in range(i - 2, i + 3) if 0 <= c < m} for i in range(m)]
    for i, r in enumerate(rows):
        r[i] = 6.0 + float(rng.random())
    second = S.from_rows(rows)
    n1, n2 = len(first[2]), len(second[2])
    assert n1 == 34 and n2 == 54 and S.structure(second[0], second[1], m) == 0
    refused = int(np.nonzero(second[0][1:] > n1)[0][0])
    assert refused == 7 and second[0][refused] <= n1

    def fill(dst, src):
        dst.zero_()
        dst[:len(src)].copy_(torch.from_numpy(src))
    crow = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
    col = torch.zeros(n2, dtype=torch.int32, device="cuda")
    val = torch.ones(n2, dtype=torch.float64, device="cuda")
    lu = torch.zeros(n2, dtype=torch.float64, device="cuda")
    fill(crow, first[0].astype(np.int32)), fill(col, first[1].astype(np.int32)), fill(val, first[2])
    A = (crow, col, val, (m, m))
    LU, info = ex.exspilu0_dev(A, out=lu)              # the warm call: the mailbox holds nnz_1 entries
    _counters(ex)
    want1 = S.ilu0_exact(*first)[0]
    _same(lu.cpu().numpy()[:n1], want1, "warm")
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exspilu0_dev(A, out=lu, info=info)
    blank = torch.from_numpy(np.full(n2, S.NAN_BITS, dtype=np.uint64).view(np.float64)).cuda()
    for csr, i0 in ((second, refused + 1), (first, 0)):
        fill(crow, csr[0].astype(np.int32)), fill(col, csr[1].astype(np.int32)), fill(val, csr[2])
        lu.copy_(blank)
        info.fill_(99)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        cnt = _counters(ex)
        got = lu.cpu().numpy()
        assert tuple(info.cpu().tolist()) == (i0, 0), (i0, info)
        if i0:
            assert (_bits(got) == S.NAN_BITS).all() and cnt == (0, 0, 0, 0), "lu was written by a refused replay"
        else:
            _same(got[:n1], want1, "the first pattern again")
            assert (_bits(got[n1:]) == S.NAN_BITS).all() and cnt[0] + cnt[1] == n1
