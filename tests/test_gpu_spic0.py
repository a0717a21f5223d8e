"""ExSpIC0 on the GPU, bit for bit against spic0_cases.ic0_exact (the definition in exact arithmetic, never the code under
test): every builder case on every path, index width, fpe, early_exit, out of place and in place; the mirror above the
diagonal; NaN above the diagonal of A; ExPOTRF on the dense cases; the counters (a tie decided in registers fails even
where it happens to give the right bits); the structural defects of both phases (ll untouched); the breakdowns; factor +
apply against trsv_exact applied with L and then with L^T; graph capture and replay on new values and beyond the captured
nnz; the reference rounding mode; the plain variant; the host entry.  After every call the watchdog flag is read."""
import ctypes

import numpy as np
import pytest

import spic0_cases as C
from helpers import assert_bits as _same, bits as _bits

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2)
ITYPES = (np.int32, np.int64)
FPES = (0, 2, 8)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_spic0_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _counters(ex):
    """the watchdog of the last call is clear (the C entry returns 0); returns the counters"""
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_spic0_info(out) == 0, "the watchdog was raised"
    return tuple(int(v) for v in out)


def _upload(csr, itype=np.int64):
    import torch
    crow, col, val = C.as_width(csr, itype)
    m = len(crow) - 1
    return (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val.copy()).cuda(), (m, m))


def _blank(n):
    return np.full(n, C.NAN_BITS, dtype=np.uint64).view(np.float64)


def _factor(ex, A, fpe=8, ee=True, inplace=False, entry=None):
    """(ll, (info0, info1), counters) of one call; out of place into a NaN-filled vector, in place on a copy of A's values"""
    import torch
    val = A[2].clone()
    out = val if inplace else torch.from_numpy(_blank(val.numel())).cuda()
    LL, info = (entry or ex.exspic0_dev)((A[0], A[1], val, A[3]), out=out, fpe=fpe, early_exit=ee)
    assert LL[2] is out and LL[0] is A[0] and LL[1] is A[1] and LL[3] == A[3]
    cnt = _counters(ex) if entry is None else None
    info = tuple(int(v) for v in info.cpu().tolist())
    assert (_bits(val.cpu().numpy()) == _bits(A[2].cpu().numpy())).all() or inplace, "A's values were written"
    return out.cpu().numpy(), info, cnt


def _mirror_ok(csr, got):
    """the stored upper triangle is the transpose of the lower one, bit for bit"""
    crow, col, _ = csr
    m = len(crow) - 1
    where = {(r, int(col[p])): p for r in range(m) for p in range(int(crow[r]), int(crow[r + 1]))}
    up = [(p, where[(c, r)]) for (r, c), p in where.items() if c > r]
    return all(_bits(got[[a for a, _ in up]]) == _bits(got[[b for _, b in up]])) if up else True


# ---------------------------------------------------------------------------------------------
# 1. bit equality with the model, the mirror, 2. the counters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.SOUND))
def test_every_case_every_path_width_variant_and_place(ex, name):
    csr = C.SOUND[name]()
    want, i0, i1, d = C.expected(name)
    assert i0 == 0
    healthy = name in C.HEALTHY
    seen = []
    try:
        for itype in ITYPES:
            A = _upload(csr, itype)
            for path in PATHS:
                ex.set_spic0_path(path)
                for fpe in FPES:
                    for ee in (False, True):
                        for inplace in (False, True):
                            got, info, cnt = _factor(ex, A, fpe, ee, inplace)
                            what = (name, itype.__name__, path, fpe, ee, inplace, cnt)
                            assert info == (0, i1), what
                            _same(got, want, what)
                            assert _mirror_ok(csr, got), ("the upper triangle is not the mirror", what)
                            if healthy:
                                assert not np.isnan(got).any(), ("a position was not written", what)
                            assert cnt[0] + cnt[1] == d.owned and cnt[2] == d.terms, what
                            assert cnt[3] == (len(csr[0]) - 1 if path == 2 else d.wide), what
                            if path == 1 or fpe == 0:
                                assert cnt[0] == 0, what
                            else:
                                assert cnt[1] >= d.ties, ("a tie was decided in registers", what)
                                if healthy and d.ranged:
                                    assert cnt[1] <= d.ties + d.nears, ("a clear entry went to the accumulator", what)
                                seen.append(cnt[1])
    finally:
        ex.set_spic0_path(0)
    print(f"{name}: owned {d.owned}, terms {d.terms}, ties {d.ties}, nears {d.nears}, accumulator entries "
          f"{min(seen)}..{max(seen)}")


@pytest.mark.parametrize("name", ["random", "planted65", "arrow_last", "breakdown_neg"])
def test_nan_above_the_diagonal_changes_nothing(ex, name):
    crow, col, val = C.SOUND[name]()
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    junk = val.copy()
    junk[col > rows] = np.nan
    want, _, i1, _ = C.expected(name)
    for path in (0, 2):
        ex.set_spic0_path(path)
        try:
            got, info, _ = _factor(ex, _upload((crow, col, junk), np.int32))
        finally:
            ex.set_spic0_path(0)
        assert info == (0, i1)
        _same(got, want, (name, path))


# ---------------------------------------------------------------------------------------------
# 3. ExPOTRF
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [24, 64])
def test_dense_cases_equal_expotrf(ex, p):
    import torch
    csr, Gd = C.dense(p)
    R, inf = ex.expotrf_dev(torch.from_numpy(Gd.copy()).cuda(), "L")
    assert int(inf.cpu()[0]) == 0
    L = np.tril(R.cpu().numpy())
    for path in PATHS:
        ex.set_spic0_path(path)
        try:
            got, info, _ = _factor(ex, _upload(csr, np.int32))
        finally:
            ex.set_spic0_path(0)
        assert info == (0, 0)
        assert (_bits(np.tril(got.reshape(p, p))) == _bits(L)).all(), (p, path)


# ---------------------------------------------------------------------------------------------
# 4. structure
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.defects()))
def test_a_structural_defect_is_named_and_ll_is_not_written(ex, name):
    csr = C.defects()[name]
    _, i0, _ = C.ic0_exact(*csr)
    assert i0 > 0 and i0 == C.DEFECT_INFO.get(name, i0)
    blank = _blank(len(csr[2]))
    try:
        for itype in ITYPES:
            for path in PATHS:
                ex.set_spic0_path(path)
                for inplace in (False, True):
                    got, info, cnt = _factor(ex, _upload(csr, itype), inplace=inplace)
                    assert info == (i0, 0), (name, itype.__name__, path, info)
                    assert cnt == (0, 0, 0, 0)
                    assert (_bits(got) == _bits(csr[2] if inplace else blank)).all(), ("ll was written", name, path)
    finally:
        ex.set_spic0_path(0)


# ---------------------------------------------------------------------------------------------
# 5. the chain, 6. graph capture
# ---------------------------------------------------------------------------------------------
def test_factor_then_apply_on_a_vector_and_a_block(ex):
    import torch
    crow, col, val = C.SOUND["random"]()
    m = len(crow) - 1
    ll_want = C.expected("random")[0]
    B = np.random.default_rng(12).random((m, 4)) - 0.5
    want = np.stack([C.apply_exact(crow, col, ll_want, B[:, j].copy()) for j in range(4)], axis=1)
    for itype in ITYPES:
        A = _upload((crow, col, val), itype)
        LL, info = ex.exspic0_dev(A)
        assert tuple(info.cpu().tolist()) == (0, 0)
        x = torch.from_numpy(B[:, 0].copy()).cuda()
        assert ex.exspic0_apply_dev(LL, x) is x
        _same(x.cpu().numpy(), want[:, 0], "vector")
        X = torch.from_numpy(B.copy()).cuda()
        assert ex.exspic0_apply_dev(LL, X) is X
        _same(X.cpu().numpy(), want, "block")


def test_graph_capture_of_factor_and_apply_replayed_on_new_values_and_beyond_its_nnz(ex):
    import torch
    crow, col, val = C.SOUND["stencil7"]()
    m = len(crow) - 1
    rows = np.repeat(np.arange(m), np.diff(crow))
    rng = np.random.default_rng(13)
    sets = []
    for _ in range(2):
        v = val * (1.0 + 0.25 * rng.random(len(val)))
        v = np.where(col > rows, 0.0, v)
        v = C.dense_of(crow, col, v)
        v = np.tril(v) + np.tril(v, -1).T                      # symmetric again
        v = np.array([v[r, int(col[p])] for r in range(m) for p in range(int(crow[r]), int(crow[r + 1]))])
        sets.append(np.where(col > rows, -1e300 * rng.random(len(val)), v))   # junk above the diagonal
    b = rng.random(m) - 0.5
    A = _upload((crow, col, val), np.int32)
    LL, info = ex.exspic0_dev(A)                       # the warm calls that size the workspace
    x = torch.from_numpy(b.copy()).cuda()
    ex.exspic0_apply_dev(LL, x)
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exspic0_dev(A, out=LL[2], info=info)
            ex.exspic0_apply_dev(LL, x)
    for v in sets:
        ll_want, i0, i1 = C.ic0_exact(crow, col, v)
        assert (i0, i1) == (0, 0)
        A[2].copy_(torch.from_numpy(v))
        x.copy_(torch.from_numpy(b))
        LL[2].fill_(7.0)
        info.fill_(5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert tuple(info.cpu().tolist()) == (0, 0)
        _same(LL[2].cpu().numpy(), ll_want, "replayed factor")
        _same(x.cpu().numpy(), C.apply_exact(crow, col, ll_want, b.copy()), "replayed apply")
    # a factor alone, captured on this pattern and replayed with a last row that ends past the captured nnz: phase 1
    # refuses that row (nothing of col_idx beyond the captured nnz is read) and ll is not written
    crow_dev = A[0].clone()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g2, stream=s):
            ex.exspic0_dev((crow_dev, A[1], A[2], A[3]), out=LL[2], info=info)
    crow_dev[m] = int(crow[m]) + 2
    LL[2].copy_(torch.from_numpy(_blank(len(val))))
    info.fill_(5)
    torch.cuda.synchronize()
    g2.replay()
    torch.cuda.synchronize()
    assert tuple(info.cpu().tolist()) == (m, 0)
    assert (_bits(LL[2].cpu().numpy()) == _bits(_blank(len(val)))).all(), "ll was written"


# ---------------------------------------------------------------------------------------------
# 7. the reference rounding mode, the plain variant, the host entry
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.PLANTED)
def test_reference_rounding_mode_follows_the_model_with_the_reference_rounding(ex, name):
    csr = C.SOUND[name]()
    want, i0, i1, d = C.ic0_exact(*csr, rounder=C.reference_round, detail=True)
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        got, info, cnt = _factor(ex, _upload(csr, np.int32))
    finally:
        lib.exblas_set_round_mode(0)
    assert (i0, i1) == (0, 0) and info == (0, 0) and cnt[0] == 0 and cnt[1] == d.owned, cnt
    _same(got, want, ("reference mode", name))


@pytest.mark.parametrize("name", ["stencil27", "planted65", "arrow_last"])
def test_plain_variant_is_the_fixed_order_fp64_form(ex, name):
    csr = C.SOUND[name]()
    want = C.plain_ic0(*csr)
    for path in (0, 2):
        ex.set_spic0_path(path)
        try:
            got, info, cnt = _factor(ex, _upload(csr, np.int64), fpe=1, ee=False)
        finally:
            ex.set_spic0_path(0)
        assert info == (0, 0) and cnt[0] == cnt[1] == 0, cnt
        _same(got, want, ("plain", name, path))


def test_host_entry_equals_the_device_entry(ex):
    for name in ("random", "planted65", "breakdown_zero"):
        csr = C.SOUND[name]()
        A = _upload(csr)
        dev, dinfo, _ = _factor(ex, A)
        keep = csr[2].copy()
        ll, hinfo = ex.exspic0((csr[0], csr[1], csr[2], A[3]))
        assert hinfo == dinfo and (_bits(csr[2]) == _bits(keep)).all(), name
        assert (_bits(ll) == _bits(dev)).all() or (np.isnan(ll) == np.isnan(dev)).all() and \
            (_bits(ll[~np.isnan(ll)]) == _bits(dev[~np.isnan(dev)])).all(), name
    bad = C.defects()["missing mirror below"]
    ll, hinfo = ex.exspic0((bad[0].astype(np.int32), bad[1].astype(np.int32), bad[2], (12, 12)))
    assert hinfo == (8, 0) and (_bits(ll) == _bits(bad[2])).all()
