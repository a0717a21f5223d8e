"""ExSpILU0 on the GPU, bit for bit against spilu0_cases.ilu0_exact (the definition in exact arithmetic, never the code
under test): every builder case on every path, index width, fpe, early_exit, out of place and in place, on a second
context on a side stream and twice in a row; the counters (a tie or a near-tie inside the register margin decided in
registers fails even where it happens to give the right bits); the batched LU on the dense no-swap cases; the structural
defects (lu untouched) and the pivots; the chain factor + apply against trsv_exact applied twice; graph capture and replay
on new values; the reference rounding mode and the plain variant.  After every call the watchdog flag is read."""
import ctypes

import numpy as np
import pytest

import spilu0_cases as S
from helpers import assert_bits as _same, bits as _bits

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2)
ITYPES = (np.int32, np.int64)
FPES = (0, 2, 4, 8)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_spilu0_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _counters(ex):
    """the watchdog of the last call is clear (the C entry returns 0); returns the counters"""
    out = (ctypes.c_int64 * 4)()
    assert ex.load_library().exblas_last_spilu0_info(out) == 0, "the watchdog was raised"
    return tuple(int(v) for v in out)


def _upload(csr, itype=np.int64):
    import torch
    crow, col, val = S.as_width(csr, itype)
    m = len(crow) - 1
    return (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val.copy()).cuda(), (m, m))


def _factor(ex, A, fpe=8, ee=True, inplace=False, entry=None):
    """(lu, (info0, info1), counters) of one call; in place on a copy of A's values"""
    import torch
    val = A[2].clone()
    out = val if inplace else torch.from_numpy(np.full(val.numel(), S.NAN_BITS, dtype=np.uint64).view(np.float64)).cuda()
    LU, info = (entry or ex.exspilu0_dev)((A[0], A[1], val, A[3]), out=out, fpe=fpe, early_exit=ee)
    assert LU[2] is out and LU[0] is A[0] and LU[1] is A[1] and LU[3] == A[3]
    cnt = _counters(ex) if entry is None else None
    info = tuple(int(v) for v in info.cpu().tolist())
    assert (_bits(val.cpu().numpy()) == _bits(A[2].cpu().numpy())).all() or inplace, "A's values were written"
    return out.cpu().numpy(), info, cnt


# ---------------------------------------------------------------------------------------------
# 1. bit equality with the model, 2. the counters
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.SOUND))
def test_every_case_every_path_width_variant_and_place(ex, name):
    csr = S.SOUND[name]()
    want, i0, i1, d = S.expected(name)
    assert i0 == 0
    nnz, seen = len(want), []
    try:
        for itype in ITYPES:
            A = _upload(csr, itype)
            for path in PATHS:
                ex.set_spilu0_path(path)
                for fpe in FPES:
                    for ee in (False, True):
                        for inplace in (False, True):
                            got, info, cnt = _factor(ex, A, fpe, ee, inplace)
                            what = (name, itype.__name__, path, fpe, ee, inplace, cnt)
                            assert info == (0, i1), what
                            _same(got, want, what)
                            assert cnt[0] + cnt[1] == nnz and cnt[2] == d.terms, what
                            wide = len(csr[0]) - 1 if path == 2 else int((np.diff(csr[0]) > 64).sum())
                            assert cnt[3] == wide, what
                            if path == 1 or fpe == 0:
                                assert cnt[0] == 0, what
                            else:
                                assert cnt[1] >= d.ties, ("a tie was decided in registers", what)
                            seen.append(cnt[1])
    finally:
        ex.set_spilu0_path(0)
    print(f"{name}: nnz {nnz}, terms {d.terms}, ties {d.ties}, nears {d.nears}, accumulator entries {min(seen)}..{max(seen)}")


def test_planted_ties_and_near_ties_are_never_decided_in_registers(ex):
    """the planted near-ties lie 2^-40 of the half unit from their ties, the register certificate keeps 2^-30 clear: on
    every path they and the ties are rounded from the accumulator; a tie-free case shows that the counter tells them apart"""
    A = _upload(S.planted(), np.int32)
    want, _, _, d = S.expected("planted")
    assert min(d.ties_l, d.ties_u, d.nears_l, d.nears_u) >= 16
    clear, _, _, dc = S.expected("stencil7")
    assert dc.ties == 0 and dc.nears == 0
    C = _upload(S.SOUND["stencil7"](), np.int32)
    try:
        for path in (0, 2):
            ex.set_spilu0_path(path)
            got, info, cnt = _factor(ex, A)
            _same(got, want, ("planted", path))
            assert cnt[1] >= d.ties + d.nears, ("a tie or a near-tie inside the margin was decided in registers", path, cnt)
            assert cnt[0] > 0, ("nothing was rounded in registers", path, cnt)
            got, info, cnt = _factor(ex, C)
            _same(got, clear, ("stencil7", path))
            assert cnt[0] > 0 and cnt[0] + cnt[1] == len(clear), (path, cnt)
            print(f"path {path}: planted accumulator entries {d.ties + d.nears} expected at least; tie-free stencil7 {cnt}")
    finally:
        ex.set_spilu0_path(0)


def test_second_context_side_stream_and_repeat_and_host_arrays(ex):
    import torch
    csr = S.SOUND["random"]()
    want, i0, i1, _ = S.expected("random")
    A = _upload(csr)
    first, info, _ = _factor(ex, A)
    again, _, _ = _factor(ex, A)
    _same(first, want, "dev")
    assert (_bits(first) == _bits(again)).all()
    ctx, side = ex.Context(), torch.cuda.Stream()
    try:
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            got, info2, _ = _factor(ex, A, entry=ctx.exspilu0)
            both, _, _ = _factor(ex, A, inplace=True, entry=ctx.exspilu0)
        side.synchronize()
        assert info2 == info == (0, i1)
        assert (_bits(got) == _bits(first)).all() and (_bits(both) == _bits(first)).all(), "context on a side stream"
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
    keep = csr[2].copy()
    lu, hinfo = ex.exspilu0((csr[0], csr[1], csr[2], A[3]))
    assert hinfo == (0, i1) and (_bits(csr[2]) == _bits(keep)).all()
    assert (_bits(lu) == _bits(first)).all()
    bad = S.defects()["no stored diagonal"]
    lu, hinfo = ex.exspilu0((bad[0].astype(np.int32), bad[1].astype(np.int32), bad[2], (12, 12)))
    assert hinfo == (9, 0) and (_bits(lu) == _bits(bad[2])).all()


# ---------------------------------------------------------------------------------------------
# 3. the batched LU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [24, 64])
def test_dense_no_swap_cases_equal_the_batched_lu(ex, p):
    import torch
    csr, Ad = S.dense(p)
    LU, piv, inf = ex.exgetrf_batched_dev(torch.from_numpy(Ad.copy()).cuda().reshape(1, p, p))
    assert int(inf[0]) == 0 and (piv.cpu().numpy()[0] == np.arange(1, p + 1)).all()
    for path in PATHS:
        ex.set_spilu0_path(path)
        try:
            got, info, _ = _factor(ex, _upload(csr, np.int32))
        finally:
            ex.set_spilu0_path(0)
        assert info == (0, 0)
        assert (_bits(got.reshape(p, p)) == _bits(LU.cpu().numpy()[0])).all(), (p, path)


# ---------------------------------------------------------------------------------------------
# 4. structure and pivots
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.defects()))
def test_a_structural_defect_is_named_and_lu_is_not_written(ex, name):
    csr = S.defects()[name]
    _, i0, _ = S.ilu0_exact(*csr)
    assert i0 > 0
    blank = np.full(len(csr[2]), S.NAN_BITS, dtype=np.uint64).view(np.float64)
    try:
        for itype in ITYPES:
            for path in PATHS:
                ex.set_spilu0_path(path)
                for inplace in (False, True):
                    got, info, cnt = _factor(ex, _upload(csr, itype), inplace=inplace)
                    assert info == (i0, 0), (name, itype.__name__, path, info)
                    assert cnt == (0, 0, 0, 0)
                    assert (_bits(got) == _bits(csr[2] if inplace else blank)).all(), ("lu was written", name, path)
    finally:
        ex.set_spilu0_path(0)


@pytest.mark.parametrize("name", ["zero_pivot", "nonfinite"])
def test_zero_and_nan_pivots_are_reported_and_the_call_returns(ex, name):
    want, i0, i1, _ = S.expected(name)
    assert i0 == 0 and i1 > 0
    for fpe in (0, 8):
        got, info, _ = _factor(ex, _upload(S.SOUND[name](), np.int32), fpe)      # (_factor reads the watchdog flag)
        assert info == (0, i1), (name, fpe, info)
        _same(got, want, (name, fpe))


# ---------------------------------------------------------------------------------------------
# 5. the chain, 6. graph capture
# ---------------------------------------------------------------------------------------------
def test_factor_then_apply_on_a_vector_and_a_block(ex):
    import torch
    crow, col, val = S.tridiagonal()
    m = len(crow) - 1
    lu_want = S.expected("tridiagonal")[0]
    B = np.random.default_rng(12).random((m, 5)) - 0.5
    want = np.stack([S.apply_exact(crow, col, lu_want, B[:, j].copy()) for j in range(5)], axis=1)
    for itype in ITYPES:
        A = _upload((crow, col, val), itype)
        LU, info = ex.exspilu0_dev(A)
        assert tuple(info.cpu().tolist()) == (0, 0)
        x = torch.from_numpy(B[:, 0].copy()).cuda()
        assert ex.exspilu0_apply_dev(LU, x) is x
        _same(x.cpu().numpy(), want[:, 0], "vector")
        X = torch.from_numpy(B.copy()).cuda()
        assert ex.exspilu0_apply_dev(LU, X) is X
        _same(X.cpu().numpy(), want, "block")


def test_graph_capture_of_factor_and_apply_replayed_on_new_values(ex):
    import torch
    crow, col, val = S.SOUND["stencil5"]()
    m = len(crow) - 1
    rng = np.random.default_rng(13)
    sets = [val * (1.0 + 0.25 * rng.random(len(val))) for _ in range(2)]
    b = rng.random(m) - 0.5
    A = _upload((crow, col, val), np.int32)
    LU, info = ex.exspilu0_dev(A)                      # the warm calls that size the workspace
    x = torch.from_numpy(b.copy()).cuda()
    ex.exspilu0_apply_dev(LU, x)
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.exspilu0_dev(A, out=LU[2], info=info)
            ex.exspilu0_apply_dev(LU, x)
    for v in sets:
        lu_want, i0, i1 = S.ilu0_exact(crow, col, v)
        assert (i0, i1) == (0, 0)
        A[2].copy_(torch.from_numpy(v))
        x.copy_(torch.from_numpy(b))
        LU[2].fill_(7.0)
        info.fill_(5)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert tuple(info.cpu().tolist()) == (0, 0)
        _same(LU[2].cpu().numpy(), lu_want, "replayed factor")
        _same(x.cpu().numpy(), S.apply_exact(crow, col, lu_want, b.copy()), "replayed apply")


# ---------------------------------------------------------------------------------------------
# 7. the reference rounding mode and the plain variant
# ---------------------------------------------------------------------------------------------
_reference_round = S.reference_round      # (shared with the CPU tests of the edge cases)


def test_reference_rounding_mode_follows_the_model_with_the_reference_rounding(ex):
    csr = S.SOUND["stencil5"]()
    want, i0, i1 = S.ilu0_exact(*csr, rounder=_reference_round)
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    try:
        got, info, cnt = _factor(ex, _upload(csr, np.int32))
    finally:
        lib.exblas_set_round_mode(0)
    assert info == (0, 0) and cnt[0] == 0 and cnt[1] == len(want), cnt
    _same(got, want, "reference mode")


def test_plain_variant_is_the_fixed_order_fp64_form(ex):
    csr = S.SOUND["stencil5"]()
    want = S.plain_ilu0(*csr)
    for path in (0, 2):
        ex.set_spilu0_path(path)
        try:
            got, info, cnt = _factor(ex, _upload(csr, np.int64), fpe=1, ee=False)
        finally:
            ex.set_spilu0_path(0)
        assert info == (0, 0) and cnt[0] == cnt[1] == 0, cnt
        _same(got, want, ("plain", path))
