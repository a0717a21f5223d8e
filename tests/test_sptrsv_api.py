"""CPU suite: argument validation of the ExSpTRSV Python layer, the CSR helpers of the GPU tests, the C signatures."""
import numpy as np
import pytest
import torch

import exact_cases as X
import exblas_amd
import sptrsv_cases as S

SYMBOLS = ("exblas_exsptrsv_csr_dev", "exblas_exsptrsv_csr_ctx", "exblas_exsptrsv_csr", "exblas_set_sptrsv_path",
           "exblas_last_sptrsv_info")
# rows of class `tie` or `carry` in the seven non-unit planted systems (the GPU test's bar for the accumulator count)
TIE_ROWS = (15, 27, 30, 90, 63, 312, 348)


def _csr(itype=torch.int64):
    crow = torch.tensor([0, 1, 3, 4, 6], dtype=itype)
    col = torch.tensor([0, 0, 1, 2, 1, 3], dtype=itype)
    val = torch.arange(1, 7, dtype=torch.float64)
    return crow, col, val, (4, 4)


def test_symbols_in_abi_list_and_signatures():
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS
    lib = exblas_amd.load_library()
    dev = lib.exblas_exsptrsv_csr_dev.argtypes
    assert len(dev) == 11 and len(lib.exblas_exsptrsv_csr_ctx.argtypes) == 12 and len(lib.exblas_exsptrsv_csr.argtypes) == 10
    assert lib.exblas_set_sptrsv_path.restype is None and len(lib.exblas_last_sptrsv_info.argtypes) == 1
    for name in ("exsptrsv_dev", "exsptrsv", "set_sptrsv_path", "last_sptrsv_info"):
        assert callable(getattr(exblas_amd, name))
    assert callable(exblas_amd.Context.exsptrsv)


@pytest.mark.parametrize("bad", ["not_square", "val_dtype", "x_dtype", "mixed_width", "int16", "crow_len", "col_len",
                                 "x_short", "x_long", "x_2d", "x_strided", "uplo", "diag", "uplo_type", "devices",
                                 "shape3", "not_csr", "x_not_tensor"])
def test_exsptrsv_dev_rejects_bad_arguments(bad):
    """every one of these is refused before a GPU is needed (ValueError / TypeError, never the no-GPU RuntimeError)"""
    crow, col, val, shape = _csr()
    x = torch.ones(4, dtype=torch.float64)
    uplo, diag, A = "L", "N", None
    if bad == "not_square":
        shape = (4, 5)
    elif bad == "val_dtype":
        val = val.float()
    elif bad == "x_dtype":
        x = x.float()
    elif bad == "mixed_width":
        col = col.int()
    elif bad == "int16":
        crow, col = crow.short(), col.short()
    elif bad == "crow_len":
        crow = crow[:-1]
    elif bad == "col_len":
        col = col[:-1]
    elif bad == "x_short":
        x = x[:3]
    elif bad == "x_long":
        x = torch.ones(5, dtype=torch.float64)
    elif bad == "x_2d":
        x = torch.ones(4, 1, dtype=torch.float64)
    elif bad == "x_strided":
        x = torch.ones(8, dtype=torch.float64)[::2]
    elif bad == "uplo":
        uplo = "X"
    elif bad == "diag":
        diag = "T"
    elif bad == "uplo_type":
        uplo = 1
    elif bad == "devices":
        x = torch.ones(4, dtype=torch.float64, device="meta")
    elif bad == "shape3":
        shape = (4, 4, 1)
    elif bad == "not_csr":
        A = torch.zeros(4, 4, dtype=torch.float64)
    elif bad == "x_not_tensor":
        x = np.ones(4)
    if A is None:
        A = (crow, col, val, shape)
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.exsptrsv_dev(A, x, uplo, diag)
    assert str(err.value).startswith("exsptrsv:")   # the routine that was called, whichever helper refused
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.Context.exsptrsv(ctx, A, x, uplo, diag)
    assert str(err.value).startswith("exsptrsv:")


def test_host_exsptrsv_rejects_bad_arguments():
    crow = np.array([0, 1, 3], dtype=np.int64)
    col = np.array([0, 0, 1], dtype=np.int64)
    val = np.ones(3)
    good = (crow, col, val, (2, 2))
    with pytest.raises(TypeError):
        exblas_amd.exsptrsv((crow.astype(np.int32), col, val, (2, 2)), np.ones(2))
    with pytest.raises(TypeError):
        exblas_amd.exsptrsv(good, np.ones(2, dtype=np.float32))
    with pytest.raises(ValueError):
        exblas_amd.exsptrsv((crow, col, val, (2, 3)), np.ones(2))
    with pytest.raises(ValueError):
        exblas_amd.exsptrsv(good, np.ones(3))
    with pytest.raises(ValueError):
        exblas_amd.exsptrsv((np.array([0, 4, 3], dtype=np.int64), col, val, (2, 2)), np.ones(2))
    with pytest.raises(ValueError):
        exblas_amd.exsptrsv(good, np.ones(2), uplo="T")
    with pytest.raises(ValueError):
        exblas_amd.exsptrsv(good, np.ones(2), diag="X")


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    crow, col, val, shape = _csr()
    with pytest.raises(RuntimeError):
        exblas_amd.exsptrsv_dev((crow, col, val, shape), torch.ones(4, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        exblas_amd.exsptrsv((crow.numpy(), col.numpy(), val.numpy(), shape), np.ones(4))


@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("shuffle,junk", [(False, False), (True, False), (True, True)])
def test_helpers_round_trip(uplo, shuffle, junk):
    n, W, mbits, filler = X.TRSV_CASES[0]
    c = X.planted_trsv(n, seed=21, W=W, mbits=mbits, filler=filler)
    for itype in (np.int32, np.int64):
        crow, col, val, idx = S.csr_of_triangular(c.L, uplo, itype, shuffle=shuffle, junk=junk)
        assert crow.dtype == itype and col.dtype == itype and len(crow) == c.n + 1 and crow[-1] == len(col) == len(val)
        back, outside = S.densify(crow, col, val, uplo)
        assert (back.view(np.int64) == c.L.view(np.int64)).all()
        assert bool(outside) == junk
        for r, cc, v in outside:
            assert np.isnan(v) and (cc > r if uplo == "L" else cc < r)
        assert (idx == (np.arange(c.n) if uplo == "L" else np.arange(c.n)[::-1])).all()
        if not shuffle and uplo == "L":
            assert all((np.diff(col[crow[r]:crow[r + 1]]) > 0).all() for r in range(c.n))
    crow, col, val, _ = S.csr_of_triangular(c.L, uplo, np.int64, diag_nan=True)
    back, _ = S.densify(crow, col, val, uplo)
    assert np.isnan(np.diag(back)).all() and (np.tril(back, -1) == np.tril(c.L, -1)).all()


def test_structures_and_variants_of_the_helpers():
    for s in (S.chain(50), S.arrow(80), S.random_earlier(60), S.block_diagonal(4, 5), S.diagonal_only(9)):
        assert (np.triu(s.L, 1) == 0).all() and (np.abs(np.diag(s.L)) >= 1).all() and (np.abs(np.diag(s.L)) < 2).all()
        want, _ = X.trsv_exact(s.L, s.b)
        assert np.isfinite(want).all()
    a = S.arrow(80)
    assert (a.L[:, 0] != 0).all() and (a.L[-1] != 0).all() and np.count_nonzero(a.L[40]) == 2
    assert np.count_nonzero(S.block_diagonal(4, 5).L[7]) == 3
    r = S.random_earlier(60)
    crow, col, val, _ = S.csr_of_triangular(r.L, "L", np.int64)
    dcrow, dcol, dval, added = S.with_duplicates(crow, col, val)
    assert added > 20 and len(dcol) == len(col) + added
    P = np.zeros_like(r.L)
    for i in range(r.n):
        for p in range(dcrow[i], dcrow[i + 1]):
            P[i, dcol[p]] += dval[p]                        # exact: the two parts of a split entry
    assert (P == r.L).all()
    scrow, scol, sval = S.with_second_diagonal(crow, col, val)
    assert len(scol) == len(col) + r.n and np.isnan(sval[scrow[1:] - 1]).all()
    keep = np.tri(r.n, dtype=bool) & (np.arange(r.n)[:, None] - np.arange(r.n)[None, :] <= 2)
    zcrow, zcol, zval, _ = S.csr_of_triangular(r.L, "L", np.int64, keep=keep | (r.L != 0))
    assert (zval == 0).sum() > 20 and (S.densify(zcrow, zcol, zval)[0] == r.L).all()


def test_tie_rows_of_the_planted_systems():
    """the counts the GPU test holds the accumulator counter against, from the classes of the construction"""
    got = []
    for n, W, mbits, filler in X.TRSV_CASES:
        c = X.planted_trsv(n, seed=21, W=W, mbits=mbits, filler=filler, unit=False)
        got.append(int(((c.classes == "tie") | (c.classes == "carry")).sum()))
    assert tuple(got) == TIE_ROWS
