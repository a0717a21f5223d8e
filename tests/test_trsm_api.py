"""CPU suite: the C signatures of ExTRSM, the layout decision of its Python layer (which triangle and which transpose the
C call gets for a column-major or a row-major A), and the argument validation, all without a device."""
import ctypes

import numpy as np
import pytest
import torch

import exblas_amd

SYMBOLS = ("exblas_extrsm_dev", "exblas_extrsm_ctx", "exblas_extrsm", "exblas_set_trsm_path", "exblas_last_trsm_info")


def test_symbols_in_abi_list_and_signatures():
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS
    lib = exblas_amd.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    dev = lib.exblas_extrsm_dev.argtypes
    assert len(dev) == 12 and len(lib.exblas_extrsm_ctx.argtypes) == 13 and len(lib.exblas_extrsm.argtypes) == 11
    # (uplo, transa, diag, n, k, a, lda, x, ldx, fpe, early_exit, stream): ldx is 64-bit, lda is an int
    assert all(dev[i] is ctypes.c_char for i in range(3)) and dev[3] is ctypes.c_int and dev[4] is ctypes.c_int
    assert dev[6] is ctypes.c_int and dev[8] is ctypes.c_int64
    assert lib.exblas_extrsm.argtypes[8] is ctypes.c_int64 and lib.exblas_extrsm_ctx.argtypes[9] is ctypes.c_int64
    assert lib.exblas_set_trsm_path.restype is None and len(lib.exblas_set_trsm_path.argtypes) == 1
    assert len(lib.exblas_last_trsm_info.argtypes) == 1
    for name in ("extrsm_dev", "extrsm", "set_trsm_path", "last_trsm_info", "_trsm_layout"):
        assert callable(getattr(exblas_amd, name))
    assert callable(exblas_amd.Context.extrsm)
    assert exblas_amd.extrsm_dev.__func__ is exblas_amd.Context.extrsm      # one body, bound to the default context


# ---------------------------------------------------------------------------------------------
# _trsm_layout
# ---------------------------------------------------------------------------------------------
def _column_major_reading(t, uplo, trans, lda):
    """op(A) as the C routine sees it: the storage of t read as column-major with leading dimension lda, the triangle
    `uplo` of that, transposed under 'T'"""
    n = t.shape[0]
    S = torch.as_strided(t, (n, n), (1, lda)).numpy()
    tri = np.tril(S) if uplo == "L" else np.triu(S)
    return tri.T if trans == "T" else tri


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("layout", ["row_major", "column_major"])
def test_layout_rebuilds_the_intended_operator(layout, uplo, trans, pad):
    n = 7
    rng = np.random.default_rng([n, pad, 5])
    full = rng.standard_normal((n, n))
    tri = np.tril(full) if uplo == "L" else np.triu(full)
    other = np.triu(full, 1) if uplo == "L" else np.tril(full, -1)
    intended = tri.T if trans == "T" else tri
    # A holds the triangle and, in the other one, values that must not come back
    wide = torch.zeros(n, n + pad, dtype=torch.float64)
    if layout == "row_major":
        wide[:, :n] = torch.from_numpy(tri + 100.0 * other)
        A = wide[:, :n]                                   # strides (n + pad, 1)
        assert A.stride(1) == 1
    else:
        wide[:, :n] = torch.from_numpy((tri + 100.0 * other).T)
        A = wide[:, :n].t()                               # strides (1, n + pad)
        assert A.stride(0) == 1
    assert (A.numpy() == tri + 100.0 * other).all()
    u, t, lda = exblas_amd._trsm_layout(A, uplo, trans)
    assert lda == n + pad and u in ("L", "U") and t in ("N", "T")
    if layout == "column_major":
        assert (u, t) == (uplo, trans)
    else:
        assert u != uplo and t != trans                   # the storage is that of A^T: both flip
    assert (_column_major_reading(A, u, t, lda) == intended).all()
    # lower case is accepted and normalised
    assert exblas_amd._trsm_layout(A, uplo.lower(), trans.lower()) == (u, t, lda)


def test_layout_refuses_what_it_cannot_pass_on():
    base = torch.zeros(8, 16, dtype=torch.float64)
    with pytest.raises(ValueError) as err:
        exblas_amd._trsm_layout(base[:, ::2], "L", "N")               # strides (16, 2): no unit stride
    assert str(err.value).startswith("extrsm:")
    with pytest.raises(ValueError):
        exblas_amd._trsm_layout(torch.zeros(1, 4, dtype=torch.float64).expand(4, 4), "L", "N")    # strides (0, 1)
    with pytest.raises(ValueError):
        exblas_amd._trsm_layout(base[:, :8], "X", "N")
    with pytest.raises(ValueError):
        exblas_amd._trsm_layout(base[:, :8], "L", "C")
    with pytest.raises(ValueError):
        exblas_amd._trsm_layout(base[:, :8], 1, "N")
    # n <= 1: any strides, lda = 1
    assert exblas_amd._trsm_layout(torch.zeros(1, 1, dtype=torch.float64), "U", "T") == ("U", "T", 1)
    assert exblas_amd._trsm_layout(torch.zeros(0, 0, dtype=torch.float64), "L", "N") == ("L", "N", 1)


# ---------------------------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", ["not_square", "a_dtype", "x_dtype", "a_1d", "a_3d", "a_no_unit_stride", "x_1d", "x_3d",
                                 "x_rows_short", "x_rows_long", "x_col_major", "x_col_strided", "x_rows_overlap", "uplo",
                                 "diag", "trans", "uplo_type", "trans_type", "devices", "a_not_tensor", "x_not_tensor",
                                 "fpe9", "fpe_negative"])
def test_extrsm_dev_rejects_bad_arguments(bad):
    """every one of these is refused before a GPU is needed (ValueError / TypeError, never the no-GPU RuntimeError)"""
    A = torch.eye(4, dtype=torch.float64)
    x = torch.ones(4, 3, dtype=torch.float64)
    uplo, trans, diag, fpe = "L", "N", "N", 8
    if bad == "not_square":
        A = torch.ones(4, 5, dtype=torch.float64)
    elif bad == "a_dtype":
        A = A.float()
    elif bad == "x_dtype":
        x = x.float()
    elif bad == "a_1d":
        A = torch.ones(4, dtype=torch.float64)
    elif bad == "a_3d":
        A = torch.ones(4, 4, 1, dtype=torch.float64)
    elif bad == "a_no_unit_stride":
        A = torch.ones(8, 8, dtype=torch.float64)[::2, ::2]      # stride (16, 2)
    elif bad == "x_1d":
        x = torch.ones(4, dtype=torch.float64)
    elif bad == "x_3d":
        x = torch.ones(4, 3, 1, dtype=torch.float64)
    elif bad == "x_rows_short":
        x = x[:3]
    elif bad == "x_rows_long":
        x = torch.ones(5, 3, dtype=torch.float64)
    elif bad == "x_col_major":
        x = torch.ones(3, 4, dtype=torch.float64).t()            # stride (1, 4)
    elif bad == "x_col_strided":
        x = torch.ones(4, 6, dtype=torch.float64)[:, ::2]        # stride (6, 2)
    elif bad == "x_rows_overlap":
        x = torch.ones(1, 3, dtype=torch.float64).expand(4, 3)   # stride (0, 1): stride(0) < k
    elif bad == "uplo":
        uplo = "X"
    elif bad == "diag":
        diag = "T"
    elif bad == "trans":
        trans = "C"
    elif bad == "uplo_type":
        uplo = 1
    elif bad == "trans_type":
        trans = None
    elif bad == "devices":
        x = torch.ones(4, 3, dtype=torch.float64, device="meta")
    elif bad == "a_not_tensor":
        A = np.eye(4)
    elif bad == "x_not_tensor":
        x = np.ones((4, 3))
    elif bad == "fpe9":
        fpe = 9
    elif bad == "fpe_negative":
        fpe = -1
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.extrsm_dev(A, x, uplo, trans, diag, fpe)
    assert str(err.value).startswith("extrsm:")                  # the routine that was called, whichever helper refused
    if bad == "x_1d":
        assert "extrsv_dev" in str(err.value)                    # one vector: the message names the routine for it
    if bad == "fpe9":
        assert isinstance(err.value, ValueError)
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.Context.extrsm(ctx, A, x, uplo, trans, diag, fpe)
    assert str(err.value).startswith("extrsm:")


def test_an_overlapping_block_with_stride_one_less_than_k_is_refused():
    base = torch.ones(16, dtype=torch.float64)
    with pytest.raises(ValueError) as err:
        exblas_amd.extrsm_dev(torch.eye(4, dtype=torch.float64), base.as_strided((4, 3), (2, 1)))
    assert str(err.value).startswith("extrsm:")


def test_host_extrsm_rejects_bad_arguments():
    A = np.eye(2)
    B = np.ones((2, 3))
    cases = [
        (TypeError, dict(A=A.astype(np.float32))),
        (TypeError, dict(B=B.astype(np.float32))),
        (ValueError, dict(A=np.ones((2, 3)))),
        (ValueError, dict(A=np.ones(2))),
        (ValueError, dict(A=np.ones((2, 2, 1)))),
        (ValueError, dict(B=np.ones((3, 3)))),
        (ValueError, dict(B=np.ones((2, 3, 1)))),
        (ValueError, dict(uplo="T")),
        (ValueError, dict(trans="X")),
        (ValueError, dict(diag="X")),
        (ValueError, dict(fpe=9)),
        (ValueError, dict(fpe=-2)),
    ]
    for exc, change in cases:
        kw = dict(A=A, B=B, uplo="L", trans="N", diag="N", fpe=8)
        kw.update(change)
        with pytest.raises(exc) as err:
            exblas_amd.extrsm(kw["A"], kw["B"], kw["uplo"], kw["trans"], kw["diag"], kw["fpe"])
        assert str(err.value).startswith("extrsm:"), change
    with pytest.raises(ValueError) as err:
        exblas_amd.extrsm(A, np.ones(2))
    assert "extrsv" in str(err.value)


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        exblas_amd.extrsm_dev(torch.eye(4, dtype=torch.float64), torch.ones(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        exblas_amd.extrsm_dev(torch.eye(4, dtype=torch.float64).t(), torch.ones(4, 3, dtype=torch.float64), "U", "T", "U", 0)
    with pytest.raises(RuntimeError):
        exblas_amd.extrsm(np.eye(4), np.ones((4, 3)))
