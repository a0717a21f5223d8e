"""CPU suite: the C signatures of ExBTRSM, the layout decision of its Python layer (which triangle and which transpose the
C call gets for a column-major or a row-major T), and the argument validation of the Python layer and of the C entries,
all without a device."""
import ctypes

import numpy as np
import pytest
import torch

import exblas_amd

SYMBOLS = ("exblas_exbtrsm_dev", "exblas_exbtrsm_ctx", "exblas_exbtrsm", "exblas_set_btrsm_path", "exblas_last_btrsm_info")
INVALID, UNSUPPORTED = 1, -1                     # hipErrorInvalidValue, EXBLAS_UNSUPPORTED


def test_symbols_in_abi_list_and_signatures():
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS
    lib = exblas_amd.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    dev, ctx, host = lib.exblas_exbtrsm_dev.argtypes, lib.exblas_exbtrsm_ctx.argtypes, lib.exblas_exbtrsm.argtypes
    assert len(dev) == 13 and len(ctx) == 14 and len(host) == 12
    # (uplo, transt, diag, n, p, alpha, t, ldt, x, ldx, fpe, early_exit, stream): n and ldx are 64-bit, p and ldt ints
    for args, off in ((dev, 0), (ctx, 1), (host, 0)):
        assert all(args[off + i] is ctypes.c_char for i in range(3))
        assert args[off + 3] is ctypes.c_int64 and args[off + 4] is ctypes.c_int and args[off + 5] is ctypes.c_double
        assert args[off + 6] is ctypes.c_void_p and args[off + 7] is ctypes.c_int
        assert args[off + 8] is ctypes.c_void_p and args[off + 9] is ctypes.c_int64
        assert args[off + 10] is ctypes.c_int and args[off + 11] is ctypes.c_int
    assert ctx[0] is ctypes.c_void_p and dev[12] is ctypes.c_void_p
    assert lib.exblas_set_btrsm_path.restype is None and len(lib.exblas_set_btrsm_path.argtypes) == 1
    assert len(lib.exblas_last_btrsm_info.argtypes) == 1
    for name in ("exbtrsm_dev", "exbtrsm", "set_btrsm_path", "last_btrsm_info"):
        assert callable(getattr(exblas_amd, name))
    assert callable(exblas_amd.Context.exbtrsm)
    assert exblas_amd.exbtrsm_dev.__func__ is exblas_amd.Context.exbtrsm    # one body, bound to the default context
    assert exblas_amd.BTRSM_MAX_P == 512
    header = open(exblas_amd.__file__.replace("exblas_amd/__init__.py", "include/exblas_hip.h")).read()
    assert "#define EXBLAS_BTRSM_MAX_P 512" in header


# ---------------------------------------------------------------------------------------------
# the layout flip
# ---------------------------------------------------------------------------------------------
def _column_major_reading(t, uplo, trans, ldt):
    """op(T) as the C routine sees it: the storage of t read as column-major with leading dimension ldt, the triangle
    `uplo` of that, transposed under 'T'"""
    p = t.shape[0]
    S = torch.as_strided(t, (p, p), (1, ldt)).numpy()
    tri = np.tril(S) if uplo == "L" else np.triu(S)
    return tri.T if trans == "T" else tri


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("trans", ["N", "T"])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("layout", ["row_major", "column_major"])
def test_layout_rebuilds_the_intended_operator(layout, uplo, trans, pad):
    p = 7
    rng = np.random.default_rng([p, pad, 6])
    full = rng.standard_normal((p, p))
    tri = np.tril(full) if uplo == "L" else np.triu(full)
    other = np.triu(full, 1) if uplo == "L" else np.tril(full, -1)
    intended = tri.T if trans == "T" else tri
    wide = torch.zeros(p, p + pad, dtype=torch.float64)
    if layout == "row_major":
        wide[:, :p] = torch.from_numpy(tri + 100.0 * other)
        T = wide[:, :p]                                   # strides (p + pad, 1)
    else:
        wide[:, :p] = torch.from_numpy((tri + 100.0 * other).T)
        T = wide[:, :p].t()                               # strides (1, p + pad)
    assert (T.numpy() == tri + 100.0 * other).all()
    x = torch.ones(5, p, dtype=torch.float64)
    # _btrsm_args refuses only at its very end, for want of a GPU: take the C arguments from the layout helper it uses
    u, t, ldt = exblas_amd._trsm_layout(T, uplo, trans, "exbtrsm")
    assert ldt == p + pad
    if layout == "column_major":
        assert (u, t) == (uplo, trans)
    else:
        assert u != uplo and t != trans                   # the storage is that of T^T: both flip
    assert (_column_major_reading(T, u, t, ldt) == intended).all()
    args = exblas_amd._btrsm_triangle(T, tuple(T.shape), T, uplo.lower(), trans.lower(), "n")
    assert args == (u.encode(), t.encode(), b"n", p, ldt)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                 # everything else was in order
            exblas_amd.exbtrsm_dev(T, x, uplo, trans)


def test_layout_names_the_routine_that_was_called():
    base = torch.zeros(8, 16, dtype=torch.float64)
    with pytest.raises(ValueError) as err:
        exblas_amd._trsm_layout(base[:, ::2], "L", "N", "exbtrsm")
    assert str(err.value).startswith("exbtrsm:")
    with pytest.raises(ValueError) as err:
        exblas_amd._trsm_layout(base[:, ::2], "L", "N")               # the default keeps ExTRSM's messages
    assert str(err.value).startswith("extrsm:")
    for bad in (("X", "N"), ("L", "C"), (1, "N")):
        with pytest.raises(ValueError) as err:
            exblas_amd._trsm_layout(base[:, :8], *bad, who="exbtrsm")
        assert str(err.value).startswith("exbtrsm:")
        with pytest.raises(ValueError) as err:
            exblas_amd._trsm_layout(base[:, :8], *bad)
        assert str(err.value).startswith("extrsm:")


# ---------------------------------------------------------------------------------------------
# argument validation: the Python layer
# ---------------------------------------------------------------------------------------------
BAD = ["t_dtype", "x_dtype", "t_not_tensor", "x_not_tensor", "t_1d", "t_3d", "t_not_square", "t_no_unit_stride", "x_1d",
       "x_3d", "x_cols_short", "x_cols_long", "x_col_major", "x_col_strided", "x_rows_overlap", "x_rows_overlap_by_one",
       "uplo", "trans", "diag", "uplo_type", "trans_type", "diag_type", "devices", "fpe9", "fpe_negative", "p_too_large",
       "x_is_t"]


@pytest.mark.parametrize("bad", BAD)
def test_exbtrsm_dev_rejects_bad_arguments(bad):
    """every one of these is a ValueError that names the routine, raised before a GPU is needed"""
    T = torch.eye(4, dtype=torch.float64)
    x = torch.ones(6, 4, dtype=torch.float64)
    uplo, trans, diag, fpe = "U", "N", "N", 8
    if bad == "t_dtype":
        T = T.float()
    elif bad == "x_dtype":
        x = x.float()
    elif bad == "t_not_tensor":
        T = np.eye(4)
    elif bad == "x_not_tensor":
        x = np.ones((6, 4))
    elif bad == "t_1d":
        T = torch.ones(4, dtype=torch.float64)
    elif bad == "t_3d":
        T = torch.ones(4, 4, 1, dtype=torch.float64)
    elif bad == "t_not_square":
        T = torch.ones(4, 5, dtype=torch.float64)
    elif bad == "t_no_unit_stride":
        T = torch.ones(8, 8, dtype=torch.float64)[::2, ::2]      # stride (16, 2)
    elif bad == "x_1d":
        x = torch.ones(4, dtype=torch.float64)
    elif bad == "x_3d":
        x = torch.ones(6, 4, 1, dtype=torch.float64)
    elif bad == "x_cols_short":
        x = torch.ones(6, 3, dtype=torch.float64)
    elif bad == "x_cols_long":
        x = torch.ones(6, 5, dtype=torch.float64)
    elif bad == "x_col_major":
        x = torch.ones(4, 6, dtype=torch.float64).t()            # stride (1, 6)
    elif bad == "x_col_strided":
        x = torch.ones(6, 8, dtype=torch.float64)[:, ::2]        # stride (8, 2)
    elif bad == "x_rows_overlap":
        x = torch.ones(1, 4, dtype=torch.float64).expand(6, 4)   # stride (0, 1)
    elif bad == "x_rows_overlap_by_one":
        x = torch.ones(32, dtype=torch.float64).as_strided((6, 4), (3, 1))   # stride(0) = 3 < p
    elif bad == "uplo":
        uplo = "X"
    elif bad == "trans":
        trans = "C"
    elif bad == "diag":
        diag = "T"
    elif bad == "uplo_type":
        uplo = 1
    elif bad == "trans_type":
        trans = None
    elif bad == "diag_type":
        diag = 0
    elif bad == "devices":
        x = torch.ones(6, 4, dtype=torch.float64, device="meta")
    elif bad == "fpe9":
        fpe = 9
    elif bad == "fpe_negative":
        fpe = -1
    elif bad == "p_too_large":
        T = torch.eye(513, dtype=torch.float64)
        x = torch.ones(2, 513, dtype=torch.float64)
    elif bad == "x_is_t":
        x = T
    with pytest.raises(ValueError) as err:
        exblas_amd.exbtrsm_dev(T, x, uplo, trans, diag, 1.0, fpe)
    assert str(err.value).startswith("exbtrsm:"), err.value
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises(ValueError) as err:
        exblas_amd.Context.exbtrsm(ctx, T, x, uplo, trans, diag, 1.0, fpe)
    assert str(err.value).startswith("exbtrsm:")


def test_host_exbtrsm_rejects_bad_arguments():
    T, B = np.eye(3), np.ones((2, 3))
    cases = [
        (TypeError, dict(T=T.astype(np.float32))),
        (TypeError, dict(B=B.astype(np.float32))),
        (ValueError, dict(T=np.ones((3, 4)))),
        (ValueError, dict(T=np.ones(3))),
        (ValueError, dict(T=np.ones((3, 3, 1)))),
        (ValueError, dict(T=np.eye(513), B=np.ones((1, 513)))),
        (ValueError, dict(B=np.ones((2, 4)))),
        (ValueError, dict(B=np.ones(3))),
        (ValueError, dict(B=np.ones((2, 3, 1)))),
        (ValueError, dict(uplo="T")),
        (ValueError, dict(trans="X")),
        (ValueError, dict(diag="X")),
        (ValueError, dict(fpe=9)),
        (ValueError, dict(fpe=-2)),
    ]
    for exc, change in cases:
        kw = dict(T=T, B=B, uplo="U", trans="N", diag="N", fpe=8)
        kw.update(change)
        with pytest.raises(exc) as err:
            exblas_amd.exbtrsm(kw["T"], kw["B"], kw["uplo"], kw["trans"], kw["diag"], 1.0, kw["fpe"])
        assert str(err.value).startswith("exbtrsm:"), change


# ---------------------------------------------------------------------------------------------
# argument validation: the C entries, before a device is touched
# ---------------------------------------------------------------------------------------------
def _c_call(entry, **change):
    lib = exblas_amd.load_library()
    t, x = np.eye(4), np.ones((6, 4))
    q = dict(uplo=b"U", trans=b"N", diag=b"N", n=6, p=4, alpha=1.0, t=ctypes.c_void_p(t.ctypes.data), ldt=4,
             x=ctypes.c_void_p(x.ctypes.data), ldx=4, fpe=8)
    q.update(change)
    args = (q["uplo"], q["trans"], q["diag"], q["n"], q["p"], q["alpha"], q["t"], q["ldt"], q["x"], q["ldx"], q["fpe"], 1)
    if entry == "dev":
        rc = lib.exblas_exbtrsm_dev(*args, None)
    elif entry == "ctx":
        rc = lib.exblas_exbtrsm_ctx(None, *args, None)
    else:
        rc = lib.exblas_exbtrsm(*args)
    assert (x == 1.0).all()
    return rc


@pytest.mark.parametrize("entry", ["dev", "ctx", "host"])
def test_c_entries_refuse_before_the_device_is_touched(entry):
    for change in (dict(uplo=b"X"), dict(trans=b"C"), dict(diag=b"T"), dict(n=-1), dict(p=-1), dict(ldt=3), dict(ldx=3),
                   dict(fpe=-1), dict(p=513, ldt=513, ldx=513), dict(p=600, ldt=600, ldx=600), dict(t=None), dict(x=None),
                   dict(p=0, ldt=0)):
        assert _c_call(entry, **change) == INVALID, change
    for fpe in (9, 12):
        assert _c_call(entry, fpe=fpe) == UNSUPPORTED
    # the limit itself passes the checks; what is then refused, without a device, is the device
    assert exblas_amd.load_library().exblas_last_btrsm_info(None) == INVALID


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    eye = torch.eye(4, dtype=torch.float64)
    with pytest.raises(RuntimeError):
        exblas_amd.exbtrsm_dev(eye, torch.ones(6, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        exblas_amd.exbtrsm_dev(eye.t(), torch.ones(6, 9, dtype=torch.float64)[:, :4], "L", "T", "U", 0.5, 0, False)
    with pytest.raises(RuntimeError):
        exblas_amd.exbtrsm_dev(torch.eye(512, dtype=torch.float64), torch.ones(2, 512, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        exblas_amd.exbtrsm(np.eye(4), np.ones((6, 4)))
    with pytest.raises(RuntimeError):
        exblas_amd.exbtrsm(np.asfortranarray(np.triu(np.ones((4, 4)))), np.ones((1, 4)), "U", "T", "U", 0.0, 0)
