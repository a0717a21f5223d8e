"""CPU suite: the C signatures of the batched ExGETRF / ExGETRS, the `order` their Python layer derives from the strides, the
argument validation of the Python layer and of the C entries, all without a device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import exblas_amd

import bjacobi_cases as J

SYMBOLS = ("exblas_exgetrf_batched_dev", "exblas_exgetrf_batched_ctx", "exblas_exgetrf_batched",
           "exblas_set_getrf_batched_path", "exblas_last_getrf_batched_info",
           "exblas_exgetrs_batched_dev", "exblas_exgetrs_batched_ctx", "exblas_exgetrs_batched",
           "exblas_set_getrs_batched_path", "exblas_last_getrs_batched_info")
INVALID, UNSUPPORTED = 1, -1                     # hipErrorInvalidValue, EXBLAS_UNSUPPORTED
c_char, c_int, c_i64, c_vp = ctypes.c_char, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p


def test_symbols_declared_listed_and_exported():
    lib = exblas_amd.load_library()
    header = open(exblas_amd.__file__.replace("exblas_amd/__init__.py", "include/exblas_hip.h")).read()
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header, name
    assert "#define EXBLAS_GETRF_BATCHED_MAX_P 64" in header and exblas_amd.GETRF_BATCHED_MAX_P == 64
    # (order, p, batch, a, lda, stride, ipiv, info, fpe, early_exit, stream)
    dev = [c_char, c_int, c_i64, c_vp, c_int, c_i64, c_vp, c_vp, c_int, c_int, c_vp]
    assert lib.exblas_exgetrf_batched_dev.argtypes == dev
    assert lib.exblas_exgetrf_batched_ctx.argtypes == [c_vp] + dev
    assert lib.exblas_exgetrf_batched.argtypes == dev[:-1]
    # (order, p, n, k, lu, ldlu, stride, ipiv, x, ldx, fpe, early_exit, stream)
    dev = [c_char, c_int, c_i64, c_int, c_vp, c_int, c_i64, c_vp, c_vp, c_i64, c_int, c_int, c_vp]
    assert lib.exblas_exgetrs_batched_dev.argtypes == dev
    assert lib.exblas_exgetrs_batched_ctx.argtypes == [c_vp] + dev
    assert lib.exblas_exgetrs_batched.argtypes == dev[:-1]
    for r in ("getrf_batched", "getrs_batched"):
        hook = getattr(lib, f"exblas_set_{r}_path")
        assert hook.restype is None and hook.argtypes == [c_int]
        assert len(getattr(lib, f"exblas_last_{r}_info").argtypes) == 1
        assert getattr(lib, f"exblas_last_{r}_info")(None) == INVALID
    for name in ("exgetrf_batched_dev", "exgetrs_batched_dev", "exgetrf_batched", "exgetrs_batched", "set_getrf_batched_path",
                 "last_getrf_batched_info", "set_getrs_batched_path", "last_getrs_batched_info"):
        assert callable(getattr(exblas_amd, name))
    # the not-built lists no longer name the LU
    assert "a batched LU" not in header


@pytest.mark.parametrize("name,names,defaults", [
    ("exgetrf_batched", ["A", "ipiv", "info", "fpe", "early_exit"], [None, None, 8, True]),
    ("exgetrs_batched", ["LU", "ipiv", "X", "fpe", "early_exit"], [8, True])])
def test_dev_functions_are_the_default_contexts_methods(name, names, defaults):
    f = getattr(exblas_amd, name + "_dev")
    assert inspect.ismethod(f) and f.__func__ is getattr(exblas_amd.Context, name)
    assert isinstance(f.__self__, exblas_amd.Context) and f.__self__.handle is None
    assert f.__self__ is exblas_amd.expotrf_dev.__self__
    params = list(inspect.signature(getattr(exblas_amd.Context, name)).parameters.values())
    assert params[0].name == "self" and inspect.signature(f) == inspect.Signature(params[1:])
    assert [q.name for q in params[1:]] == names
    assert [q.default for q in params[1:] if q.default is not inspect.Parameter.empty] == defaults


@pytest.mark.parametrize("pad,gap", [(0, 0), (3, 5)])
@pytest.mark.parametrize("layout", ["row", "col"])
def test_order_follows_the_unit_stride(layout, pad, gap):
    p, batch = 5, 3
    full = np.arange(1.0, batch * p * p + 1.0).reshape(batch, p, p)
    buf, ld, stride, strides = J.pack(full, layout, pad, gap)
    A = torch.from_numpy(buf).as_strided((batch, p, p), strides)
    assert (A.numpy() == full).all()
    order, b, pp, lda, st = exblas_amd._batched_matrices("exgetrf_batched", "A", tuple(A.shape), A)
    assert (order, b, pp, lda, st) == (b"C" if layout == "col" else b"R", batch, p, ld, stride)
    # the C routine's addressing: 'C' (i, j) at b * stride + i + j * lda, 'R' at b * stride + i * lda + j
    flat = buf.ravel()
    for m in range(batch):
        for i in range(p):
            for j in range(p):
                at = m * st + (i + j * lda if order == b"C" else i * lda + j)
                assert flat[at] == full[m, i, j]
    one = torch.ones(1, 1, 1, dtype=torch.float64)
    assert exblas_amd._batched_matrices("w", "A", (1, 1, 1), one) == (b"C", 1, 1, 1, 1)
    none = torch.ones(0, 4, 4, dtype=torch.float64)
    assert exblas_amd._batched_matrices("w", "A", (0, 4, 4), none)[:4] == (b"R", 0, 4, 4)   # contiguous: row-major
    # a contiguous tensor is row-major, its transposed view column-major; neither is copied
    T = torch.arange(32.0, dtype=torch.float64).reshape(2, 4, 4)
    assert exblas_amd._batched_matrices("w", "A", (2, 4, 4), T) == (b"R", 2, 4, 4, 16)
    assert exblas_amd._batched_matrices("w", "A", (2, 4, 4), T.transpose(1, 2)) == (b"C", 2, 4, 4, 16)


BAD_F = ["dtype", "not_tensor", "2d", "4d", "not_square", "no_unit_stride", "overlapping", "batch_overlap", "fpe9",
         "fpe_negative", "p_65", "ipiv_dtype", "ipiv_shape", "ipiv_1d", "ipiv_strided", "ipiv_not_tensor", "ipiv_device",
         "info_dtype", "info_short", "info_2d", "info_strided", "info_not_tensor", "info_device"]


@pytest.mark.parametrize("bad", BAD_F)
def test_exgetrf_batched_dev_rejects_bad_arguments(bad):
    """every one of these is a ValueError that names the routine, raised before a GPU is needed"""
    A = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    fpe, ipiv, info = 8, None, None
    if bad == "dtype":
        A = A.float()
    elif bad == "not_tensor":
        A = np.zeros((3, 4, 4))
    elif bad == "2d":
        A = A[0]
    elif bad == "4d":
        A = A[None]
    elif bad == "not_square":
        A = torch.ones(3, 4, 5, dtype=torch.float64)
    elif bad == "no_unit_stride":
        A = torch.ones(3, 8, 8, dtype=torch.float64)[:, ::2, ::2]
    elif bad == "overlapping":
        A = torch.ones(64, dtype=torch.float64).as_strided((3, 4, 4), (16, 3, 1))
    elif bad == "batch_overlap":
        A = torch.ones(64, dtype=torch.float64).as_strided((3, 4, 4), (15, 4, 1))
    elif bad == "fpe9":
        fpe = 9
    elif bad == "fpe_negative":
        fpe = -1
    elif bad == "p_65":
        A = torch.ones(2, 65, 65, dtype=torch.float64)
    elif bad == "ipiv_dtype":
        ipiv = torch.zeros(3, 4, dtype=torch.int64)
    elif bad == "ipiv_shape":
        ipiv = torch.zeros(4, 3, dtype=torch.int32)
    elif bad == "ipiv_1d":
        ipiv = torch.zeros(12, dtype=torch.int32)
    elif bad == "ipiv_strided":
        ipiv = torch.zeros(3, 8, dtype=torch.int32)[:, ::2]
    elif bad == "ipiv_not_tensor":
        ipiv = np.zeros((3, 4), dtype=np.int32)
    elif bad == "ipiv_device":
        ipiv = torch.zeros(3, 4, dtype=torch.int32, device="meta")
    elif bad == "info_dtype":
        info = torch.zeros(3, dtype=torch.int64)
    elif bad == "info_short":
        info = torch.zeros(2, dtype=torch.int32)
    elif bad == "info_2d":
        info = torch.zeros(3, 1, dtype=torch.int32)
    elif bad == "info_strided":
        info = torch.zeros(6, dtype=torch.int32)[::2]
    elif bad == "info_not_tensor":
        info = np.zeros(3, dtype=np.int32)
    elif bad == "info_device":
        info = torch.zeros(3, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError) as err:
        exblas_amd.exgetrf_batched_dev(A, ipiv, info, fpe)
    assert str(err.value).startswith("exgetrf_batched:"), err.value
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises(ValueError) as err:
        exblas_amd.Context.exgetrf_batched(ctx, A, ipiv, info, fpe)
    assert str(err.value).startswith("exgetrf_batched:")


BAD_S = ["lu_dtype", "x_dtype", "x_not_tensor", "lu_2d", "x_1d", "x_3d", "blocks_few", "blocks_many", "p_65", "p_0",
         "x_col_major", "x_rows_overlap", "lu_no_unit_stride", "lu_batch_overlap", "fpe9", "fpe_negative", "device",
         "x_overlaps_lu", "ipiv_none", "ipiv_dtype", "ipiv_shape", "ipiv_strided", "ipiv_not_tensor", "ipiv_device"]


@pytest.mark.parametrize("bad", BAD_S)
def test_exgetrs_batched_dev_rejects_bad_arguments(bad):
    LU = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    X = torch.ones(10, 2, dtype=torch.float64)                 # three blocks, the last one of two rows
    ipiv = torch.arange(1, 5, dtype=torch.int32).repeat(3, 1)
    fpe = 8
    if bad == "lu_dtype":
        LU = LU.float()
    elif bad == "x_dtype":
        X = X.float()
    elif bad == "x_not_tensor":
        X = np.ones((10, 2))
    elif bad == "lu_2d":
        LU = LU[0]
    elif bad == "x_1d":
        X = X[:, 0]
    elif bad == "x_3d":
        X = X[None]
    elif bad == "blocks_few":
        X = torch.ones(13, 2, dtype=torch.float64)
    elif bad == "blocks_many":
        X = torch.ones(8, 2, dtype=torch.float64)
    elif bad == "p_65":
        LU, X = torch.ones(1, 65, 65, dtype=torch.float64), torch.ones(65, 2, dtype=torch.float64)
        ipiv = torch.ones(1, 65, dtype=torch.int32)
    elif bad == "p_0":
        LU, ipiv = torch.ones(3, 0, 0, dtype=torch.float64), torch.ones(3, 0, dtype=torch.int32)
    elif bad == "x_col_major":
        X = torch.ones(2, 10, dtype=torch.float64).t()
    elif bad == "x_rows_overlap":
        X = torch.ones(32, dtype=torch.float64).as_strided((10, 2), (1, 1))
    elif bad == "lu_no_unit_stride":
        LU = torch.ones(3, 8, 8, dtype=torch.float64)[:, ::2, ::2]
    elif bad == "lu_batch_overlap":
        LU = torch.ones(64, dtype=torch.float64).as_strided((3, 4, 4), (15, 4, 1))
    elif bad == "fpe9":
        fpe = 9
    elif bad == "fpe_negative":
        fpe = -1
    elif bad == "device":
        X = torch.ones(10, 2, dtype=torch.float64, device="meta")
    elif bad == "x_overlaps_lu":
        whole = torch.ones(80, dtype=torch.float64)
        LU, X = whole.as_strided((3, 4, 4), (16, 4, 1)), whole[40:60].reshape(10, 2)
    elif bad == "ipiv_none":
        ipiv = None
    elif bad == "ipiv_dtype":
        ipiv = ipiv.long()
    elif bad == "ipiv_shape":
        ipiv = ipiv[:2]
    elif bad == "ipiv_strided":
        ipiv = torch.ones(3, 8, dtype=torch.int32)[:, ::2]
    elif bad == "ipiv_not_tensor":
        ipiv = ipiv.numpy()
    elif bad == "ipiv_device":
        ipiv = torch.ones(3, 4, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError) as err:
        exblas_amd.exgetrs_batched_dev(LU, ipiv, X, fpe)
    assert str(err.value).startswith("exgetrs_batched:"), err.value
    ctx = object.__new__(exblas_amd.Context)
    ctx.handle = None
    with pytest.raises(ValueError) as err:
        exblas_amd.Context.exgetrs_batched(ctx, LU, ipiv, X, fpe)
    assert str(err.value).startswith("exgetrs_batched:")


def test_host_forms_reject_bad_arguments():
    A = np.eye(3)[None].repeat(2, axis=0)
    for exc, args in ((TypeError, (A.astype(np.float32),)), (ValueError, (np.ones((2, 3, 4)),)), (ValueError, (np.eye(3),)),
                      (ValueError, (np.ones((1, 65, 65)),)), (ValueError, (A, 9)), (ValueError, (A, -2))):
        with pytest.raises(exc) as err:
            exblas_amd.exgetrf_batched(*args)
        assert str(err.value).startswith("exgetrf_batched:"), args[1:]
    B = np.ones((6, 2))
    ip = np.arange(1, 4, dtype=np.int32)[None].repeat(2, axis=0)
    for exc, args in ((TypeError, (A, ip, B.astype(np.float32))), (ValueError, (A, ip, np.ones(6))),
                      (ValueError, (A, ip, np.ones((7, 2)))), (ValueError, (A, ip, B, 9)), (ValueError, (np.eye(3), ip, B)),
                      (ValueError, (A, ip.astype(np.int64), B)), (ValueError, (A, ip[:1], B)), (ValueError, (A, ip.ravel(), B))):
        with pytest.raises(exc) as err:
            exblas_amd.exgetrs_batched(*args)
        assert str(err.value).startswith("exgetrs_batched:"), args[3:]


def _getrf_call(entry, **change):
    lib = exblas_amd.load_library()
    a, ipiv, info = 2.0 * np.eye(4)[None].repeat(3, axis=0), np.full(12, 66, dtype=np.int32), np.full(3, 77, dtype=np.int32)
    q = dict(order=b"C", p=4, batch=3, a=c_vp(a.ctypes.data), lda=4, stride=16, ipiv=c_vp(ipiv.ctypes.data),
             info=c_vp(info.ctypes.data), fpe=8)
    q.update(change)
    args = (q["order"], q["p"], q["batch"], q["a"], q["lda"], q["stride"], q["ipiv"], q["info"], q["fpe"], 1)
    if entry == "dev":
        rc = lib.exblas_exgetrf_batched_dev(*args, None)
    elif entry == "ctx":
        rc = lib.exblas_exgetrf_batched_ctx(None, *args, None)
    else:
        rc = lib.exblas_exgetrf_batched(*args)
    assert (a == 2.0 * np.eye(4)).all() and (ipiv == 66).all() and (info == 77).all()
    return rc


@pytest.mark.parametrize("entry", ["dev", "ctx", "host"])
def test_getrf_c_entries_refuse_before_the_device_is_touched(entry):
    """(without a device, any path that reaches the context ends the process: these all return)"""
    for change in (dict(order=b"X"), dict(order=b"U"), dict(order=b"N"), dict(p=-1), dict(batch=-1), dict(lda=3), dict(lda=0),
                   dict(fpe=-1), dict(p=65, lda=65, stride=65 * 65), dict(p=512, lda=512, stride=512 * 512), dict(stride=15),
                   dict(stride=0), dict(stride=-16), dict(lda=5, stride=19), dict(a=None), dict(p=0, lda=0)):
        assert _getrf_call(entry, **change) == INVALID, change
    if entry != "host":                                      # the host form may be called without pivots or info words
        assert _getrf_call(entry, info=None) == INVALID and _getrf_call(entry, ipiv=None) == INVALID
    for fpe in (9, 12):
        assert _getrf_call(entry, fpe=fpe) == UNSUPPORTED
        assert _getrf_call(entry, fpe=fpe, order=b"r") == UNSUPPORTED
    if entry == "host":                                      # nothing to do: success before the context is looked up
        assert _getrf_call(entry, p=0, lda=1) == 0 and _getrf_call(entry, batch=0) == 0
        assert _getrf_call(entry, batch=0, stride=0, order=b"R") == 0    # one matrix or none: the stride is not looked at


def _getrs_call(entry, **change):
    lib = exblas_amd.load_library()
    lu, x = 2.0 * np.eye(4)[None].repeat(3, axis=0), np.full((10, 3), 5.0)
    ipiv = np.full(12, 66, dtype=np.int32)
    q = dict(order=b"R", p=4, n=10, k=2, lu=c_vp(lu.ctypes.data), ldlu=4, stride=16, ipiv=c_vp(ipiv.ctypes.data),
             x=c_vp(x.ctypes.data), ldx=3, fpe=8)
    q.update(change)
    args = (q["order"], q["p"], q["n"], q["k"], q["lu"], q["ldlu"], q["stride"], q["ipiv"], q["x"], q["ldx"], q["fpe"], 1)
    if entry == "dev":
        rc = lib.exblas_exgetrs_batched_dev(*args, None)
    elif entry == "ctx":
        rc = lib.exblas_exgetrs_batched_ctx(None, *args, None)
    else:
        rc = lib.exblas_exgetrs_batched(*args)
    assert (lu == 2.0 * np.eye(4)).all() and (x == 5.0).all() and (ipiv == 66).all()
    return rc


@pytest.mark.parametrize("entry", ["dev", "ctx", "host"])
def test_getrs_c_entries_refuse_before_the_device_is_touched(entry):
    for change in (dict(order=b"X"), dict(order=b"L"), dict(order=b"T"), dict(p=65, ldlu=65, stride=65 * 65), dict(p=0),
                   dict(p=-1), dict(n=-1), dict(k=-1), dict(ldlu=3), dict(ldlu=0), dict(stride=15), dict(stride=-1), dict(ldx=1),
                   dict(fpe=-1), dict(lu=None), dict(x=None), dict(ipiv=None), dict(p=65, n=0, ldlu=65)):
        assert _getrs_call(entry, **change) == INVALID, change
    for fpe in (9, 12):
        assert _getrs_call(entry, fpe=fpe) == UNSUPPORTED
    if entry == "host":
        assert _getrs_call(entry, n=0) == 0 and _getrs_call(entry, k=0) == 0 and _getrs_call(entry, n=0, p=0, ldlu=1) == 0
        assert _getrs_call(entry, n=4, stride=0, k=0, order=b"c") == 0   # one block: the stride is not looked at


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        return
    A = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    X = torch.ones(10, 2, dtype=torch.float64)
    ip = torch.arange(1, 5, dtype=torch.int32).repeat(3, 1)
    for call in (lambda: exblas_amd.exgetrf_batched_dev(A), lambda: exblas_amd.exgetrf_batched_dev(A.transpose(1, 2), None, None, 0),
                 lambda: exblas_amd.exgetrs_batched_dev(A, ip, X), lambda: exblas_amd.exgetrs_batched_dev(A, ip, X, 0, False),
                 lambda: exblas_amd.exgetrf_batched(A.numpy()),
                 lambda: exblas_amd.exgetrs_batched(A.numpy(), ip.numpy(), X.numpy())):
        with pytest.raises(RuntimeError):
            call()
