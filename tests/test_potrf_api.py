"""CPU suite: the C signatures of ExPOTRF, the layout decision of its Python layer and the argument validation of the
Python layer and of the C entries, all without a device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import exblas_amd

SYMBOLS = ("exblas_expotrf_dev", "exblas_expotrf_ctx", "exblas_expotrf", "exblas_set_potrf_path", "exblas_last_potrf_info")
INVALID, UNSUPPORTED = 1, -1                     # hipErrorInvalidValue, EXBLAS_UNSUPPORTED


def test_symbols_declared_listed_and_exported():
    lib = exblas_amd.load_library()
    header = open(exblas_amd.__file__.replace("exblas_amd/__init__.py", "include/exblas_hip.h")).read()
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header, name
    dev, ctx, host = lib.exblas_expotrf_dev.argtypes, lib.exblas_expotrf_ctx.argtypes, lib.exblas_expotrf.argtypes
    assert len(dev) == 8 and len(ctx) == 9 and len(host) == 7
    # (uplo, p, g, ldg, info, fpe, early_exit, stream)
    for args, off in ((dev, 0), (ctx, 1), (host, 0)):
        assert args[off] is ctypes.c_char and args[off + 1] is ctypes.c_int and args[off + 2] is ctypes.c_void_p
        assert args[off + 3] is ctypes.c_int and args[off + 5] is ctypes.c_int and args[off + 6] is ctypes.c_int
    assert ctx[0] is ctypes.c_void_p and dev[7] is ctypes.c_void_p and dev[4] is ctypes.c_void_p
    assert lib.exblas_set_potrf_path.restype is None and len(lib.exblas_set_potrf_path.argtypes) == 1
    for name in ("expotrf_dev", "expotrf", "set_potrf_path", "last_potrf_info", "excholqr_dev"):
        assert callable(getattr(exblas_amd, name))


def test_expotrf_dev_is_the_default_contexts_method():
    f = exblas_amd.expotrf_dev
    assert inspect.ismethod(f) and f.__func__ is exblas_amd.Context.expotrf
    assert isinstance(f.__self__, exblas_amd.Context) and f.__self__.handle is None
    assert f.__self__ is exblas_amd.exbtrsm_dev.__self__
    params = list(inspect.signature(exblas_amd.Context.expotrf).parameters.values())
    assert params[0].name == "self" and inspect.signature(f) == inspect.Signature(params[1:])
    assert [q.name for q in params[1:]] == ["G", "uplo", "info", "fpe", "early_exit"]
    assert [q.default for q in params[2:]] == ["U", None, 8, True]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("layout", ["row_major", "column_major"])
def test_layout_names_the_triangle_as_python_indexes_it(layout, uplo, pad):
    p = 6
    full = np.arange(1.0, p * p + 1.0).reshape(p, p)
    wide = torch.zeros(p, p + pad, dtype=torch.float64)
    if layout == "row_major":
        wide[:, :p] = torch.from_numpy(full)
        G = wide[:, :p]
    else:
        wide[:, :p] = torch.from_numpy(full.T)
        G = wide[:, :p].t()
    assert (G.numpy() == full).all()
    u, pp, ldg = exblas_amd._potrf_triangle(tuple(G.shape), G, uplo.lower())
    assert pp == p and ldg == p + pad
    assert u == (uplo if layout == "column_major" else ("U" if uplo == "L" else "L")).encode()
    # the C routine reads the storage as column-major: its triangle u holds the entries Python calls `uplo`
    S = torch.as_strided(G, (p, p), (1, ldg)).numpy()
    mine = np.tril(S) if u == b"L" else np.triu(S)
    want = np.tril(full) if uplo == "L" else np.triu(full)
    assert (mine == (want if layout == "column_major" else want.T)).all()
    assert exblas_amd._potrf_triangle((1, 1), torch.ones(1, 1, dtype=torch.float64), "U") == (b"U", 1, 1)
    assert exblas_amd._potrf_triangle((0, 0), torch.ones(0, 0, dtype=torch.float64), "L") == (b"L", 0, 1)


BAD = ["dtype", "not_tensor", "1d", "3d", "not_square", "no_unit_stride", "overlapping", "uplo", "uplo_type", "fpe9",
       "fpe_negative", "p_513", "info_dtype", "info_two", "info_not_tensor", "info_device"]


@pytest.mark.parametrize("bad", BAD)
def test_expotrf_dev_rejects_bad_arguments(bad):
    """every one of these is a ValueError that names the routine, raised before a GPU is needed"""
    G = torch.eye(4, dtype=torch.float64)
    uplo, fpe, info = "U", 8, None
    if bad == "dtype":
        G = G.float()
    elif bad == "not_tensor":
        G = np.eye(4)
    elif bad == "1d":
        G = torch.ones(4, dtype=torch.float64)
    elif bad == "3d":
        G = torch.ones(4, 4, 1, dtype=torch.float64)
    elif bad == "not_square":
        G = torch.ones(4, 5, dtype=torch.float64)
    elif bad == "no_unit_stride":
        G = torch.ones(8, 8, dtype=torch.float64)[::2, ::2]
    elif bad == "overlapping":
        G = torch.ones(16, dtype=torch.float64).as_strided((4, 4), (3, 1))
    elif bad == "uplo":
        uplo = "X"
    elif bad == "uplo_type":
        uplo = 1
    elif bad == "fpe9":
        fpe = 9
    elif bad == "fpe_negative":
        fpe = -1
    elif bad == "p_513":
        G = torch.eye(513, dtype=torch.float64)
    elif bad == "info_dtype":
        info = torch.zeros(1, dtype=torch.int64)
    elif bad == "info_two":
        info = torch.zeros(2, dtype=torch.int32)
    elif bad == "info_not_tensor":
        info = np.zeros(1, dtype=np.int32)
    elif bad == "info_device":
        info = torch.zeros(1, dtype=torch.int32, device="meta")
    with pytest.raises(ValueError) as err:
        exblas_amd.expotrf_dev(G, uplo, info, fpe)
    assert str(err.value).startswith("expotrf:"), err.value
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises(ValueError) as err:
        exblas_amd.Context.expotrf(ctx, G, uplo, info, fpe)
    assert str(err.value).startswith("expotrf:")


def test_host_expotrf_rejects_bad_arguments():
    cases = [
        (TypeError, dict(G=np.eye(3, dtype=np.float32))),
        (ValueError, dict(G=np.ones((3, 4)))),
        (ValueError, dict(G=np.ones(3))),
        (ValueError, dict(G=np.ones((3, 3, 1)))),
        (ValueError, dict(G=np.eye(513))),
        (ValueError, dict(uplo="T")),
        (ValueError, dict(fpe=9)),
        (ValueError, dict(fpe=-2)),
    ]
    for exc, change in cases:
        kw = dict(G=np.eye(3), uplo="U", fpe=8)
        kw.update(change)
        with pytest.raises(exc) as err:
            exblas_amd.expotrf(kw["G"], kw["uplo"], kw["fpe"])
        assert str(err.value).startswith("expotrf:"), change


def _c_call(entry, **change):
    lib = exblas_amd.load_library()
    g, info = 2.0 * np.eye(4), np.full(1, 77, dtype=np.int32)
    q = dict(uplo=b"U", p=4, g=ctypes.c_void_p(g.ctypes.data), ldg=4, info=ctypes.c_void_p(info.ctypes.data), fpe=8)
    q.update(change)
    if entry == "dev":
        rc = lib.exblas_expotrf_dev(q["uplo"], q["p"], q["g"], q["ldg"], q["info"], q["fpe"], 1, None)
    elif entry == "ctx":
        rc = lib.exblas_expotrf_ctx(None, q["uplo"], q["p"], q["g"], q["ldg"], q["info"], q["fpe"], 1, None)
    else:
        rc = lib.exblas_expotrf(q["uplo"], q["p"], q["g"], q["ldg"], ctypes.cast(q["info"], ctypes.POINTER(ctypes.c_int)),
                                q["fpe"], 1)
    assert (g == 2.0 * np.eye(4)).all() and info[0] == 77
    return rc


@pytest.mark.parametrize("entry", ["dev", "ctx", "host"])
def test_c_entries_refuse_before_the_device_is_touched(entry):
    """(without a device, any path that reaches the context ends the process: these all return)"""
    for change in (dict(uplo=b"X"), dict(uplo=b"N"), dict(p=-1), dict(ldg=3), dict(ldg=0), dict(fpe=-1), dict(p=513, ldg=513),
                   dict(p=600, ldg=600), dict(g=None), dict(p=0, ldg=0)):
        assert _c_call(entry, **change) == INVALID, change
    if entry != "host":                                      # the host form may be called without an info word
        assert _c_call(entry, info=None) == INVALID
    for fpe in (9, 12):
        assert _c_call(entry, fpe=fpe) == UNSUPPORTED
    if entry == "host":                                      # nothing to do: success before the context is looked up
        assert _c_call(entry, p=0, ldg=1) == 0               # (the device forms go on to the context, as ExBTRSM's do)
    assert exblas_amd.load_library().exblas_last_potrf_info(None) == INVALID


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        return
    eye = torch.eye(4, dtype=torch.float64)
    for call in (lambda: exblas_amd.expotrf_dev(eye), lambda: exblas_amd.expotrf_dev(eye.t(), "L", None, 0, False),
                 lambda: exblas_amd.expotrf_dev(torch.eye(512, dtype=torch.float64)),
                 lambda: exblas_amd.expotrf(np.eye(4)), lambda: exblas_amd.expotrf(np.asfortranarray(np.eye(4)), "L", 0),
                 lambda: exblas_amd.excholqr_dev(torch.ones(6, 2, dtype=torch.float64))):
        with pytest.raises(RuntimeError):
            call()
