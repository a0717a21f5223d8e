"""CPU suite: the C signatures of the batched ExPOTRF / ExPOTRS, the layout decision of their Python layer, the argument
validation of the Python layer and of the C entries, and csr_diag_blocks_dev, all without a device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import exblas_amd

import bjacobi_cases as J

SYMBOLS = ("exblas_expotrf_batched_dev", "exblas_expotrf_batched_ctx", "exblas_expotrf_batched",
           "exblas_set_potrf_batched_path", "exblas_last_potrf_batched_info",
           "exblas_expotrs_batched_dev", "exblas_expotrs_batched_ctx", "exblas_expotrs_batched",
           "exblas_set_potrs_batched_path", "exblas_last_potrs_batched_info")
INVALID, UNSUPPORTED = 1, -1                     # hipErrorInvalidValue, EXBLAS_UNSUPPORTED
c_char, c_int, c_i64, c_vp = ctypes.c_char, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p


def test_symbols_declared_listed_and_exported():
    lib = exblas_amd.load_library()
    header = open(exblas_amd.__file__.replace("exblas_amd/__init__.py", "include/exblas_hip.h")).read()
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header, name
    assert "#define EXBLAS_POTRF_BATCHED_MAX_P 64" in header and exblas_amd.POTRF_BATCHED_MAX_P == 64
    # (uplo, p, batch, g, ldg, stride, info, fpe, early_exit, stream)
    dev = [c_char, c_int, c_i64, c_vp, c_int, c_i64, c_vp, c_int, c_int, c_vp]
    assert lib.exblas_expotrf_batched_dev.argtypes == dev
    assert lib.exblas_expotrf_batched_ctx.argtypes == [c_vp] + dev
    assert lib.exblas_expotrf_batched.argtypes == dev[:-1]
    # (uplo, sweep, p, n, k, r, ldr, stride, x, ldx, fpe, early_exit, stream)
    dev = [c_char, c_char, c_int, c_i64, c_int, c_vp, c_int, c_i64, c_vp, c_i64, c_int, c_int, c_vp]
    assert lib.exblas_expotrs_batched_dev.argtypes == dev
    assert lib.exblas_expotrs_batched_ctx.argtypes == [c_vp] + dev
    assert lib.exblas_expotrs_batched.argtypes == dev[:-1]
    for r in ("potrf_batched", "potrs_batched"):
        hook = getattr(lib, f"exblas_set_{r}_path")
        assert hook.restype is None and hook.argtypes == [c_int]
        assert len(getattr(lib, f"exblas_last_{r}_info").argtypes) == 1
        assert getattr(lib, f"exblas_last_{r}_info")(None) == INVALID
    for name in ("expotrf_batched_dev", "expotrs_batched_dev", "expotrf_batched", "expotrs_batched", "set_potrf_batched_path",
                 "last_potrf_batched_info", "set_potrs_batched_path", "last_potrs_batched_info", "csr_diag_blocks_dev"):
        assert callable(getattr(exblas_amd, name))


@pytest.mark.parametrize("name,names,defaults", [
    ("expotrf_batched", ["G", "uplo", "info", "fpe", "early_exit"], ["U", None, 8, True]),
    ("expotrs_batched", ["R", "X", "uplo", "sweep", "fpe", "early_exit"], ["U", "B", 8, True])])
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
@pytest.mark.parametrize("uplo", ["L", "U"])
@pytest.mark.parametrize("layout", ["row", "col"])
def test_layout_names_the_triangle_as_python_indexes_it(layout, uplo, pad, gap):
    p, batch = 5, 3
    full = np.arange(1.0, batch * p * p + 1.0).reshape(batch, p, p)
    buf, ld, stride, strides = J.pack(full, layout, pad, gap)
    G = torch.from_numpy(buf).as_strided((batch, p, p), strides)
    assert (G.numpy() == full).all()
    u, b, pp, ldg, st = exblas_amd._batched_triangles("expotrf_batched", "G", tuple(G.shape), G, uplo.lower())
    assert (b, pp, ldg, st) == (batch, p, ld, stride)
    assert u == (uplo if layout == "col" else ("U" if uplo == "L" else "L")).encode()
    # the C routine reads matrix b as column-major at b * stride: its triangle u holds the entries Python calls `uplo`
    for m in range(batch):
        S = np.lib.stride_tricks.as_strided(buf.ravel()[m * st:], (p, p), (8, 8 * ldg))
        mine = np.tril(S) if u == b"L" else np.triu(S)
        want = np.tril(full[m]) if uplo == "L" else np.triu(full[m])
        assert (mine == (want if layout == "col" else want.T)).all()
    one = torch.ones(1, 1, 1, dtype=torch.float64)
    assert exblas_amd._batched_triangles("w", "G", (1, 1, 1), one, "U") == (b"U", 1, 1, 1, 1)
    none = torch.ones(0, 4, 4, dtype=torch.float64)
    assert exblas_amd._batched_triangles("w", "G", (0, 4, 4), none, "L")[:4] == (b"U", 0, 4, 4)   # contiguous: row-major
    # the host-array form keeps the order of the matrices
    for arr in (full, np.ascontiguousarray(full.transpose(0, 2, 1)).transpose(0, 2, 1)):
        keep = exblas_amd._batched_host("w", "G", arr)
        assert keep is not arr and (keep == full).all() and keep.strides == arr.strides


BAD_F = ["dtype", "not_tensor", "2d", "4d", "not_square", "no_unit_stride", "overlapping", "batch_overlap", "uplo",
         "uplo_type", "fpe9", "fpe_negative", "p_65", "info_dtype", "info_short", "info_2d", "info_strided",
         "info_not_tensor", "info_device"]


@pytest.mark.parametrize("bad", BAD_F)
def test_expotrf_batched_dev_rejects_bad_arguments(bad):
    """every one of these is a ValueError that names the routine, raised before a GPU is needed"""
    G = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    uplo, fpe, info = "U", 8, None
    if bad == "dtype":
        G = G.float()
    elif bad == "not_tensor":
        G = np.zeros((3, 4, 4))
    elif bad == "2d":
        G = G[0]
    elif bad == "4d":
        G = G[None]
    elif bad == "not_square":
        G = torch.ones(3, 4, 5, dtype=torch.float64)
    elif bad == "no_unit_stride":
        G = torch.ones(3, 8, 8, dtype=torch.float64)[:, ::2, ::2]
    elif bad == "overlapping":
        G = torch.ones(64, dtype=torch.float64).as_strided((3, 4, 4), (16, 3, 1))
    elif bad == "batch_overlap":
        G = torch.ones(64, dtype=torch.float64).as_strided((3, 4, 4), (15, 4, 1))
    elif bad == "uplo":
        uplo = "X"
    elif bad == "uplo_type":
        uplo = 1
    elif bad == "fpe9":
        fpe = 9
    elif bad == "fpe_negative":
        fpe = -1
    elif bad == "p_65":
        G = torch.ones(2, 65, 65, dtype=torch.float64)
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
        exblas_amd.expotrf_batched_dev(G, uplo, info, fpe)
    assert str(err.value).startswith("expotrf_batched:"), err.value
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises(ValueError) as err:
        exblas_amd.Context.expotrf_batched(ctx, G, uplo, info, fpe)
    assert str(err.value).startswith("expotrf_batched:")


BAD_S = ["r_dtype", "x_dtype", "x_not_tensor", "r_2d", "x_1d", "x_3d", "blocks_few", "blocks_many", "p_65", "p_0",
         "x_col_major", "x_rows_overlap", "r_no_unit_stride", "r_batch_overlap", "uplo", "sweep", "sweep_3", "sweep_type",
         "fpe9", "fpe_negative", "device", "x_overlaps_r"]


@pytest.mark.parametrize("bad", BAD_S)
def test_expotrs_batched_dev_rejects_bad_arguments(bad):
    R = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    X = torch.ones(10, 2, dtype=torch.float64)                 # three blocks, the last one of two rows
    uplo, sweep, fpe = "U", "B", 8
    if bad == "r_dtype":
        R = R.float()
    elif bad == "x_dtype":
        X = X.float()
    elif bad == "x_not_tensor":
        X = np.ones((10, 2))
    elif bad == "r_2d":
        R = R[0]
    elif bad == "x_1d":
        X = X[:, 0]
    elif bad == "x_3d":
        X = X[None]
    elif bad == "blocks_few":
        X = torch.ones(13, 2, dtype=torch.float64)
    elif bad == "blocks_many":
        X = torch.ones(8, 2, dtype=torch.float64)
    elif bad == "p_65":
        R, X = torch.ones(1, 65, 65, dtype=torch.float64), torch.ones(65, 2, dtype=torch.float64)
    elif bad == "p_0":
        R = torch.ones(3, 0, 0, dtype=torch.float64)
    elif bad == "x_col_major":
        X = torch.ones(2, 10, dtype=torch.float64).t()
    elif bad == "x_rows_overlap":
        X = torch.ones(32, dtype=torch.float64).as_strided((10, 2), (1, 1))
    elif bad == "r_no_unit_stride":
        R = torch.ones(3, 8, 8, dtype=torch.float64)[:, ::2, ::2]
    elif bad == "r_batch_overlap":
        R = torch.ones(64, dtype=torch.float64).as_strided((3, 4, 4), (15, 4, 1))
    elif bad == "uplo":
        uplo = "N"
    elif bad == "sweep":
        sweep = "T"
    elif bad == "sweep_3":
        sweep = 3
    elif bad == "sweep_type":
        sweep = None
    elif bad == "fpe9":
        fpe = 9
    elif bad == "fpe_negative":
        fpe = -1
    elif bad == "device":
        X = torch.ones(10, 2, dtype=torch.float64, device="meta")
    elif bad == "x_overlaps_r":
        whole = torch.ones(80, dtype=torch.float64)
        R, X = whole.as_strided((3, 4, 4), (16, 4, 1)), whole[40:60].reshape(10, 2)
    with pytest.raises(ValueError) as err:
        exblas_amd.expotrs_batched_dev(R, X, uplo, sweep, fpe)
    assert str(err.value).startswith("expotrs_batched:"), err.value
    ctx = object.__new__(exblas_amd.Context)
    ctx.handle = None
    with pytest.raises(ValueError) as err:
        exblas_amd.Context.expotrs_batched(ctx, R, X, uplo, sweep, fpe)
    assert str(err.value).startswith("expotrs_batched:")


def test_sweeps_are_spelled_one_two_and_both():
    assert [exblas_amd._potrs_sweep(s) for s in ("1", "2", "B", "b", 1, 2)] == [b"1", b"2", b"B", b"B", b"1", b"2"]
    for s in (True, 0, "12", "", None, 1.0):
        with pytest.raises(ValueError):
            exblas_amd._potrs_sweep(s)


def test_host_forms_reject_bad_arguments():
    G = np.eye(3)[None].repeat(2, axis=0)
    for exc, args in ((TypeError, (G.astype(np.float32),)), (ValueError, (np.ones((2, 3, 4)),)), (ValueError, (np.eye(3),)),
                      (ValueError, (np.ones((1, 65, 65)),)), (ValueError, (G, "T")), (ValueError, (G, "U", 9)),
                      (ValueError, (G, "U", -2))):
        with pytest.raises(exc) as err:
            exblas_amd.expotrf_batched(*args)
        assert str(err.value).startswith("expotrf_batched:"), args[1:]
    B = np.ones((6, 2))
    for exc, args in ((TypeError, (G, B.astype(np.float32))), (ValueError, (G, np.ones(6))), (ValueError, (G, np.ones((7, 2)))),
                      (ValueError, (G, B, "X")), (ValueError, (G, B, "U", "3")), (ValueError, (G, B, "U", "B", 9)),
                      (ValueError, (np.eye(3), B))):
        with pytest.raises(exc) as err:
            exblas_amd.expotrs_batched(*args)
        assert str(err.value).startswith("expotrs_batched:"), args[2:]


def _potrf_call(entry, **change):
    lib = exblas_amd.load_library()
    g, info = 2.0 * np.eye(4)[None].repeat(3, axis=0), np.full(3, 77, dtype=np.int32)
    q = dict(uplo=b"U", p=4, batch=3, g=c_vp(g.ctypes.data), ldg=4, stride=16, info=c_vp(info.ctypes.data), fpe=8)
    q.update(change)
    args = (q["uplo"], q["p"], q["batch"], q["g"], q["ldg"], q["stride"], q["info"], q["fpe"], 1)
    if entry == "dev":
        rc = lib.exblas_expotrf_batched_dev(*args, None)
    elif entry == "ctx":
        rc = lib.exblas_expotrf_batched_ctx(None, *args, None)
    else:
        rc = lib.exblas_expotrf_batched(*args)
    assert (g == 2.0 * np.eye(4)).all() and (info == 77).all()
    return rc


@pytest.mark.parametrize("entry", ["dev", "ctx", "host"])
def test_potrf_c_entries_refuse_before_the_device_is_touched(entry):
    """(without a device, any path that reaches the context ends the process: these all return)"""
    for change in (dict(uplo=b"X"), dict(uplo=b"N"), dict(p=-1), dict(batch=-1), dict(ldg=3), dict(ldg=0), dict(fpe=-1),
                   dict(p=65, ldg=65, stride=65 * 65), dict(p=512, ldg=512, stride=512 * 512), dict(stride=15), dict(stride=0),
                   dict(stride=-16), dict(ldg=5, stride=19), dict(g=None), dict(p=0, ldg=0)):
        assert _potrf_call(entry, **change) == INVALID, change
    if entry != "host":                                      # the host form may be called without the info words
        assert _potrf_call(entry, info=None) == INVALID
    for fpe in (9, 12):
        assert _potrf_call(entry, fpe=fpe) == UNSUPPORTED
    if entry == "host":                                      # nothing to do: success before the context is looked up
        assert _potrf_call(entry, p=0, ldg=1) == 0 and _potrf_call(entry, batch=0) == 0
        assert _potrf_call(entry, batch=0, stride=0) == 0    # one matrix or none: the stride is not looked at


def _potrs_call(entry, **change):
    lib = exblas_amd.load_library()
    r, x = 2.0 * np.eye(4)[None].repeat(3, axis=0), np.full((10, 3), 5.0)
    q = dict(uplo=b"U", sweep=b"B", p=4, n=10, k=2, r=c_vp(r.ctypes.data), ldr=4, stride=16, x=c_vp(x.ctypes.data), ldx=3,
             fpe=8)
    q.update(change)
    args = (q["uplo"], q["sweep"], q["p"], q["n"], q["k"], q["r"], q["ldr"], q["stride"], q["x"], q["ldx"], q["fpe"], 1)
    if entry == "dev":
        rc = lib.exblas_expotrs_batched_dev(*args, None)
    elif entry == "ctx":
        rc = lib.exblas_expotrs_batched_ctx(None, *args, None)
    else:
        rc = lib.exblas_expotrs_batched(*args)
    assert (r == 2.0 * np.eye(4)).all() and (x == 5.0).all()
    return rc


@pytest.mark.parametrize("entry", ["dev", "ctx", "host"])
def test_potrs_c_entries_refuse_before_the_device_is_touched(entry):
    for change in (dict(uplo=b"X"), dict(sweep=b"3"), dict(sweep=b"N"), dict(sweep=b"0"), dict(p=65, ldr=65, stride=65 * 65),
                   dict(p=0), dict(p=-1), dict(n=-1), dict(k=-1), dict(ldr=3), dict(ldr=0), dict(stride=15), dict(stride=-1),
                   dict(ldx=1), dict(fpe=-1), dict(r=None), dict(x=None), dict(p=65, n=0, ldr=65)):
        assert _potrs_call(entry, **change) == INVALID, change
    for fpe in (9, 12):
        assert _potrs_call(entry, fpe=fpe) == UNSUPPORTED
    if entry == "host":
        assert _potrs_call(entry, n=0) == 0 and _potrs_call(entry, k=0) == 0 and _potrs_call(entry, n=0, p=0, ldr=1) == 0
        assert _potrs_call(entry, n=4, stride=0, k=0) == 0   # one block: the stride is not looked at


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        return
    G = torch.eye(4, dtype=torch.float64).repeat(3, 1, 1)
    X = torch.ones(10, 2, dtype=torch.float64)
    for call in (lambda: exblas_amd.expotrf_batched_dev(G), lambda: exblas_amd.expotrf_batched_dev(G.transpose(1, 2), "L", None, 0),
                 lambda: exblas_amd.expotrs_batched_dev(G, X), lambda: exblas_amd.expotrs_batched_dev(G, X, "L", "1", 0, False),
                 lambda: exblas_amd.expotrf_batched(G.numpy()), lambda: exblas_amd.expotrs_batched(G.numpy(), X.numpy())):
        with pytest.raises(RuntimeError):
            call()


@pytest.mark.parametrize("itype", [torch.int32, torch.int64])
@pytest.mark.parametrize("p", [1, 3, 8, 64])
def test_csr_diag_blocks_against_a_dense_restatement(p, itype):
    """on CPU tensors: the helper is plain torch indexing and needs no GPU"""
    rng = np.random.default_rng(p)
    n = 29
    A = np.where(rng.random((n, n)) < 0.3, rng.standard_normal((n, n)), 0.0)
    A[np.arange(n), np.arange(n)] = 5.0 + rng.random(n)
    A[7, :] = 0.0                                                # an empty row
    sp = torch.from_numpy(A).to_sparse_csr()
    crow, col, val = sp.crow_indices().to(itype), sp.col_indices().to(itype), sp.values()
    want = J.diag_blocks(A, p)
    for op in (sp, (crow, col, val, (n, n))):
        D = exblas_amd.csr_diag_blocks_dev(op, p)
        assert D.dtype == torch.float64 and tuple(D.shape) == (-(-n // p), p, p) and D.is_contiguous()
        assert (D.numpy() == want).all()
    for exc, args in ((ValueError, (sp, 0)), (ValueError, (sp, 65)), (ValueError, ((crow, col, val, (n, n + 1)), 4)),
                      (TypeError, (torch.from_numpy(A), 4))):
        with pytest.raises(exc):
            exblas_amd.csr_diag_blocks_dev(*args)
