"""CPU suite: the C signatures of ExBGEMM, the argument validation of its Python layer without a device, and the case
helpers of the GPU tests (tests/bgemm_cases.py)."""
import ctypes

import numpy as np
import pytest
import torch

import bgemm_cases as B
import exact_cases as X
import exblas_amd

SYMBOLS = ("exblas_exbgemm_dev", "exblas_exbgemm_ctx", "exblas_exbgemm", "exblas_set_bgemm_path", "exblas_last_bgemm_info")


def test_symbols_in_abi_list_and_signatures():
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS
    lib = exblas_amd.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    dev, ctx, host = lib.exblas_exbgemm_dev.argtypes, lib.exblas_exbgemm_ctx.argtypes, lib.exblas_exbgemm.argtypes
    assert len(dev) == 14 and len(ctx) == 15 and len(host) == 13
    # (n, p, q, alpha, x, ldx, c, ldc, beta, y, ldy, fpe, early_exit, stream): n and the leading dimensions are 64-bit
    for args, off in ((dev, 0), (ctx, 1), (host, 0)):
        assert args[off + 0] is ctypes.c_int64 and args[off + 1] is ctypes.c_int and args[off + 2] is ctypes.c_int
        assert args[off + 3] is ctypes.c_double and args[off + 8] is ctypes.c_double
        assert all(args[off + i] is ctypes.c_int64 for i in (5, 7, 10))
        assert all(args[off + i] is ctypes.c_void_p for i in (4, 6, 9))
        assert args[off + 11] is ctypes.c_int and args[off + 12] is ctypes.c_int
    assert ctx[0] is ctypes.c_void_p and dev[13] is ctypes.c_void_p
    assert lib.exblas_set_bgemm_path.restype is None and len(lib.exblas_set_bgemm_path.argtypes) == 1
    assert len(lib.exblas_last_bgemm_info.argtypes) == 1
    for name in ("exbgemm_dev", "exbgemm", "set_bgemm_path", "last_bgemm_info"):
        assert callable(getattr(exblas_amd, name))
    assert callable(exblas_amd.Context.exbgemm)
    assert exblas_amd.exbgemm_dev.__func__ is exblas_amd.Context.exbgemm    # one body, bound to the default context


def _f64(*shape):
    return torch.ones(*shape, dtype=torch.float64)


BAD = ["x_dtype", "c_dtype", "y_dtype", "x_not_tensor", "c_not_tensor", "y_not_tensor", "x_1d", "c_1d", "y_3d", "x_col_major",
       "x_col_strided", "c_col_strided", "y_col_strided", "x_rows_overlap", "y_rows_overlap", "c_rows", "y_rows", "y_cols",
       "devices", "y_device", "y_is_x", "y_overlaps_x_tail", "y_overlaps_c", "fpe_negative"]


@pytest.mark.parametrize("bad", BAD)
def test_exbgemm_dev_rejects_bad_arguments(bad):
    """every one of these is a ValueError that names the routine, raised before a GPU is needed"""
    x, c, y, fpe = _f64(6, 4), _f64(4, 3), _f64(6, 3), 8
    if bad == "x_dtype":
        x = x.float()
    elif bad == "c_dtype":
        c = c.float()
    elif bad == "y_dtype":
        y = y.float()
    elif bad == "x_not_tensor":
        x = np.ones((6, 4))
    elif bad == "c_not_tensor":
        c = np.ones((4, 3))
    elif bad == "y_not_tensor":
        y = np.ones((6, 3))
    elif bad == "x_1d":
        x = _f64(6)
    elif bad == "c_1d":
        c = _f64(4)
    elif bad == "y_3d":
        y = _f64(6, 3, 1)
    elif bad == "x_col_major":
        x = _f64(4, 6).t()                                   # stride (1, 6)
    elif bad == "x_col_strided":
        x = _f64(6, 8)[:, ::2]                               # stride (8, 2)
    elif bad == "c_col_strided":
        c = _f64(4, 6)[:, ::2]
    elif bad == "y_col_strided":
        y = _f64(6, 6)[:, ::2]
    elif bad == "x_rows_overlap":
        x = _f64(1, 4).expand(6, 4)                          # stride (0, 1)
    elif bad == "y_rows_overlap":
        y = _f64(16).as_strided((6, 3), (2, 1))              # stride(0) = 2 < q
    elif bad == "c_rows":
        c = _f64(5, 3)
    elif bad == "y_rows":
        y = _f64(7, 3)
    elif bad == "y_cols":
        y = _f64(6, 4)
    elif bad == "devices":
        x = torch.ones(6, 4, dtype=torch.float64, device="meta")
    elif bad == "y_device":
        y = torch.ones(6, 3, dtype=torch.float64, device="meta")
    elif bad == "y_is_x":
        x, c = _f64(6, 3), _f64(3, 3)
        y = x
    elif bad == "y_overlaps_x_tail":
        base = _f64(6, 7)
        x, y = base[:, :4], base[:, 3:6]                     # two views of one buffer that share its column 3
    elif bad == "y_overlaps_c":
        base = _f64(40)
        c, y = base[:12].view(4, 3), base[9:27].view(6, 3)
    elif bad == "fpe_negative":
        fpe = -1
    with pytest.raises(ValueError) as err:
        exblas_amd.exbgemm_dev(x, c, 1.0, 1.0, y, fpe)
    assert str(err.value).startswith("exbgemm:"), err.value
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises(ValueError) as err:
        exblas_amd.Context.exbgemm(ctx, x, c, 1.0, 1.0, y, fpe)
    assert str(err.value).startswith("exbgemm:")


def test_host_exbgemm_rejects_bad_arguments():
    x, c, y = np.ones((6, 4)), np.ones((4, 3)), np.ones((6, 3))
    for exc, kw in ((TypeError, dict(X=x.astype(np.float32))), (TypeError, dict(C=c.astype(np.float32))),
                    (ValueError, dict(X=np.ones(6))), (ValueError, dict(C=np.ones((4, 3, 1)))),
                    (ValueError, dict(C=np.ones((5, 3)))), (ValueError, dict(Y=np.ones((6, 4)))),
                    (ValueError, dict(Y=np.ones((5, 3)))), (ValueError, dict(fpe=-1))):
        args = dict(X=x, C=c, Y=y, fpe=8)
        args.update(kw)
        with pytest.raises(exc) as err:
            exblas_amd.exbgemm(args["X"], args["C"], 1.0, 1.0, args["Y"], args["fpe"])
        assert str(err.value).startswith("exbgemm:"), kw


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(RuntimeError):
        exblas_amd.exbgemm_dev(_f64(6, 4), _f64(4, 3))
    with pytest.raises(RuntimeError):
        exblas_amd.exbgemm_dev(_f64(6, 8)[:, :4], _f64(4, 5)[:, :3], 2.0, 1.0, _f64(6, 9)[:, :3], 0, False)
    with pytest.raises(RuntimeError):
        exblas_amd.exbgemm(np.ones((6, 4)), np.ones((4, 3)))
    base = _f64(6, 8)                                        # [X | Y |pad] in one buffer: different columns, no overlap
    with pytest.raises(RuntimeError):
        exblas_amd.exbgemm_dev(base[:, :4], _f64(4, 3), 1.0, 1.0, base[:, 4:7])


# ---------------------------------------------------------------------------------------------
# tests/bgemm_cases.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("itype", [np.int32, np.int64])
def test_dense_csr_is_the_dense_block(itype):
    rng = np.random.default_rng(3)
    n, p, q = 7, 5, 3
    xb = rng.integers(-9, 10, (n, p)).astype(np.float64)
    cb = rng.integers(-9, 10, (p, q)).astype(np.float64)
    crow, col = B.dense_csr(n, p, itype)
    assert crow.dtype == itype and col.dtype == itype and len(crow) == n + 1 and len(col) == n * p
    assert (crow == np.arange(n + 1) * p).all() and (col.reshape(n, p) == np.arange(p)).all()
    val = xb.reshape(-1)
    got = np.zeros((n, q))
    for r in range(n):
        for k in range(int(crow[r]), int(crow[r + 1])):
            got[r] += val[k] * cb[col[k]]
    assert (got == xb @ cb).all()
    # the degenerate blocks
    crow, col = B.dense_csr(4, 0, itype)
    assert (crow == 0).all() and len(crow) == 5 and len(col) == 0
    crow, col = B.dense_csr(0, 3, itype)
    assert len(crow) == 1 and crow[0] == 0 and len(col) == 0


def test_identity_shapes_cover_every_size_and_seam():
    shapes = B.identity_shapes()
    assert len(shapes) == B.IDENTITY_COUNT == len(set(shapes)) and 35 <= len(shapes) <= 45
    assert {s[0] for s in shapes} == set(B.IDENTITY_N)
    assert {s[1] for s in shapes} == set(B.IDENTITY_Q)
    assert {s[2] for s in shapes} == set(B.IDENTITY_P)
    pairs = {(q, p) for _, q, p in shapes}
    for lo, hi in ((4, 5), (64, 65)):                        # both sides of the seam in q and in p, together
        assert {(q, p) for q in (lo, hi) for p in (lo, hi)} <= pairs


def test_planted_rotation_and_shapes():
    rot = [B.planted_rotation(i) for i in range(len(B.PLANTED_SHAPES))]
    assert {r[0] for r in rot} == set(B.PLANTED_S) and {r[1] for r in rot} == set(X.LAYOUTS)
    assert {r[2] for r in rot} == set(B.PLANTED_YTERM)
    assert len(set(rot)) == len(rot)
    # what the generator needs, and a case without a term in Y for the non-vacuity rule of the counters
    assert all(rows >= 16 and p >= 5 for rows, _, p in B.PLANTED_SHAPES) and min(B.PLANTED_S) >= 54
    assert any(s in (54, 63) and y == (None, 0) for s, _, y in rot)
    # the smallest case builds, every output in a planted class
    rows, q, p = B.PLANTED_SHAPES[0]
    S, layout, (plant, beta) = rot[0]
    c = X.planted_spmm(rows, q, p, S, seed=21, layout=layout, plant=plant, beta=beta)
    assert c.g.shape == (rows, p) and c.x.shape == (p, q) and c.want.shape == (rows, q)
    assert set(c.classes.ravel().tolist()) <= {"tie", "carry", "tie+1", "tie-1", "zero", "exact"}


def test_wide_block_spans_the_exponents():
    blk = B.wide_block(np.random.default_rng(1), 50, 40)
    e = np.frexp(blk)[1]
    assert blk.shape == (50, 40) and e.min() < -150 and e.max() > 150 and np.isfinite(blk).all() and (blk != 0).all()
