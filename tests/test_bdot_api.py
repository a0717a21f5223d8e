"""CPU suite: argument validation of ExBDOT (the Python layer and the C entry point, both before a device is needed), and
the loud failure without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import exblas_amd

INVALID = 1   # hipErrorInvalidValue


def _blocks(n=6, p=3, q=4):
    return torch.ones(n, p, dtype=torch.float64), torch.ones(n, q, dtype=torch.float64)


def test_symbols_in_abi_list():
    for name in ("exblas_exbdot_dev", "exblas_exbdot_ctx", "exblas_exbdot", "exblas_set_bdot_path"):
        assert name in exblas_amd.C_ABI_SYMBOLS
        assert hasattr(exblas_amd.load_library(), name)
    for name in ("exbdot_dev", "exbdot", "set_bdot_path"):
        assert callable(getattr(exblas_amd, name))
    assert callable(exblas_amd.Context.exbdot)


@pytest.mark.parametrize("bad", ["mode", "mode_type", "x_dtype", "y_dtype", "x_numpy", "x_3d", "y_1d", "rows", "x_stride1",
                                 "x_stride0", "y_transposed", "d_p_ne_q", "fpe", "out_shape", "out_shape_d", "out_dtype",
                                 "out_stride", "out_ld", "out_type", "out_d_stride"])
def test_exbdot_dev_rejects_bad_arguments(bad):
    X, Y = _blocks()
    mode, out, fpe = "G", None, 8
    if bad == "mode":
        mode = "T"
    elif bad == "mode_type":
        mode = 0
    elif bad == "x_dtype":
        X = X.float()
    elif bad == "y_dtype":
        Y = Y.to(torch.int64)
    elif bad == "x_numpy":
        X = np.ones((6, 3))
    elif bad == "x_3d":
        X = torch.ones(6, 3, 1, dtype=torch.float64)
    elif bad == "y_1d":
        Y = torch.ones(6, dtype=torch.float64)
    elif bad == "rows":
        Y = Y[:5]
    elif bad == "x_stride1":
        X = torch.ones(6, 6, dtype=torch.float64)[:, ::2]          # stride(1) == 2
    elif bad == "x_stride0":
        X = torch.ones(1, 3, dtype=torch.float64).expand(6, 3)     # stride(0) == 0 < 3
    elif bad == "y_transposed":
        Y = torch.ones(4, 6, dtype=torch.float64).t()              # column-major
    elif bad == "d_p_ne_q":
        mode = "D"
    elif bad == "fpe":
        fpe = -1
    elif bad == "out_shape":
        out = torch.zeros(4, 3, dtype=torch.float64)
    elif bad == "out_shape_d":
        mode, Y, out = "D", X, torch.zeros(3, 1, dtype=torch.float64)
    elif bad == "out_dtype":
        out = torch.zeros(3, 4, dtype=torch.float32)
    elif bad == "out_stride":
        out = torch.zeros(4, 3, dtype=torch.float64).t()           # 3 x 4 with stride(1) == 3
    elif bad == "out_ld":
        out = torch.zeros(1, 4, dtype=torch.float64).expand(3, 4)  # stride(0) == 0 < 4
    elif bad == "out_type":
        out = np.zeros((3, 4))
    elif bad == "out_d_stride":
        mode, Y, out = "D", X, torch.zeros(6, dtype=torch.float64)[::2]
    with pytest.raises((TypeError, ValueError)) as err:   # before any GPU check: RuntimeError would mean it came too late
        exblas_amd.exbdot_dev(X, Y, mode, out, fpe)
    assert str(err.value).startswith("exbdot:")


def test_one_dimensional_x_points_to_exdot_dev():
    with pytest.raises(ValueError, match="exdot_dev"):
        exblas_amd.exbdot_dev(torch.ones(5, dtype=torch.float64), torch.ones(5, dtype=torch.float64), "D")


def test_valid_blocks_are_accepted_up_to_the_device_check():
    wide = torch.ones(6, 9, dtype=torch.float64)
    calls = [(wide[:, :3], wide[:, 4:8], "G", None),                       # views of a wider block
             (wide[:, 1:4], None, "G", torch.zeros(3, 7, dtype=torch.float64)[:, :3]),   # Y = X, padded out
             (wide[:, :5], wide[:, 4:], "D", torch.zeros(5, dtype=torch.float64)),
             (wide[:, :1], torch.ones(6, 2, dtype=torch.float64)[:, ::2], "d", None),   # one column: stride(1) is not looked at
             (wide[:0], wide[:0, :2], "g", None)]                         # no rows
    for X, Y, mode, out in calls:
        if torch.cuda.is_available():
            with pytest.raises(ValueError, match="exbdot: the tensors must be on the GPU"):
                exblas_amd.exbdot_dev(X, Y, mode, out)
        else:
            with pytest.raises(RuntimeError):   # no GPU: no CPU fallback
                exblas_amd.exbdot_dev(X, Y, mode, out)


def test_host_exbdot_rejects_bad_arguments():
    X, Y = np.ones((6, 3)), np.ones((6, 4))
    for args, kw in (((X.astype(np.float32), Y), {}), ((X, Y.astype(np.int64)), {})):
        with pytest.raises(TypeError, match="^exbdot:"):
            exblas_amd.exbdot(*args, **kw)
    for args, kw in (((np.ones(6), np.ones(6)), {}), ((X, Y[:5]), {}), ((X, Y), {"mode": "D"}), ((X, Y), {"mode": "N"}),
                     ((X, Y), {"fpe": -2}), ((X, np.ones((6, 4, 1))), {})):
        with pytest.raises(ValueError, match="^exbdot:"):
            exblas_amd.exbdot(*args, **kw)
    with pytest.raises(ValueError, match="exdot"):
        exblas_amd.exbdot(np.ones(6))


def test_no_gpu_means_loud_failure():
    X, Y = np.ones((6, 3)), np.ones((6, 4))
    if torch.cuda.is_available():
        assert exblas_amd.exbdot(X, Y).shape == (3, 4)
    else:
        with pytest.raises(RuntimeError):
            exblas_amd.exbdot(X, Y)
        with pytest.raises(RuntimeError):
            exblas_amd.exbdot_dev(*_blocks())


def test_c_entry_refuses_before_it_needs_a_device():
    """exblas_exbdot_dev checks its arguments, and returns for p == 0 or q == 0, before it asks for a context: on a
    machine without a device a later check would end the process.  The pointers are never dereferenced."""
    f = exblas_amd.load_library().exblas_exbdot_dev
    buf = np.zeros(64)
    ptr = C.c_void_p(buf.ctypes.data)

    def call(mode=b"G", n=4, p=2, q=3, ldx=2, ldy=3, ldc=3, fpe=8, x=ptr, y=ptr, c=ptr):
        return f(mode, n, p, q, x, ldx, y, ldy, c, ldc, fpe, 1, None)

    for kw in ({"n": -1}, {"n": 2 ** 31}, {"p": -1}, {"q": -1}, {"ldx": 1}, {"ldy": 2}, {"ldc": 2}, {"mode": b"T"},
               {"mode": b"\0"}, {"fpe": -1}, {"mode": b"D"}, {"mode": b"d", "q": 2, "ldx": 1}, {"c": None}, {"x": None},
               {"y": None}):
        assert call(**kw) == INVALID, kw
    before = buf.copy()
    for kw in ({"p": 0, "ldx": 0}, {"q": 0, "ldy": 0, "ldc": 0}, {"mode": b"D", "p": 0, "q": 0, "ldx": 0, "ldy": 0},
               {"p": 0, "ldx": 0, "c": None}):
        assert call(**kw) == 0, kw
    assert (buf == before).all()
