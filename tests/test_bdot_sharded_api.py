"""CPU suite: the row-sharded ExBDOT entry points exist in the library, the header and the Python layer, and refuse bad
operands before a device is needed (the Python wrappers with TypeError / ValueError, the C entry points with
hipErrorInvalidValue)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import exblas_amd

INVALID = 1   # hipErrorInvalidValue
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("exblas_exbdot_export_dev", "exblas_exbdot_export_ctx", "exblas_exbdot_round_dev", "exblas_exbdot_round_ctx",
           "exblas_exbdot_allreduce_dev")


def test_symbols_in_library_header_and_python():
    lib = exblas_amd.load_library()
    header = open(os.path.join(ROOT, "include", "exblas_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS and hasattr(lib, name), name
        assert re.search(r"\bint " + name + r"\s*\(", header), name
        assert getattr(lib, name).argtypes is not None, name
    for name in ("exbdot_export_dev", "exbdot_round_dev", "exbdot_allreduce"):
        assert callable(getattr(exblas_amd, name))
    assert exblas_amd.exbdot_allreduce is exblas_amd.dist.exbdot_allreduce
    assert callable(exblas_amd.Context.exbdot_export) and callable(exblas_amd.Context.exbdot_round)
    assert "a row-sharded form" not in open(os.path.join(ROOT, "include", "exblas_hip.h")).read()   # (was: not provided)


def _blocks(n=6, p=3, q=4):
    return torch.ones(n, p, dtype=torch.float64), torch.ones(n, q, dtype=torch.float64)


def _sets(*shape, dtype=torch.int64):
    return torch.zeros(*shape, dtype=dtype)


@pytest.mark.parametrize("bad", ["x_dtype", "y_dtype", "x_numpy", "x_1d", "x_stride1", "y_transposed", "rows", "d_p_ne_q",
                                 "mode", "fpe_negative", "fpe_1", "fpe_9_early_exit", "sets_dtype", "sets_shape", "sets_words",
                                 "sets_3d", "sets_strided", "sets_numpy"])
def test_export_rejects_bad_arguments(bad):
    X, Y = _blocks()
    mode, sets, fpe, ee = "G", None, 8, True
    if bad == "x_dtype":
        X = X.float()
    elif bad == "y_dtype":
        Y = Y.to(torch.int64)
    elif bad == "x_numpy":
        X = np.ones((6, 3))
    elif bad == "x_1d":
        X = torch.ones(6, dtype=torch.float64)
    elif bad == "x_stride1":
        X = torch.ones(6, 6, dtype=torch.float64)[:, ::2]
    elif bad == "y_transposed":
        Y = torch.ones(4, 6, dtype=torch.float64).t()
    elif bad == "rows":
        Y = Y[:5]
    elif bad == "d_p_ne_q":
        mode = "D"
    elif bad == "mode":
        mode = "N"
    elif bad == "fpe_negative":
        fpe = -1
    elif bad == "fpe_1":
        fpe = 1
    elif bad == "fpe_9_early_exit":
        fpe = 9
    elif bad == "sets_dtype":
        sets = _sets(12, 72, dtype=torch.int32)
    elif bad == "sets_shape":
        sets = _sets(11, 72)
    elif bad == "sets_words":
        sets = _sets(12, 68)
    elif bad == "sets_3d":
        sets = _sets(1, 12, 72)
    elif bad == "sets_strided":
        sets = _sets(12, 144)[:, ::2]
    elif bad == "sets_numpy":
        sets = np.zeros((12, 72), dtype=np.int64)
    with pytest.raises((TypeError, ValueError)) as err:   # before any GPU check: RuntimeError would mean it came too late
        exblas_amd.exbdot_export_dev(X, Y, mode, sets, fpe, ee)
    assert str(err.value).startswith("exbdot:")
    if bad in ("x_dtype", "y_dtype", "x_numpy", "sets_dtype", "sets_numpy"):
        assert err.type is TypeError


@pytest.mark.parametrize("bad", ["sets_dtype", "sets_float", "sets_2d_count", "sets_3d_count", "sets_words", "sets_empty_stack",
                                 "sets_4d", "sets_strided", "sets_numpy", "d_p_ne_q", "mode", "negative", "out_shape",
                                 "out_dtype", "out_stride", "out_d_stride"])
def test_round_rejects_bad_arguments(bad):
    sets, mode, p, q, out = _sets(2, 12, 72), "G", 3, 4, None
    if bad == "sets_dtype":
        sets = _sets(12, 72, dtype=torch.int32)
    elif bad == "sets_float":
        sets = _sets(12, 72, dtype=torch.float64)
    elif bad == "sets_2d_count":
        sets = _sets(13, 72)
    elif bad == "sets_3d_count":
        sets = _sets(2, 11, 72)
    elif bad == "sets_words":
        sets = _sets(2, 12, 71)
    elif bad == "sets_empty_stack":
        sets = _sets(0, 12, 72)
    elif bad == "sets_4d":
        sets = _sets(1, 2, 12, 72)
    elif bad == "sets_strided":
        sets = _sets(4, 12, 72)[::2]
    elif bad == "sets_numpy":
        sets = np.zeros((12, 72), dtype=np.int64)
    elif bad == "d_p_ne_q":
        mode = "D"
    elif bad == "mode":
        mode = "T"
    elif bad == "negative":
        p, sets = -1, _sets(0, 72)
    elif bad == "out_shape":
        out = torch.zeros(4, 3, dtype=torch.float64)
    elif bad == "out_dtype":
        out = torch.zeros(3, 4, dtype=torch.float32)
    elif bad == "out_stride":
        out = torch.zeros(4, 3, dtype=torch.float64).t()
    elif bad == "out_d_stride":
        sets, mode, p, q, out = _sets(3, 72), "D", 3, 3, torch.zeros(6, dtype=torch.float64)[::2]
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.exbdot_round_dev(sets, mode, p, q, out)
    assert str(err.value).startswith("exbdot:")
    if bad in ("sets_dtype", "sets_float", "sets_numpy"):
        assert err.type is TypeError


@pytest.mark.parametrize("bad", ["x_dtype", "x_1d", "x_stride1", "d_p_ne_q", "fpe_1", "out_shape"])
def test_allreduce_rejects_bad_arguments_before_the_communicator_is_looked_at(bad):
    X, Y = _blocks()
    mode, out, fpe = "G", None, 8
    if bad == "x_dtype":
        X = X.float()
    elif bad == "x_1d":
        X = torch.ones(6, dtype=torch.float64)
    elif bad == "x_stride1":
        X = torch.ones(6, 6, dtype=torch.float64)[:, ::2]
    elif bad == "d_p_ne_q":
        mode = "D"
    elif bad == "fpe_1":
        fpe = 1
    elif bad == "out_shape":
        out = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.exbdot_allreduce(None, X, Y, mode, out, fpe)
    assert str(err.value).startswith("exbdot:")


def test_valid_operands_are_accepted_up_to_the_device_check():
    X, Y = _blocks()
    calls = [lambda: exblas_amd.exbdot_export_dev(X, Y), lambda: exblas_amd.exbdot_export_dev(X, None, "D", _sets(3, 72)),
             lambda: exblas_amd.exbdot_export_dev(X, Y, fpe=9, early_exit=False),
             lambda: exblas_amd.exbdot_round_dev(_sets(12, 72), "G", 3, 4),
             lambda: exblas_amd.exbdot_round_dev(_sets(5, 3, 72), "d", 3, 3, torch.zeros(3, dtype=torch.float64))]
    for f in calls:
        if torch.cuda.is_available():
            with pytest.raises(ValueError, match="exbdot: the tensors must be on the GPU"):
                f()
        else:
            with pytest.raises(RuntimeError):   # no GPU: no CPU fallback
                f()


def test_c_entries_refuse_before_they_need_a_device():
    """The pointers are never dereferenced; on a machine without a device a later check would end the process."""
    lib = exblas_amd.load_library()
    buf = np.zeros(64)
    ptr = C.c_void_p(buf.ctypes.data)

    def export(mode=b"G", n=4, p=2, q=3, ldx=2, ldy=3, fpe=8, ee=1, x=ptr, y=ptr, s=ptr):
        return lib.exblas_exbdot_export_dev(mode, n, p, q, x, ldx, y, ldy, s, fpe, ee, None)

    for kw in ({"n": -1}, {"n": 2 ** 31}, {"p": -1}, {"q": -1}, {"ldx": 1}, {"ldy": 2}, {"mode": b"T"}, {"fpe": -1},
               {"mode": b"D"}, {"s": None}, {"x": None}, {"y": None}, {"fpe": 1}, {"fpe": 1, "ee": 0}, {"fpe": 9},
               {"fpe": 1, "p": 0, "ldx": 0}):
        assert export(**kw) == INVALID, kw
    for kw in ({"p": 0, "ldx": 0}, {"q": 0, "ldy": 0}, {"mode": b"D", "p": 0, "q": 0, "ldx": 0, "ldy": 0}):
        assert export(**kw) == 0, kw

    def rnd(mode=b"G", p=2, q=3, s=ptr, nsets=1, c=ptr, ldc=3):
        return lib.exblas_exbdot_round_dev(mode, p, q, s, nsets, c, ldc, None)

    for kw in ({"nsets": 0}, {"nsets": -3}, {"p": -1}, {"q": -1}, {"ldc": 2}, {"mode": b"x"}, {"mode": b"D"}, {"s": None},
               {"c": None}):
        assert rnd(**kw) == INVALID, kw
    for kw in ({"p": 0}, {"q": 0, "ldc": 0}, {"mode": b"D", "p": 0, "q": 0}):
        assert rnd(**kw) == 0, kw
    # the all-reduce: no communicator, refused at once
    assert lib.exblas_exbdot_allreduce_dev(None, b"G", 4, 2, 3, ptr, 2, ptr, 3, ptr, 3, 8, 1, None) == INVALID
    assert (buf == 0).all()
