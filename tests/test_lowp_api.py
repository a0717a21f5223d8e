"""The narrow-input entries (ExSUM / ExDOT on float32, float16, bfloat16; round_records; round_digits_host) as an
interface: declarations, argument types, Python wrappers and what is refused before any device is touched.  No GPU."""
import ctypes as C
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1    # hipErrorInvalidValue
NEW = ["exblas_exsum_lp_dev", "exblas_exdot_lp_dev", "exblas_exsum_lp_accumulate_dev", "exblas_exdot_lp_accumulate_dev",
       "exblas_exsum_lp_ctx", "exblas_exdot_lp_ctx", "exblas_exsum_lp_accumulate_ctx", "exblas_exdot_lp_accumulate_ctx",
       "exblas_round_records_dev", "exblas_round_records_ctx", "exblas_round_digits_host", "exblas_exsum_lp",
       "exblas_exdot_lp"]


@pytest.fixture(scope="module")
def ex():
    import exblas_amd
    exblas_amd.load_library()
    return exblas_amd


def test_declared_exported_and_typed(ex):
    lib = ex.load_library()
    header = open(os.path.join(ROOT, "include", "exblas_hip.h")).read()
    vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int
    for name in NEW:
        assert name + "(" in header and name in ex.C_ABI_SYMBOLS and hasattr(lib, name), name
    for k, v in (("EXBLAS_DT_F64", 0), ("EXBLAS_DT_F32", 1), ("EXBLAS_DT_F16", 2), ("EXBLAS_DT_BF16", 3)):
        assert f"#define {k} {v}\n" in header
    assert (ex.DT_F64, ex.DT_F32, ex.DT_F16, ex.DT_BF16) == (0, 1, 2, 3)
    assert lib.exblas_exsum_lp_dev.argtypes == [i32, vp, i64, i64, i32, i32, vp, vp]
    assert lib.exblas_exdot_lp_dev.argtypes == [i32, vp, i64, vp, i64, i64, i32, i32, vp, vp]
    assert lib.exblas_exsum_lp_accumulate_dev.argtypes == [i32, vp, i64, i64, i32, i32, vp]
    assert lib.exblas_exdot_lp_accumulate_dev.argtypes == [i32, vp, i64, vp, i64, i64, i32, i32, vp]
    assert lib.exblas_exsum_lp_ctx.argtypes == [vp] + lib.exblas_exsum_lp_dev.argtypes
    assert lib.exblas_exdot_lp_ctx.argtypes == [vp] + lib.exblas_exdot_lp_dev.argtypes
    assert lib.exblas_exsum_lp_accumulate_ctx.argtypes == [vp] + lib.exblas_exsum_lp_accumulate_dev.argtypes
    assert lib.exblas_exdot_lp_accumulate_ctx.argtypes == [vp] + lib.exblas_exdot_lp_accumulate_dev.argtypes
    assert lib.exblas_round_records_dev.argtypes == [vp, i64, i64, i32, vp, vp]
    assert lib.exblas_round_records_ctx.argtypes == [vp] + lib.exblas_round_records_dev.argtypes
    assert lib.exblas_round_digits_host.argtypes == [vp, i32, C.POINTER(C.c_uint64)]
    assert lib.exblas_exsum_lp.argtypes == [i32, vp, i64, i64, i32, i32, vp]
    assert lib.exblas_exdot_lp.argtypes == [i32, vp, i64, vp, i64, i64, i32, i32, vp]
    assert "5 contiguous ExSUM, 6 strided ExSUM, 7 vector ExDOT" in " ".join(header.split())   # the new kernel ids


def test_dev_functions_are_the_default_contexts_methods(ex):
    """as tests/test_abi.py describes for the existing ones: one body per routine, a Context method; X_dev is that method
    bound to the context without a handle"""
    for name in ("exsum_lp", "exdot_lp", "exsum_lp_accumulate", "exdot_lp_accumulate", "round_records", "exsum_to", "exdot_to"):
        f = getattr(ex, name + "_dev")
        assert inspect.ismethod(f) and f.__func__ is getattr(ex.Context, name), name
        assert f.__self__ is ex.exsum_dev.__self__ and f.__self__.handle is None, name
    sig = inspect.signature(ex.Context.exsum_lp)
    assert list(sig.parameters) == ["self", "x", "fpe", "early_exit", "inca", "n", "out"]
    assert (sig.parameters["fpe"].default, sig.parameters["early_exit"].default, sig.parameters["inca"].default) == (8, True, 1)
    assert list(inspect.signature(ex.Context.round_records).parameters) == ["self", "records", "dtype", "out"]
    assert list(inspect.signature(ex.Context.exsum_to).parameters)[:3] == ["self", "x", "dtype"]
    assert list(inspect.signature(ex.Context.exdot_to).parameters)[:4] == ["self", "x", "y", "dtype"]
    # the fp64 methods keep their signatures
    assert list(inspect.signature(ex.Context.exsum).parameters) == ["self", "x", "fpe", "early_exit", "inca", "n", "out"]


def test_python_argument_checks_raise_before_any_device_call(ex):
    import torch
    x32, x16 = torch.zeros(8), torch.zeros(8, dtype=torch.float16)
    for bad in (torch.zeros(8, dtype=torch.int32), torch.zeros(8, dtype=torch.complex64), torch.zeros(8, dtype=torch.uint8)):
        with pytest.raises(TypeError):
            ex.exsum_lp_dev(bad)
        with pytest.raises(TypeError):
            ex.exsum_lp_accumulate_dev(bad)
        with pytest.raises(TypeError):
            ex.exdot_lp_dev(bad, bad)
        with pytest.raises(TypeError):
            ex.exsum_to_dev(bad)
    with pytest.raises(TypeError):
        ex.exdot_lp_dev(x32, x16)
    with pytest.raises(TypeError):
        ex.exdot_lp_accumulate_dev(x16, x32)
    with pytest.raises(TypeError):
        ex.exdot_to_dev(x32, x32.double())
    for t in (x32, x16, x32.double(), x32.bfloat16()):      # the right dtypes, but not on the device
        with pytest.raises(ValueError):
            ex.exsum_lp_dev(t)
        with pytest.raises(ValueError):
            ex.exdot_lp_dev(t, t)
        with pytest.raises(ValueError):
            ex.exsum_to_dev(t)
    recs = torch.zeros(3, 128, dtype=torch.int64)
    with pytest.raises(TypeError):
        ex.round_records_dev(recs, torch.int32)
    with pytest.raises(ValueError):
        ex.round_records_dev(recs, torch.float16)
    with pytest.raises(TypeError):
        ex.exsum_lp(np.zeros(4, dtype=np.int64))
    with pytest.raises(TypeError):
        ex.exdot_lp(np.zeros(4, dtype=np.float32), np.zeros(4, dtype=np.float16))
    with pytest.raises(TypeError):
        ex.round_digits_host(np.zeros(68, dtype=np.int64), np.int16)
    with pytest.raises(ValueError):
        ex.round_digits_host(np.zeros(67, dtype=np.int64), np.float32)


def test_round_digits_host_needs_no_device(ex):
    import torch
    one = np.zeros(68, dtype=np.int64)
    one[33] = 1 << 18                                          # 2^(32 * 33 + 18) units of 2^-1074 = 1.0
    assert ex.round_digits_host(one, np.float64) == 0x3ff0000000000000
    assert ex.round_digits_host(one, np.float32) == 0x3f800000
    assert ex.round_digits_host(one, "float16") == 0x3c00
    assert ex.round_digits_host(one, torch.bfloat16) == 0x3f80
    # 1 + 2^-24 + 2^-60: the example of the double rounding.  Through a double it is 1.0; rounded once, 1 + 2^-23
    trap = one.copy()
    trap[32] = 1 << 26                                         # 2^-24
    trap[31] = 1 << 22                                         # 2^-60
    assert ex.round_digits_host(trap, np.float32) == 0x3f800001
    assert ex.round_digits_host(trap, np.float64) == 0x3ff0000010000000     # 1 + 2^-24: then the cast ties to even, 1.0
    lib = ex.load_library()
    bits = C.c_uint64()
    assert lib.exblas_round_digits_host(None, 1, C.byref(bits)) == INVALID
    assert lib.exblas_round_digits_host(C.c_void_p(one.ctypes.data), 4, C.byref(bits)) == INVALID
    assert lib.exblas_round_digits_host(C.c_void_p(one.ctypes.data), 1, None) == INVALID


REFUSALS = """
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import exblas_amd
L = exblas_amd.load_library()
buf = (C.c_char * 256)()
p = C.addressof(buf)
p += (-p) % 16
ok = lambda off=0: C.c_void_p(p + off)
out = []
def sum_(dt=1, a=ok(), n=4, inca=1, fpe=8):
    for f, extra in ((L.exblas_exsum_lp_dev, (None, None)), (L.exblas_exsum_lp_accumulate_dev, (None,))):
        out.append(f(dt, a, n, inca, fpe, 1, *extra))
    out.append(L.exblas_exsum_lp_ctx(None, dt, a, n, inca, fpe, 1, None, None))
    out.append(L.exblas_exsum_lp_accumulate_ctx(None, dt, a, n, inca, fpe, 1, None))
    out.append(L.exblas_exsum_lp(dt, a, n, inca, fpe, 1, ok(128)))
def dot_(dt=1, a=ok(), inca=1, b=ok(64), incb=1, n=4, fpe=8):
    for f, extra in ((L.exblas_exdot_lp_dev, (None, None)), (L.exblas_exdot_lp_accumulate_dev, (None,))):
        out.append(f(dt, a, inca, b, incb, n, fpe, 1, *extra))
    out.append(L.exblas_exdot_lp_ctx(None, dt, a, inca, b, incb, n, fpe, 1, None, None))
    out.append(L.exblas_exdot_lp_accumulate_ctx(None, dt, a, inca, b, incb, n, fpe, 1, None))
    out.append(L.exblas_exdot_lp(dt, a, inca, b, incb, n, fpe, 1, ok(128)))
for dt in (-1, 4, 77):
    sum_(dt=dt); dot_(dt=dt)
for fpe in (-1, 9, 100):
    sum_(fpe=fpe); dot_(fpe=fpe)
sum_(inca=0); sum_(inca=-2); dot_(inca=0); dot_(incb=0); dot_(incb=-1)
sum_(n=-1); dot_(n=-1); sum_(n=1 << 31); dot_(n=1 << 31); sum_(n=1 << 40)
sum_(dt=1, a=ok(2)); sum_(dt=2, a=ok(1)); sum_(dt=3, a=ok(3)); sum_(dt=0, a=ok(4))
dot_(dt=1, b=ok(66)); dot_(dt=2, a=ok(1)); dot_(dt=3, b=ok(65)); dot_(dt=0, b=ok(68))
for args in ((ok(), 2, 128, 9, ok(128)), (ok(), -1, 128, 1, ok(128)), (ok(), 2, 127, 1, ok(128)), (None, 1, 128, 1, ok(128)),
             (ok(), 1, 128, 1, None)):
    out.append(L.exblas_round_records_dev(*args, None))
    out.append(L.exblas_round_records_ctx(None, *args, None))
print('ret', len(out), sorted(set(out)))
"""


def test_c_entries_refuse_bad_arguments_without_a_device():
    """an unknown dtype, fpe outside 0..8, an increment < 1, n < 0, n >= 2^31, a pointer that is not a multiple of the
    element size: hipErrorInvalidValue from every entry (_dev, _ctx, accumulate, host), and the refusals of
    exblas_round_records_*.  A fresh child process, as test_set_tuning_refuses_a_kernel_variant: without a device any
    path that reaches a context ends the process, so returning at all shows that none was touched.  30 argument sets
    through 5 entries each and 5 through the two round_records entries: 160 refusals."""
    r = subprocess.run([sys.executable, "-c", REFUSALS, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ret 160 [1]"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
