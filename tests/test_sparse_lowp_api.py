"""CPU suite (no GPU): the interface of the narrow ExSpMV / ExSpMM -- the C symbols are declared, exported and listed; the
Python functions are Context methods; every refusal is raised before a device is needed."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import exblas_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["exblas_exspmv_csr_lp_dev", "exblas_exspmv_csr_lp_ctx", "exblas_exspmv_csr_lp",
       "exblas_exspmm_csr_lp_dev", "exblas_exspmm_csr_lp_ctx", "exblas_exspmm_csr_lp", "exblas_round_interval_host",
       "exblas_round_window_host"]
INVALID, UNSUPPORTED = 1, -1          # hipErrorInvalidValue, EXBLAS_UNSUPPORTED
F64, F32, F16, BF16 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def lib():
    return exblas_amd.load_library()


def test_symbols_declared_exported_and_listed(lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "exblas_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(exblas_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared and name in exblas_amd.C_ABI_SYMBOLS and hasattr(lib, name), name
    assert len(lib.exblas_exspmv_csr_lp_dev.argtypes) == 15 and len(lib.exblas_exspmm_csr_lp_dev.argtypes) == 18
    assert len(lib.exblas_exspmv_csr_lp_ctx.argtypes) == 16 and len(lib.exblas_exspmv_csr_lp.argtypes) == 14


@pytest.mark.parametrize("name", ["exspmv_lp", "exspmm_lp"])
def test_dev_functions_are_the_default_contexts_methods(name):
    f = getattr(exblas_amd, name + "_dev")
    assert inspect.ismethod(f) and f.__func__ is getattr(exblas_amd.Context, name)
    assert isinstance(f.__self__, exblas_amd.Context) and f.__self__.handle is None
    assert f.__self__ is exblas_amd.exspmv_dev.__self__
    params = list(inspect.signature(getattr(exblas_amd.Context, name)).parameters.values())
    assert params[0].name == "self" and inspect.signature(f) == inspect.Signature(params[1:])
    assert [p.name for p in params[3:]] == ["alpha", "beta", "y" if name == "exspmv_lp" else "Y", "fpe", "early_exit"]
    assert [p.default for p in params[3:]] == [1.0, 0.0, None, 8, True]
    assert callable(exblas_amd.exspmv_lp) and callable(exblas_amd.exspmm_lp) and callable(exblas_amd.round_interval_host)


def _buffers():
    rp = np.array([0, 1, 2], dtype=np.int32)
    ci = np.array([0, 1], dtype=np.int32)
    buf = np.zeros(64, dtype=np.uint8)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    return rp, ci, buf, base


def _spmv(lib, vdt, val, xdt, x, y, fpe=8, m=2, n=2, bits=32, rp=None, ci=None, entry="dev"):
    keep = _buffers()
    rp = keep[0].ctypes.data if rp is None else rp
    ci = keep[1].ctypes.data if ci is None else ci
    args = [m, n, bits, C.c_void_p(rp), C.c_void_p(ci), vdt, C.c_void_p(val), 1.0, xdt, C.c_void_p(x), 0.0, C.c_void_p(y), fpe, 1]
    if entry == "dev":
        return lib.exblas_exspmv_csr_lp_dev(*args, None)
    if entry == "ctx":
        return lib.exblas_exspmv_csr_lp_ctx(None, *args, None)
    return lib.exblas_exspmv_csr_lp(*args)


def _spmm(lib, vdt, val, xdt, x, y, fpe=8, m=2, n=2, k=3, ldx=3, ldy=3, bits=32, entry="dev"):
    keep = _buffers()
    args = [m, n, k, bits, C.c_void_p(keep[0].ctypes.data), C.c_void_p(keep[1].ctypes.data), vdt, C.c_void_p(val), 1.0, xdt,
            C.c_void_p(x), ldx, 0.0, C.c_void_p(y), ldy, fpe, 1]
    if entry == "dev":
        return lib.exblas_exspmm_csr_lp_dev(*args, None)
    if entry == "ctx":
        return lib.exblas_exspmm_csr_lp_ctx(None, *args, None)
    return lib.exblas_exspmm_csr_lp(*args)


@pytest.mark.parametrize("entry", ["dev", "ctx", "host"])
def test_c_refusals_need_no_device(lib, entry):
    """an fp64 matrix with narrow vectors, two narrow types, an unknown dtype, a pointer that is no multiple of its element
    size, fpe = 1 (EXBLAS_UNSUPPORTED) and any other bad fpe, and the shape errors of the fp64 entries: all answered from
    the arguments alone (this process has no GPU to ask)"""
    _, _, buf, b = _buffers()
    for call in (_spmv, _spmm):
        ok = dict(entry=entry)
        assert call(lib, F64, b, F32, b, b, **ok) == INVALID
        assert call(lib, F64, b, BF16, b, b, **ok) == INVALID
        assert call(lib, F32, b, F16, b, b, **ok) == INVALID
        assert call(lib, F16, b, BF16, b, b, **ok) == INVALID
        assert call(lib, 4, b, F64, b, b, **ok) == INVALID
        assert call(lib, F32, b, -1, b, b, **ok) == INVALID
        assert call(lib, F32, b + 2, F32, b, b, **ok) == INVALID
        assert call(lib, F32, b, F32, b + 2, b, **ok) == INVALID
        assert call(lib, F16, b, F16, b, b + 1, **ok) == INVALID
        assert call(lib, BF16, b + 2, F64, b + 4, b, **ok) == INVALID
        for vdt, xdt in ((F32, F32), (F16, F64), (BF16, BF16)):
            assert call(lib, vdt, b, xdt, b, b, fpe=1, **ok) == UNSUPPORTED
            assert call(lib, vdt, b, xdt, b, b, fpe=9, **ok) == INVALID
            assert call(lib, vdt, b, xdt, b, b, fpe=-1, **ok) == INVALID
            assert call(lib, vdt, b, xdt, b, b, m=-1, **ok) == INVALID
            assert call(lib, vdt, b, xdt, b, b, n=-2, **ok) == INVALID
            assert call(lib, vdt, b, xdt, b, b, bits=16, **ok) == INVALID
            assert call(lib, vdt, b, xdt, b, 0, **ok) == INVALID              # y == NULL with m > 0
        assert call(lib, F64, b, F64, b, b, fpe=-1, **ok) == INVALID           # forwarded: the fp64 entry's own refusal
    assert _spmm(lib, F32, b, F32, b, b, ldx=2, entry=entry) == INVALID
    assert _spmm(lib, F32, b, F64, b, b, ldy=2, entry=entry) == INVALID
    assert _spmm(lib, F32, b, F32, b, b, k=-1, ldx=0, ldy=0, entry=entry) == INVALID


def _csr(vdtype, itype=torch.int32):
    return (torch.tensor([0, 1, 2], dtype=itype), torch.tensor([0, 1], dtype=itype), torch.ones(2, dtype=vdtype), (2, 2))


def test_python_refusals_need_no_device():
    ex = exblas_amd
    x32, x16, xb, x64 = (torch.ones(2, dtype=t) for t in (torch.float32, torch.float16, torch.bfloat16, torch.float64))
    with pytest.raises(TypeError):
        ex.exspmv_lp_dev(_csr(torch.float64), x32)                # fp64 matrix, narrow vectors
    with pytest.raises(TypeError):
        ex.exspmv_lp_dev(_csr(torch.float32), x16)                # two narrow types
    with pytest.raises(TypeError):
        ex.exspmm_lp_dev(_csr(torch.bfloat16), torch.ones((2, 3), dtype=torch.float16))
    with pytest.raises(TypeError):
        ex.exspmv_lp_dev(_csr(torch.int32), x64)                  # an unknown value dtype
    with pytest.raises(TypeError):
        ex.exspmv_lp_dev(_csr(torch.float32), torch.ones(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        ex.exspmv_lp_dev(_csr(torch.float32), x32, y=torch.zeros(2, dtype=torch.float64))    # y of another type than x
    with pytest.raises(NotImplementedError):
        ex.exspmv_lp_dev(_csr(torch.float32), x32, fpe=1)
    with pytest.raises(NotImplementedError):
        ex.exspmm_lp_dev(_csr(torch.float16), torch.ones((2, 3), dtype=torch.float64), fpe=1)
    with pytest.raises(ValueError):
        ex.exspmv_lp_dev(_csr(torch.float32), x32, fpe=9)
    with pytest.raises(ValueError):
        ex.exspmv_lp_dev(_csr(torch.float32), torch.ones(1, dtype=torch.float32))            # x shorter than n
    with pytest.raises(ValueError):
        ex.exspmm_lp_dev(_csr(torch.float32), x32)                                            # X must be 2-D
    with pytest.raises(ValueError):
        ex.exspmm_lp_dev(_csr(torch.float32), torch.ones((2, 3), dtype=torch.float32), Y=torch.zeros((2, 2), dtype=torch.float32))
    with pytest.raises(TypeError):
        ex.exspmv_lp_dev((torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int64),
                          torch.ones(2, dtype=torch.float32), (2, 2)), x32)
    # the host forms
    A = (np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=np.float32), (2, 2))
    with pytest.raises(TypeError):
        ex.exspmv_lp(A, np.ones(2, dtype=np.float16))
    with pytest.raises(NotImplementedError):
        ex.exspmv_lp(A, np.ones(2, dtype=np.float32), fpe=1)
    with pytest.raises(TypeError):
        ex.exspmm_lp((A[0], A[1], np.ones(2), (2, 2)), torch.ones((2, 2), dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        ex.exspmm_lp(A, np.ones(2, dtype=np.float32))


def test_fp64_entries_still_refuse_narrow_values():
    ex = exblas_amd
    for vd in (torch.float32, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError, match="values must be float64"):
            ex.exspmv_dev(_csr(vd), torch.ones(2, dtype=torch.float64))
        with pytest.raises(TypeError, match="values must be float64"):
            ex.exspmm_dev(_csr(vd), torch.ones((2, 2), dtype=torch.float64))
        with pytest.raises(TypeError, match="values must be float64"):
            ex.exsptrsv_dev(_csr(vd), torch.ones(2, dtype=torch.float64))
    A = (np.array([0, 1, 2], dtype=np.int32), np.array([0, 1], dtype=np.int32), np.ones(2, dtype=np.float32), (2, 2))
    with pytest.raises(TypeError, match="values must be float64"):
        ex.exspmv(A, np.ones(2))
    with pytest.raises(TypeError, match="must be float64"):
        ex.exspmv_dev(_csr(torch.float64), torch.ones(2, dtype=torch.float32))
