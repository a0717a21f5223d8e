"""CPU suite: argument validation of the ExSpIC0 Python layer and of its C entries.  Everything here is refused before a
GPU is needed (ValueError / TypeError, never the no-GPU RuntimeError; hipErrorInvalidValue from the C entries)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import exblas_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("exblas_exspic0_csr_dev", "exblas_exspic0_csr_ctx", "exblas_exspic0_csr", "exblas_set_spic0_path",
           "exblas_last_spic0_info")
INVALID = 1                                      # hipErrorInvalidValue


def _csr(itype=torch.int64):
    crow = torch.tensor([0, 2, 4, 6, 8], dtype=itype)
    col = torch.tensor([0, 1, 0, 1, 2, 3, 2, 3], dtype=itype)
    val = torch.tensor([4.0, 1.0, 1.0, 4.0, 4.0, 1.0, 1.0, 4.0], dtype=torch.float64)
    return crow, col, val, (4, 4)


def test_symbols_declared_listed_and_exported():
    lib = exblas_amd.load_library()
    header = open(os.path.join(ROOT, "include", "exblas_hip.h")).read()
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS and hasattr(lib, name) and name + "(" in header, name
    assert len(lib.exblas_exspic0_csr_dev.argtypes) == 10 and len(lib.exblas_exspic0_csr_ctx.argtypes) == 11
    assert len(lib.exblas_exspic0_csr.argtypes) == 9
    assert lib.exblas_set_spic0_path.restype is None and len(lib.exblas_last_spic0_info.argtypes) == 1
    for name in ("exspic0_dev", "exspic0_apply_dev", "exspic0", "set_spic0_path", "last_spic0_info"):
        assert callable(getattr(exblas_amd, name))


def test_dev_entries_are_the_default_contexts_bound_methods():
    assert exblas_amd.exspic0_dev.__func__ is exblas_amd.Context.exspic0
    assert exblas_amd.exspic0_apply_dev.__func__ is exblas_amd.Context.exspic0_apply
    assert exblas_amd.exspic0_dev.__self__ is exblas_amd.exsptrsv_dev.__self__


@pytest.mark.parametrize("bad", ["not_square", "val_dtype", "mixed_width", "int16", "crow_len", "col_len", "shape3", "not_csr",
                                 "dense_layout", "out_short", "out_long", "out_dtype", "out_2d", "out_strided", "out_device",
                                 "out_not_tensor", "info_dtype", "info_len", "info_device", "fpe_negative"])
def test_exspic0_dev_rejects_bad_arguments(bad):
    crow, col, val, shape = _csr()
    out, info, A, fpe = None, None, None, 8
    if bad == "not_square":
        shape = (4, 5)
    elif bad == "val_dtype":
        val = val.float()
    elif bad == "mixed_width":
        col = col.int()
    elif bad == "int16":
        crow, col = crow.short(), col.short()
    elif bad == "crow_len":
        crow = crow[:-1]
    elif bad == "col_len":
        col = col[:-1]
    elif bad == "shape3":
        shape = (4, 4, 1)
    elif bad == "not_csr":
        A = np.zeros((4, 4))
    elif bad == "dense_layout":
        A = torch.zeros(4, 4, dtype=torch.float64)
    elif bad == "out_short":
        out = torch.zeros(7, dtype=torch.float64)
    elif bad == "out_long":
        out = torch.zeros(9, dtype=torch.float64)
    elif bad == "out_dtype":
        out = torch.zeros(8, dtype=torch.float32)
    elif bad == "out_2d":
        out = torch.zeros(8, 1, dtype=torch.float64)
    elif bad == "out_strided":
        out = torch.zeros(16, dtype=torch.float64)[::2]
    elif bad == "out_device":
        out = torch.zeros(8, dtype=torch.float64, device="meta")
    elif bad == "out_not_tensor":
        out = np.zeros(8)
    elif bad == "info_dtype":
        info = torch.zeros(2, dtype=torch.int32)
    elif bad == "info_len":
        info = torch.zeros(1, dtype=torch.int64)
    elif bad == "info_device":
        info = torch.zeros(2, dtype=torch.int64, device="meta")
    elif bad == "fpe_negative":
        fpe = -1
    if A is None:
        A = (crow, col, val, shape)
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.exspic0_dev(A, out=out, info=info, fpe=fpe)
    assert str(err.value).startswith("exspic0:")
    if bad == "fpe_negative":
        assert "fpe" in str(err.value)
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.Context.exspic0(ctx, A, out, info, fpe)
    assert str(err.value).startswith("exspic0:")


def test_apply_takes_a_vector_or_a_block_and_refuses_the_rest():
    LL = _csr()
    for X, kind in ((torch.ones(4, 1, 1, dtype=torch.float64), ValueError), (np.ones(4), (TypeError, ValueError)),
                    (torch.ones(5, dtype=torch.float64), ValueError),
                    (torch.ones(5, 3, dtype=torch.float64), ValueError),
                    (torch.ones(4, dtype=torch.float32), TypeError),
                    (torch.ones(4, 3, dtype=torch.float64).t().contiguous().t(), ValueError),
                    (torch.ones(4, dtype=torch.float64, device="meta"), ValueError)):
        with pytest.raises(kind):
            exblas_amd.exspic0_apply_dev(LL, X)
    with pytest.raises(ValueError, match="^exsptrsv:"):
        exblas_amd.exspic0_apply_dev(LL, torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="^exsptrsm:"):
        exblas_amd.exspic0_apply_dev(LL, torch.ones(3, 2, dtype=torch.float64))


def test_host_form_rejects_bad_arguments_and_is_loud_without_a_device():
    crow = np.array([0, 2, 4], dtype=np.int64)
    col = np.array([0, 1, 0, 1], dtype=np.int64)
    val = np.array([4.0, 1.0, 1.0, 3.0])
    with pytest.raises(TypeError):
        exblas_amd.exspic0((crow.astype(np.int32), col, val, (2, 2)))
    with pytest.raises(TypeError):
        exblas_amd.exspic0((crow, col, val.astype(np.float32), (2, 2)))
    with pytest.raises(ValueError):
        exblas_amd.exspic0((crow, col, val, (2, 3)))
    with pytest.raises(ValueError):
        exblas_amd.exspic0((np.array([0, 5, 4], dtype=np.int64), col, val, (2, 2)))
    with pytest.raises(ValueError):
        exblas_amd.exspic0((crow, col, val))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            exblas_amd.exspic0((crow, col, val, (2, 2)))
        with pytest.raises(RuntimeError):
            exblas_amd.exspic0_dev((torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), (2, 2)))


# The C entries, in a child process: each call below must be refused before a context is looked up (without a device,
# a path that reaches it ends the process, which the parent then sees).
_CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import exblas_amd
L = exblas_amd.load_library()
rp = np.array([0, 2, 4], dtype=np.int64); rp32 = rp.astype(np.int32); neg = np.array([0, -1, 4], dtype=np.int64)
ci = np.array([0, 1, 0, 1], dtype=np.int64); v = np.array([4.0, 1.0, 1.0, 3.0]); ll = v.copy()
info = np.full(2, 77, dtype=np.int64)
P = lambda a: ctypes.c_void_p(a.ctypes.data)
out = {}
def dev(name, m=2, bits=64, r=rp, inf=info, fpe=8):
    out["dev " + name] = L.exblas_exspic0_csr_dev(m, bits, None if r is None else P(r), P(ci), P(v), P(ll),
                                                  None if inf is None else P(inf), fpe, 1, None)
    out["ctx " + name] = L.exblas_exspic0_csr_ctx(None, m, bits, None if r is None else P(r), P(ci), P(v), P(ll),
                                                  None if inf is None else P(inf), fpe, 1, None)
def host(name, m=2, bits=64, r=rp, inf=info, fpe=8, o=ll):
    out["host " + name] = L.exblas_exspic0_csr(m, bits, None if r is None else P(r), P(ci), P(v),
                                               None if o is None else P(o), None if inf is None else P(inf), fpe, 1)
for f in (dev, host):
    f("m negative", m=-1)
    f("index bits 16", bits=16)
    f("index bits 0", bits=0)
    f("info null", inf=None)
    f("row_ptr null", r=None)
dev("fpe negative", fpe=-1)
dev("fpe negative, m 0", m=0, fpe=-1)
host("fpe negative, m 0", m=0, fpe=-1)
host("fpe negative", fpe=-1)
host("negative row_ptr entry", r=neg)
host("ll null", o=None)
host("int32 row_ptr with 64-bit columns read as 32", bits=32, r=rp32, fpe=-3)
out["last info null"] = L.exblas_last_spic0_info(None)
out["unchanged"] = bool((ll == v).all())
print("RESULT " + json.dumps(out))
"""


def test_c_entries_refuse_invalid_arguments_in_a_child_process():
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert line, r.stdout[-2000:]
    got = json.loads(line[-1][len("RESULT "):])
    assert got.pop("unchanged") is True
    bad = {k: v for k, v in got.items() if v != INVALID}
    assert not bad, bad
    assert len(got) == 25
