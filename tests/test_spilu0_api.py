"""CPU suite: argument validation of the ExSpILU0 Python layer and the C signatures.  Everything here is refused before a
GPU is needed (ValueError / TypeError, never the no-GPU RuntimeError)."""
import numpy as np
import pytest
import torch

import exblas_amd

SYMBOLS = ("exblas_exspilu0_csr_dev", "exblas_exspilu0_csr_ctx", "exblas_exspilu0_csr", "exblas_set_spilu0_path",
           "exblas_last_spilu0_info")


def _csr(itype=torch.int64):
    crow = torch.tensor([0, 2, 4, 6, 8], dtype=itype)
    col = torch.tensor([0, 1, 0, 1, 2, 3, 2, 3], dtype=itype)
    val = torch.arange(1, 9, dtype=torch.float64)
    return crow, col, val, (4, 4)


def test_symbols_in_abi_list_and_signatures():
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS
    lib = exblas_amd.load_library()
    assert len(lib.exblas_exspilu0_csr_dev.argtypes) == 10 and len(lib.exblas_exspilu0_csr_ctx.argtypes) == 11
    assert len(lib.exblas_exspilu0_csr.argtypes) == 9
    assert lib.exblas_set_spilu0_path.restype is None and len(lib.exblas_last_spilu0_info.argtypes) == 1
    for name in ("exspilu0_dev", "exspilu0_apply_dev", "exspilu0", "set_spilu0_path", "last_spilu0_info"):
        assert callable(getattr(exblas_amd, name))


def test_dev_entries_are_the_default_contexts_bound_methods():
    assert exblas_amd.exspilu0_dev.__func__ is exblas_amd.Context.exspilu0
    assert exblas_amd.exspilu0_apply_dev.__func__ is exblas_amd.Context.exspilu0_apply
    assert exblas_amd.exspilu0_dev.__self__ is exblas_amd.exsptrsv_dev.__self__


@pytest.mark.parametrize("bad", ["not_square", "val_dtype", "mixed_width", "int16", "crow_len", "col_len", "shape3", "not_csr",
                                 "dense_layout", "out_short", "out_long", "out_dtype", "out_2d", "out_strided", "out_device",
                                 "out_not_tensor", "info_dtype", "info_len", "info_device"])
def test_exspilu0_dev_rejects_bad_arguments(bad):
    crow, col, val, shape = _csr()
    out, info, A = None, None, None
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
    if A is None:
        A = (crow, col, val, shape)
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.exspilu0_dev(A, out=out, info=info)
    assert str(err.value).startswith("exspilu0:")
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.Context.exspilu0(ctx, A, out, info)
    assert str(err.value).startswith("exspilu0:")


def test_apply_takes_a_vector_or_a_block_and_refuses_the_rest():
    LU = _csr()
    for X, kind in ((torch.ones(4, 1, 1, dtype=torch.float64), ValueError), (np.ones(4), (TypeError, ValueError)),
                    (torch.ones(5, dtype=torch.float64), ValueError),              # a vector of the wrong length
                    (torch.ones(5, 3, dtype=torch.float64), ValueError),           # a block of the wrong height
                    (torch.ones(4, dtype=torch.float32), TypeError),
                    (torch.ones(4, 3, dtype=torch.float64).t().contiguous().t(), ValueError),   # a column-major block
                    (torch.ones(4, dtype=torch.float64, device="meta"), ValueError)):
        with pytest.raises(kind):
            exblas_amd.exspilu0_apply_dev(LU, X)
    # a 1-D X goes to ExSpTRSV and a 2-D X to ExSpTRSM: each names itself when it refuses
    with pytest.raises(ValueError, match="^exsptrsv:"):
        exblas_amd.exspilu0_apply_dev(LU, torch.ones(3, dtype=torch.float64))
    with pytest.raises(ValueError, match="^exsptrsm:"):
        exblas_amd.exspilu0_apply_dev(LU, torch.ones(3, 2, dtype=torch.float64))


def test_host_form_rejects_bad_arguments_and_is_loud_without_a_device():
    crow = np.array([0, 2, 4], dtype=np.int64)
    col = np.array([0, 1, 0, 1], dtype=np.int64)
    val = np.array([4.0, 1.0, 2.0, 3.0])
    with pytest.raises(TypeError):
        exblas_amd.exspilu0((crow.astype(np.int32), col, val, (2, 2)))
    with pytest.raises(TypeError):
        exblas_amd.exspilu0((crow, col, val.astype(np.float32), (2, 2)))
    with pytest.raises(ValueError):
        exblas_amd.exspilu0((crow, col, val, (2, 3)))
    with pytest.raises(ValueError):
        exblas_amd.exspilu0((np.array([0, 5, 4], dtype=np.int64), col, val, (2, 2)))
    with pytest.raises(ValueError):
        exblas_amd.exspilu0((crow, col, val))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):
            exblas_amd.exspilu0((crow, col, val, (2, 2)))
        with pytest.raises(RuntimeError):
            exblas_amd.exspilu0_dev((torch.from_numpy(crow), torch.from_numpy(col), torch.from_numpy(val), (2, 2)))
