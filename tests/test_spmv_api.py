"""CPU suite: argument validation of the ExSpMV Python layer, and the loud failure without a GPU."""
import numpy as np
import pytest
import torch

import exblas_amd


def _csr(m=4, n=5, itype=torch.int64):
    crow = torch.tensor([0, 2, 2, 3, 5], dtype=itype)
    col = torch.tensor([0, 4, 1, 2, 3], dtype=itype)
    val = torch.arange(5, dtype=torch.float64)
    return crow, col, val, (m, n)


def test_symbols_in_abi_list():
    for name in ("exblas_exspmv_csr_dev", "exblas_exspmv_csr_ctx", "exblas_exspmv_csr", "exblas_set_spmv_path",
                 "exblas_last_spmv_info"):
        assert name in exblas_amd.C_ABI_SYMBOLS


@pytest.mark.parametrize("bad", ["val_dtype", "x_dtype", "mixed_width", "int16", "crow_len", "col_len", "x_short",
                                 "y_len", "y_dtype", "shape3", "not_csr"])
def test_exspmv_dev_rejects_bad_arguments(bad):
    crow, col, val, shape = _csr()
    x = torch.ones(5, dtype=torch.float64)
    y = None
    A = None
    if bad == "val_dtype":
        val = val.float()
    elif bad == "x_dtype":
        x = x.float()
    elif bad == "mixed_width":
        col = col.int()
    elif bad == "int16":
        crow, col = crow.short(), col.short()
    elif bad == "crow_len":
        crow = crow[:-1]
    elif bad == "col_len":
        col = col[:-1]
    elif bad == "x_short":
        x = x[:4]
    elif bad == "y_len":
        y = torch.zeros(3, dtype=torch.float64)
    elif bad == "y_dtype":
        y = torch.zeros(4, dtype=torch.float32)
    elif bad == "shape3":
        shape = (4, 5, 1)
    elif bad == "not_csr":
        A = torch.zeros(4, 5, dtype=torch.float64)
    if A is None:
        A = (crow, col, val, shape)
    with pytest.raises((TypeError, ValueError)):
        exblas_amd.exspmv_dev(A, x, 1.0, 0.0, y)


def test_sparse_csr_tensor_is_accepted_up_to_the_device_check():
    crow, col, val, shape = _csr()
    A = torch.sparse_csr_tensor(crow, col, val, size=shape)
    x = torch.ones(5, dtype=torch.float64)
    if torch.cuda.is_available():
        with pytest.raises(ValueError):   # CPU tensors on a GPU machine: wrong device
            exblas_amd.exspmv_dev(A, x)
    else:
        with pytest.raises(RuntimeError):  # no GPU: no CPU fallback
            exblas_amd.exspmv_dev(A, x)


def test_host_exspmv_rejects_bad_arguments():
    crow = np.array([0, 2, 3], dtype=np.int32)
    col = np.array([0, 1, 1], dtype=np.int64)
    val = np.ones(3)
    with pytest.raises(TypeError):
        exblas_amd.exspmv((crow, col, val, (2, 2)), np.ones(2))
    with pytest.raises(ValueError):
        exblas_amd.exspmv((crow.astype(np.int64), col, val, (2, 2)), np.ones(1))
    with pytest.raises(ValueError):
        exblas_amd.exspmv((np.array([0, 4, 3], dtype=np.int64), col, val, (2, 2)), np.ones(2))


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    crow, col, val, shape = _csr()
    with pytest.raises(RuntimeError):
        exblas_amd.exspmv_dev((crow, col, val, shape), torch.ones(5, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        exblas_amd.exspmv((crow.numpy(), col.numpy(), val.numpy(), shape), np.ones(5))
