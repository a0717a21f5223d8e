"""CPU suite: argument validation of the ExSpMM Python layer, and the loud failure without a GPU."""
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
    for name in ("exblas_exspmm_csr_dev", "exblas_exspmm_csr_ctx", "exblas_exspmm_csr", "exblas_set_spmm_path",
                 "exblas_last_spmm_info"):
        assert name in exblas_amd.C_ABI_SYMBOLS
    for name in ("exspmm_dev", "exspmm", "set_spmm_path", "last_spmm_info"):
        assert callable(getattr(exblas_amd, name))
    assert callable(exblas_amd.Context.exspmm)


@pytest.mark.parametrize("bad", ["val_dtype", "x_dtype", "mixed_width", "int16", "crow_len", "col_len", "x_1d",
                                 "x_short", "y_shape", "y_1d", "y_dtype", "y_stride", "shape3", "not_csr"])
def test_exspmm_dev_rejects_bad_arguments(bad):
    crow, col, val, shape = _csr()
    x = torch.ones(5, 3, dtype=torch.float64)
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
    elif bad == "x_1d":
        x = torch.ones(5, dtype=torch.float64)
    elif bad == "x_short":
        x = x[:4]
    elif bad == "y_shape":
        y = torch.zeros(4, 2, dtype=torch.float64)
    elif bad == "y_1d":
        y = torch.zeros(12, dtype=torch.float64)
    elif bad == "y_dtype":
        y = torch.zeros(4, 3, dtype=torch.float32)
    elif bad == "y_stride":
        y = torch.zeros(3, 4, dtype=torch.float64).t()   # 4 x 3 with stride(1) == 4
    elif bad == "shape3":
        shape = (4, 5, 1)
    elif bad == "not_csr":
        A = torch.zeros(4, 5, dtype=torch.float64)
    if A is None:
        A = (crow, col, val, shape)
    with pytest.raises((TypeError, ValueError)) as err:   # before any GPU check: RuntimeError would mean it came too late
        exblas_amd.exspmm_dev(A, x, 1.0, 0.0, y)
    assert str(err.value).startswith("exspmm:")   # the routine that was called, whichever helper refused


def test_one_dimensional_x_points_to_exspmv():
    crow, col, val, shape = _csr()
    with pytest.raises(ValueError, match="exspmv_dev"):
        exblas_amd.exspmm_dev((crow, col, val, shape), torch.ones(5, dtype=torch.float64))


def test_sparse_csr_tensor_is_accepted_up_to_the_device_check():
    crow, col, val, shape = _csr()
    A = torch.sparse_csr_tensor(crow, col, val, size=shape)
    x = torch.ones(5, 3, dtype=torch.float64)
    y = torch.zeros(4, 8, dtype=torch.float64)[:, :3]   # a padded Y (stride(0) = 8) is valid
    if torch.cuda.is_available():
        with pytest.raises(ValueError):   # CPU tensors on a GPU machine: wrong device
            exblas_amd.exspmm_dev(A, x, 1.0, 0.0, y)
    else:
        with pytest.raises(RuntimeError):  # no GPU: no CPU fallback
            exblas_amd.exspmm_dev(A, x, 1.0, 0.0, y)


def test_host_exspmm_rejects_bad_arguments():
    crow = np.array([0, 2, 3], dtype=np.int32)
    col = np.array([0, 1, 1], dtype=np.int64)
    val = np.ones(3)
    with pytest.raises(TypeError):
        exblas_amd.exspmm((crow, col, val, (2, 2)), np.ones((2, 3)))
    col = col.astype(np.int64)
    crow = crow.astype(np.int64)
    with pytest.raises(ValueError):
        exblas_amd.exspmm((crow, col, val, (2, 2)), np.ones((1, 3)))          # X too short
    with pytest.raises(ValueError):
        exblas_amd.exspmm((crow, col, val, (2, 2)), np.ones(2))               # 1-D X
    with pytest.raises(ValueError):
        exblas_amd.exspmm((crow, col[:-1], val, (2, 2)), np.ones((2, 3)))     # col / val differ
    with pytest.raises(ValueError):
        exblas_amd.exspmm((crow, col, val, (2, 2)), np.ones((2, 3)), 1.0, 1.0, np.ones((2, 2)))   # Y shape
    with pytest.raises(ValueError):
        exblas_amd.exspmm((np.array([0, 4, 3], dtype=np.int64), col, val, (2, 2)), np.ones((2, 3)))
    with pytest.raises(ValueError):
        exblas_amd.exspmm((np.array([0, -1, 3], dtype=np.int64), col, val, (2, 2)), np.ones((2, 3)))


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    crow, col, val, shape = _csr()
    with pytest.raises(RuntimeError):
        exblas_amd.exspmm_dev((crow, col, val, shape), torch.ones(5, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        exblas_amd.exspmm((crow.numpy(), col.numpy(), val.numpy(), shape), np.ones((5, 3)))
