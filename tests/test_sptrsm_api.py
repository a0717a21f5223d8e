"""CPU suite: argument validation of the ExSpTRSM Python layer, the C signatures, and the block of right-hand sides the
GPU tests use (tests/sptrsm_cases.py)."""
import numpy as np
import pytest
import torch

import exact_cases as X
import exblas_amd
import sptrsm_cases as M

SYMBOLS = ("exblas_exsptrsm_csr_dev", "exblas_exsptrsm_csr_ctx", "exblas_exsptrsm_csr", "exblas_set_sptrsm_path",
           "exblas_last_sptrsm_info")


def _csr(itype=torch.int64):
    crow = torch.tensor([0, 1, 3, 4, 6], dtype=itype)
    col = torch.tensor([0, 0, 1, 2, 1, 3], dtype=itype)
    val = torch.arange(1, 7, dtype=torch.float64)
    return crow, col, val, (4, 4)


def test_symbols_in_abi_list_and_signatures():
    for name in SYMBOLS:
        assert name in exblas_amd.C_ABI_SYMBOLS
    lib = exblas_amd.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
    dev = lib.exblas_exsptrsm_csr_dev.argtypes
    assert len(dev) == 13 and len(lib.exblas_exsptrsm_csr_ctx.argtypes) == 14 and len(lib.exblas_exsptrsm_csr.argtypes) == 12
    # (uplo, diag, m, k, index_bits, row_ptr, col_idx, val, x, ldx, fpe, early_exit, stream): ldx is 64-bit
    import ctypes
    assert dev[0] is ctypes.c_char and dev[1] is ctypes.c_char and dev[9] is ctypes.c_int64 and dev[3] is ctypes.c_int
    assert lib.exblas_set_sptrsm_path.restype is None and len(lib.exblas_set_sptrsm_path.argtypes) == 1
    assert len(lib.exblas_last_sptrsm_info.argtypes) == 1
    for name in ("exsptrsm_dev", "exsptrsm", "set_sptrsm_path", "last_sptrsm_info"):
        assert callable(getattr(exblas_amd, name))
    assert callable(exblas_amd.Context.exsptrsm)


@pytest.mark.parametrize("bad", ["not_square", "val_dtype", "x_dtype", "mixed_width", "int16", "crow_len", "col_len",
                                 "x_1d", "x_3d", "x_rows_short", "x_rows_long", "x_col_major", "x_col_strided",
                                 "x_rows_overlap", "uplo", "diag", "uplo_type", "devices", "shape3", "not_csr",
                                 "x_not_tensor", "val_not_tensor"])
def test_exsptrsm_dev_rejects_bad_arguments(bad):
    """every one of these is refused before a GPU is needed (ValueError / TypeError, never the no-GPU RuntimeError)"""
    crow, col, val, shape = _csr()
    x = torch.ones(4, 3, dtype=torch.float64)
    uplo, diag, A = "L", "N", None
    if bad == "not_square":
        shape = (4, 5)
    elif bad == "val_dtype":
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
        x = torch.ones(4, dtype=torch.float64)
    elif bad == "x_3d":
        x = torch.ones(4, 3, 1, dtype=torch.float64)
    elif bad == "x_rows_short":
        x = x[:3]
    elif bad == "x_rows_long":
        x = torch.ones(5, 3, dtype=torch.float64)
    elif bad == "x_col_major":
        x = torch.ones(3, 4, dtype=torch.float64).t()            # stride (1, 4)
    elif bad == "x_col_strided":
        x = torch.ones(4, 6, dtype=torch.float64)[:, ::2]        # stride (6, 2)
    elif bad == "x_rows_overlap":
        x = torch.ones(1, 3, dtype=torch.float64).expand(4, 3)   # stride (0, 1): stride(0) < k
    elif bad == "uplo":
        uplo = "X"
    elif bad == "diag":
        diag = "T"
    elif bad == "uplo_type":
        uplo = 1
    elif bad == "devices":
        x = torch.ones(4, 3, dtype=torch.float64, device="meta")
    elif bad == "shape3":
        shape = (4, 4, 1)
    elif bad == "not_csr":
        A = torch.zeros(4, 4, dtype=torch.float64)
    elif bad == "x_not_tensor":
        x = np.ones((4, 3))
    elif bad == "val_not_tensor":
        val = val.numpy()
    if A is None:
        A = (crow, col, val, shape)
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.exsptrsm_dev(A, x, uplo, diag)
    assert str(err.value).startswith("exsptrsm:")               # the routine that was called, whichever helper refused
    if bad == "x_1d":
        assert "exsptrsv_dev" in str(err.value)                  # one vector: the message names the routine for it
    ctx = object.__new__(exblas_amd.Context)     # the method validates before it touches the handle
    ctx.handle = None
    with pytest.raises((TypeError, ValueError)) as err:
        exblas_amd.Context.exsptrsm(ctx, A, x, uplo, diag)
    assert str(err.value).startswith("exsptrsm:")


def test_an_overlapping_block_with_stride_one_less_than_k_is_refused():
    base = torch.ones(16, dtype=torch.float64)
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm_dev(_csr(), base.as_strided((4, 3), (2, 1)))


def test_host_exsptrsm_rejects_bad_arguments():
    crow = np.array([0, 1, 3], dtype=np.int64)
    col = np.array([0, 0, 1], dtype=np.int64)
    val = np.ones(3)
    good = (crow, col, val, (2, 2))
    B = np.ones((2, 3))
    with pytest.raises(TypeError):
        exblas_amd.exsptrsm((crow.astype(np.int32), col, val, (2, 2)), B)
    with pytest.raises(TypeError):
        exblas_amd.exsptrsm(good, B.astype(np.float32))
    with pytest.raises(TypeError):
        exblas_amd.exsptrsm((crow, col, val.astype(np.float32), (2, 2)), B)
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm((crow, col, val, (2, 3)), B)
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm(good, np.ones((3, 3)))
    with pytest.raises(ValueError) as err:
        exblas_amd.exsptrsm(good, np.ones(2))
    assert "exsptrsv" in str(err.value)
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm(good, np.ones((2, 3, 1)))
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm((np.array([0, 4, 3], dtype=np.int64), col, val, (2, 2)), B)
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm(good, B, uplo="T")
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm(good, B, diag="X")
    with pytest.raises(ValueError):
        exblas_amd.exsptrsm((crow, col, val), B)


def test_no_gpu_means_loud_failure():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    crow, col, val, shape = _csr()
    with pytest.raises(RuntimeError):
        exblas_amd.exsptrsm_dev((crow, col, val, shape), torch.ones(4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        exblas_amd.exsptrsm((crow.numpy(), col.numpy(), val.numpy(), shape), np.ones((4, 3)))


def test_column_plan_cycles_kinds_signs_and_scales():
    plans = [M.column_plan(j) for j in range(30)]
    assert [p[0] for p in plans[:6]] == ["b", "control", "random"] * 2
    assert {p[2] for p in plans} == set(M.SCALES) and {p[1] for p in plans} == {1.0, -1.0}
    assert {(p[1], p[2]) for p in plans if p[0] == "b"} == {(s, e) for s in (1.0, -1.0) for e in M.SCALES}


@pytest.mark.parametrize("unit", [False, True], ids=["nonunit", "unit"])
@pytest.mark.parametrize("case", [0, 2])
def test_scaled_columns_keep_their_ties(case, unit):
    """a sign and a power of two scale the whole substitution exactly: for every column that derives from b or from
    b_control, trsv_exact on the scaled column is the scaled solution, bit for bit"""
    n, W, mbits, filler = X.TRSV_CASES[case]
    c = X.planted_trsv(n, seed=21, W=W, mbits=mbits, filler=filler, unit=unit)
    blk = M.rhs_block(c, 33)
    assert blk.B.shape == (n, 33) and blk.B.flags.c_contiguous and blk.from_b == 11 and blk.kinds.count("control") == 11
    want = M.expected_block(c, blk, exact_b=True)                # trsv_exact on every column
    short = M.expected_block(c, blk)
    assert (want.view(np.int64) == short.view(np.int64)).all()
    control, _ = X.trsv_exact(c.L, c.b_control, unit)
    seen = set()
    for j, kind in enumerate(blk.kinds):
        if kind == "random":
            assert blk.scale[j] == 1.0 and (np.abs(blk.B[:, j]) >= 1).all() and (np.abs(blk.B[:, j]) < 2).all()
            continue
        base = c.want if kind == "b" else control
        assert (want[:, j].view(np.int64) == (base * blk.scale[j]).view(np.int64)).all(), (j, kind, blk.scale[j])
        seen.add(blk.scale[j])
    assert {2.0 ** -200, -(2.0 ** 40), 1.0, -(2.0 ** -3), 2.0 ** 5} <= seen
    assert np.isfinite(want).all()
    # a narrower block is a prefix of a wider one
    assert (M.rhs_block(c, 8).B.view(np.int64) == blk.B[:, :8].view(np.int64)).all()
    # the control moves every planted total off its tie: the two solutions differ
    assert (control.view(np.int64) != c.want.view(np.int64)).any()
