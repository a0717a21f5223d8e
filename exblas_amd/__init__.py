"""exblas_amd -- MI355X-native (gfx950, HIP) ExBLAS hot path: exact, reproducible sum / dot / gemv / gemm.

This package is the host-side mirror of the reference's public API (include/blas1.hpp:48,74,
blas2.hpp:95, blas3.hpp:56 of nikolovjovan/exblas) on top of the C ABI of ``lib/libexblas.so``
(``include/exblas_hip.h``).  PyTorch is used only as plumbing (device memory, streams,
``torch.distributed``); every reduction runs in the hand-written HIP kernels under ``csrc/``.

There is NO CPU fallback: importing works without a GPU (so the ABI can be inspected), but any
compute call without a HIP device fails loudly.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libexblas.so")

OUT_WORDS, OUT_EXACT, OUT_REFMODE, OUT_FLAGS, OUT_CANON, OUT_DIGITS = 128, 0, 1, 2, 4, 48
NDIGITS, NCANON, SET_WORDS = 68, 41, 72
GEN_KINDS = {"naive": 0, "fpuniform": 1, "lognormal": 2, "ill_cond": 3, "cancel": 4, "fpuniform_signed": 5}

# every symbol include/exblas_hip.h declares (checked by tests/test_abi.py)
C_ABI_SYMBOLS = [
    "exblas_hip_init", "exblas_hip_device_count", "exblas_hip_version", "exblas_set_round_mode",
    "exblas_get_round_mode", "exblas_exsum_dev", "exblas_exdot_dev", "exblas_finalize_dev", "exblas_exgemv_dev",
    "exblas_exgemm_dev", "exblas_gen_dev", "exblas_stream_read_dev", "exblas_exsum", "exblas_exdot",
    "exblas_exgemv", "exblas_exgemm", "exblas_exsum_record", "exblas_exdot_record",
    "exblas_exsum_accumulate_dev", "exblas_exdot_accumulate_dev", "exblas_finish_dev", "exblas_set_tuning",
    "exblas_set_gemm_path", "exblas_last_gemm_slices", "exblas_exsum_segmented_dev",
    "exblas_set_accumulator_slot", "exblas_set_launch_events", "exblas_stream_read2_dev", "exblas_extrsv_dev", "exblas_extrsv",
    "exblas_extrsv_last_slow_rows", "exblas_reserve_workspace", "exblas_release_retired_workspaces", "exblas_release_workspace",
    "exblas_comm_unique_id", "exblas_comm_init_rccl", "exblas_comm_adopt_rccl", "exblas_comm_init_host",
    "exblas_comm_destroy", "exblas_comm_rank", "exblas_comm_size", "exblas_shard_range",
    "exblas_exsum_allreduce_dev", "exblas_exdot_allreduce_dev", "exblas_allreduce_finish_dev",
    "exblas_exgemv_sharded_dev", "exblas_exgemm_sharded_dev", "exblas_last_gemm_info", "exblas_last_blas1_info",
    "exblas_set_gemm_max_slices",
    "exblas_set_gemm_max_moduli", "exblas_crt_selftest",
    "exblas_set_host_devices", "exblas_workspace_bytes",
    "exblas_exsum_allreduce_pipelined_dev", "exblas_exdot_allreduce_pipelined_dev", "exblas_pipeline_drain_dev",
    "exblas_ctx_create", "exblas_ctx_destroy", "exblas_exsum_ctx", "exblas_exdot_ctx", "exblas_exsum_accumulate_ctx",
    "exblas_exdot_accumulate_ctx", "exblas_finish_ctx", "exblas_exgemv_ctx", "exblas_extrsv_ctx", "exblas_exgemm_ctx",
    "exblas_reserve_workspace_ctx", "exblas_workspace_bytes_ctx", "exblas_last_gemm_info_ctx",
    "exblas_exspmv_csr_dev", "exblas_exspmv_csr_ctx", "exblas_exspmv_csr", "exblas_set_spmv_path",
    "exblas_last_spmv_info",
    "exblas_exspmm_csr_dev", "exblas_exspmm_csr_ctx", "exblas_exspmm_csr", "exblas_set_spmm_path",
    "exblas_last_spmm_info",
    "exblas_exspmv_csr_lp_dev", "exblas_exspmv_csr_lp_ctx", "exblas_exspmv_csr_lp",
    "exblas_exspmm_csr_lp_dev", "exblas_exspmm_csr_lp_ctx", "exblas_exspmm_csr_lp", "exblas_round_interval_host",
    "exblas_round_window_host",
    "exblas_exsptrsv_csr_dev", "exblas_exsptrsv_csr_ctx", "exblas_exsptrsv_csr", "exblas_set_sptrsv_path",
    "exblas_last_sptrsv_info",
    "exblas_exspilu0_csr_dev", "exblas_exspilu0_csr_ctx", "exblas_exspilu0_csr", "exblas_set_spilu0_path",
    "exblas_last_spilu0_info",
    "exblas_exspic0_csr_dev", "exblas_exspic0_csr_ctx", "exblas_exspic0_csr", "exblas_set_spic0_path", "exblas_last_spic0_info",
    "exblas_exsptrsm_csr_dev", "exblas_exsptrsm_csr_ctx", "exblas_exsptrsm_csr", "exblas_set_sptrsm_path",
    "exblas_last_sptrsm_info",
    "exblas_extrsm_dev", "exblas_extrsm_ctx", "exblas_extrsm", "exblas_set_trsm_path", "exblas_last_trsm_info",
    "exblas_exbdot_dev", "exblas_exbdot_ctx", "exblas_exbdot", "exblas_set_bdot_path",
    "exblas_exbdot_export_dev", "exblas_exbdot_export_ctx", "exblas_exbdot_round_dev", "exblas_exbdot_round_ctx",
    "exblas_exbdot_allreduce_dev",
    "exblas_exbgemm_dev", "exblas_exbgemm_ctx", "exblas_exbgemm", "exblas_set_bgemm_path", "exblas_last_bgemm_info",
    "exblas_exbtrsm_dev", "exblas_exbtrsm_ctx", "exblas_exbtrsm", "exblas_set_btrsm_path", "exblas_last_btrsm_info",
    "exblas_expotrf_dev", "exblas_expotrf_ctx", "exblas_expotrf", "exblas_set_potrf_path", "exblas_last_potrf_info",
    "exblas_expotrf_batched_dev", "exblas_expotrf_batched_ctx", "exblas_expotrf_batched", "exblas_set_potrf_batched_path",
    "exblas_last_potrf_batched_info",
    "exblas_expotrs_batched_dev", "exblas_expotrs_batched_ctx", "exblas_expotrs_batched", "exblas_set_potrs_batched_path",
    "exblas_last_potrs_batched_info",
    "exblas_exgetrf_batched_dev", "exblas_exgetrf_batched_ctx", "exblas_exgetrf_batched", "exblas_set_getrf_batched_path",
    "exblas_last_getrf_batched_info",
    "exblas_exgetrs_batched_dev", "exblas_exgetrs_batched_ctx", "exblas_exgetrs_batched", "exblas_set_getrs_batched_path",
    "exblas_last_getrs_batched_info",
    "exblas_exsum_lp_dev", "exblas_exdot_lp_dev", "exblas_exsum_lp_accumulate_dev", "exblas_exdot_lp_accumulate_dev",
    "exblas_exsum_lp_ctx", "exblas_exdot_lp_ctx", "exblas_exsum_lp_accumulate_ctx", "exblas_exdot_lp_accumulate_ctx",
    "exblas_round_records_dev", "exblas_round_records_ctx", "exblas_round_digits_host", "exblas_exsum_lp",
    "exblas_exdot_lp",
]

# element / target formats of the narrow entries (EXBLAS_DT_* of include/exblas_hip.h), keyed by the dtype's name so
# that torch and numpy dtypes resolve alike: (code, bytes per element)
DT_F64, DT_F32, DT_F16, DT_BF16 = 0, 1, 2, 3
_DT_BY_NAME = {"float64": (DT_F64, 8), "float32": (DT_F32, 4), "float16": (DT_F16, 2), "bfloat16": (DT_BF16, 2)}

# host-transport callback types of include/exblas_hip.h
HOST_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int64)
HOST_BCAST_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)
HOST_ALLGATHERV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64))
UNIQUE_ID_BYTES = 128
COMM_ERROR = -2

_lib = None


def load_library():
    """Load (building first if sources are newer) lib/libexblas.so.  Raises if it cannot be had."""
    global _lib, LIB_PATH
    if _lib is not None:
        return _lib
    alt = os.environ.get("EXBLAS_AMD_LIB")  # A/B of an alternative build (tools/): load exactly this file
    if alt:
        LIB_PATH = os.path.abspath(alt)
        _build.stale = lambda: False
    if not os.path.exists(LIB_PATH) or _build.stale():
        have_hipcc = bool(_build.hipcc()) and os.path.exists(_build.hipcc())
        if have_hipcc:
            # a failed rebuild is fatal: a library older than its sources must never be loaded in its place
            try:
                _build.build()
            except Exception as exc:  # noqa: BLE001
                raise ImportError(f"exblas_amd: building {LIB_PATH} failed ({exc}); refusing to load a stale "
                                  "library") from exc
        elif os.path.exists(LIB_PATH):
            raise ImportError(f"exblas_amd: {LIB_PATH} is older than its sources and hipcc is not available to "
                              "rebuild it")
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"exblas_amd: {LIB_PATH} is missing and hipcc is not available; "
                          "there is no CPU fallback")
    # PyTorch wheels bundle their own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one process do
    # not share devices, streams or pointers (and the second one to initialise finds no device), so when
    # torch is importable it must be loaded FIRST: libexblas.so's NEEDED libamdhip64.so.7 then resolves to
    # the runtime torch already mapped.  Stand-alone C/C++ users simply get /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i64, i32, dbl = C.c_void_p, C.c_int64, C.c_int, C.c_double
    L.exblas_hip_init.argtypes = [i32]
    L.exblas_hip_version.restype = C.c_char_p
    L.exblas_set_round_mode.argtypes = [i32]
    L.exblas_set_tuning.argtypes = [i32, i32, i32]
    L.exblas_set_accumulator_slot.argtypes = [i32]
    L.exblas_set_launch_events.argtypes = [vp, vp]
    L.exblas_set_gemm_path.argtypes = [i32]
    L.exblas_set_gemm_path.restype = None
    L.exblas_exsum_dev.argtypes = [vp, i64, i64, i32, i32, vp, vp]
    L.exblas_exdot_dev.argtypes = [vp, i64, vp, i64, i64, i32, i32, vp, vp]
    L.exblas_finalize_dev.argtypes = [vp, i32, C.c_uint32, vp, vp]
    L.exblas_exsum_accumulate_dev.argtypes = [vp, i64, i64, i32, i32, vp]
    L.exblas_exdot_accumulate_dev.argtypes = [vp, i64, vp, i64, i64, i32, i32, vp]
    L.exblas_finish_dev.argtypes = [vp, vp]
    L.exblas_exsum_segmented_dev.argtypes = [vp, vp, i64, i32, i32, vp, vp]
    L.exblas_exgemv_dev.argtypes = [C.c_char, i32, i32, dbl, vp, i32, vp, i32, dbl, vp, i32, i32, i32, vp]
    L.exblas_exgemm_dev.argtypes = [C.c_char, C.c_char, i32, i32, i32, dbl, vp, i32, vp, i32, dbl, vp, i32, i32,
                                    i32, vp]
    L.exblas_extrsv_dev.argtypes = [C.c_char, C.c_char, C.c_char, i32, vp, i32, vp, i32, i32, i32, vp]
    L.exblas_extrsv.argtypes = [C.c_char, C.c_char, C.c_char, i32, vp, i32, i32, vp, i32, i32, i32, i32]
    L.exblas_gen_dev.argtypes = [i32, C.c_uint64, i64, i64, i64, dbl, dbl, vp, vp]
    L.exblas_stream_read_dev.argtypes = [vp, i64, vp, vp]
    L.exblas_stream_read2_dev.argtypes = [vp, vp, i64, i32, vp, vp]
    L.exblas_exsum.restype = dbl
    L.exblas_exsum.argtypes = [i32, vp, i32, i32, i32, i32]
    L.exblas_exdot.restype = dbl
    L.exblas_exdot.argtypes = [i32, vp, i32, i32, vp, i32, i32, i32, i32]
    L.exblas_exgemv.argtypes = [C.c_char, i32, i32, dbl, vp, i32, i32, vp, i32, i32, dbl, vp, i32, i32, i32, i32]
    L.exblas_exgemm.argtypes = [C.c_char, C.c_char, i32, i32, i32, dbl, vp, i32, vp, i32, dbl, vp, i32, i32, i32]
    L.exblas_reserve_workspace.argtypes = [C.c_size_t]
    L.exblas_workspace_bytes.restype = C.c_size_t
    L.exblas_ctx_create.argtypes = [C.POINTER(vp)]
    L.exblas_ctx_destroy.argtypes = [vp]
    L.exblas_exsum_ctx.argtypes = [vp] + L.exblas_exsum_dev.argtypes
    L.exblas_exdot_ctx.argtypes = [vp] + L.exblas_exdot_dev.argtypes
    L.exblas_exsum_accumulate_ctx.argtypes = [vp] + L.exblas_exsum_accumulate_dev.argtypes
    L.exblas_exdot_accumulate_ctx.argtypes = [vp] + L.exblas_exdot_accumulate_dev.argtypes
    L.exblas_finish_ctx.argtypes = [vp] + L.exblas_finish_dev.argtypes
    L.exblas_exgemv_ctx.argtypes = [vp] + L.exblas_exgemv_dev.argtypes
    L.exblas_extrsv_ctx.argtypes = [vp] + L.exblas_extrsv_dev.argtypes
    L.exblas_exgemm_ctx.argtypes = [vp] + L.exblas_exgemm_dev.argtypes
    L.exblas_reserve_workspace_ctx.argtypes = [vp, C.c_size_t]
    L.exblas_workspace_bytes_ctx.argtypes = [vp]
    L.exblas_workspace_bytes_ctx.restype = C.c_size_t
    L.exblas_last_gemm_info_ctx.argtypes = [vp, C.POINTER(C.c_int)]
    L.exblas_set_host_devices.argtypes = [i32, C.POINTER(C.c_int)]
    L.exblas_last_gemm_info.argtypes = [C.POINTER(C.c_int)]
    L.exblas_last_blas1_info.argtypes = [C.POINTER(C.c_int)]
    L.exblas_set_gemm_max_slices.argtypes = [i32]
    L.exblas_set_gemm_max_slices.restype = None
    L.exblas_set_gemm_max_moduli.argtypes = [i32]
    L.exblas_set_gemm_max_moduli.restype = None
    L.exblas_crt_selftest.argtypes = [i32, C.c_uint]
    L.exblas_crt_selftest.restype = i32
    L.exblas_comm_unique_id.argtypes = [vp]
    L.exblas_comm_init_rccl.argtypes = [C.POINTER(vp), i32, i32, vp]
    L.exblas_comm_adopt_rccl.argtypes = [C.POINTER(vp), vp, i32, i32]
    L.exblas_comm_init_host.argtypes = [C.POINTER(vp), i32, i32, HOST_ALLREDUCE_FN, HOST_BCAST_FN, HOST_ALLGATHERV_FN,
                                        vp]
    L.exblas_comm_destroy.argtypes = [vp]
    L.exblas_comm_rank.argtypes = [vp]
    L.exblas_comm_size.argtypes = [vp]
    L.exblas_shard_range.argtypes = [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)]
    L.exblas_shard_range.restype = None
    L.exblas_exsum_allreduce_dev.argtypes = [vp, vp, i64, i64, i32, i32, vp, vp]
    L.exblas_exdot_allreduce_dev.argtypes = [vp, vp, i64, vp, i64, i64, i32, i32, vp, vp]
    L.exblas_allreduce_finish_dev.argtypes = [vp, vp, vp]
    L.exblas_exsum_allreduce_pipelined_dev.argtypes = [vp, vp, i64, i64, i32, i32, vp, vp, vp, vp]
    L.exblas_exdot_allreduce_pipelined_dev.argtypes = [vp, vp, i64, vp, i64, i64, i32, i32, vp, vp, vp, vp]
    L.exblas_pipeline_drain_dev.argtypes = [vp, vp]
    L.exblas_exgemv_sharded_dev.argtypes = [vp, C.c_char, i32, i32, dbl, vp, i32, vp, i32, i32, dbl, vp, i32, i32, i32,
                                            i32, vp]
    L.exblas_exgemm_sharded_dev.argtypes = [vp, C.c_char, C.c_char, i32, i32, i32, dbl, vp, i32, vp, i32, i32, dbl,
                                            vp, i32, i32, i32, i32, vp]
    L.exblas_exspmv_csr_dev.argtypes = [i32, i32, i32, vp, vp, vp, dbl, vp, dbl, vp, i32, i32, vp]
    L.exblas_exspmv_csr_ctx.argtypes = [vp] + L.exblas_exspmv_csr_dev.argtypes
    L.exblas_exspmv_csr.argtypes = [i32, i32, i32, vp, vp, vp, dbl, vp, dbl, vp, i32, i32]
    L.exblas_set_spmv_path.argtypes = [i32]
    L.exblas_set_spmv_path.restype = None
    L.exblas_last_spmv_info.argtypes = [C.POINTER(i64)]
    L.exblas_exspmm_csr_dev.argtypes = [i32, i32, i32, i32, vp, vp, vp, dbl, vp, i64, dbl, vp, i64, i32, i32, vp]
    L.exblas_exspmm_csr_ctx.argtypes = [vp] + L.exblas_exspmm_csr_dev.argtypes
    L.exblas_exspmm_csr.argtypes = [i32, i32, i32, i32, vp, vp, vp, dbl, vp, i64, dbl, vp, i64, i32, i32]
    L.exblas_set_spmm_path.argtypes = [i32]
    L.exblas_set_spmm_path.restype = None
    L.exblas_last_spmm_info.argtypes = [C.POINTER(i64)]
    L.exblas_exspmv_csr_lp_dev.argtypes = [i32, i32, i32, vp, vp, i32, vp, dbl, i32, vp, dbl, vp, i32, i32, vp]
    L.exblas_exspmv_csr_lp_ctx.argtypes = [vp] + L.exblas_exspmv_csr_lp_dev.argtypes
    L.exblas_exspmv_csr_lp.argtypes = L.exblas_exspmv_csr_lp_dev.argtypes[:-1]
    L.exblas_exspmm_csr_lp_dev.argtypes = [i32, i32, i32, i32, vp, vp, i32, vp, dbl, i32, vp, i64, dbl, vp, i64, i32, i32, vp]
    L.exblas_exspmm_csr_lp_ctx.argtypes = [vp] + L.exblas_exspmm_csr_lp_dev.argtypes
    L.exblas_exspmm_csr_lp.argtypes = L.exblas_exspmm_csr_lp_dev.argtypes[:-1]
    L.exblas_round_interval_host.argtypes = [dbl, dbl, i32, C.POINTER(C.c_uint64)]
    L.exblas_round_window_host.argtypes = [vp, i32, C.POINTER(C.c_uint64)]
    L.exblas_exsptrsv_csr_dev.argtypes = [C.c_char, C.c_char, i32, i32, vp, vp, vp, vp, i32, i32, vp]
    L.exblas_exsptrsv_csr_ctx.argtypes = [vp] + L.exblas_exsptrsv_csr_dev.argtypes
    L.exblas_exsptrsv_csr.argtypes = [C.c_char, C.c_char, i32, i32, vp, vp, vp, vp, i32, i32]
    L.exblas_set_sptrsv_path.argtypes = [i32]
    L.exblas_set_sptrsv_path.restype = None
    L.exblas_last_sptrsv_info.argtypes = [C.POINTER(i64)]
    L.exblas_exspilu0_csr_dev.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, i32, vp]
    L.exblas_exspilu0_csr_ctx.argtypes = [vp] + L.exblas_exspilu0_csr_dev.argtypes
    L.exblas_exspilu0_csr.argtypes = [i32, i32, vp, vp, vp, vp, vp, i32, i32]
    L.exblas_set_spilu0_path.argtypes = [i32]
    L.exblas_set_spilu0_path.restype = None
    L.exblas_last_spilu0_info.argtypes = [C.POINTER(i64)]
    L.exblas_exspic0_csr_dev.argtypes = L.exblas_exspilu0_csr_dev.argtypes
    L.exblas_exspic0_csr_ctx.argtypes = L.exblas_exspilu0_csr_ctx.argtypes
    L.exblas_exspic0_csr.argtypes = L.exblas_exspilu0_csr.argtypes
    L.exblas_set_spic0_path.argtypes = [i32]
    L.exblas_set_spic0_path.restype = None
    L.exblas_last_spic0_info.argtypes = [C.POINTER(i64)]
    L.exblas_exsptrsm_csr_dev.argtypes = [C.c_char, C.c_char, i32, i32, i32, vp, vp, vp, vp, i64, i32, i32, vp]
    L.exblas_exsptrsm_csr_ctx.argtypes = [vp] + L.exblas_exsptrsm_csr_dev.argtypes
    L.exblas_exsptrsm_csr.argtypes = [C.c_char, C.c_char, i32, i32, i32, vp, vp, vp, vp, i64, i32, i32]
    L.exblas_set_sptrsm_path.argtypes = [i32]
    L.exblas_set_sptrsm_path.restype = None
    L.exblas_last_sptrsm_info.argtypes = [C.POINTER(i64)]
    L.exblas_extrsm_dev.argtypes = [C.c_char, C.c_char, C.c_char, i32, i32, vp, i32, vp, i64, i32, i32, vp]
    L.exblas_extrsm_ctx.argtypes = [vp] + L.exblas_extrsm_dev.argtypes
    L.exblas_extrsm.argtypes = [C.c_char, C.c_char, C.c_char, i32, i32, vp, i32, vp, i64, i32, i32]
    L.exblas_set_trsm_path.argtypes = [i32]
    L.exblas_set_trsm_path.restype = None
    L.exblas_last_trsm_info.argtypes = [C.POINTER(i64)]
    L.exblas_exbdot_dev.argtypes = [C.c_char, i64, i32, i32, vp, i64, vp, i64, vp, i64, i32, i32, vp]
    L.exblas_exbdot_ctx.argtypes = [vp] + L.exblas_exbdot_dev.argtypes
    L.exblas_exbdot.argtypes = [C.c_char, i64, i32, i32, vp, i64, vp, i64, vp, i64, i32, i32]
    L.exblas_set_bdot_path.argtypes = [i32]
    L.exblas_set_bdot_path.restype = None
    L.exblas_exbdot_export_dev.argtypes = [C.c_char, i64, i32, i32, vp, i64, vp, i64, vp, i32, i32, vp]
    L.exblas_exbdot_export_ctx.argtypes = [vp] + L.exblas_exbdot_export_dev.argtypes
    L.exblas_exbdot_round_dev.argtypes = [C.c_char, i32, i32, vp, i32, vp, i64, vp]
    L.exblas_exbdot_round_ctx.argtypes = [vp] + L.exblas_exbdot_round_dev.argtypes
    L.exblas_exbdot_allreduce_dev.argtypes = [vp, C.c_char, i64, i32, i32, vp, i64, vp, i64, vp, i64, i32, i32, vp]
    L.exblas_exbgemm_dev.argtypes = [i64, i32, i32, dbl, vp, i64, vp, i64, dbl, vp, i64, i32, i32, vp]
    L.exblas_exbgemm_ctx.argtypes = [vp] + L.exblas_exbgemm_dev.argtypes
    L.exblas_exbgemm.argtypes = [i64, i32, i32, dbl, vp, i64, vp, i64, dbl, vp, i64, i32, i32]
    L.exblas_set_bgemm_path.argtypes = [i32]
    L.exblas_set_bgemm_path.restype = None
    L.exblas_last_bgemm_info.argtypes = [C.POINTER(i64)]
    L.exblas_exbtrsm_dev.argtypes = [C.c_char, C.c_char, C.c_char, i64, i32, dbl, vp, i32, vp, i64, i32, i32, vp]
    L.exblas_exbtrsm_ctx.argtypes = [vp] + L.exblas_exbtrsm_dev.argtypes
    L.exblas_exbtrsm.argtypes = [C.c_char, C.c_char, C.c_char, i64, i32, dbl, vp, i32, vp, i64, i32, i32]
    L.exblas_set_btrsm_path.argtypes = [i32]
    L.exblas_set_btrsm_path.restype = None
    L.exblas_last_btrsm_info.argtypes = [C.POINTER(i64)]
    L.exblas_expotrf_dev.argtypes = [C.c_char, i32, vp, i32, vp, i32, i32, vp]
    L.exblas_expotrf_ctx.argtypes = [vp] + L.exblas_expotrf_dev.argtypes
    L.exblas_expotrf.argtypes = [C.c_char, i32, vp, i32, C.POINTER(i32), i32, i32]
    L.exblas_set_potrf_path.argtypes = [i32]
    L.exblas_set_potrf_path.restype = None
    L.exblas_last_potrf_info.argtypes = [C.POINTER(i64)]
    L.exblas_expotrf_batched_dev.argtypes = [C.c_char, i32, i64, vp, i32, i64, vp, i32, i32, vp]
    L.exblas_expotrf_batched_ctx.argtypes = [vp] + L.exblas_expotrf_batched_dev.argtypes
    L.exblas_expotrf_batched.argtypes = [C.c_char, i32, i64, vp, i32, i64, vp, i32, i32]
    L.exblas_set_potrf_batched_path.argtypes = [i32]
    L.exblas_set_potrf_batched_path.restype = None
    L.exblas_last_potrf_batched_info.argtypes = [C.POINTER(i64)]
    L.exblas_expotrs_batched_dev.argtypes = [C.c_char, C.c_char, i32, i64, i32, vp, i32, i64, vp, i64, i32, i32, vp]
    L.exblas_expotrs_batched_ctx.argtypes = [vp] + L.exblas_expotrs_batched_dev.argtypes
    L.exblas_expotrs_batched.argtypes = [C.c_char, C.c_char, i32, i64, i32, vp, i32, i64, vp, i64, i32, i32]
    L.exblas_set_potrs_batched_path.argtypes = [i32]
    L.exblas_set_potrs_batched_path.restype = None
    L.exblas_last_potrs_batched_info.argtypes = [C.POINTER(i64)]
    L.exblas_exgetrf_batched_dev.argtypes = [C.c_char, i32, i64, vp, i32, i64, vp, vp, i32, i32, vp]
    L.exblas_exgetrf_batched_ctx.argtypes = [vp] + L.exblas_exgetrf_batched_dev.argtypes
    L.exblas_exgetrf_batched.argtypes = [C.c_char, i32, i64, vp, i32, i64, vp, vp, i32, i32]
    L.exblas_set_getrf_batched_path.argtypes = [i32]
    L.exblas_set_getrf_batched_path.restype = None
    L.exblas_last_getrf_batched_info.argtypes = [C.POINTER(i64)]
    L.exblas_exgetrs_batched_dev.argtypes = [C.c_char, i32, i64, i32, vp, i32, i64, vp, vp, i64, i32, i32, vp]
    L.exblas_exgetrs_batched_ctx.argtypes = [vp] + L.exblas_exgetrs_batched_dev.argtypes
    L.exblas_exgetrs_batched.argtypes = [C.c_char, i32, i64, i32, vp, i32, i64, vp, vp, i64, i32, i32]
    L.exblas_set_getrs_batched_path.argtypes = [i32]
    L.exblas_set_getrs_batched_path.restype = None
    L.exblas_last_getrs_batched_info.argtypes = [C.POINTER(i64)]
    L.exblas_exsum_lp_dev.argtypes = [i32, vp, i64, i64, i32, i32, vp, vp]
    L.exblas_exdot_lp_dev.argtypes = [i32, vp, i64, vp, i64, i64, i32, i32, vp, vp]
    L.exblas_exsum_lp_accumulate_dev.argtypes = [i32, vp, i64, i64, i32, i32, vp]
    L.exblas_exdot_lp_accumulate_dev.argtypes = [i32, vp, i64, vp, i64, i64, i32, i32, vp]
    L.exblas_exsum_lp_ctx.argtypes = [vp, i32, vp, i64, i64, i32, i32, vp, vp]
    L.exblas_exdot_lp_ctx.argtypes = [vp, i32, vp, i64, vp, i64, i64, i32, i32, vp, vp]
    L.exblas_exsum_lp_accumulate_ctx.argtypes = [vp, i32, vp, i64, i64, i32, i32, vp]
    L.exblas_exdot_lp_accumulate_ctx.argtypes = [vp, i32, vp, i64, vp, i64, i64, i32, i32, vp]
    L.exblas_round_records_dev.argtypes = [vp, i64, i64, i32, vp, vp]
    L.exblas_round_records_ctx.argtypes = [vp, vp, i64, i64, i32, vp, vp]
    L.exblas_round_digits_host.argtypes = [vp, i32, C.POINTER(C.c_uint64)]
    L.exblas_exsum_lp.argtypes = [i32, vp, i64, i64, i32, i32, vp]
    L.exblas_exdot_lp.argtypes = [i32, vp, i64, vp, i64, i64, i32, i32, vp]
    L.exblas_exsum_record.argtypes = [i32, vp, i32, i32, i32, i32, vp]
    L.exblas_exdot_record.argtypes = [i32, vp, i32, i32, vp, i32, i32, i32, i32, vp]
    _lib = L
    return L


def _torch():
    import torch
    return torch


def _require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise RuntimeError("exblas_amd: no HIP device visible; the MI355X path has no CPU fallback")
    return torch


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"exblas_amd: {what} failed with HIP error {rc}")


def _stream_ptr(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Record:
    """Decoded result record of one reduction (see include/exblas_hip.h)."""

    def __init__(self, words):
        w = np.asarray(words, dtype=np.int64)
        self.words = w
        self.exact = float(w[OUT_EXACT:OUT_EXACT + 1].view(np.float64)[0])
        self.refmode = float(w[OUT_REFMODE:OUT_REFMODE + 1].view(np.float64)[0])
        self.flags = int(w[OUT_FLAGS])
        self.canon = w[OUT_CANON:OUT_CANON + NCANON].copy()
        self.digits = w[OUT_DIGITS:OUT_DIGITS + NDIGITS].copy()

    def value(self, mode=None):
        if mode is None:
            mode = load_library().exblas_get_round_mode()
        return self.refmode if mode else self.exact


# ---------------------------------------------------------------------------------------------
# device-resident API (torch CUDA tensors): what bench.py and the multi-GPU path use
# ---------------------------------------------------------------------------------------------
def new_record_buffer():
    torch = _require_gpu()
    return torch.zeros(OUT_WORDS, dtype=torch.int64, device="cuda")


def set_launch_events(ev_start, ev_stop):
    """The next exsum / exdot accumulate call attaches these torch events (already recorded once, so that they own a
    handle; either may be None) to its streaming kernel's dispatch packet: kernel start / stop timestamps, no packets."""
    h = lambda e: C.c_void_p(e.cuda_event) if e is not None else None  # noqa: E731
    _check(load_library().exblas_set_launch_events(h(ev_start), h(ev_stop)), "set_launch_events")


def set_accumulator_slot(slot):
    """Select which of the context's two accumulator sets the next accumulate/finish calls use (pipelining)."""
    _check(load_library().exblas_set_accumulator_slot(int(slot)), "set_accumulator_slot")


def last_blas1_info():
    """(kernel, grid, group accumulators, compute units) of the last streaming ExSUM / ExDOT launch of the device's
    default context: kernel 1 fp64 ExSUM on k_blas1_stream, 2 on k_blas1_strided, 3 fp64 vector ExDOT (k_blas1_stream),
    4 fp64 strided ExDOT (k_blas1_strided), 5 narrow ExSUM, 6 narrow strided ExSUM, 7 narrow vector ExDOT, 8 narrow strided
    ExDOT, 0 before the first launch.
    Host state recorded at launch; does not synchronise."""
    v = (C.c_int * 8)()
    _check(load_library().exblas_last_blas1_info(v), "last_blas1_info")
    return tuple(int(x) for x in v[:4])


def exsum_segmented_dev(values, offsets, fpe=8, early_exit=True, out=None):
    """out[s] = exact sum of values[offsets[s]:offsets[s+1]] (CUDA float64 / int64 tensors), one launch."""
    torch = _require_gpu()
    assert values.is_cuda and values.dtype == torch.float64 and offsets.is_cuda and offsets.dtype == torch.int64
    nseg = offsets.numel() - 1
    if out is None:
        out = torch.empty(max(nseg, 0), dtype=torch.float64, device="cuda")
    _check(load_library().exblas_exsum_segmented_dev(C.c_void_p(values.data_ptr()), C.c_void_p(offsets.data_ptr()),
                                                     nseg, fpe, int(early_exit), _stream_ptr(torch),
                                                     C.c_void_p(out.data_ptr())), "exsum_segmented_dev")
    return out


def finalize_dev(digit_sets, flags_or=0, out=None):
    """Sum [nsets, 72] int64 digit sets (record words 48..119), carry-propagate once, round."""
    torch = _require_gpu()
    assert digit_sets.is_cuda and digit_sets.dtype == torch.int64 and digit_sets.is_contiguous()
    nsets = digit_sets.numel() // SET_WORDS
    if out is None:
        out = new_record_buffer()
    _check(load_library().exblas_finalize_dev(C.c_void_p(digit_sets.data_ptr()), nsets, flags_or, _stream_ptr(torch),
                                              C.c_void_p(out.data_ptr())), "finalize_dev")
    return out


def _csr_value_rule(who, xp, val, narrow):
    """The dtype rule of the CSR values: float64, or with `narrow` (the *_lp routines) any of the four dtypes."""
    if narrow:
        _dt(val.dtype, who)
    elif val.dtype != xp.float64:
        raise TypeError(f"{who}: values must be float64")


def _csr_rules(who, xp, crow, col, val, shape, square, narrow=False):
    """The rules the CSR arrays of routine `who` obey, whatever holds them (xp: torch or numpy); returns (m, n, index_bits)."""
    if len(shape) != 2:
        raise ValueError(f"{who}: A must be 2-D, got shape {tuple(shape)}")
    m, n = int(shape[0]), int(shape[1])
    if m < 0 or n < 0 or m > 0x7fffffff or n > 0x7fffffff:
        raise ValueError(f"{who}: unsupported shape {tuple(shape)}")
    if square and m != n:
        raise ValueError(f"{who}: A must be square, got shape ({m}, {n})")
    _csr_value_rule(who, xp, val, narrow)
    if crow.dtype not in (xp.int32, xp.int64) or col.dtype != crow.dtype:
        raise TypeError(f"{who}: row pointers and column indices must both be int32 or both int64")
    if crow.ndim != 1 or col.ndim != 1 or val.ndim != 1:
        raise ValueError(f"{who}: crow, col and val must be 1-D")
    if crow.shape[0] != m + 1:
        raise ValueError(f"{who}: crow has {crow.shape[0]} entries, expected m + 1 = {m + 1}")
    if col.shape[0] != val.shape[0]:
        raise ValueError(f"{who}: col and val differ in length")
    return m, n, (32 if crow.dtype == xp.int32 else 64)


def _csr_dev(who, A, square=False, narrow=False):
    """The CSR operand of the device routine `who`: a torch.sparse_csr_tensor or a (crow, col, val, shape) tuple of torch
    tensors.  Refuses what is wrong with it without needing a GPU; returns (crow, col, val, m, n, index_bits)."""
    torch = _torch()
    if isinstance(A, (tuple, list)):
        if len(A) != 4:
            raise ValueError(f"{who}: A must be a sparse CSR tensor or a (crow, col, val, shape) tuple")
        crow, col, val, shape = A
    else:
        if getattr(A, "layout", None) != torch.sparse_csr:
            raise TypeError(f"{who}: A must be a torch.sparse_csr_tensor or a (crow, col, val, shape) tuple")
        crow, col, val, shape = A.crow_indices(), A.col_indices(), A.values(), tuple(A.shape)
    for name, t in (("crow", crow), ("col", col), ("val", val)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{who}: {name} must be a torch tensor")
    m, n, bits = _csr_rules(who, torch, crow, col, val, shape, square, narrow)
    return crow.contiguous(), col.contiguous(), val.contiguous(), m, n, bits


def _dense_dev(who, name, t, ndim):
    """The type rules of the dense operand `name` of the device routine `who`."""
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch tensor")
    if t.dtype != torch.float64:
        raise TypeError(f"{who}: {name} must be float64")
    if t.dim() != ndim:
        raise ValueError(f"{who}: {name} must be {ndim}-D")


def _on_gpu(who, **tensors):
    """The tensors of a device call lie on one device (refused without needing a GPU), and that device is a GPU."""
    if len({t.device for t in tensors.values()}) != 1:
        raise ValueError(f"{who}: {', '.join(tensors)} must be on one device")
    _require_gpu()
    if not all(t.is_cuda for t in tensors.values()):
        raise ValueError(f"{who}: the tensors must be on the GPU")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


SPTRSV_STALLED = -3  # EXBLAS_SPTRSV_STALLED: the watchdog of an ExSpTRSV or ExSpTRSM call was raised


def _check_sparse(rc, what):
    """_check for the sparse routines: a solve whose watchdog was raised is an error of its own."""
    if rc == SPTRSV_STALLED:
        raise RuntimeError(f"exblas_amd: {what} stalled: a wave gave up waiting for a solved value")
    _check(rc, what)


def _last_info(routine):
    """The four counters of the last call of a sparse routine ("spmv", "spmm", "sptrsv", "sptrsm")."""
    out = (C.c_int64 * 4)()
    _check_sparse(getattr(load_library(), f"exblas_last_{routine}_info")(out), f"the last ex{routine}")
    return tuple(int(v) for v in out)


def _set_path(routine, mode):
    """The body of every set_*_path test hook: the routine's exblas_set_<routine>_path(mode)."""
    getattr(load_library(), f"exblas_set_{routine}_path")(int(mode))


def _spmv_args(A, x, y, alpha, beta, fpe, early_exit):
    """Validates a device ExSpMV call before anything is launched; returns (y, the C arguments up to the stream)."""
    crow, col, val, m, n, bits = _csr_dev("exspmv", A)
    _dense_dev("exspmv", "x", x, 1)
    if x.numel() < n:
        raise ValueError(f"exspmv: x has {x.numel()} entries, fewer than n = {n}")
    if y is not None:
        _dense_dev("exspmv", "y", y, 1)
        if y.numel() != m or not y.is_contiguous():
            raise ValueError(f"exspmv: y must be a contiguous vector of m = {m} entries")
    _on_gpu("exspmv", crow=crow, col=col, val=val, x=x, **({} if y is None else {"y": y}))
    x = x.contiguous()
    if y is None:
        y = _torch().zeros(m, dtype=x.dtype, device=x.device)
    return y, (m, n, bits, _ptr(crow), _ptr(col), _ptr(val), float(alpha), _ptr(x), float(beta), _ptr(y), int(fpe),
               int(bool(early_exit)))


EXBLAS_UNSUPPORTED = -1


def _lp_pair(who, val_dtype, vec_dtype, fpe):
    """The accepted type pairs of the narrow sparse products: values float32 / float16 / bfloat16 (or float64 with float64
    vectors), vectors float64 or of the values' type; fpe 0 or 2..8 (1: no plain narrow kernel).  Returns the two codes."""
    vcode, xcode = _dt(val_dtype, who)[0], _dt(vec_dtype, who)[0]
    if xcode != DT_F64 and xcode != vcode:
        raise TypeError(f"exblas_amd.{who}: the vectors must be float64 or of the values' type, not {vec_dtype} with "
                        f"{val_dtype} values")
    if vcode != DT_F64:
        if int(fpe) == 1:
            raise NotImplementedError(f"exblas_amd.{who}: fpe = 1 (the plain sums) has no narrow kernel "
                                      f"(EXBLAS_UNSUPPORTED)")
        if not 0 <= int(fpe) <= 8:
            raise ValueError(f"exblas_amd.{who}: fpe must be 0 or 2..8")
    return vcode, xcode


def _check_lp(rc, what):
    if rc == EXBLAS_UNSUPPORTED:
        raise NotImplementedError(f"exblas_amd: {what}: fpe = 1 has no narrow kernel (EXBLAS_UNSUPPORTED)")
    _check(rc, what)


def _dense_lp(who, name, t, ndim, dtype=None):
    """The type rules of a dense operand of a narrow device routine: a torch tensor of ndim dimensions (of `dtype`)."""
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: {name} must be a torch tensor")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{who}: {name} must be {dtype}, the type of the other dense operand")
    if t.dim() != ndim:
        raise ValueError(f"{who}: {name} must be {ndim}-D")


def _spmv_lp_args(A, x, y, alpha, beta, fpe, early_exit):
    """Validates a narrow device ExSpMV call before anything is launched; returns (y, the C arguments up to the stream)."""
    who = "exspmv_lp"
    crow, col, val, m, n, bits = _csr_dev(who, A, narrow=True)
    _dense_lp(who, "x", x, 1)
    vcode, xcode = _lp_pair(who, val.dtype, x.dtype, fpe)
    if x.numel() < n:
        raise ValueError(f"{who}: x has {x.numel()} entries, fewer than n = {n}")
    if y is not None:
        _dense_lp(who, "y", y, 1, x.dtype)
        if y.numel() != m or not y.is_contiguous():
            raise ValueError(f"{who}: y must be a contiguous vector of m = {m} entries")
    _on_gpu(who, crow=crow, col=col, val=val, x=x, **({} if y is None else {"y": y}))
    x = x.contiguous()
    if y is None:
        y = _torch().zeros(m, dtype=x.dtype, device=x.device)
    return y, (m, n, bits, _ptr(crow), _ptr(col), vcode, _ptr(val), float(alpha), xcode, _ptr(x), float(beta), _ptr(y),
               int(fpe), int(bool(early_exit)))


def set_spmv_path(mode):
    """Test hook: 0 automatic, 1 accumulator finish for every row, 2 in-register rounding wherever certified (no row
    split), 3 every row split at a small chunk.  Same bits on every path."""
    _set_path("spmv", mode)


def last_spmv_info():
    """(rows rounded in registers, rows rounded from their accumulator, rows split, chunks) of the last ExSpMV."""
    return _last_info("spmv")


def _solve_flags(who, uplo, diag):
    if not isinstance(uplo, str) or uplo not in ("L", "l", "U", "u"):
        raise ValueError(f"{who}: uplo must be 'L' or 'U', got {uplo!r}")
    if not isinstance(diag, str) or diag not in ("N", "n", "U", "u"):
        raise ValueError(f"{who}: diag must be 'N' or 'U', got {diag!r}")
    return uplo.encode(), diag.encode()


def _sptrsv_args(A, x, uplo, diag, fpe, early_exit):
    """Validates a device ExSpTRSV call before anything is launched; returns the C arguments up to the stream."""
    crow, col, val, m, _, bits = _csr_dev("exsptrsv", A, square=True)
    u, d = _solve_flags("exsptrsv", uplo, diag)
    _dense_dev("exsptrsv", "x", x, 1)
    if x.numel() != m or not x.is_contiguous():
        raise ValueError(f"exsptrsv: x must be a contiguous vector of m = {m} entries (it is solved in place)")
    _on_gpu("exsptrsv", crow=crow, col=col, val=val, x=x)
    return (u, d, m, bits, _ptr(crow), _ptr(col), _ptr(val), _ptr(x), int(fpe), int(bool(early_exit)))


def set_sptrsv_path(mode):
    """Test hook: 0 automatic, 1 every row rounded from its integer accumulator, 2 every row in the one-row-per-wave
    form.  Same bits on every path."""
    _set_path("sptrsv", mode)


def last_sptrsv_info():
    """(rows rounded in registers, rows rounded from their accumulator, rows without a stored diagonal under 'N', stored
    entries skipped) of the last ExSpTRSV; raises when that call's watchdog was raised."""
    return _last_info("sptrsv")


def _factor_args(who, A, out, info, fpe, early_exit):
    """Validates a device ExSpILU0 / ExSpIC0 call (who: "exspilu0" / "exspic0") before anything is launched; returns
    (the factor, info, the C arguments up to the stream)."""
    torch = _torch()
    crow, col, val, m, _, bits = _csr_dev(who, A, square=True)
    given = {}
    if out is not None:
        _dense_dev(who, "out", out, 1)
        if out.numel() != val.numel() or not out.is_contiguous():
            raise ValueError(f"{who}: out must be a contiguous vector of nnz = {val.numel()} values")
        given["out"] = out
    if info is not None:
        if not isinstance(info, torch.Tensor) or info.dtype != torch.int64 or info.numel() != 2 or not info.is_contiguous():
            raise ValueError(f"{who}: info must be a contiguous int64 torch tensor of 2 words")
        given["info"] = info
    _on_gpu(who, crow=crow, col=col, val=val, **given)
    if out is None:
        out = torch.empty_like(val)
    if info is None:
        info = torch.zeros(2, dtype=torch.int64, device=val.device)
    return (crow, col, out, (m, m)), info, (m, bits, _ptr(crow), _ptr(col), _ptr(val), _ptr(out), _ptr(info), int(fpe),
                                            int(bool(early_exit)))


def set_spilu0_path(mode):
    """Test hook: 0 automatic, 1 every rounding through the wave's integer accumulator, 2 every row in the
    several-entries-per-lane form.  Same bits on every path."""
    _set_path("spilu0", mode)


def last_spilu0_info():
    """(entries rounded in registers, entries rounded from the accumulator, product terms summed, rows in the
    several-entries-per-lane form) of the last ExSpILU0; raises when that call's watchdog was raised."""
    return _last_info("spilu0")


def set_spic0_path(mode):
    """Test hook: 0 automatic, 1 every rounding through the wave's integer accumulator, 2 every row in the
    several-entries-per-lane form.  Same bits on every path."""
    _set_path("spic0", mode)


def last_spic0_info():
    """(entries on and below the diagonal rounded in registers, ... rounded from the accumulator, product terms summed,
    rows whose owned part is in the several-entries-per-lane form) of the last ExSpIC0; raises when that call's watchdog
    was raised."""
    return _last_info("spic0")


def _sptrsm_args(A, X, uplo, diag, fpe, early_exit):
    """Validates a device ExSpTRSM call before anything is launched; returns the C arguments up to the stream."""
    crow, col, val, m, _, bits = _csr_dev("exsptrsm", A, square=True)
    u, d = _solve_flags("exsptrsm", uplo, diag)
    if getattr(X, "ndim", 2) == 1:
        raise ValueError("exsptrsm: X must be a 2-D block of right-hand sides; for one vector use exsptrsv_dev")
    _dense_dev("exsptrsm", "X", X, 2)
    if X.shape[0] != m:
        raise ValueError(f"exsptrsm: X must have m = {m} rows")
    k = int(X.shape[1])
    # a block that does not conform is refused, not copied: it is solved in place
    if X.stride(1) != 1:
        raise ValueError("exsptrsm: X must be row-major with stride(1) == 1 (it is solved in place)")
    if X.stride(0) < k:
        raise ValueError(f"exsptrsm: the rows of X overlap: stride(0) = {X.stride(0)} < k = {k}")
    _on_gpu("exsptrsm", crow=crow, col=col, val=val, X=X)
    return (u, d, m, k, bits, _ptr(crow), _ptr(col), _ptr(val), _ptr(X), int(X.stride(0)), int(fpe), int(bool(early_exit)))


def set_sptrsm_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 one row per work item, 3 column
    panels and tiles of 4 columns.  Same bits on every path."""
    _set_path("sptrsm", mode)


def last_sptrsm_info():
    """(outputs rounded in registers, outputs rounded from the accumulator, rows without a stored diagonal under 'N',
    stored entries skipped) of the last ExSpTRSM; raises when that call's watchdog was raised."""
    return _last_info("sptrsm")


def _trsm_layout(A, uplo, trans, who="extrsm"):
    """How ExTRSM reads the 2-D operand A (anything with shape and stride(i), strides in elements) without copying it:
    returns (uplo, trans, lda) for the C call, which takes column-major storage.  `uplo` names the triangle of A[i, j] as
    Python indexes it.  stride(0) == 1 is column-major, lda = stride(1); stride(1) == 1 is row-major, the column-major
    storage of A^T: the other triangle, the other trans, lda = stride(0).  `who` names the routine in the messages
    (ExBTRSM reads its triangle the same way)."""
    if not isinstance(uplo, str) or uplo not in ("L", "l", "U", "u"):
        raise ValueError(f"{who}: uplo must be 'L' or 'U', got {uplo!r}")
    if not isinstance(trans, str) or trans not in ("N", "n", "T", "t"):
        raise ValueError(f"{who}: trans must be 'N' or 'T', got {trans!r}")
    uplo, trans = uplo.upper(), trans.upper()
    n = int(A.shape[0])
    s0, s1 = int(A.stride(0)), int(A.stride(1))
    if n <= 1:                                  # nothing, or one entry: any strides do
        return uplo, trans, 1
    if s0 == 1 and s1 >= n:
        return uplo, trans, s1
    if s1 == 1 and s0 >= n:
        return ("U" if uplo == "L" else "L"), ("T" if trans == "N" else "N"), s0
    raise ValueError(f"{who}: A must have one unit stride and the other >= n = {n} (it is not copied), got strides "
                     f"({s0}, {s1})")


def _fpe_0_to_8(who, fpe):
    """fpe of the routines that refuse what they have no variant for (ExTRSM, ExBTRSM, ExPOTRF)."""
    fpe = int(fpe)
    if fpe < 0 or fpe >= 9:
        raise ValueError(f"{who}: fpe must be 0 (accumulators only), 1 (plain fp64) or 2..8, got {fpe}")
    return fpe


def _trsm_args(A, X, uplo, trans, diag, fpe, early_exit):
    """Validates a device ExTRSM call before anything is launched; returns the C arguments up to the stream."""
    _dense_dev("extrsm", "A", A, 2)
    n = int(A.shape[0])
    if A.shape[1] != n:
        raise ValueError(f"extrsm: A must be square, got shape {tuple(A.shape)}")
    if n > 0x7fffffff:
        raise ValueError(f"extrsm: unsupported shape {tuple(A.shape)}")
    u, t, lda = _trsm_layout(A, uplo, trans)
    _, d = _solve_flags("extrsm", "L", diag)
    if getattr(X, "ndim", 2) == 1:
        raise ValueError("extrsm: X must be a 2-D block of right-hand sides; for one vector use extrsv_dev")
    _dense_dev("extrsm", "X", X, 2)
    if X.shape[0] != n:
        raise ValueError(f"extrsm: X must have n = {n} rows")
    k = int(X.shape[1])
    # a block that does not conform is refused, not copied: it is solved in place
    if X.stride(1) != 1:
        raise ValueError("extrsm: X must be row-major with stride(1) == 1 (it is solved in place)")
    if X.stride(0) < k:
        raise ValueError(f"extrsm: the rows of X overlap: stride(0) = {X.stride(0)} < k = {k}")
    fpe = _fpe_0_to_8("extrsm", fpe)
    _on_gpu("extrsm", A=A, X=X)
    return (u.encode(), t.encode(), d, n, k, _ptr(A), lda, _ptr(X), max(int(X.stride(0)), 1), fpe, int(bool(early_exit)))


def set_trsm_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 one row per work item, 3 column
    panels and tiles of 4 columns.  Same bits on every path."""
    _set_path("trsm", mode)


def last_trsm_info():
    """(outputs rounded in registers, outputs rounded from the accumulator, 0, 0) of the last ExTRSM; raises when that
    call's watchdog was raised."""
    return _last_info("trsm")


def _ld(t, k):
    """Leading dimension of a row-major 2-D tensor with unit column stride (a single row: k)."""
    return max(int(t.stride(0)), k) if t.shape[0] > 1 else k


def _spmm_args(A, X, Y, alpha, beta, fpe, early_exit):
    """Validates a device ExSpMM call before anything is launched; returns (Y, the C arguments up to the stream)."""
    crow, col, val, m, n, bits = _csr_dev("exspmm", A)
    if getattr(X, "ndim", 2) == 1:
        raise ValueError("exspmm: X must be 2-D (n x k); for one vector use exspmv_dev")
    _dense_dev("exspmm", "X", X, 2)
    if X.shape[0] < n:
        raise ValueError(f"exspmm: X has {X.shape[0]} rows, fewer than n = {n}")
    k = int(X.shape[1])
    if Y is not None:
        torch = _torch()
        if not isinstance(Y, torch.Tensor) or Y.dtype != torch.float64 or Y.dim() != 2 or tuple(Y.shape) != (m, k):
            raise ValueError(f"exspmm: Y must be a 2-D float64 tensor of shape ({m}, {k})")
        if m > 0 and k > 0 and (Y.stride(1) != 1 or (m > 1 and Y.stride(0) < k)):
            raise ValueError("exspmm: Y is updated in place: it needs stride(1) == 1 and stride(0) >= k")
    _on_gpu("exspmm", crow=crow, col=col, val=val, X=X, **({} if Y is None else {"Y": Y}))
    if k > 0 and X.shape[0] > 0 and (X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < k)):
        X = X.contiguous()
    if Y is None:
        Y = _torch().zeros((m, k), dtype=X.dtype, device=X.device)
    return Y, (m, n, k, bits, _ptr(crow), _ptr(col), _ptr(val), float(alpha), _ptr(X), _ld(X, k), float(beta), _ptr(Y),
               _ld(Y, k), int(fpe), int(bool(early_exit)))


def _spmm_lp_args(A, X, Y, alpha, beta, fpe, early_exit):
    """Validates a narrow device ExSpMM call before anything is launched; returns (Y, the C arguments up to the stream)."""
    who = "exspmm_lp"
    crow, col, val, m, n, bits = _csr_dev(who, A, narrow=True)
    if getattr(X, "ndim", 2) == 1:
        raise ValueError(f"{who}: X must be 2-D (n x k); for one vector use exspmv_lp_dev")
    _dense_lp(who, "X", X, 2)
    vcode, xcode = _lp_pair(who, val.dtype, X.dtype, fpe)
    if X.shape[0] < n:
        raise ValueError(f"{who}: X has {X.shape[0]} rows, fewer than n = {n}")
    k = int(X.shape[1])
    if Y is not None:
        _dense_lp(who, "Y", Y, 2, X.dtype)
        if tuple(Y.shape) != (m, k):
            raise ValueError(f"{who}: Y must have shape ({m}, {k})")
        if m > 0 and k > 0 and (Y.stride(1) != 1 or (m > 1 and Y.stride(0) < k)):
            raise ValueError(f"{who}: Y is updated in place: it needs stride(1) == 1 and stride(0) >= k")
    _on_gpu(who, crow=crow, col=col, val=val, X=X, **({} if Y is None else {"Y": Y}))
    if k > 0 and X.shape[0] > 0 and (X.stride(1) != 1 or (X.shape[0] > 1 and X.stride(0) < k)):
        X = X.contiguous()
    if Y is None:
        Y = _torch().zeros((m, k), dtype=X.dtype, device=X.device)
    return Y, (m, n, k, bits, _ptr(crow), _ptr(col), vcode, _ptr(val), float(alpha), xcode, _ptr(X), _ld(X, k),
               float(beta), _ptr(Y), _ld(Y, k), int(fpe), int(bool(early_exit)))


def set_spmm_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from an integer accumulator, 2 in-register rounding wherever
    certified (no row split), 3 every row split at a small chunk.  Same bits on every path."""
    _set_path("spmm", mode)


def last_spmm_info():
    """(outputs rounded in registers, outputs rounded from an accumulator, rows split, chunks) of the last ExSpMM."""
    return _last_info("spmm")


def _bdot_mode(mode):
    if not isinstance(mode, str) or mode not in ("G", "g", "D", "d"):
        raise ValueError(f"exbdot: mode must be 'G' (Gram) or 'D' (diagonal), not {mode!r}")
    return mode.upper()


def _bdot_sizes(mode, n, p, q, fpe):
    if mode == "D" and p != q:
        raise ValueError(f"exbdot: mode 'D' needs as many columns in X as in Y, not {p} and {q}")
    if n > 0x7fffffff:
        raise ValueError(f"exbdot: n = {n} rows exceed INT_MAX")
    if int(fpe) < 0:
        raise ValueError("exbdot: fpe must be >= 0")


def _bdot_blocks(X, Y, mode, fpe):
    """The rules of the two blocks of a device ExBDOT call; returns (X, Y, mode, n, p, q)."""
    mode = _bdot_mode(mode)
    if getattr(X, "ndim", 2) == 1:
        raise ValueError("exbdot: X must be 2-D (n x p); for two vectors use exdot_dev")
    if Y is None:
        Y = X
    for name, t in (("X", X), ("Y", Y)):
        _dense_dev("exbdot", name, t, 2)
        if t.shape[0] > 0 and ((t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
            raise ValueError(f"exbdot: {name} must be row-major with stride(1) == 1 and stride(0) >= its column count "
                             "(a block is never copied)")
    if X.shape[0] != Y.shape[0]:
        raise ValueError(f"exbdot: X has {X.shape[0]} rows and Y has {Y.shape[0]}")
    n, p, q = int(X.shape[0]), int(X.shape[1]), int(Y.shape[1])
    _bdot_sizes(mode, n, p, q, fpe)
    return X, Y, mode, n, p, q


def _bdot_out(mode, p, q, out, device, **others):
    """The rules of C (checked, or allocated on `device` when None) once `others` lie on the GPU; returns (out, ldc)."""
    torch = _torch()
    shape = (p, q) if mode == "G" else (p,)
    if out is not None:
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or tuple(out.shape) != shape:
            raise ValueError(f"exbdot: out must be a float64 tensor of shape {shape}")
        if mode == "G" and p > 0 and ((q > 1 and out.stride(1) != 1) or (p > 1 and out.stride(0) < q)):
            raise ValueError("exbdot: out needs stride(1) == 1 and stride(0) >= q")
        if mode == "D" and p > 1 and out.stride(0) != 1:
            raise ValueError("exbdot: out must be contiguous in mode 'D'")
    _on_gpu("exbdot", **others, **({} if out is None else {"out": out}))
    if out is None:
        out = torch.empty(shape, dtype=torch.float64, device=device)
    return out, (_ld(out, q) if mode == "G" else 1)


def _bdot_args(X, Y, mode, out, fpe, early_exit):
    """Validates a device ExBDOT call before anything is launched; returns (out, the C arguments up to the stream)."""
    X, Y, mode, n, p, q = _bdot_blocks(X, Y, mode, fpe)
    out, ldc = _bdot_out(mode, p, q, out, X.device, X=X, Y=Y)
    return out, (mode.encode(), n, p, q, _ptr(X), _ld(X, p), _ptr(Y), _ld(Y, q), _ptr(out), ldc, int(fpe),
                 int(bool(early_exit)))


def _bdot_sets(sets, outputs, stacked):
    """`sets`: a contiguous int64 tensor [outputs, SET_WORDS], or, where `stacked`, also [nsets >= 1, outputs, SET_WORDS]"""
    torch = _torch()
    if not isinstance(sets, torch.Tensor):
        raise TypeError("exbdot: sets must be a torch tensor")
    if sets.dtype != torch.int64:
        raise TypeError("exbdot: sets must be int64")
    one = (outputs, SET_WORDS)
    if tuple(sets.shape) != one and not (stacked and sets.dim() == 3 and sets.shape[0] >= 1 and tuple(sets.shape[1:]) == one):
        raise ValueError(f"exbdot: sets must have shape {one}" + (f" or (nsets >= 1, {outputs}, {SET_WORDS})" if stacked else "")
                         + f", not {tuple(sets.shape)}")
    if not sets.is_contiguous():
        raise ValueError("exbdot: sets must be contiguous")


def _bdot_export_args(X, Y, mode, sets, fpe, early_exit):
    """Validates a device ExBDOT export before anything is launched; returns (sets, the C arguments up to the stream)."""
    X, Y, mode, n, p, q = _bdot_blocks(X, Y, mode, fpe)
    if int(fpe) == 1:
        raise ValueError("exbdot: fpe == 1 (plain fp64 sums) has no digit sets to export")
    if early_exit and int(fpe) > 8:
        raise ValueError("exbdot: early_exit with fpe > 8 computes nothing: there are no digit sets to export")
    outputs = p * q if mode == "G" else p
    if sets is not None:
        _bdot_sets(sets, outputs, False)
    _on_gpu("exbdot", X=X, Y=Y, **({} if sets is None else {"sets": sets}))
    if sets is None:
        sets = _torch().empty((outputs, SET_WORDS), dtype=_torch().int64, device=X.device)
    return sets, (mode.encode(), n, p, q, _ptr(X), _ld(X, p), _ptr(Y), _ld(Y, q), _ptr(sets), int(fpe),
                  int(bool(early_exit)))


def _bdot_round_args(sets, mode, p, q, out):
    """Validates a device ExBDOT round before anything is launched; returns (out, the C arguments up to the stream)."""
    mode = _bdot_mode(mode)
    p, q = int(p), int(q)
    if p < 0 or q < 0:
        raise ValueError("exbdot: p and q must be >= 0")
    _bdot_sizes(mode, 0, p, q, 0)
    _bdot_sets(sets, p * q if mode == "G" else p, True)
    nsets = int(sets.shape[0]) if sets.dim() == 3 else 1
    out, ldc = _bdot_out(mode, p, q, out, sets.device, sets=sets)
    return out, (mode.encode(), p, q, _ptr(sets), nsets, _ptr(out), ldc)


def set_bdot_path(mode):
    """Test hook: 0 automatic, 1 the smallest row slab per workgroup, 2 column panels and output tiles of width 4.
    Same bits on every path."""
    _set_path("bdot", mode)


def _bgemm_block(name, t, rows=None, cols=None):
    """The rules of one row-major block of a device ExBGEMM call (a block is never copied); returns (rows, cols)."""
    torch = _torch()
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
        raise ValueError(f"exbgemm: {name} must be a float64 torch tensor")
    if t.dim() != 2:
        raise ValueError(f"exbgemm: {name} must be 2-D")
    r, c = int(t.shape[0]), int(t.shape[1])
    if (rows is not None and r != rows) or (cols is not None and c != cols):
        want = ("n" if rows is None else str(rows), "q" if cols is None else str(cols))
        raise ValueError(f"exbgemm: {name} must have shape ({want[0]}, {want[1]}), not ({r}, {c})")
    if r > 0 and ((c > 1 and t.stride(1) != 1) or (r > 1 and t.stride(0) < c)):
        raise ValueError(f"exbgemm: {name} must be row-major with stride(1) == 1 and stride(0) >= its column count")
    return r, c


def _bgemm_overlap(a, b):
    """Whether two row-major blocks share an element.  Two views of one wider buffer (equal row strides) that take
    different columns of it do not; otherwise the byte spans decide."""
    spans = []
    for t in (a, b):
        r, c = int(t.shape[0]), int(t.shape[1])
        if r == 0 or c == 0:
            return False
        spans.append((t.data_ptr(), t.data_ptr() + 8 * ((r - 1) * _ld(t, c) + c)))
    if spans[0][0] >= spans[1][1] or spans[1][0] >= spans[0][1]:
        return False
    lda, ldb = _ld(a, int(a.shape[1])), _ld(b, int(b.shape[1]))
    if lda == ldb and (spans[1][0] - spans[0][0]) % 8 == 0:
        first = ((spans[1][0] - spans[0][0]) // 8) % lda     # the column of the shared buffer where b's rows start
        return not (first >= int(a.shape[1]) and first + int(b.shape[1]) <= lda)
    return True


def _bgemm_args(X, Cm, alpha, beta, Y, fpe, early_exit):
    """Validates a device ExBGEMM call before anything is launched; returns (Y, the C arguments up to the stream)."""
    n, p = _bgemm_block("X", X)
    _, q = _bgemm_block("C", Cm, rows=p)
    if n > 0x7fffffff:
        raise ValueError(f"exbgemm: n = {n} rows exceed INT_MAX")
    if int(fpe) < 0:
        raise ValueError("exbgemm: fpe must be >= 0")
    if Y is not None:
        _bgemm_block("Y", Y, rows=n, cols=q)
    tensors = {"X": X, "C": Cm, **({} if Y is None else {"Y": Y})}
    if len({t.device for t in tensors.values()}) != 1:
        raise ValueError(f"exbgemm: {', '.join(tensors)} must be on one device")
    if Y is not None:
        for name, t in (("X", X), ("C", Cm)):
            if _bgemm_overlap(t, Y):
                raise ValueError(f"exbgemm: Y overlaps {name} (Y is updated in place while {name} is read)")
    _on_gpu("exbgemm", **tensors)
    if Y is None:
        Y = _torch().zeros((n, q), dtype=X.dtype, device=X.device)
    return Y, (n, p, q, float(alpha), _ptr(X), _ld(X, p), _ptr(Cm), _ld(Cm, q), float(beta), _ptr(Y), _ld(Y, q), int(fpe),
               int(bool(early_exit)))


def set_bgemm_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 a register block of one row,
    3 column tiles of 4 and chunks of 4 rows of C.  Same bits on every path."""
    _set_path("bgemm", mode)


def last_bgemm_info():
    """(outputs rounded in registers, outputs rounded from the accumulator, 0, 0) of the last ExBGEMM."""
    return _last_info("bgemm")


BTRSM_MAX_P = 512  # EXBLAS_BTRSM_MAX_P: a wider triangle is refused


def _small_square(who, name, shape, stride_of, uplo, trans):
    """The rules of the small operand `name` of ExBTRSM and ExPOTRF, device or host: 2-D, square, at most BTRSM_MAX_P wide,
    one unit stride (_trsm_layout); returns (uplo, trans, p, ld) for the C call."""
    if len(shape) != 2:
        raise ValueError(f"{who}: {name} must be 2-D")
    p = int(shape[0])
    if shape[1] != p:
        raise ValueError(f"{who}: {name} must be square, got shape {tuple(shape)}")
    if p > BTRSM_MAX_P:
        raise ValueError(f"{who}: p = {p} exceeds EXBLAS_BTRSM_MAX_P = {BTRSM_MAX_P}")
    u, t, ld = _trsm_layout(stride_of, uplo, trans, who)
    return u.encode(), t.encode(), p, max(ld, 1)


def _btrsm_triangle(T, shape, stride_of, uplo, trans, diag):
    """The rules of the triangle of an ExBTRSM call, device or host; returns (uplo, trans, diag, p, ldt) for the C call."""
    u, t, p, ldt = _small_square("exbtrsm", "T", shape, stride_of, uplo, trans)
    _, d = _solve_flags("exbtrsm", "L", diag)
    return u, t, d, p, ldt


def _btrsm_args(T, X, uplo, trans, diag, alpha, fpe, early_exit):
    """Validates a device ExBTRSM call before anything is launched (no GPU needed for that); returns the C arguments up
    to the stream.  Neither operand is copied."""
    torch = _torch()
    for name, t in (("T", T), ("X", X)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError(f"exbtrsm: {name} must be a float64 torch tensor")
    if X.dim() != 2:
        raise ValueError("exbtrsm: X must be 2-D (n x p, one row per system)")
    u, t, d, p, ldt = _btrsm_triangle(T, tuple(T.shape), T, uplo, trans, diag)
    n = int(X.shape[0])
    if X.shape[1] != p:
        raise ValueError(f"exbtrsm: X must have p = {p} columns, not {int(X.shape[1])}")
    # a block that does not conform is refused, not copied: it is solved in place
    if n > 0 and ((p > 1 and X.stride(1) != 1) or (n > 1 and X.stride(0) < p)):
        raise ValueError("exbtrsm: X must be row-major with stride(1) == 1 and stride(0) >= p (its rows must not overlap; "
                         "it is solved in place)")
    fpe = _fpe_0_to_8("exbtrsm", fpe)
    if T.device != X.device:
        raise ValueError("exbtrsm: T, X must be on one device")
    if _bgemm_overlap(T, X) if T.stride(1) == 1 else _bgemm_overlap(T.t(), X):
        raise ValueError("exbtrsm: X overlaps T (X is solved in place while T is read)")
    _on_gpu("exbtrsm", T=T, X=X)
    return (u, t, d, n, p, float(alpha), _ptr(T), ldt, _ptr(X), _ld(X, max(p, 1)), fpe, int(bool(early_exit)))


def set_btrsm_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 a register block of one column,
    3 four rows per wave item and chunks of 4 x 4 of T.  Same bits on every path."""
    _set_path("btrsm", mode)


def last_btrsm_info():
    """(outputs rounded in registers, outputs rounded from the accumulator, 0, 0) of the last ExBTRSM."""
    return _last_info("btrsm")


def _potrf_triangle(shape, stride_of, uplo):
    """The rules of the matrix of an ExPOTRF call, device or host; returns (uplo, p, ldg) for the C call.  A row-major
    matrix is passed as the other triangle of its transpose."""
    u, _, p, ldg = _small_square("expotrf", "G", shape, stride_of, uplo, "N")
    return u, p, ldg


def _potrf_args(G, uplo, info, fpe, early_exit):
    """Validates a device ExPOTRF call before anything is launched (no GPU needed for that); returns (info, the C
    arguments up to the stream).  G is never copied; info is allocated when None."""
    torch = _torch()
    if not isinstance(G, torch.Tensor) or G.dtype != torch.float64:
        raise ValueError("expotrf: G must be a float64 torch tensor")
    u, p, ldg = _potrf_triangle(tuple(G.shape), G, uplo)
    fpe = _fpe_0_to_8("expotrf", fpe)
    if info is not None:
        if not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or info.numel() != 1:
            raise ValueError("expotrf: info must be a one-element int32 torch tensor")
        if info.device != G.device:
            raise ValueError("expotrf: G, info must be on one device")
    _on_gpu("expotrf", G=G)
    if info is None:
        info = torch.zeros(1, dtype=torch.int32, device=G.device)
    return info, (u, p, _ptr(G), ldg, _ptr(info), fpe, int(bool(early_exit)))


def set_potrf_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 a register block of one row,
    3 column tiles of 4 and no staging in LDS.  Same bits on every path."""
    _set_path("potrf", mode)


def last_potrf_info():
    """(outputs rounded in registers, outputs rounded from the accumulator, 0, 0) of the last ExPOTRF; their sum is the
    number of entries that call fixed."""
    return _last_info("potrf")


POTRF_BATCHED_MAX_P = 64  # EXBLAS_POTRF_BATCHED_MAX_P: a wider block is refused


class _Last2:
    """the last two dimensions of a 3-D operand (shape and element strides), as _trsm_layout reads them"""

    def __init__(self, shape, stride_of):
        self.shape = tuple(shape[1:])
        self._strides = (int(stride_of.stride(1)), int(stride_of.stride(2)))

    def stride(self, i):
        return self._strides[i]


def _batched_squares(who, name, shape, stride_of, uplo, max_p, max_name):
    """The rules of the 3-D operand `name` ([batch, p, p]) of the batched routines, device or host: every matrix has one
    unit stride among its last two dimensions (_trsm_layout: a row-major matrix is the other triangle of its transpose),
    stride(0) is the batch stride and the matrices do not overlap.  Returns (uplo as _trsm_layout flipped it, batch, p, ld,
    stride)."""
    if len(shape) != 3:
        raise ValueError(f"{who}: {name} must be 3-D [batch, p, p]")
    batch, p = int(shape[0]), int(shape[1])
    if shape[2] != p:
        raise ValueError(f"{who}: the matrices of {name} must be square, got shape {tuple(shape)}")
    if p > max_p:
        raise ValueError(f"{who}: p = {p} exceeds {max_name} = {max_p}")
    last2 = _Last2(shape, stride_of)
    if batch == 0:
        last2._strides = (p, 1)                     # no matrix: any strides do
    u, _, ld = _trsm_layout(last2, uplo, "N", who)
    ld = max(ld, 1)
    stride = int(stride_of.stride(0))
    if batch > 1 and stride < ld * p:
        raise ValueError(f"{who}: the matrices of {name} overlap: stride(0) = {stride} < {ld * p}")
    return u, batch, p, ld, (stride if batch > 1 else ld * max(p, 1))


def _batched_triangles(who, name, shape, stride_of, uplo):
    """_batched_squares for the Cholesky routines; returns (uplo, batch, p, ld, stride) for the C call."""
    u, *rest = _batched_squares(who, name, shape, stride_of, uplo, POTRF_BATCHED_MAX_P, "EXBLAS_POTRF_BATCHED_MAX_P")
    return (u.encode(), *rest)


def _batched_blocks(who, name, n, p, batch):
    """n rows in blocks of p need ceil(n / p) factors in the operand `name`"""
    if n > 0 and p < 1:
        raise ValueError(f"{who}: the blocks of {name} are empty (p = 0) but X has rows")
    want = -(-n // p) if p > 0 else 0
    if batch != want:
        raise ValueError(f"{who}: {name} holds {batch} blocks of p = {p}, X with n = {n} rows needs {want}")


def _batched_apply_args(who, name, F, X, factors, fpe):  # noqa: N803
    """What the device batched ExPOTRS and ExGETRS ask of their operands, in the order the checks are made: F (the operand
    `name`) and X are float64 tensors, X is 2-D; factors() then holds F (and what goes with it) to its own rules and
    returns a tuple that ends in (batch, p, ld, stride); X has a row per row of the blocks, is row-major and solved in
    place, lies on F's device and does not overlap F.  Returns (what factors() returned, n, k, fpe)."""
    torch = _torch()
    for nm, t in ((name, F), ("X", X)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64:
            raise ValueError(f"{who}: {nm} must be a float64 torch tensor")
    if X.dim() != 2:
        raise ValueError(f"{who}: X must be 2-D (n x k, one column per right-hand side)")
    geo = factors()
    batch, p, ld, stride = geo[-4:]
    n, k = int(X.shape[0]), int(X.shape[1])
    _batched_blocks(who, name, n, p, batch)
    # a block that does not conform is refused, not copied: it is solved in place
    if n > 0 and k > 0 and ((k > 1 and X.stride(1) != 1) or (n > 1 and X.stride(0) < k)):
        raise ValueError(f"{who}: X must be row-major with stride(1) == 1 and stride(0) >= k (its rows must not "
                         "overlap; it is solved in place)")
    fpe = _fpe_0_to_8(who, fpe)
    if F.device != X.device:
        raise ValueError(f"{who}: {name}, X must be on one device")
    if batch > 0 and n > 0 and k > 0:
        r0, x0 = F.data_ptr(), X.data_ptr()
        r1 = r0 + 8 * ((batch - 1) * stride + (p - 1) * ld + p)
        x1 = x0 + 8 * ((n - 1) * _ld(X, k) + k)
        if r0 < x1 and x0 < r1:
            raise ValueError(f"{who}: X overlaps {name} (X is solved in place while {name} is read)")
    _on_gpu(who, **{name: F, "X": X})
    return geo, n, k, fpe


def _potrf_batched_args(G, uplo, info, fpe, early_exit):
    """Validates a device batched ExPOTRF call before anything is launched (no GPU needed for that); returns (info, the
    C arguments up to the stream).  G is never copied; info is allocated when None."""
    torch = _torch()
    if not isinstance(G, torch.Tensor) or G.dtype != torch.float64:
        raise ValueError("expotrf_batched: G must be a float64 torch tensor")
    u, batch, p, ldg, stride = _batched_triangles("expotrf_batched", "G", tuple(G.shape), G, uplo)
    fpe = _fpe_0_to_8("expotrf_batched", fpe)
    if info is not None:
        if (not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or info.dim() != 1 or info.numel() != batch
                or (batch > 1 and info.stride(0) != 1)):
            raise ValueError(f"expotrf_batched: info must be a contiguous int32 torch tensor of batch = {batch} words")
        if info.device != G.device:
            raise ValueError("expotrf_batched: G, info must be on one device")
    _on_gpu("expotrf_batched", G=G)
    if info is None:
        info = torch.zeros(batch, dtype=torch.int32, device=G.device)
    return info, (u, p, batch, _ptr(G), ldg, stride, _ptr(info), fpe, int(bool(early_exit)))


def _potrs_sweep(sweep):
    """'1' (F^T Y = B), '2' (F Z = Y) or 'B' (both) of the batched ExPOTRS, as a C char"""
    s = str(sweep).upper() if isinstance(sweep, (str, int)) and not isinstance(sweep, bool) else None
    if s not in ("1", "2", "B"):
        raise ValueError(f"expotrs_batched: sweep must be '1', '2' or 'B', got {sweep!r}")
    return s.encode()


def _potrs_batched_args(R, X, uplo, sweep, fpe, early_exit):
    """Validates a device batched ExPOTRS call before anything is launched (no GPU needed for that); returns the C
    arguments up to the stream.  Neither operand is copied."""
    def factors():
        u, *geo = _batched_triangles("expotrs_batched", "R", tuple(R.shape), R, uplo)
        return (u, _potrs_sweep(sweep), *geo)

    (u, s, batch, p, ldr, stride), n, k, fpe = _batched_apply_args("expotrs_batched", "R", R, X, factors, fpe)
    return (u, s, p, n, k, _ptr(R), ldr, stride, _ptr(X), _ld(X, max(k, 1)), fpe, int(bool(early_exit)))


def set_potrf_batched_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 one matrix per wave (no packing),
    3 one matrix per workgroup item on a handful of workgroups.  Same bits on every path."""
    _set_path("potrf_batched", mode)


def last_potrf_batched_info():
    """(entries rounded in registers, entries rounded from the accumulator, 0, 0) of the last batched ExPOTRF; their sum is
    the number of entries that call fixed over the whole batch."""
    return _last_info("potrf_batched")


def set_potrs_batched_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 one block per wave, 3 column tiles
    of 4.  Same bits on every path."""
    _set_path("potrs_batched", mode)


def last_potrs_batched_info():
    """(outputs rounded in registers, outputs rounded from the accumulator, 0, 0) of the last batched ExPOTRS; their sum is
    n * k per sweep."""
    return _last_info("potrs_batched")


GETRF_BATCHED_MAX_P = 64  # EXBLAS_GETRF_BATCHED_MAX_P: a wider block is refused


def _batched_matrices(who, name, shape, stride_of):
    """_batched_squares for the LU routines.  A general matrix has no other triangle to flip to: the unit stride picks the C
    routine's `order`, 'C' for stride(1) == 1 and 'R' for stride(2) == 1 ('U' comes back flipped for a row-major matrix).
    Returns (order, batch, p, ld, stride) for the C call."""
    u, *rest = _batched_squares(who, name, shape, stride_of, "U", GETRF_BATCHED_MAX_P, "EXBLAS_GETRF_BATCHED_MAX_P")
    return ((b"C" if u == "U" else b"R"), *rest)


def _getrf_batched_args(A, ipiv, info, fpe, early_exit):
    """Validates a device batched ExGETRF call before anything is launched (no GPU needed for that); returns (ipiv, info,
    the C arguments up to the stream).  A is never copied; ipiv and info are allocated when None."""
    torch = _torch()
    if not isinstance(A, torch.Tensor) or A.dtype != torch.float64:
        raise ValueError("exgetrf_batched: A must be a float64 torch tensor")
    order, batch, p, lda, stride = _batched_matrices("exgetrf_batched", "A", tuple(A.shape), A)
    fpe = _fpe_0_to_8("exgetrf_batched", fpe)
    if ipiv is not None:
        _getrf_pivots("exgetrf_batched", ipiv, batch, p, A)
    if info is not None:
        if (not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or info.dim() != 1 or info.numel() != batch
                or (batch > 1 and info.stride(0) != 1)):
            raise ValueError(f"exgetrf_batched: info must be a contiguous int32 torch tensor of batch = {batch} words")
        if info.device != A.device:
            raise ValueError("exgetrf_batched: A, info must be on one device")
    _on_gpu("exgetrf_batched", A=A)
    if ipiv is None:
        ipiv = torch.zeros((batch, p), dtype=torch.int32, device=A.device)
    if info is None:
        info = torch.zeros(batch, dtype=torch.int32, device=A.device)
    return ipiv, info, (order, p, batch, _ptr(A), lda, stride, _ptr(ipiv), _ptr(info), fpe, int(bool(early_exit)))


def _getrf_pivots(who, ipiv, batch, p, like):
    """ipiv of the batched LU routines: a contiguous int32 torch tensor [batch, p] on the device of `like`"""
    torch = _torch()
    if (not isinstance(ipiv, torch.Tensor) or ipiv.dtype != torch.int32 or tuple(ipiv.shape) != (batch, p)
            or not ipiv.is_contiguous()):
        raise ValueError(f"{who}: ipiv must be a contiguous int32 torch tensor of shape [batch, p] = [{batch}, {p}]")
    if ipiv.device != like.device:
        raise ValueError(f"{who}: ipiv must be on the device of the matrices")


def _getrs_batched_args(LU, ipiv, X, fpe, early_exit):
    """Validates a device batched ExGETRS call before anything is launched (no GPU needed for that); returns the C
    arguments up to the stream.  No operand is copied."""
    def factors():
        geo = _batched_matrices("exgetrs_batched", "LU", tuple(LU.shape), LU)
        _getrf_pivots("exgetrs_batched", ipiv, geo[1], geo[2], LU)
        return geo

    (order, _, p, ldlu, stride), n, k, fpe = _batched_apply_args("exgetrs_batched", "LU", LU, X, factors, fpe)
    return (order, p, n, k, _ptr(LU), ldlu, stride, _ptr(ipiv), _ptr(X), _ld(X, max(k, 1)), fpe, int(bool(early_exit)))


def set_getrf_batched_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 one matrix per wave (no packing),
    3 one matrix per workgroup item on a handful of workgroups.  Same bits on every path."""
    _set_path("getrf_batched", mode)


def last_getrf_batched_info():
    """(roundings done in registers, roundings done from the accumulator, 0, 0) of the last batched ExGETRF; their sum is
    p^2 per complete matrix, sum_{s<j} (2 (p - s) - 1) + (p - j) for a matrix that broke down at step j."""
    return _last_info("getrf_batched")


def set_getrs_batched_path(mode):
    """Test hook: 0 automatic, 1 every output rounded from the integer accumulator, 2 one block per wave, 3 column tiles
    of 4.  Same bits on every path."""
    _set_path("getrs_batched", mode)


def last_getrs_batched_info():
    """(outputs rounded in registers, outputs rounded from the accumulator, 0, 0) of the last batched ExGETRS; their sum is
    2 n k."""
    return _last_info("getrs_batched")


def csr_diag_blocks_dev(A, p):
    """The dense diagonal blocks of a square CSR operand (as for exspmv_dev: a torch.sparse_csr_tensor or a (crow, col, val,
    shape) tuple of torch tensors) as a float64 tensor [ceil(n / p), p, p] on A's device: block b holds A[b p : (b + 1) p,
    b p : (b + 1) p].  Entries outside the blocks are dropped, missing entries are zero, and the rows of the last block
    beyond n carry an identity diagonal.  A must store each (row, column) at most once (a second copy would overwrite the
    first instead of adding to it).  Plain torch indexing, no kernel of this library; works on CPU tensors too.  With it
    a block-Jacobi preconditioner is
        D = csr_diag_blocks_dev(A, p);  R, info = expotrf_batched_dev(D);  expotrs_batched_dev(R, X)."""
    torch = _torch()
    crow, col, val, n, _, _ = _csr_dev("csr_diag_blocks", A, square=True)
    p = int(p)
    if p < 1 or p > POTRF_BATCHED_MAX_P:
        raise ValueError(f"csr_diag_blocks: p must lie in 1 .. {POTRF_BATCHED_MAX_P}, got {p}")
    if len({crow.device, col.device, val.device}) != 1:
        raise ValueError("csr_diag_blocks: crow, col, val must be on one device")
    nb = -(-n // p)
    D = torch.zeros((nb, p, p), dtype=torch.float64, device=val.device)
    rows = torch.repeat_interleave(torch.arange(n, device=val.device, dtype=torch.int64), (crow[1:] - crow[:-1]).to(torch.int64))
    cols = col.to(torch.int64)
    keep = (rows // p == cols // p) & (cols >= 0) & (cols < n)
    rows, cols = rows[keep], cols[keep]
    D[rows // p, rows % p, cols % p] = val[keep]
    pad = torch.arange(n, nb * p, device=val.device, dtype=torch.int64)
    D[pad // p, pad % p, pad % p] = 1.0
    return D


def _dt(dtype, who):
    """(EXBLAS_DT_* code, bytes per element) of a torch / numpy dtype or its name; TypeError for any other"""
    name = str(dtype).rsplit(".", 1)[-1]
    try:
        name = np.dtype(dtype).name
    except TypeError:
        pass
    if name not in _DT_BY_NAME:
        raise TypeError(f"exblas_amd.{who}: dtype must be float64, float32, float16 or bfloat16, not {dtype}")
    return _DT_BY_NAME[name]


def _lp_operands(who, *tensors):
    """The checks of the narrow device forms, before any device call: one of the four dtypes (TypeError), the same for
    every operand (TypeError), CUDA tensors (ValueError).  Returns the EXBLAS_DT_* code."""
    code = _dt(tensors[0].dtype, who)[0]
    for t in tensors[1:]:
        if t.dtype != tensors[0].dtype:
            raise TypeError(f"exblas_amd.{who}: the operands have different dtypes ({tensors[0].dtype}, {t.dtype})")
    for t in tensors:
        if not getattr(t, "is_cuda", False):
            raise ValueError(f"exblas_amd.{who}: the device forms take CUDA tensors")
    return code


class Context:
    """Owner of an ``exblas_ctx_t *``: private accumulators, flags and workspace on the current device, so that work
    enqueued through different contexts (on different streams) needs no ordering.  Tensors are CUDA float64 / int64 on
    the context's device, calls go to the CURRENT torch stream.  Every routine with a handle form is implemented here,
    once; the module's ``*_dev`` functions are these methods bound to the context whose handle is None, the device's
    default context (``exblas_X_ctx(NULL, ...)`` is exactly ``exblas_X_dev(...)``)."""

    def __init__(self):
        _require_gpu()
        h = C.c_void_p()
        _check(load_library().exblas_ctx_create(C.byref(h)), "ctx_create")
        self.handle = h

    def destroy(self):
        if self.handle is not None:
            load_library().exblas_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:  # noqa: BLE001
            pass

    def exsum(self, x, fpe=8, early_exit=True, inca=1, n=None, out=None):
        """ExSUM of a CUDA float64 tensor, stream-ordered; returns the int64 record tensor (on device)."""
        torch = _require_gpu()
        assert x.is_cuda and x.dtype == torch.float64
        if n is None:
            n = (x.numel() + inca - 1) // inca
        if out is None:
            out = new_record_buffer()
        _check(load_library().exblas_exsum_ctx(self.handle, C.c_void_p(x.data_ptr()), n, inca, fpe, int(early_exit),
                                               _stream_ptr(torch), C.c_void_p(out.data_ptr())), "exsum")
        return out

    def exdot(self, x, y, fpe=8, early_exit=True, incx=1, incy=1, n=None, out=None):
        torch = _require_gpu()
        assert x.is_cuda and y.is_cuda and x.dtype == torch.float64 and y.dtype == torch.float64
        if n is None:
            n = (x.numel() + incx - 1) // incx
        if out is None:
            out = new_record_buffer()
        _check(load_library().exblas_exdot_ctx(self.handle, C.c_void_p(x.data_ptr()), incx, C.c_void_p(y.data_ptr()), incy,
                                               n, fpe, int(early_exit), _stream_ptr(torch), C.c_void_p(out.data_ptr())),
               "exdot")
        return out

    def exsum_accumulate(self, x, fpe=8, early_exit=True, inca=1, n=None):
        """Phase 1 only: stream x into the context accumulators (several calls fold into one exact sum)."""
        torch = _require_gpu()
        if n is None:
            n = (x.numel() + inca - 1) // inca
        _check(load_library().exblas_exsum_accumulate_ctx(self.handle, C.c_void_p(x.data_ptr()), n, inca, fpe,
                                                          int(early_exit), _stream_ptr(torch)), "exsum_accumulate")

    def exdot_accumulate(self, x, y, fpe=8, early_exit=True, incx=1, incy=1, n=None):
        torch = _require_gpu()
        if n is None:
            n = (x.numel() + incx - 1) // incx
        _check(load_library().exblas_exdot_accumulate_ctx(self.handle, C.c_void_p(x.data_ptr()), incx,
                                                          C.c_void_p(y.data_ptr()), incy, n, fpe, int(early_exit),
                                                          _stream_ptr(torch)), "exdot_accumulate")

    def finish(self, out=None):
        """Phase 2: carry-propagate + round the context accumulators into a record; zeroes them."""
        torch = _require_gpu()
        if out is None:
            out = new_record_buffer()
        _check(load_library().exblas_finish_ctx(self.handle, _stream_ptr(torch), C.c_void_p(out.data_ptr())), "finish")
        return out

    def exsum_lp_accumulate(self, x, fpe=8, early_exit=True, inca=1, n=None):
        """Phase 1 of exsum_lp: stream a float32 / float16 / bfloat16 (or float64) CUDA tensor into the context
        accumulators, read at its own width.  Folds with every other accumulate call, the fp64 ones included."""
        code = _lp_operands("exsum_lp_accumulate", x)
        torch = _require_gpu()
        if n is None:
            n = (x.numel() + inca - 1) // inca
        _check(load_library().exblas_exsum_lp_accumulate_ctx(self.handle, code, C.c_void_p(x.data_ptr()), n, inca, fpe,
                                                             int(early_exit), _stream_ptr(torch)), "exsum_lp_accumulate")

    def exdot_lp_accumulate(self, x, y, fpe=8, early_exit=True, incx=1, incy=1, n=None):
        code = _lp_operands("exdot_lp_accumulate", x, y)
        torch = _require_gpu()
        if n is None:
            n = (x.numel() + incx - 1) // incx
        _check(load_library().exblas_exdot_lp_accumulate_ctx(self.handle, code, C.c_void_p(x.data_ptr()), incx,
                                                             C.c_void_p(y.data_ptr()), incy, n, fpe, int(early_exit),
                                                             _stream_ptr(torch)), "exdot_lp_accumulate")

    def exsum_lp(self, x, fpe=8, early_exit=True, inca=1, n=None, out=None):
        """ExSUM of a float32 / float16 / bfloat16 (or float64) CUDA tensor, stream-ordered: the record of the exact sum
        of the widened values -- what exsum(x.double()) returns, without the temporary."""
        self.exsum_lp_accumulate(x, fpe, early_exit, inca, n)
        return self.finish(out)

    def exdot_lp(self, x, y, fpe=8, early_exit=True, incx=1, incy=1, n=None, out=None):
        self.exdot_lp_accumulate(x, y, fpe, early_exit, incx, incy, n)
        return self.finish(out)

    def round_records(self, records, dtype, out=None):
        """The exact totals of int64 records ([count, 128], or one record [128]) rounded ONCE into `dtype`: a tensor of
        that dtype, one element per record (0-d for one record).  Stream-ordered, capturable."""
        code = _dt(dtype, "round_records")[0]
        if not getattr(records, "is_cuda", False):
            raise ValueError("exblas_amd.round_records: the device forms take CUDA tensors")
        torch = _require_gpu()
        if records.dtype != torch.int64 or records.dim() not in (1, 2) or records.shape[-1] != OUT_WORDS \
                or records.stride(-1) != 1:
            raise ValueError("exblas_amd.round_records: records must be int64 [count, 128] or [128], rows contiguous")
        count = records.shape[0] if records.dim() == 2 else 1
        stride = records.stride(0) if records.dim() == 2 else OUT_WORDS
        tdt = getattr(torch, next(k for k, v in _DT_BY_NAME.items() if v[0] == code))
        if out is None:
            out = torch.empty((count,) if records.dim() == 2 else (), dtype=tdt, device=records.device)
        _check(load_library().exblas_round_records_ctx(self.handle, C.c_void_p(records.data_ptr()), count, stride, code,
                                                       C.c_void_p(out.data_ptr()), _stream_ptr(torch)), "round_records")
        return out

    def exsum_to(self, x, dtype=None, fpe=8, early_exit=True):
        """The exact sum of x rounded once into `dtype` (default: x's own): a 0-d tensor."""
        return self.round_records(self.exsum_lp(x, fpe, early_exit), x.dtype if dtype is None else dtype)

    def exdot_to(self, x, y, dtype=None, fpe=8, early_exit=True):
        """The exact dot product of x and y rounded once into `dtype` (default: the operands' own): a 0-d tensor."""
        return self.round_records(self.exdot_lp(x, y, fpe, early_exit), x.dtype if dtype is None else dtype)

    def exgemv(self, trans, m, n, alpha, a, lda, x, beta, y, fpe=0, early_exit=False, incx=1, incy=1):
        torch = _require_gpu()
        _check(load_library().exblas_exgemv_ctx(self.handle, trans.encode(), m, n, alpha, C.c_void_p(a.data_ptr()), lda,
                                                C.c_void_p(x.data_ptr()), incx, beta, C.c_void_p(y.data_ptr()), incy,
                                                fpe, int(early_exit), _stream_ptr(torch)), "exgemv")
        return y

    def extrsv(self, uplo, trans, diag, n, a, lda, x, fpe=0, early_exit=False, incx=1):
        """x := A^-1 x (or A^-T x) in place on device tensors; returns 0, or -1 for the unsupported fpe >= 9."""
        torch = _require_gpu()
        rc = load_library().exblas_extrsv_ctx(self.handle, uplo.encode(), trans.encode(), diag.encode(), n,
                                              C.c_void_p(a.data_ptr()), lda, C.c_void_p(x.data_ptr()), incx, fpe,
                                              int(early_exit), _stream_ptr(torch))
        if rc != -1:
            _check(rc, "extrsv")
        return rc

    def extrsm(self, A, X, uplo="L", trans="N", diag="N", fpe=8, early_exit=True):
        """ExTRSM: solves op(A) X = B in place on the n x k block X (B on entry) for k right-hand sides at once, exact and
        reproducible, stream-ordered on the current stream: column j is bit for bit what extrsv_dev gives on B[:, j], and
        the chain of n rounded divisions is walked once, not k times.  A: a 2-D float64 tensor with one unit stride, never
        copied -- column-major (stride(0) == 1) or row-major (stride(1) == 1); `uplo` names the triangle of A[i, j] as
        Python indexes it, the other triangle is never read.  X: a 2-D float64 tensor with stride(1) == 1 and
        stride(0) >= k (a view [:, :k] of a wider block is fine: its padding is not touched).  fpe: 0, 1 or 2..8.
        Returns X."""
        args = _trsm_args(A, X, uplo, trans, diag, fpe, early_exit)
        _check_sparse(load_library().exblas_extrsm_ctx(self.handle, *args, _stream_ptr(_torch())), "extrsm")
        return X

    def exgemm(self, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, fpe=0, early_exit=False):
        torch = _require_gpu()
        _check(load_library().exblas_exgemm_ctx(self.handle, transa.encode(), transb.encode(), m, n, k, alpha,
                                                C.c_void_p(a.data_ptr()), lda, C.c_void_p(b.data_ptr()), ldb, beta,
                                                C.c_void_p(c.data_ptr()), ldc, fpe, int(early_exit),
                                                _stream_ptr(torch)), "exgemm")
        return c

    def exspmv(self, A, x, alpha=1.0, beta=0.0, y=None, fpe=8, early_exit=True):
        """ExSpMV: y = Round(alpha A x + beta y) row by row, exact and reproducible, stream-ordered on the current stream.
        A: torch.sparse_csr_tensor (float64 values, int32 or int64 indices) or (crow, col, val, (m, n)) on the GPU; x a
        float64 vector of at least n entries; y (m entries) is updated in place, or allocated (zeros) when None."""
        y, args = _spmv_args(A, x, y, alpha, beta, fpe, early_exit)
        _check(load_library().exblas_exspmv_csr_ctx(self.handle, *args, _stream_ptr(_torch())), "exspmv")
        return y

    def exspmv_lp(self, A, x, alpha=1.0, beta=0.0, y=None, fpe=8, early_exit=True):
        """Narrow ExSpMV: A with float32 / float16 / bfloat16 values read at their own width, x and y float64 or of the
        values' type.  The exact sum of exspmv on the widened operands, rounded ONCE into the type of x: float64 results
        are bit for bit exspmv(A.double(), ...), narrow ones are rounded to nearest even straight from the exact sum
        (never the double cast afterwards).  y=None allocates zeros of x's type.  fpe 0 or 2..8."""
        y, args = _spmv_lp_args(A, x, y, alpha, beta, fpe, early_exit)
        _check_lp(load_library().exblas_exspmv_csr_lp_ctx(self.handle, *args, _stream_ptr(_torch())), "exspmv_lp")
        return y

    def exspmm_lp(self, A, X, alpha=1.0, beta=0.0, Y=None, fpe=8, early_exit=True):
        """Narrow ExSpMM: column j of Y is bit for bit exspmv_lp(A, X[:, j], alpha, beta, Y[:, j]).  A as for exspmv_lp; X
        and Y row-major blocks (stride(1) == 1) of float64 or of the values' type; the padding of Y is not written."""
        Y, args = _spmm_lp_args(A, X, Y, alpha, beta, fpe, early_exit)
        _check_lp(load_library().exblas_exspmm_csr_lp_ctx(self.handle, *args, _stream_ptr(_torch())), "exspmm_lp")
        return Y

    def exspmm(self, A, X, alpha=1.0, beta=0.0, Y=None, fpe=8, early_exit=True):
        """ExSpMM: Y = Round(alpha A X + beta Y) output by output, exact and reproducible, stream-ordered on the current
        stream; column j is bit for bit exspmv_dev(A, X[:, j], alpha, beta, Y[:, j]).  A as for exspmv_dev; X a 2-D float64
        tensor with at least n rows (row-major: a copy is made when X.stride(1) != 1, otherwise ldx = X.stride(0)); Y (m x k,
        stride(1) == 1, stride(0) >= k) is updated in place, or allocated (zeros) when None."""
        Y, args = _spmm_args(A, X, Y, alpha, beta, fpe, early_exit)
        _check(load_library().exblas_exspmm_csr_ctx(self.handle, *args, _stream_ptr(_torch())), "exspmm")
        return Y

    def exsptrsv(self, A, x, uplo="L", diag="N", fpe=8, early_exit=True):
        """ExSpTRSV: solves A x = b in place on x (b on entry), exact and reproducible, stream-ordered on the current stream:
        x_i = Round(b_i - sum of the stored val * x_j before the diagonal) / d_i in substitution order (diag 'U': no division),
        bit for bit what extrsv_dev gives on the densified matrix.  A: square torch.sparse_csr_tensor or (crow, col, val,
        (m, m)) on the GPU (float64 values, int32 or int64 indices); entries of the other triangle are skipped.  Returns x."""
        args = _sptrsv_args(A, x, uplo, diag, fpe, early_exit)
        _check(load_library().exblas_exsptrsv_csr_ctx(self.handle, *args, _stream_ptr(_torch())), "exsptrsv")
        return x

    def exspilu0(self, A, out=None, info=None, fpe=8, early_exit=True):
        """ExSpILU0: the exact-sum ILU(0) factor of the square CSR matrix A on its own pattern, reproducible bit for bit,
        stream-ordered on the current stream.  Rows in ascending order, for every stored (i, j):
        c_ij = Round(a_ij - sum_k l_ik u_kj) over the k < min(i, j) stored in row i and column j, the sum exact and rounded
        once; l_ij = c_ij / u_jj below the diagonal, u_ij = c_ij on and above it.  A as for exsptrsv_dev, with strictly
        ascending columns and a stored diagonal in every row.  `out` (float64, nnz values; may be A's own values tensor)
        and `info` (int64, 2 words) are allocated when None.  Returns (LU, info): LU = (crow, col, out, (m, m)) shares A's
        index tensors and holds L (unit diagonal, not stored) below and U on and above the diagonal; info[0] is 0 or r + 1
        for the first row with a structural defect (out is then untouched), info[1] 0 or r + 1 for the first zero or NaN
        pivot.  Apply it with exspilu0_apply_dev."""
        LU, info, args = _factor_args("exspilu0", A, out, info, fpe, early_exit)
        _check(load_library().exblas_exspilu0_csr_ctx(self.handle, *args, _stream_ptr(_torch())), "exspilu0")
        return LU, info

    def exspilu0_apply(self, LU, X, fpe=8, early_exit=True):  # noqa: N803
        """Applies the factor of exspilu0_dev in place: X := U^-1 L^-1 X, the unit lower sweep and then the upper one, through
        ExSpTRSV for a 1-D X and ExSpTRSM for a 2-D block (each column bit for bit what the vector form gives).  Returns X."""
        if getattr(X, "ndim", None) == 1:
            solve = self.exsptrsv
        elif getattr(X, "ndim", None) == 2:
            solve = self.exsptrsm
        else:
            _dense_dev("exspilu0_apply", "X", X, 1)
            raise ValueError("exspilu0_apply: X must be a vector or a 2-D block of right-hand sides")
        solve(LU, X, uplo="L", diag="U", fpe=fpe, early_exit=early_exit)
        return solve(LU, X, uplo="U", diag="N", fpe=fpe, early_exit=early_exit)

    def exspic0(self, A, out=None, info=None, fpe=8, early_exit=True):
        """ExSpIC0: the exact-sum IC(0) factor of the symmetric square CSR matrix A on its own pattern, reproducible bit for
        bit, stream-ordered on the current stream.  Rows in ascending order, for every stored (i, j) with j <= i:
        c_ij = Round(a_ij - sum_k l_ik l_jk) over the k < j stored in rows i and j, the sum exact and rounded once;
        l_ij = c_ij / l_jj below the diagonal, l_ii = sqrt(c_ii) on it.  A as for exsptrsv_dev, with strictly ascending
        columns, a stored diagonal in every row and a structurally symmetric pattern; values above the diagonal are never
        read.  `out` (float64, nnz values; may be A's own values tensor) and `info` (int64, 2 words) are allocated when
        None.  Returns (LL, info): LL = (crow, col, out, (m, m)) shares A's index tensors and holds L on and below the
        diagonal and its mirror L^T above it; info[0] is 0 or r + 1 for the first row with a structural defect (phase 1:
        ExSpILU0's defects; phase 2, when there is none: a stored (r, j) without (j, r); out is then untouched), info[1]
        0 or r + 1 for the first radicand that is not > 0 (the factorisation goes on in IEEE arithmetic).  Apply it with
        exspic0_apply_dev."""
        if int(fpe) < 0:
            raise ValueError(f"exspic0: fpe must be >= 0, got {fpe}")
        LL, info, args = _factor_args("exspic0", A, out, info, fpe, early_exit)
        _check(load_library().exblas_exspic0_csr_ctx(self.handle, *args, _stream_ptr(_torch())), "exspic0")
        return LL, info

    def exspic0_apply(self, LL, X, fpe=8, early_exit=True):  # noqa: N803
        """Applies the factor of exspic0_dev in place: X := L^-T L^-1 X, the lower sweep and then the upper one (the mirror
        L^T), through ExSpTRSV for a 1-D X and ExSpTRSM for a 2-D block (each column bit for bit what the vector form
        gives).  Returns X."""
        if getattr(X, "ndim", None) == 1:
            solve = self.exsptrsv
        elif getattr(X, "ndim", None) == 2:
            solve = self.exsptrsm
        else:
            _dense_dev("exspic0_apply", "X", X, 1)
            raise ValueError("exspic0_apply: X must be a vector or a 2-D block of right-hand sides")
        solve(LL, X, uplo="L", diag="N", fpe=fpe, early_exit=early_exit)
        return solve(LL, X, uplo="U", diag="N", fpe=fpe, early_exit=early_exit)

    def exsptrsm(self, A, X, uplo="L", diag="N", fpe=8, early_exit=True):
        """ExSpTRSM: solves A X = B in place on the m x k block X (B on entry) for k right-hand sides at once, exact and
        reproducible, stream-ordered on the current stream: column j is bit for bit what exsptrsv_dev gives on B[:, j], and
        the matrix is paid for once per row, not once per row and column.  A as for exsptrsv_dev; X a 2-D float64 tensor
        with stride(1) == 1 and stride(0) >= k (a view [:, :k] of a wider block is fine: its padding is not touched).
        Returns X."""
        args = _sptrsm_args(A, X, uplo, diag, fpe, early_exit)
        _check(load_library().exblas_exsptrsm_csr_ctx(self.handle, *args, _stream_ptr(_torch())), "exsptrsm")
        return X

    def exbdot(self, X, Y=None, mode="G", out=None, fpe=8, early_exit=True):
        """ExBDOT: exact, reproducible inner products of the columns of two row-major blocks, stream-ordered on the current
        stream, both blocks read once.  mode 'G': out[i, j] = Round(sum_r X[r, i] Y[r, j]) (p x q); mode 'D' (p == q):
        out[j] = Round(sum_r X[r, j] Y[r, j]).  Every output is bit for bit what exdot_dev gives for the two columns.  X and
        Y are 2-D float64 tensors with stride(1) == 1 and stride(0) >= their column count (a view [:, :k] of a wider block is
        fine; anything else is refused, not copied) and equal row counts; Y=None means Y = X.  `out` is allocated when None,
        otherwise checked; it is returned."""
        out, args = _bdot_args(X, Y, mode, out, fpe, early_exit)
        _check(load_library().exblas_exbdot_ctx(self.handle, *args, _stream_ptr(_torch())), "exbdot")
        return out

    def exbgemm(self, X, C, alpha=1.0, beta=0.0, Y=None, fpe=8, early_exit=True):  # noqa: N803
        """ExBGEMM: Y = Round(alpha X C + beta Y) output by output, exact, reproducible and rounded once, stream-ordered on
        the current stream: the block update that ends a block-Krylov iteration (X += P a, R -= Q a, P = Z + P b).  Bit for
        bit exspmm_dev on X stored as a dense CSR matrix against C.  X (n x p), C (p x q) and Y (n x q) are 2-D float64
        tensors with stride(1) == 1 and stride(0) >= their column count (a view [:, :k] of a wider block is fine; anything
        else is refused, not copied); Y is updated in place and must not overlap X or C, or is allocated (zeros) when
        None.  The design range is p, q <= 64.  Returns Y."""
        Y, args = _bgemm_args(X, C, alpha, beta, Y, fpe, early_exit)
        _check(load_library().exblas_exbgemm_ctx(self.handle, *args, _stream_ptr(_torch())), "exbgemm")
        return Y

    def exbtrsm(self, T, X, uplo="U", trans="N", diag="N", alpha=1.0, fpe=8, early_exit=True):  # noqa: N803
        """ExBTRSM: solves X op(T) = alpha B in place on the tall n x p block X (B on entry) from the right, exact,
        reproducible and rounded once per output, stream-ordered on the current stream: Q = X R^-1 of CholQR, the
        normalisation of a block Krylov method.  With alpha = 1, row r is bit for bit what extrsv_dev gives for the other
        trans on B[r, :].  T: a p x p float64 tensor with one unit stride, never copied -- column-major (stride(0) == 1) or
        row-major (stride(1) == 1); `uplo` names the triangle of T[i, j] as Python indexes it, the other triangle is never
        read; p <= 512.  X: a 2-D float64 tensor with stride(1) == 1 and stride(0) >= p (a view [:, :p] of a wider block
        is fine: its padding is not touched; anything else is refused, not copied).  fpe: 0, 1 or 2..8.  One kernel launch,
        no mailbox.  The design range is p <= 64.  Returns X."""
        args = _btrsm_args(T, X, uplo, trans, diag, alpha, fpe, early_exit)
        _check(load_library().exblas_exbtrsm_ctx(self.handle, *args, _stream_ptr(_torch())), "exbtrsm")
        return X

    def expotrf(self, G, uplo="U", info=None, fpe=8, early_exit=True):  # noqa: N803
        """ExPOTRF: the exact-sum Cholesky factor of the p x p Gram matrix G, in place, stream-ordered on the current stream
        and never synchronising: uplo 'U' leaves R upper with G = R^T R, 'L' leaves L = R^T.  Every sum is exact and
        rounded once, followed by one correctly rounded square root or division, so the factor is reproducible bit for
        bit and is what exbtrsm_dev / extrsm_dev take.  G: a float64 tensor with one unit stride, never copied --
        column-major (stride(0) == 1) or row-major (stride(1) == 1); `uplo` names the triangle of G[i, j] as Python
        indexes it, the other triangle is neither read nor written; p <= 512.  info: a one-element int32 device tensor
        (allocated when None) that receives 0, or j + 1 when the radicand of pivot j (0-based) is not > 0: that value is
        stored at (j, j), and row j beyond it and the later rows stay as they were (LAPACK's rule).  fpe: 0, 1 or 2..8.
        One kernel launch of one workgroup.  The design range is p <= 64.  Returns (G, info)."""
        info, args = _potrf_args(G, uplo, info, fpe, early_exit)
        _check(load_library().exblas_expotrf_ctx(self.handle, *args, _stream_ptr(_torch())), "expotrf")
        return G, info

    def expotrf_batched(self, G, uplo="U", info=None, fpe=8, early_exit=True):  # noqa: N803
        """Batched ExPOTRF: the exact-sum Cholesky factors of the batch matrices of G ([batch, p, p] float64, p <= 64), in
        place, in one stream-ordered launch that never synchronises: the factor step of a block-Jacobi preconditioner.
        Every matrix is bit for bit what expotrf_dev gives on it alone, whatever the batch, its place in it and its
        neighbours.  Each matrix has one unit stride among its last two dimensions -- column-major (stride(1) == 1) or
        row-major (stride(2) == 1); `uplo` names the triangle of G[b, i, j] as Python indexes it, the other triangle is
        neither read nor written -- and G.stride(0) is the batch stride (the matrices must not overlap); G is never
        copied.  info: a contiguous int32 device tensor of batch words (allocated when None); info[b] receives 0, or
        j + 1 when the radicand of pivot j of matrix b is not > 0 (that value is stored at its pivot, the rest of that
        matrix stays as it was; the other matrices are not affected).  fpe: 0, 1 or 2..8.  Returns (G, info)."""
        info, args = _potrf_batched_args(G, uplo, info, fpe, early_exit)
        _check(load_library().exblas_expotrf_batched_ctx(self.handle, *args, _stream_ptr(_torch())), "expotrf_batched")
        return G, info

    def expotrs_batched(self, R, X, uplo="U", sweep="B", fpe=8, early_exit=True):  # noqa: N803
        """Batched ExPOTRS: applies blockdiag(G_b)^-1 to the n x k row-major block X in place, G_b = F^T F with the factors
        R ([ceil(n / p), p, p], as expotrf_batched_dev leaves them, same layout rules and `uplo`), exact, reproducible and
        rounded once per output, in one stream-ordered launch: the apply step of a block-Jacobi preconditioner.  Block b
        covers the rows b p .. min(n, (b + 1) p) - 1 of X; a shorter last block uses the leading part of its triangle.
        sweep '1' solves F^T Y = B, '2' solves F Z = Y, 'B' (the default) both, bit for bit '1' then '2'.  Every column of
        a block is bit for bit what extrsv_dev / extrsm_dev give on that block.  X: a 2-D float64 tensor with
        stride(1) == 1 and stride(0) >= k (a view of a wider block is fine: its padding is not touched; anything else
        is refused, not copied).  The info words of the factorisation are NOT consulted: a block whose factorisation
        broke down is the caller's concern.  fpe: 0, 1 or 2..8.  Returns X."""
        args = _potrs_batched_args(R, X, uplo, sweep, fpe, early_exit)
        _check(load_library().exblas_expotrs_batched_ctx(self.handle, *args, _stream_ptr(_torch())), "expotrs_batched")
        return X

    def exgetrf_batched(self, A, ipiv=None, info=None, fpe=8, early_exit=True):  # noqa: N803
        """Batched ExGETRF: the exact-sum LU factorisation with partial pivoting of the batch general matrices of A
        ([batch, p, p] float64, p <= 64), in place, in one stream-ordered launch that never synchronises: the factor step of
        a block-Jacobi preconditioner whose blocks are not symmetric positive definite.  Storage follows LAPACK: the
        unit-lower L strictly below the diagonal of A[b], U on and above it, ipiv[b, j] the 1-based row exchanged with row j
        at step j.  Every entry is one exact sum rounded once (the entries of L then take ONE IEEE division); the pivot
        is the first row with the largest candidate.  The bits of a matrix depend on its data and the rounding mode only.
        Each matrix has one unit stride among its last two dimensions, column-major (stride(1) == 1) or row-major
        (stride(2) == 1), and A.stride(0) is the batch stride (the matrices must not overlap); A is never copied, its
        padding and gaps are not touched.  ipiv: a contiguous int32 device tensor [batch, p]; info: a contiguous int32
        device tensor of batch words (each allocated when None).  info[b] receives 0, or j + 1 when the pivot of step j of
        matrix b is zero or NaN: the candidates of that step are stored, ipiv[b, i] = i + 1 from there on, the rest of
        that matrix stays as it was, and no other matrix is affected.  fpe: 0, 1 or 2..8.  Returns (A, ipiv, info)."""
        ipiv, info, args = _getrf_batched_args(A, ipiv, info, fpe, early_exit)
        _check(load_library().exblas_exgetrf_batched_ctx(self.handle, *args, _stream_ptr(_torch())), "exgetrf_batched")
        return A, ipiv, info

    def exgetrs_batched(self, LU, ipiv, X, fpe=8, early_exit=True):  # noqa: N803
        """Batched ExGETRS: applies blockdiag(A_b)^-1 to the n x k row-major block X in place, with the factors LU
        ([ceil(n / p), p, p]) and pivots ipiv as exgetrf_batched_dev leaves them (same layout rules), exact, reproducible
        and rounded once per output, in one stream-ordered launch: the apply step of a block-Jacobi preconditioner.  Block
        b covers the rows b p .. min(n, (b + 1) p) - 1 of X; a shorter last block uses the leading part of its factors
        and its first pivots.  The rows are interchanged as ipiv says (an index outside the block is skipped), then the
        unit-lower sweep runs forward and the upper sweep backward: every column of a block is bit for bit what
        extrsv_dev gives twice on the permuted column.  X: a 2-D float64 tensor with stride(1) == 1 and stride(0) >= k
        (anything else is refused, not copied).  The info words of the factorisation are NOT consulted.  fpe: 0, 1 or
        2..8.  Returns X."""
        args = _getrs_batched_args(LU, ipiv, X, fpe, early_exit)
        _check(load_library().exblas_exgetrs_batched_ctx(self.handle, *args, _stream_ptr(_torch())), "exgetrs_batched")
        return X

    def exbdot_export(self, X, Y=None, mode="G", sets=None, fpe=8, early_exit=True):
        """First half of a row-sharded ExBDOT: X and Y (as for exbdot_dev) are the rows of one shard.  Returns an int64 tensor
        [outputs, 72] (`sets`, or a new one) -- output i * q + j in mode 'G', output j in mode 'D': the exact sum of the
        shard's products as 68 normalised base-2^32 digits under a signed top digit, three 0 / 1 indicators (+Inf, -Inf, NaN
        seen) and a zero word.  Sets of different shards add as plain int64; exbdot_round_dev rounds the sum.  fpe == 1 and
        early_exit with fpe > 8 are refused: they have no digit sets."""
        sets, args = _bdot_export_args(X, Y, mode, sets, fpe, early_exit)
        _check(load_library().exblas_exbdot_export_ctx(self.handle, *args, _stream_ptr(_torch())), "exbdot_export")
        return sets

    def exbdot_round(self, sets, mode, p, q, out=None):
        """Second half: `sets` is a contiguous int64 tensor [outputs, 72] or [nsets, outputs, 72] (the exports of nsets shards
        stacked, or a sum of exports); the nsets copies of every output are added and rounded once, under the current
        rounding mode, into `out` (as for exbdot_dev: p x q in mode 'G', p in mode 'D'; allocated when None).  Bit for bit
        exbdot_dev on the rows of all shards together.  `sets` is only read."""
        out, args = _bdot_round_args(sets, mode, p, q, out)
        _check(load_library().exblas_exbdot_round_ctx(self.handle, *args, _stream_ptr(_torch())), "exbdot_round")
        return out

    def workspace_bytes(self):
        return load_library().exblas_workspace_bytes_ctx(self.handle)


# The device's default context: no handle, so nothing is created (importing needs no GPU) and destroy() does nothing.
_default = object.__new__(Context)
_default.handle = None
exsum_dev, exdot_dev, finish_dev = _default.exsum, _default.exdot, _default.finish
exsum_accumulate_dev, exdot_accumulate_dev = _default.exsum_accumulate, _default.exdot_accumulate
exsum_lp_dev, exdot_lp_dev, round_records_dev = _default.exsum_lp, _default.exdot_lp, _default.round_records
exsum_lp_accumulate_dev, exdot_lp_accumulate_dev = _default.exsum_lp_accumulate, _default.exdot_lp_accumulate
exsum_to_dev, exdot_to_dev = _default.exsum_to, _default.exdot_to
exgemv_dev, extrsv_dev, exgemm_dev = _default.exgemv, _default.extrsv, _default.exgemm
extrsm_dev = _default.extrsm
exspmv_dev, exspmm_dev, exsptrsv_dev, exsptrsm_dev = _default.exspmv, _default.exspmm, _default.exsptrsv, _default.exsptrsm
exspmv_lp_dev, exspmm_lp_dev = _default.exspmv_lp, _default.exspmm_lp
exspilu0_dev, exspilu0_apply_dev = _default.exspilu0, _default.exspilu0_apply
exspic0_dev, exspic0_apply_dev = _default.exspic0, _default.exspic0_apply
exbdot_dev, exbdot_export_dev, exbdot_round_dev = _default.exbdot, _default.exbdot_export, _default.exbdot_round
exbgemm_dev = _default.exbgemm
exbtrsm_dev = _default.exbtrsm
expotrf_dev = _default.expotrf
expotrf_batched_dev, expotrs_batched_dev = _default.expotrf_batched, _default.expotrs_batched
exgetrf_batched_dev, exgetrs_batched_dev = _default.exgetrf_batched, _default.exgetrs_batched


def excholqr_dev(X, fpe=8, early_exit=True):  # noqa: N803
    """CholQR of the tall n x p row-major block X on the default context, all on the device: G = exbdot_dev(X),
    R = expotrf_dev(G, 'U'), X := X R^-1 by exbtrsm_dev, in place.  Three stream-ordered launches, no synchronisation,
    capturable as a whole (after one call).  Returns (X, R, info): X holds Q; R is p x p with the factor in its upper
    triangle (the strict lower triangle keeps G's entries); info is expotrf_dev's word, to be read when the caller wants
    to -- when it is not 0, X^T X was not numerically positive definite and Q, R are not to be used."""
    G = exbdot_dev(X, fpe=fpe, early_exit=early_exit)
    R, info = expotrf_dev(G, "U", fpe=fpe, early_exit=early_exit)
    exbtrsm_dev(R, X, "U", "N", fpe=fpe, early_exit=early_exit)
    return X, R, info


def gen_dev(kind, n, seed=1, p0=0.0, p1=0.0, first=0, count=None, n_total=None, out=None):
    """Counter-based generator on the GPU; bit-identical to oracle.pyoracle.gen()."""
    torch = _require_gpu()
    k = GEN_KINDS[kind] if isinstance(kind, str) else int(kind)
    if count is None:
        count = n
    if n_total is None:
        n_total = n
    if out is None:
        out = torch.empty(count, dtype=torch.float64, device="cuda")
    _check(load_library().exblas_gen_dev(k, seed, first, count, n_total, p0, p1, C.c_void_p(out.data_ptr()),
                                         _stream_ptr(torch)), "gen_dev")
    return out


def stream_read_dev(x, sink=None):
    torch = _require_gpu()
    if sink is None:
        sink = torch.zeros(1, dtype=torch.float64, device="cuda")
    _check(load_library().exblas_stream_read_dev(C.c_void_p(x.data_ptr()), x.numel(), _stream_ptr(torch),
                                                 C.c_void_p(sink.data_ptr())), "stream_read_dev")
    return sink


def read_record(rec_tensor):
    """Synchronising D2H read of a record tensor."""
    return Record(rec_tensor.cpu().numpy())


# ---------------------------------------------------------------------------------------------
# reference-style API (host arrays in, doubles out) -- same argument order as the C++ headers
# ---------------------------------------------------------------------------------------------
def _host(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def exsum(Ng, ag, inca, offset, fpe, early_exit=False, parallel=True):
    """double exsum(Ng, ag, inca, offset, fpe, early_exit, parallel) -- include/blas1.hpp:48."""
    _require_gpu()
    a = _host(ag)
    return load_library().exblas_exsum(int(Ng), C.c_void_p(a.ctypes.data), int(inca), int(offset), int(fpe),
                                       int(bool(early_exit)))


def exdot(Ng, ag, inca, offseta, bg, incb, offsetb, fpe, early_exit=False):
    """double exdot(...) -- include/blas1.hpp:74."""
    _require_gpu()
    a, b = _host(ag), _host(bg)
    return load_library().exblas_exdot(int(Ng), C.c_void_p(a.ctypes.data), int(inca), int(offseta),
                                       C.c_void_p(b.ctypes.data), int(incb), int(offsetb), int(fpe),
                                       int(bool(early_exit)))


def exsum_record(Ng, ag, inca, offset, fpe, early_exit=False):
    _require_gpu()
    a = _host(ag)
    out = np.zeros(OUT_WORDS, dtype=np.int64)
    load_library().exblas_exsum_record(int(Ng), C.c_void_p(a.ctypes.data), int(inca), int(offset), int(fpe),
                                       int(bool(early_exit)), C.c_void_p(out.ctypes.data))
    return Record(out)


def exdot_record(Ng, ag, inca, offseta, bg, incb, offsetb, fpe, early_exit=False):
    _require_gpu()
    a, b = _host(ag), _host(bg)
    out = np.zeros(OUT_WORDS, dtype=np.int64)
    load_library().exblas_exdot_record(int(Ng), C.c_void_p(a.ctypes.data), int(inca), int(offseta),
                                       C.c_void_p(b.ctypes.data), int(incb), int(offsetb), int(fpe),
                                       int(bool(early_exit)), C.c_void_p(out.ctypes.data))
    return Record(out)


def _host_lp(a, who):
    """(EXBLAS_DT_* code, address, keep-alive) of a contiguous numpy array or torch CPU tensor (bfloat16: torch only)"""
    if hasattr(a, "data_ptr"):
        if a.is_cuda:
            raise ValueError(f"exblas_amd.{who}: the host forms take numpy arrays or torch CPU tensors")
        a = a.contiguous()
        return _dt(a.dtype, who)[0], a.data_ptr(), a
    a = np.ascontiguousarray(a)
    return _dt(a.dtype, who)[0], a.ctypes.data, a


def exsum_lp(a, fpe=8, early_exit=True):
    """ExSUM of a host array of float64 / float32 / float16 (numpy, torch CPU) or bfloat16 (torch CPU): the Record."""
    code, ptr, keep = _host_lp(a, "exsum_lp")
    _require_gpu()
    out = np.zeros(OUT_WORDS, dtype=np.int64)
    _check(load_library().exblas_exsum_lp(code, C.c_void_p(ptr), keep.size if hasattr(keep, "ctypes") else keep.numel(),
                                          1, fpe, int(bool(early_exit)), C.c_void_p(out.ctypes.data)), "exsum_lp")
    return Record(out)


def exdot_lp(a, b, fpe=8, early_exit=True):
    """ExDOT of two host arrays of one of the four dtypes (see exsum_lp): the Record."""
    code, pa, ka = _host_lp(a, "exdot_lp")
    codeb, pb, kb = _host_lp(b, "exdot_lp")
    if code != codeb:
        raise TypeError("exblas_amd.exdot_lp: the operands have different dtypes")
    na, nb = (k.size if hasattr(k, "ctypes") else k.numel() for k in (ka, kb))
    if na != nb:
        raise ValueError("exblas_amd.exdot_lp: the operands have different lengths")
    _require_gpu()
    out = np.zeros(OUT_WORDS, dtype=np.int64)
    _check(load_library().exblas_exdot_lp(code, C.c_void_p(pa), 1, C.c_void_p(pb), 1, na, fpe, int(bool(early_exit)),
                                          C.c_void_p(out.ctypes.data)), "exdot_lp")
    return Record(out)


def round_digits_host(digits, dtype):
    """The 68 normalised digits of a record rounded once into `dtype`, on the CPU (no device): the bit pattern, an int."""
    code = _dt(dtype, "round_digits_host")[0]
    d = np.ascontiguousarray(digits, dtype=np.int64)
    if d.shape != (NDIGITS,):
        raise ValueError("exblas_amd.round_digits_host: 68 digits expected")
    bits = C.c_uint64()
    _check(load_library().exblas_round_digits_host(C.c_void_p(d.ctypes.data), code, C.byref(bits)), "round_digits_host")
    return int(bits.value)


def round_window_host(digits, dtype):
    """round_digits_host computed the way the narrow sparse products round an accumulator (the leading 64 bits and a sticky):
    the bit pattern, an int; no device"""
    code = _dt(dtype, "round_window_host")[0]
    d = np.ascontiguousarray(digits, dtype=np.int64)
    if d.shape != (NDIGITS,):
        raise ValueError("exblas_amd.round_window_host: 68 digits expected")
    bits = C.c_uint64()
    _check(load_library().exblas_round_window_host(C.c_void_p(d.ctypes.data), code, C.byref(bits)), "round_window_host")
    return int(bits.value)


def round_interval_host(res, bound, dtype):
    """The certificate of the narrow sparse products' in-register rounding, on the CPU (no device): the bit pattern (an int)
    of the one `dtype` value that every real number of [res - bound, res + bound] rounds to, or None when the interval
    reaches a rounding boundary of the format.  bound = 0 declares res exact (ties are then decided, to even)."""
    code = _dt(dtype, "round_interval_host")[0]
    bits = C.c_uint64()
    rc = load_library().exblas_round_interval_host(float(res), float(bound), code, C.byref(bits))
    if rc < 0:
        raise RuntimeError("exblas_amd: round_interval_host refused its arguments")
    return int(bits.value) if rc == 1 else None


def exgemv(transa, m, n, alpha, a, lda, offseta, x, incx, offsetx, beta, y, incy, offsety, fpe, early_exit=False):
    """int exgemv(...) -- include/blas2.hpp:95; y (numpy float64) is updated in place."""
    _require_gpu()
    a_, x_ = _host(a), _host(x)
    assert isinstance(y, np.ndarray) and y.dtype == np.float64 and y.flags.c_contiguous
    return load_library().exblas_exgemv(transa.encode(), m, n, alpha, C.c_void_p(a_.ctypes.data), lda, offseta,
                                        C.c_void_p(x_.ctypes.data), incx, offsetx, beta, C.c_void_p(y.ctypes.data),
                                        incy, offsety, fpe, int(bool(early_exit)))


def extrsv(uplo, transa, diag, n, a, lda, offseta, x, incx, offsetx, fpe, early_exit=False):
    """int extrsv(...) -- include/blas2.hpp:57; x (numpy float64) holds b on entry and the solution on return."""
    _require_gpu()
    a_ = _host(a)
    assert isinstance(x, np.ndarray) and x.dtype == np.float64 and x.flags.c_contiguous
    return load_library().exblas_extrsv(uplo.encode(), transa.encode(), diag.encode(), n, C.c_void_p(a_.ctypes.data),
                                        lda, offseta, C.c_void_p(x.ctypes.data), incx, offsetx, fpe,
                                        int(bool(early_exit)))


def exgemm(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, fpe, early_exit=False):
    """int exgemm(...) -- include/blas3.hpp:56; c (numpy float64) is updated in place."""
    _require_gpu()
    a_, b_ = _host(a), _host(b)
    assert isinstance(c, np.ndarray) and c.dtype == np.float64 and c.flags.c_contiguous
    return load_library().exblas_exgemm(transa.encode(), transb.encode(), m, n, k, alpha, C.c_void_p(a_.ctypes.data),
                                        lda, C.c_void_p(b_.ctypes.data), ldb, beta, C.c_void_p(c.ctypes.data), ldc,
                                        fpe, int(bool(early_exit)))


def _csr_host(who, A, square=False):
    """The CSR operand of the host routine `who`: a (row_ptr, col_idx, val, shape) tuple of numpy arrays.  Returns
    (crow, col, val, m, n, index_bits) with the arrays contiguous."""
    if not isinstance(A, (tuple, list)) or len(A) != 4:
        raise ValueError(f"{who}: A must be a (row_ptr, col_idx, val, shape) tuple of numpy arrays")
    crow, col, val = (np.asarray(a) for a in A[:3])
    m, n, bits = _csr_rules(who, np, crow, col, val, A[3], square)
    if m > 0 and (crow.min() < 0 or crow.max() > col.size):
        raise ValueError(f"{who}: row_ptr entries must lie in [0, nnz]")
    return np.ascontiguousarray(crow), np.ascontiguousarray(col), np.ascontiguousarray(val), m, n, bits


def _dense_host(who, name, a, ndim, hint=""):
    """The dense operand `name` of the host routine `who` as a float64 array of `ndim` dimensions."""
    a = np.asarray(a)
    if a.dtype != np.float64:
        raise TypeError(f"{who}: {name} must be float64")
    if a.ndim != ndim:
        raise ValueError(f"{who}: {name} must be {ndim}-D{hint}")
    return a


def _hptr(a):
    return C.c_void_p(a.ctypes.data) if a.size else None


def exspmv(A, x, alpha=1.0, beta=0.0, y=None, fpe=8, early_exit=True):
    """ExSpMV on host arrays: A = (row_ptr, col_idx, val, (m, n)) as numpy arrays (int32 or int64 indices of one width,
    float64 values), x float64 of at least n entries; returns y (a new float64 array; the y passed in is not changed)."""
    crow, col, val, m, n, bits = _csr_host("exspmv", A)
    x = np.ascontiguousarray(_dense_host("exspmv", "x", x, 1))
    if x.size < n:
        raise ValueError(f"exspmv: x has {x.size} entries, fewer than n = {n}")
    y = np.zeros(m) if y is None else np.array(y, dtype=np.float64, copy=True)
    if y.ndim != 1 or y.size != m:
        raise ValueError(f"exspmv: y must have m = {m} entries")
    _require_gpu()
    _check(load_library().exblas_exspmv_csr(m, n, bits, _hptr(crow), _hptr(col), _hptr(val), float(alpha), _hptr(x),
                                            float(beta), _hptr(y), int(fpe), int(bool(early_exit))), "exspmv")
    return y


def _host_lp_csr(who, A):
    """The CSR operand of a narrow host routine: (row_ptr, col_idx, val, shape) with numpy index arrays and the values a
    numpy array or torch CPU tensor (bfloat16: torch only).  Returns (crow, col, (code, address, keep-alive), m, n, bits)."""
    if not isinstance(A, (tuple, list)) or len(A) != 4:
        raise ValueError(f"{who}: A must be a (row_ptr, col_idx, val, shape) tuple")
    crow, col = np.asarray(A[0]), np.asarray(A[1])
    val = A[2] if hasattr(A[2], "data_ptr") else np.asarray(A[2])
    m, n, bits = _csr_rules(who, np, crow, col, val, A[3], False, narrow=True)
    if m > 0 and (crow.min() < 0 or crow.max() > col.size):
        raise ValueError(f"{who}: row_ptr entries must lie in [0, nnz]")
    return np.ascontiguousarray(crow), np.ascontiguousarray(col), _host_lp(val, who), m, n, bits


def _host_like(x, shape):
    """zeros of the kind and dtype of the host operand x (numpy array or torch CPU tensor)"""
    return _torch().zeros(shape, dtype=x.dtype) if hasattr(x, "data_ptr") else np.zeros(shape, dtype=x.dtype)


def _host_copy(y, x, who):
    """a contiguous copy of y in the kind and dtype of x"""
    if hasattr(x, "data_ptr"):
        torch = _torch()
        if not isinstance(y, torch.Tensor) or y.dtype != x.dtype:
            raise TypeError(f"{who}: y must be a torch CPU tensor of x's dtype")
        return y.detach().clone().contiguous()
    y = np.asarray(y)
    if y.dtype != x.dtype:
        raise TypeError(f"{who}: y must have x's dtype")
    return np.array(y, copy=True, order="C")


def _hp(ptr_keep):
    code, ptr, keep = ptr_keep
    return C.c_void_p(ptr) if (keep.size if hasattr(keep, "ctypes") else keep.numel()) else None


def exspmv_lp(A, x, alpha=1.0, beta=0.0, y=None, fpe=8, early_exit=True):
    """Narrow ExSpMV on host arrays: A = (row_ptr, col_idx, val, (m, n)) with float32 / float16 / bfloat16 values, x float64
    or of the values' type; numpy arrays or torch CPU tensors (bfloat16: torch CPU tensors).  Returns a new y of x's kind
    and dtype (the y passed in is not changed)."""
    who = "exspmv_lp"
    crow, col, hv, m, n, bits = _host_lp_csr(who, A)
    hx = _host_lp(x, who)
    if hx[2].ndim != 1:
        raise ValueError(f"{who}: x must be 1-D")
    vcode, xcode = hv[0], hx[0]
    _lp_pair(who, hv[2].dtype, hx[2].dtype, fpe)
    if (hx[2].size if hasattr(hx[2], "ctypes") else hx[2].numel()) < n:
        raise ValueError(f"{who}: x has fewer than n = {n} entries")
    y = _host_like(hx[2], m) if y is None else _host_copy(y, hx[2], who)
    if y.ndim != 1 or y.shape[0] != m:
        raise ValueError(f"{who}: y must have m = {m} entries")
    hy = _host_lp(y, who)
    _require_gpu()
    _check_lp(load_library().exblas_exspmv_csr_lp(m, n, bits, _hptr(crow), _hptr(col), vcode, _hp(hv), float(alpha), xcode,
                                                  _hp(hx), float(beta), _hp(hy), int(fpe), int(bool(early_exit))), who)
    return y


def exspmm_lp(A, X, alpha=1.0, beta=0.0, Y=None, fpe=8, early_exit=True):
    """Narrow ExSpMM on host arrays (see exspmv_lp): X of shape (n', k) with n' >= n; returns a new Y (m x k)."""
    who = "exspmm_lp"
    crow, col, hv, m, n, bits = _host_lp_csr(who, A)
    hx = _host_lp(X, who)
    if hx[2].ndim != 2:
        raise ValueError(f"{who}: X must be 2-D (n x k; for one vector use exspmv_lp)")
    vcode, xcode = hv[0], hx[0]
    _lp_pair(who, hv[2].dtype, hx[2].dtype, fpe)
    if hx[2].shape[0] < n:
        raise ValueError(f"{who}: X has {hx[2].shape[0]} rows, fewer than n = {n}")
    k = int(hx[2].shape[1])
    Y = _host_like(hx[2], (m, k)) if Y is None else _host_copy(Y, hx[2], who)
    if tuple(Y.shape) != (m, k):
        raise ValueError(f"{who}: Y must have shape ({m}, {k})")
    hy = _host_lp(Y, who)
    _require_gpu()
    _check_lp(load_library().exblas_exspmm_csr_lp(m, n, k, bits, _hptr(crow), _hptr(col), vcode, _hp(hv), float(alpha),
                                                  xcode, _hp(hx), k, float(beta), _hp(hy), k, int(fpe),
                                                  int(bool(early_exit))), who)
    return Y


def exsptrsv(A, b, uplo="L", diag="N", fpe=8, early_exit=True):
    """ExSpTRSV on host arrays: A = (row_ptr, col_idx, val, (m, m)) as numpy arrays (as for exspmv), b float64 of m entries;
    returns the solution (a new float64 array; b is not changed)."""
    crow, col, val, m, _, bits = _csr_host("exsptrsv", A, square=True)
    u, d = _solve_flags("exsptrsv", uplo, diag)
    b = _dense_host("exsptrsv", "b", b, 1)
    if b.size != m:
        raise ValueError(f"exsptrsv: b must have m = {m} entries")
    x = np.array(b, dtype=np.float64, copy=True)
    _require_gpu()
    _check_sparse(load_library().exblas_exsptrsv_csr(u, d, m, bits, _hptr(crow), _hptr(col), _hptr(val), _hptr(x),
                                                     int(fpe), int(bool(early_exit))), "exsptrsv")
    return x


def _factor_host(who, A, fpe, early_exit):
    crow, col, val, m, _, bits = _csr_host(who, A, square=True)
    out = np.array(val, dtype=np.float64, copy=True)
    info = np.zeros(2, dtype=np.int64)
    _require_gpu()
    _check_sparse(getattr(load_library(), f"exblas_{who}_csr")(m, bits, _hptr(crow), _hptr(col), _hptr(val), _hptr(out),
                                                                C.c_void_p(info.ctypes.data), int(fpe),
                                                                int(bool(early_exit))), who)
    return out, (int(info[0]), int(info[1]))


def exspilu0(A, fpe=8, early_exit=True):
    """ExSpILU0 on host arrays: A = (row_ptr, col_idx, val, (m, m)) as numpy arrays (as for exspmv; strictly ascending
    columns and a stored diagonal in every row); returns (lu_values, (info0, info1)): the factor's values on A's pattern
    (a new float64 array, a copy of A's values when info0 reports a structural defect) and the two info words."""
    return _factor_host("exspilu0", A, fpe, early_exit)


def exspic0(A, fpe=8, early_exit=True):
    """ExSpIC0 on host arrays: A = (row_ptr, col_idx, val, (m, m)) as numpy arrays (as for exspmv; strictly ascending
    columns, a stored diagonal in every row, a structurally symmetric pattern); returns (ll_values, (info0, info1)): the
    factor's values on A's pattern, L and its mirror (a new float64 array, a copy of A's values when info0 reports a
    structural defect) and the two info words."""
    return _factor_host("exspic0", A, fpe, early_exit)


def exsptrsm(A, B, uplo="L", diag="N", fpe=8, early_exit=True):
    """ExSpTRSM on host arrays: A = (row_ptr, col_idx, val, (m, m)) as numpy arrays (as for exspmv), B float64 of shape
    (m, k); returns the solution (a new m x k float64 array; B is not changed)."""
    crow, col, val, m, _, bits = _csr_host("exsptrsm", A, square=True)
    u, d = _solve_flags("exsptrsm", uplo, diag)
    B = _dense_host("exsptrsm", "B", B, 2, " (a block of right-hand sides; for one vector use exsptrsv)")
    if B.shape[0] != m:
        raise ValueError(f"exsptrsm: B must have m = {m} rows")
    X = np.array(B, dtype=np.float64, copy=True, order="C")
    k = int(X.shape[1])
    _require_gpu()
    _check_sparse(load_library().exblas_exsptrsm_csr(u, d, m, k, bits, _hptr(crow), _hptr(col), _hptr(val), _hptr(X),
                                                     max(k, 1), int(fpe), int(bool(early_exit))), "exsptrsm")
    return X


class _HostStrides:
    """shape and element strides of a numpy array, as _trsm_layout reads them"""

    def __init__(self, a):
        self.shape = a.shape
        self._strides = tuple(s // a.itemsize for s in a.strides)

    def stride(self, i):
        return self._strides[i]


def extrsm(A, B, uplo="L", trans="N", diag="N", fpe=8, early_exit=True):
    """ExTRSM on host arrays: A float64 of shape (n, n), C- or Fortran-ordered (anything else is copied to C order; `uplo`
    names the triangle of A[i, j]), B float64 of shape (n, k); returns the solution (a new n x k float64 array; B is not
    changed)."""
    A = _dense_host("extrsm", "A", A, 2)
    n = int(A.shape[0])
    if A.shape[1] != n:
        raise ValueError(f"extrsm: A must be square, got shape {tuple(A.shape)}")
    if not (A.flags.c_contiguous or A.flags.f_contiguous):
        A = np.ascontiguousarray(A)
    u, t, lda = _trsm_layout(_HostStrides(A), uplo, trans)
    _, d = _solve_flags("extrsm", "L", diag)
    B = _dense_host("extrsm", "B", B, 2, " (a block of right-hand sides; for one vector use extrsv)")
    if B.shape[0] != n:
        raise ValueError(f"extrsm: B must have n = {n} rows")
    fpe = _fpe_0_to_8("extrsm", fpe)
    X = np.array(B, dtype=np.float64, copy=True, order="C")
    k = int(X.shape[1])
    _require_gpu()
    _check_sparse(load_library().exblas_extrsm(u.encode(), t.encode(), d, n, k, _hptr(A), max(lda, 1), _hptr(X), max(k, 1),
                                               fpe, int(bool(early_exit))), "extrsm")
    return X


def exspmm(A, X, alpha=1.0, beta=0.0, Y=None, fpe=8, early_exit=True):
    """ExSpMM on host arrays: A = (row_ptr, col_idx, val, (m, n)) as numpy arrays (as for exspmv), X float64 of shape
    (rows >= n, k); returns Y (a new m x k float64 array; the Y passed in is not changed)."""
    crow, col, val, m, n, bits = _csr_host("exspmm", A)
    X = np.ascontiguousarray(_dense_host("exspmm", "X", X, 2, " (n x k; for one vector use exspmv)"))
    if X.shape[0] < n:
        raise ValueError(f"exspmm: X has {X.shape[0]} rows, fewer than n = {n}")
    k = int(X.shape[1])
    Y = np.zeros((m, k)) if Y is None else np.array(Y, dtype=np.float64, copy=True, order="C")
    if Y.shape != (m, k):
        raise ValueError(f"exspmm: Y must have shape ({m}, {k})")
    _require_gpu()
    _check(load_library().exblas_exspmm_csr(m, n, k, bits, _hptr(crow), _hptr(col), _hptr(val), float(alpha), _hptr(X), k,
                                            float(beta), _hptr(Y), k, int(fpe), int(bool(early_exit))), "exspmm")
    return Y


def exbdot(X, Y=None, mode="G", fpe=8, early_exit=True):
    """ExBDOT on host arrays: X (n x p) and Y (n x q, None: Y = X) float64; returns a new p x q array (mode 'G') or a new
    array of p entries (mode 'D', p == q)."""
    mode = _bdot_mode(mode)
    hint = " (n x p; for two vectors use exdot)"
    X = np.ascontiguousarray(_dense_host("exbdot", "X", X, 2, hint))
    Y = X if Y is None else np.ascontiguousarray(_dense_host("exbdot", "Y", Y, 2, hint))
    if X.shape[0] != Y.shape[0]:
        raise ValueError(f"exbdot: X has {X.shape[0]} rows and Y has {Y.shape[0]}")
    n, p, q = int(X.shape[0]), int(X.shape[1]), int(Y.shape[1])
    _bdot_sizes(mode, n, p, q, fpe)
    out = np.zeros((p, q) if mode == "G" else (p,))
    _require_gpu()
    _check(load_library().exblas_exbdot(mode.encode(), n, p, q, _hptr(X), max(p, 1), _hptr(Y), max(q, 1), _hptr(out),
                                        max(q, 1), int(fpe), int(bool(early_exit))), "exbdot")
    return out


def exbgemm(X, C, alpha=1.0, beta=0.0, Y=None, fpe=8, early_exit=True):  # noqa: N803
    """ExBGEMM on host arrays: X (n x p), C (p x q) and Y (n x q, None: zeros) float64; returns the updated block (a new
    n x q float64 array; the Y passed in is not changed)."""
    X = np.ascontiguousarray(_dense_host("exbgemm", "X", X, 2))
    Cm = np.ascontiguousarray(_dense_host("exbgemm", "C", C, 2))
    n, p, q = int(X.shape[0]), int(X.shape[1]), int(Cm.shape[1])
    if Cm.shape[0] != p:
        raise ValueError(f"exbgemm: C must have p = {p} rows, not {Cm.shape[0]}")
    if n > 0x7fffffff or int(fpe) < 0:
        raise ValueError("exbgemm: n must not exceed INT_MAX and fpe must be >= 0")
    Y = np.zeros((n, q)) if Y is None else np.array(Y, dtype=np.float64, copy=True, order="C")
    if Y.shape != (n, q):
        raise ValueError(f"exbgemm: Y must have shape ({n}, {q})")
    _require_gpu()
    _check(load_library().exblas_exbgemm(n, p, q, float(alpha), _hptr(X), max(p, 1), _hptr(Cm), max(q, 1), float(beta),
                                         _hptr(Y), max(q, 1), int(fpe), int(bool(early_exit))), "exbgemm")
    return Y


def exbtrsm(T, B, uplo="U", trans="N", diag="N", alpha=1.0, fpe=8, early_exit=True):  # noqa: N803
    """ExBTRSM on host arrays: T float64 of shape (p, p), C- or Fortran-ordered (anything else is copied to C order; `uplo`
    names the triangle of T[i, j]), B float64 of shape (n, p); returns the solution of X op(T) = alpha B (a new n x p
    float64 array; B is not changed)."""
    T = _dense_host("exbtrsm", "T", T, 2)
    if not (T.flags.c_contiguous or T.flags.f_contiguous):
        T = np.ascontiguousarray(T)
    u, t, d, p, ldt = _btrsm_triangle(T, T.shape, _HostStrides(T), uplo, trans, diag)
    B = _dense_host("exbtrsm", "B", B, 2, " (n x p, one row per system; for one vector use extrsv)")
    if B.shape[1] != p:
        raise ValueError(f"exbtrsm: B must have p = {p} columns, not {B.shape[1]}")
    fpe = _fpe_0_to_8("exbtrsm", fpe)
    X = np.array(B, dtype=np.float64, copy=True, order="C")
    n = int(X.shape[0])
    _require_gpu()
    _check(load_library().exblas_exbtrsm(u, t, d, n, p, float(alpha), _hptr(T), ldt, _hptr(X), max(p, 1), fpe,
                                         int(bool(early_exit))), "exbtrsm")
    return X


def expotrf(G, uplo="U", fpe=8, early_exit=True):  # noqa: N803
    """ExPOTRF on a host array: G float64 of shape (p, p), C- or Fortran-ordered (anything else is copied to C order;
    `uplo` names the triangle of G[i, j]); returns (R, info): a new array with the factor in that triangle (the other
    triangle as it was in G; G is not changed) and the info word as an int."""
    G = _dense_host("expotrf", "G", G, 2)
    R = np.array(G, dtype=np.float64, copy=True, order="F" if (G.flags.f_contiguous and not G.flags.c_contiguous) else "C")
    u, p, ldg = _potrf_triangle(R.shape, _HostStrides(R), uplo)
    fpe = _fpe_0_to_8("expotrf", fpe)
    info = C.c_int32(0)
    _require_gpu()
    _check(load_library().exblas_expotrf(u, p, _hptr(R), ldg, C.byref(info), fpe, int(bool(early_exit))), "expotrf")
    return R, int(info.value)


def _batched_host(who, name, a):
    """the 3-D operand `name` of a host batched routine as an array whose matrices are C- or Fortran-ordered and packed
    (anything else is copied to C order); always a copy"""
    a = _dense_host(who, name, a, 3)
    at = a.transpose(0, 2, 1)
    if at.flags.c_contiguous and not a.flags.c_contiguous:   # every matrix Fortran-ordered: the copy keeps that
        return np.array(at, dtype=np.float64, copy=True, order="C").transpose(0, 2, 1)
    return np.array(a, dtype=np.float64, copy=True, order="C")


def expotrf_batched(G, uplo="U", fpe=8, early_exit=True):  # noqa: N803
    """Batched ExPOTRF on a host array: G float64 of shape (batch, p, p), every matrix C-ordered, or Fortran-ordered as
    np.transpose of a C-ordered batch gives it (anything else is copied to C order; `uplo` names the triangle of
    G[b, i, j]); returns (R, info): a new array with the factors in that triangle (the other triangle as it was in G; G is
    not changed) and the batch info words as an int32 array."""
    R = _batched_host("expotrf_batched", "G", G)
    u, batch, p, ldg, stride = _batched_triangles("expotrf_batched", "G", R.shape, _HostStrides(R), uplo)
    fpe = _fpe_0_to_8("expotrf_batched", fpe)
    info = np.zeros(batch, dtype=np.int32)
    _require_gpu()
    _check(load_library().exblas_expotrf_batched(u, p, batch, _hptr(R), ldg, stride, _hptr(info), fpe,
                                                 int(bool(early_exit))), "expotrf_batched")
    return R, info


def expotrs_batched(R, B, uplo="U", sweep="B", fpe=8, early_exit=True):  # noqa: N803
    """Batched ExPOTRS on host arrays: R float64 of shape (ceil(n / p), p, p) as expotrf_batched returns it, B float64 of
    shape (n, k); returns the solution (a new n x k float64 array; B is not changed)."""
    R = _batched_host("expotrs_batched", "R", R)
    u, batch, p, ldr, stride = _batched_triangles("expotrs_batched", "R", R.shape, _HostStrides(R), uplo)
    s = _potrs_sweep(sweep)
    B = _dense_host("expotrs_batched", "B", B, 2, " (n x k, one column per right-hand side)")
    X = np.array(B, dtype=np.float64, copy=True, order="C")
    n, k = int(X.shape[0]), int(X.shape[1])
    _batched_blocks("expotrs_batched", "R", n, p, batch)
    fpe = _fpe_0_to_8("expotrs_batched", fpe)
    _require_gpu()
    _check(load_library().exblas_expotrs_batched(u, s, p, n, k, _hptr(R), ldr, stride, _hptr(X), max(k, 1), fpe,
                                                 int(bool(early_exit))), "expotrs_batched")
    return X


def exgetrf_batched(A, fpe=8, early_exit=True):  # noqa: N803
    """Batched ExGETRF on a host array: A float64 of shape (batch, p, p), every matrix C-ordered, or Fortran-ordered as
    np.transpose of a C-ordered batch gives it (anything else is copied to C order); returns (LU, ipiv, info): a new array
    with L and U in LAPACK's storage (A is not changed), the 1-based pivots as an int32 array (batch, p) and the batch
    info words as an int32 array."""
    LU = _batched_host("exgetrf_batched", "A", A)
    order, batch, p, lda, stride = _batched_matrices("exgetrf_batched", "A", LU.shape, _HostStrides(LU))
    fpe = _fpe_0_to_8("exgetrf_batched", fpe)
    ipiv = np.zeros((batch, p), dtype=np.int32)
    info = np.zeros(batch, dtype=np.int32)
    _require_gpu()
    _check(load_library().exblas_exgetrf_batched(order, p, batch, _hptr(LU), lda, stride, _hptr(ipiv), _hptr(info), fpe,
                                                 int(bool(early_exit))), "exgetrf_batched")
    return LU, ipiv, info


def exgetrs_batched(LU, ipiv, B, fpe=8, early_exit=True):  # noqa: N803
    """Batched ExGETRS on host arrays: LU float64 of shape (ceil(n / p), p, p) and ipiv int32 of shape (ceil(n / p), p) as
    exgetrf_batched returns them, B float64 of shape (n, k); returns the solution (a new n x k float64 array; B is not
    changed)."""
    LU = _batched_host("exgetrs_batched", "LU", LU)
    order, batch, p, ldlu, stride = _batched_matrices("exgetrs_batched", "LU", LU.shape, _HostStrides(LU))
    ipiv = np.asarray(ipiv)
    if ipiv.dtype != np.int32 or ipiv.shape != (batch, p):
        raise ValueError(f"exgetrs_batched: ipiv must be an int32 array of shape (batch, p) = ({batch}, {p})")
    ipiv = np.ascontiguousarray(ipiv)
    B = _dense_host("exgetrs_batched", "B", B, 2, " (n x k, one column per right-hand side)")
    X = np.array(B, dtype=np.float64, copy=True, order="C")
    n, k = int(X.shape[0]), int(X.shape[1])
    _batched_blocks("exgetrs_batched", "LU", n, p, batch)
    fpe = _fpe_0_to_8("exgetrs_batched", fpe)
    _require_gpu()
    _check(load_library().exblas_exgetrs_batched(order, p, n, k, _hptr(LU), ldlu, stride, _hptr(ipiv), _hptr(X), max(k, 1),
                                                 fpe, int(bool(early_exit))), "exgetrs_batched")
    return X


from .dist import (Comm, exsum_allreduce, exdot_allreduce, allreduce_finish, allreduce_record,  # noqa: E402,F401
                   shard_range, row_block, exgemv_sharded, exgemm_sharded, exsum_allreduce_pipelined,
                   exdot_allreduce_pipelined, pipeline_drain, exbdot_allreduce)
