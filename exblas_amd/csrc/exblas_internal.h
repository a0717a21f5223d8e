// exblas_internal.h -- per-device context and cross-file declarations of libexblas.so
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <type_traits>
#include <vector>

namespace exb {

// The knobs a new context inherits: the environment sets them for layer 0, the exblas_set_* calls for every context of
// the device that exists, and a context created later (a host-layer context, a handle) takes layer 0's with one
// assignment of this struct (capi.hip: init_ctx).  A knob declared here is inherited; nothing else has to be edited.
struct CtxKnobs {
    int blocks_per_cu = 8;   // EXBLAS_BLOCKS_PER_CU: generic cap of resident blocks per CU
    // Measured on MI355X (tools/tune.py, n = 2^28): the one-stream ExSUM kernel is fastest with FEW fat
    // blocks (2 per CU: 7.15 TB/s vs 6.46 at 8), the two-stream ExDOT kernel with many (16-32 per CU).
    int bpc_sum = 2, bpc_dot = 48;   // ExDOT: 48 (an odd grid of 12289 workgroups) edges out 32 by ~1 %, 16 and 96 lose 2-3 %
    int bpc_sa = 3;          // superaccumulator-only ExSUM (LDS-atomic bound; 3/CU: 6.65 TB/s, 2/CU: 6.0)
    // The narrow-input kernels (blas1_lowp.hip; EXBLAS_BPC_LP_SUM / EXBLAS_BPC_LP_DOT; exblas_set_tuning sets them too).
    // Measured at n = 2^28 (tools/bench_lowp.py --sweep, profiles/lowp_sweep.jsonl): they convert and run the cascade on
    // 2 to 4 times the elements per byte, so they want more waves than the fp64 kernels -- ExSUM float32 0.193 ms at 2 per
    // CU, 0.176 at 8 to 16, 0.179 from 24 on; bfloat16 0.181 / 0.154 / 0.156; ExDOT float32 0.354 at 4, 0.321 at 16 to 32,
    // float16 0.217 / 0.193 to 0.196 at 8 to 16 / 0.200 at 48
    int bpc_lp_sum = 16, bpc_lp_dot = 16;
    int bpc_heavy = 4;       // ExSUM variants without early exit, N >= 5, in -DEXBLAS_FULL_CASCADE=1 builds only (VALU-latency-bound)
    int ngroups = 32;        // EXBLAS_NGROUPS: global group accumulators the blocks add into
    int grid_adj = 0;        // EXBLAS_GRID_ADJ: workgroups added to the grid of the streaming ExSUM / ExDOT kernels
    int gemm_path = 0;       // 0: int8 matrix cores when the data qualifies (decided on the device) -- residues modulo
                             // 8-bit moduli for min(m, n) >= 192, base-256 digit slices below; 2: digit slices always;
                             // 4: residues always; 1: scalar kernel only; 3: fp64 slices on MFMA-F64 (host-decided)
    int gemm_max_slices = 0; // 0 = default (16): digits per operand the int8 path reserves workspace for
    int gemm_max_moduli = 0; // 0 = default (39): moduli the residue path reserves workspace for
    int spmv_path = 0;       // exblas_set_spmv_path: 0 automatic, 1 accumulator finish for every row, 2 in-register
                             // rounding wherever certified (no row split), 3 every row split at a small chunk
    int spmm_path = 0;       // exblas_set_spmm_path: 0 automatic, 1 every output rounded from an integer accumulator,
                             // 2 in-register rounding wherever certified (no row split), 3 every row split at a small chunk
    int sptrsv_path = 0;     // exblas_set_sptrsv_path: 0 automatic, 1 every row rounded from its integer accumulator,
                             // 2 every row in the one-row-per-wave form
    int spilu0_path = 0;     // exblas_set_spilu0_path: 0 automatic, 1 every rounding from the wave's integer accumulator,
                             // 2 every row in the several-entries-per-lane form
    int spic0_path = 0;      // exblas_set_spic0_path: 0 automatic, 1 every rounding from the wave's integer accumulator,
                             // 2 every row in the several-entries-per-lane form
    int sptrsm_path = 0;     // exblas_set_sptrsm_path: 0 automatic, 1 every output rounded from the accumulator, 2 one row
                             // per item, 3 column panels and tiles of 4 columns
    int trsm_path = 0;       // exblas_set_trsm_path: 0 automatic, 1 every output rounded from the accumulator, 2 one row
                             // per item, 3 column panels and tiles of 4 columns
    int bgemm_path = 0;      // exblas_set_bgemm_path: 0 automatic, 1 every output rounded from the accumulator, 2 a register
                             // block of one row, 3 column tiles of 4 and chunks of 4 rows of C
    int btrsm_path = 0;      // exblas_set_btrsm_path: 0 automatic, 1 every output rounded from the accumulator, 2 a register
                             // block of one column, 3 4 rows per wave item and chunks of 4 rows and columns of T
    int potrf_path = 0;      // exblas_set_potrf_path: 0 automatic, 1 every output rounded from the accumulator, 2 a register
                             // block of one row, 3 column tiles of 4 and no staging in LDS
    int potrf_batched_path = 0;   // exblas_set_potrf_batched_path: 0 automatic, 1 every output rounded from the accumulator,
                                  // 2 one matrix per wave, 3 one matrix per workgroup item and a handful of workgroups
    int potrs_batched_path = 0;   // exblas_set_potrs_batched_path: 0 automatic, 1 every output rounded from the accumulator,
                                  // 2 one block per wave, 3 column tiles of 4
    int getrf_batched_path = 0;   // exblas_set_getrf_batched_path: 0 automatic, 1 every output rounded from the accumulator,
                                  // 2 one matrix per wave, 3 one matrix per workgroup item and a handful of workgroups
    int getrs_batched_path = 0;   // exblas_set_getrs_batched_path: 0 automatic, 1 every output rounded from the accumulator,
                                  // 2 one block per wave, 3 column tiles of 4
    int bdot_path = 0;       // exblas_set_bdot_path: 0 automatic, 1 the smallest row slab, 2 column panels and output tiles
                             // of width 4
};

// The counter slots a block routine's kernel left in the workspace (block_common.hip.h): a pair per workgroup
struct SlotInfo {
    const long long *dev = nullptr;   // nullptr: the call launched nothing
    int blocks = 0;                   // how many workgroups there were
};

// The pointers of a context that point INTO its workspace block (Ctx::ws): exblas_release_workspace resets this struct
// whole when it frees the block, so a pointer declared here is forgotten with it; nothing else has to be edited.
// Known wart, left as it is: the block is shared, so a last_*_info query after a DIFFERENT routine has reused the
// workspace reads that routine's header through the older pointer.
struct CtxWsPtrs {
    // which ExGEMM implementation the last call used.  The int8 path decides on the device: gemm_info_dev then points
    // at its info block (read lazily, with a synchronisation, by exblas_last_gemm_info); otherwise the host knows
    // (Ctx::last_gemm_slices).
    const int *gemm_info_dev = nullptr;
    const long long *spmv_info_dev = nullptr;    // header of the last ExSpMV call's workspace (exblas_last_spmv_info)
    const long long *spmm_info_dev = nullptr;    // header of the last ExSpMM call's workspace (exblas_last_spmm_info)
    const long long *sptrsv_info_dev = nullptr;  // header of the last ExSpTRSV call's workspace (nullptr: it launched nothing)
    const long long *spilu0_info_dev = nullptr;  // header of the last ExSpILU0 call's workspace (nullptr: it launched nothing)
    int spilu0_m = -1;                           // ... and what its mailbox was sized for: a call that is being captured
    long long spilu0_nnz = 0;                    // cannot read row_ptr[m] and takes these (spilu0.hip)
    const long long *spic0_info_dev = nullptr;   // the same for the last ExSpIC0 call (spic0.hip)
    int spic0_m = -1;
    long long spic0_nnz = 0;
    const long long *sptrsm_info_dev = nullptr;  // header of the last ExSpTRSM call's workspace (nullptr: it launched nothing)
    const long long *trsm_info_dev = nullptr;    // header of the last ExTRSM call's workspace (nullptr: it launched nothing)
    SlotInfo bgemm_slots, btrsm_slots, potrf_slots;   // of the last ExBGEMM, ExBTRSM and ExPOTRF (one workgroup) call
    SlotInfo potrf_batched_slots, potrs_batched_slots;   // of the last batched ExPOTRF and batched ExPOTRS call
    SlotInfo getrf_batched_slots, getrs_batched_slots;   // of the last batched ExGETRF and batched ExGETRS call
};

// Lazily created, one per device.  Replaces the file-static kernel/buffer globals of the reference
// launchers (ExSUM.Launcher.cpp:16-36), which make the reference GPU library non re-entrant, and the
// per-call OpenCL context + JIT (gpu:ExSUM.cpp:86-209).
struct Ctx : CtxKnobs, CtxWsPtrs {
    int device = -1;
    int num_cu = 256;
    // when set, the NEXT streaming ExSUM / ExDOT launch carries this event as the completion signal of its own dispatch
    // packet (hipExtLaunchKernelGGL) and clears the field: no separate event packet follows the kernel in the queue
    // (comm.hip: pipelined_step)
    hipEvent_t launch_stop_event = nullptr;
    hipEvent_t launch_start_event = nullptr;
    int last_gemm_slices = 0;  // host-decided ExGEMM paths: 0 scalar kernel; 2..4: fp64-slice MFMA path with that many slices
    int gemm_ws_moduli = 0;  // moduli the last residue-path call actually reserved for (fewer after an out-of-memory retry)
    // the last streaming ExSUM / ExDOT launch of this context (exblas_last_blas1_info), written on the host when it
    // launches: kernel (BLAS1_K_*) and grid, both 0 before the first launch
    int last_blas1_kernel = 0, last_blas1_grid = 0;
    long long *gacc = nullptr;   // ACTIVE accumulator set: [ngroups][NL] int64, zero between calls
    unsigned *gflags = nullptr;  // non-finite input flags of the active set, zero between calls
    // two sets, so that the finalize of step i (side stream) can overlap the streaming kernel of step i+1
    // (exblas_set_accumulator_slot); single-stream callers never leave slot 0
    long long *gacc_all = nullptr;
    unsigned *gflags_all = nullptr;
    int slot = 0;
    // host-pointer API staging
    hipStream_t stream = nullptr;
    void *stage[3] = {nullptr, nullptr, nullptr};
    size_t stage_bytes[3] = {0, 0, 0};
    long long *d_record = nullptr;  // OUT_WORDS
    long long *h_record = nullptr;  // pinned
    // blas2/blas3 workspaces.  Growth never frees the old block (a hipGraph captured earlier may still replay into
    // it): it is parked in `retired` until exblas_release_retired_workspaces(); growth while the stream is being
    // captured is refused (hipErrorStreamCaptureUnsupported) -- reserve first (exblas_reserve_workspace).
    void *ws = nullptr;
    size_t ws_bytes = 0;
    std::vector<void *> retired;
    int layer = 0;      // 0: the *_dev layer's context, >= 1: a private context of the host-pointer layer
    std::mutex mu;      // guards launches that touch the context workspace
};

// layer 0: context of the device-pointer (*_dev) entry points; layers 1..: the host-pointer API's own contexts (own
// accumulators, flags, workspace, stream; one per "virtual device" a host call spreads its data over), so that a
// host call can never touch state an in-flight *_dev call uses
constexpr int MAX_LAYERS = 9;
Ctx &ctx(int device, int layer = 0);
void *stage_buf(Ctx &c, int slot, size_t bytes);
// nullptr + *err set when the block would have to grow while `st` is being captured into a graph
void *workspace(Ctx &c, size_t bytes, hipStream_t st, hipError_t *err);
[[noreturn]] void die(const char *what, hipError_t e, const char *file, int line);

#define EXB_CHECK(expr)                                          \
    do {                                                         \
        hipError_t _e = (expr);                                  \
        if (_e != hipSuccess) exb::die(#expr, _e, __FILE__, __LINE__); \
    } while (0)

// The reference's (fpe, early_exit) -> kernel-variant rule, shared by every routine (gpu:ExSUM.cpp:64-84,
// ExDOT.cpp:69-98, ExGEMV.cpp:81-107, ExGEMM.cpp:78-99, ExTRSV.cpp:70-123).  For fpe >= MIN_N, calls
// f(std::integral_constant<int, N>, std::bool_constant<EE>) with the expansion size N and early-exit flag EE of the
// variant and returns true; returns false without calling f where the reference has no variant.
//  - early exit: the sizes fall into the buckets 4 / 6 / 8; with fpe > 8 the reference silently does nothing
//    (gpu:ExSUM.cpp:72-83, ExGEMV.cpp:96-106, ExGEMM.cpp:88-99).
//  - no early exit: every size up to 8 has its own instantiation.  Above 8 the reference builds its *.FPE.cl with
//    -DNBFPE=fpe (gpu:ExSUM.cpp:80-81, ExDOT.cpp:93-94, ExGEMV.cpp:103-104, ExGEMM.cpp:96-97); the exact result does not
//    depend on the expansion size, so the largest instantiation returns the same bits.
// What a routine does below MIN_N (superaccumulators only, the plain kernels of fpe == 1) and what "no variant" means
// to its caller stay at the call site.  MIN_N is 2 or 3; sizes below it are not instantiated.
template <int MIN_N, class F>
bool select_variant(int fpe, int early_exit, F &&f)
{
    static_assert(MIN_N == 2 || MIN_N == 3, "expansion sizes start at 2 (sum, gemv, trsv) or 3 (dot, gemm)");
    using std::false_type;
    using std::integral_constant;
    using std::true_type;
    if (early_exit) {
        if (fpe <= 4) f(integral_constant<int, 4>(), true_type());
        else if (fpe <= 6) f(integral_constant<int, 6>(), true_type());
        else if (fpe <= 8) f(integral_constant<int, 8>(), true_type());
        else return false;
        return true;
    }
    switch (fpe) {
    case 2:
        if constexpr (MIN_N <= 2) f(integral_constant<int, 2>(), false_type());
        break;
    case 3: f(integral_constant<int, 3>(), false_type()); break;
    case 4: f(integral_constant<int, 4>(), false_type()); break;
    case 5: f(integral_constant<int, 5>(), false_type()); break;
    case 6: f(integral_constant<int, 6>(), false_type()); break;
    case 7: f(integral_constant<int, 7>(), false_type()); break;
    default: f(integral_constant<int, 8>(), false_type()); break;
    }
    return true;
}

struct GemmChunks;

// blas1.hip
// Ctx::last_blas1_kernel: which streaming kernel the last ExSUM / ExDOT launch of the context was
enum {
    BLAS1_K_EXSUM = 1, BLAS1_K_EXSUM_STRIDED = 2, BLAS1_K_EXDOT = 3, BLAS1_K_EXDOT_STRIDED = 4,
    // blas1_lowp.hip: float32 / float16 / bfloat16 inputs
    BLAS1_K_EXSUM_LP = 5, BLAS1_K_EXSUM_LP_STRIDED = 6, BLAS1_K_EXDOT_LP = 7, BLAS1_K_EXDOT_LP_STRIDED = 8
};
hipError_t exsum_dispatch(Ctx &c, const double *a, long long n, long long inca, int fpe, int early_exit,
                          hipStream_t st);
hipError_t exdot_dispatch(Ctx &c, const double *a, long long inca, const double *b, long long incb, long long n,
                          int fpe, int early_exit, hipStream_t st);
hipError_t exsum_segmented_dispatch(const double *values, const long long *offsets, long long nseg, int fpe,
                                    int early_exit, int round_mode, hipStream_t st, double *out);
hipError_t finalize_groups(Ctx &c, hipStream_t st, long long *d_out, long long *d_ext_out = nullptr);
hipError_t finalize_sets(const long long *d_sets, int nsets, unsigned flags_or, hipStream_t st, long long *d_out,
                         const long long *d_ext_sets = nullptr);
// blas1_lowp.hip: dtype is DT_F32 / DT_F16 / DT_BF16 (round_lowp.hip.h) and fpe 0..8, both checked by the caller; the
// kernels add into the same accumulators as the fp64 ones.  round_records_dispatch: any of the four formats.
hipError_t exsum_lp_dispatch(Ctx &c, int dtype, const void *a, long long n, long long inca, int fpe, hipStream_t st);
hipError_t exdot_lp_dispatch(Ctx &c, int dtype, const void *a, long long inca, const void *b, long long incb, long long n,
                             int fpe, hipStream_t st);
hipError_t round_records_dispatch(const long long *d_records, long long count, long long stride_words, int dtype,
                                  void *d_out, hipStream_t st);
// the *_dev layer's context of the current device (comm.hip finishes its accumulators with exported low / high sets)
Ctx &default_ctx();

// blas2.hip / blas3.hip
hipError_t exgemv_dispatch(Ctx &c, char transa, int m, int n, double alpha, const double *a, int lda,
                           const double *x, int incx, double beta, double *y, int incy, int fpe, int early_exit,
                           int round_mode, hipStream_t st);
hipError_t exgemm_dispatch(Ctx &c, char transa, char transb, int m, int n, int k, double alpha, const double *a,
                           int lda, const double *b, int ldb, double beta, double *cmat, int ldc, int fpe,
                           int early_exit, int round_mode, hipStream_t st, const GemmChunks *chunks = nullptr);

// spmv.hip
hipError_t exspmv_dispatch(Ctx &c, int m, int n, int index_bits, const void *row_ptr, const void *col_idx,
                           const double *val, double alpha, const double *x, double beta, double *y, int fpe,
                           int early_exit, int round_mode, hipStream_t st);
// values of val_dtype (DT_F32 / DT_F16 / DT_BF16), x and y of vec_dtype (DT_F64 or val_dtype), fpe 0 or 2..8: all checked
// by the caller
hipError_t exspmv_lp_dispatch(Ctx &c, int m, int n, int index_bits, const void *row_ptr, const void *col_idx,
                              int val_dtype, const void *val, double alpha, int vec_dtype, const void *x, double beta,
                              void *y, int fpe, int round_mode, hipStream_t st);

// spmm.hip
hipError_t exspmm_dispatch(Ctx &c, int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx,
                           const double *val, double alpha, const double *x, long long ldx, double beta, double *y,
                           long long ldy, int fpe, int early_exit, int round_mode, hipStream_t st);
hipError_t exspmm_lp_dispatch(Ctx &c, int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx,
                              int val_dtype, const void *val, double alpha, int vec_dtype, const void *x, long long ldx,
                              double beta, void *y, long long ldy, int fpe, int round_mode, hipStream_t st);

// sptrsv.hip
hipError_t exsptrsv_dispatch(Ctx &c, char uplo, char diag, int m, int index_bits, const void *row_ptr, const void *col_idx,
                             const double *val, double *x, int fpe, int early_exit, int round_mode, hipStream_t st);

// spilu0.hip
hipError_t exspilu0_dispatch(Ctx &c, int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                             double *lu, long long *info, int fpe, int early_exit, int round_mode, hipStream_t st);

// spic0.hip
hipError_t exspic0_dispatch(Ctx &c, int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                            double *ll, long long *info, int fpe, int early_exit, int round_mode, hipStream_t st);

// sptrsm.hip
hipError_t exsptrsm_dispatch(Ctx &c, char uplo, char diag, int m, int k, int index_bits, const void *row_ptr,
                             const void *col_idx, const double *val, double *x, long long ldx, int fpe, int early_exit,
                             int round_mode, hipStream_t st);

// bdot.hip
hipError_t exbdot_dispatch(Ctx &c, char mode, long long n, int p, int q, const double *x, long long ldx, const double *y,
                           long long ldy, double *out, long long ldc, int fpe, int early_exit, int round_mode,
                           hipStream_t st);
// the row-sharded forms.  BdotMerge: the int64-sum all-reduce of one batch's exported sets (comm.hip), 0 or an error of
// the comm layer; the three below return that, or a hipError_t
struct BdotMerge {
    int (*allreduce)(void *user, long long *d_words, size_t count, hipStream_t st) = nullptr;
    void *user = nullptr;
};
int exbdot_export_dispatch(Ctx &c, char mode, long long n, int p, int q, const double *x, long long ldx, const double *y,
                           long long ldy, long long *d_sets, int fpe, int early_exit, hipStream_t st);
int exbdot_merge_dispatch(Ctx &c, char mode, long long n, int p, int q, const double *x, long long ldx, const double *y,
                          long long ldy, double *out, long long ldc, int fpe, int early_exit, int round_mode,
                          const BdotMerge *merge, hipStream_t st);
hipError_t exbdot_round_dispatch(char mode, int p, int q, const long long *d_sets, int nsets, double *out, long long ldc,
                                 int round_mode, hipStream_t st);
// capi.hip: exblas_exbdot_dev on the default context with the batches' sets summed by `merge` before they are rounded;
// everything that can be refused, and the silent return, is decided before the first merge call
int exbdot_merged_dev(char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y, int64_t ldy,
                      double *d_c, int64_t ldc, int fpe, int early_exit, hipStream_t st, const BdotMerge *merge);

// trsv.hip
hipError_t extrsv_dispatch(Ctx &c, char uplo, char transa, char diag, int n, const double *a, int lda, double *x,
                           int incx, int fpe, int early_exit, int round_mode, hipStream_t st);

// trsm.hip
hipError_t extrsm_dispatch(Ctx &c, char uplo, char transa, char diag, int n, int k, const double *a, int lda, double *x,
                           long long ldx, int fpe, int early_exit, int round_mode, hipStream_t st);

// bgemm.hip
hipError_t exbgemm_dispatch(Ctx &c, long long n, int p, int q, double alpha, const double *x, long long ldx,
                            const double *cm, long long ldc, double beta, double *y, long long ldy, int fpe, int early_exit,
                            int round_mode, hipStream_t st);

// btrsm.hip
hipError_t exbtrsm_dispatch(Ctx &c, char uplo, char transt, char diag, long long n, int p, double alpha, const double *t,
                            int ldt, double *x, long long ldx, int fpe, int early_exit, int round_mode, hipStream_t st);

// potrf.hip
hipError_t expotrf_dispatch(Ctx &c, char uplo, int p, double *g, int ldg, int *info, int fpe, int early_exit, int round_mode,
                            hipStream_t st);

// potrf_batched.hip
hipError_t expotrf_batched_dispatch(Ctx &c, char uplo, int p, long long batch, double *g, int ldg, long long stride, int *info,
                                    int fpe, int early_exit, int round_mode, hipStream_t st);

// getrf_batched.hip
hipError_t exgetrf_batched_dispatch(Ctx &c, char order, int p, long long batch, double *a, int lda, long long stride, int *ipiv,
                                    int *info, int fpe, int early_exit, int round_mode, hipStream_t st);

// bjacobi_apply.hip: the batched ExPOTRS and the batched ExGETRS, one kernel
hipError_t expotrs_batched_dispatch(Ctx &c, char uplo, char sweep, int p, long long n, int k, const double *r, int ldr,
                                    long long stride, double *x, long long ldx, int fpe, int early_exit, int round_mode,
                                    hipStream_t st);
hipError_t exgetrs_batched_dispatch(Ctx &c, char order, int p, long long n, int k, const double *lu, int ldlu, long long stride,
                                    const int *ipiv, double *x, long long ldx, int fpe, int early_exit, int round_mode,
                                    hipStream_t st);

// ExGEMM's info block: the words the operand scan and the device-side decisions of the int8 paths write into the
// workspace, and the values of INFO_PATH (= exblas_last_gemm_info out[0]; the fp64-slice path, 1, decides on the host)
enum {
    INFO_NEED_A = 0, INFO_NEED_B = 1, INFO_FLAGS = 2, INFO_EMIN = 3, INFO_EMAX = 4,   // the scan (blas3.hip)
    INFO_SA = 5, INFO_SB = 6, INFO_PATH = 7, INFO_BS = 8, INFO_EXACT = 9,           // digit slices (blas3_i8.hip)
    INFO_CRT_L = 10, INFO_CRT_NA = 11, INFO_CRT_NB = 12,                           // residues (blas3_crt.hip)
    INFO_WORDS = 16,
    PATH_SCALAR = 0, PATH_I8 = 2, PATH_CRT = 4
};

// blas3.hip: the operand scan of the three matrix-core paths.  EA heads the block EA | EB | LA | LB of 2 (m + n) ints
// (scale and lowest set bit per row of A' = fl(alpha A), then per column of B); info gets the scan's words.
void gemm_scan(hipStream_t st, int ta, int tb, int m, int n, int k, double alpha, const double *a, int lda, const double *b,
               int ldb, int *info, int *EA);

// blas3_i8.hip / blas3_crt.hip: the two int8 ExGEMM paths, each in two steps (whole operands, then rows of C).  The
// prepare of a path fills the plan and sets path when it has enqueued its work on the whole operands; the device may
// still leave the product to the scalar kernel (info[INFO_PATH]).
struct GemmPlan {
    int path = PATH_SCALAR;   // PATH_I8 or PATH_CRT: that path's rows function runs; PATH_SCALAR: nothing was enqueued
    int m = 0, n = 0, KC = 0;
    int *info = nullptr, *EA = nullptr, *EB = nullptr;
    signed char *PA = nullptr, *PB = nullptr;   // digit planes (residue path: one plane per modulus, of one row chunk of A')
    double beta = 0.0;
    double *c = nullptr;
    int ldc = 0, round_mode = 0;
    struct {
        int kpasses = 0, dblocks = 0, force_multi = 0, maybe_multi = 0;
        unsigned long long *W = nullptr;
    } i8;
    struct {   // A' is reduced row chunk by row chunk; R holds the residues of the chunk's rows of C
        unsigned *R = nullptr;
        size_t plane_a = 0, plane_b = 0;
        int lcap = 0, m4 = 0, num_cu = 256, chunk_rows = 0, lda = 0, ta = 0, k = 0;
        const double *a = nullptr;
        double alpha = 1.0;
    } crt;
};
hipError_t exgemm_i8_prepare(Ctx &c, char transa, char transb, int m, int n, int k, double alpha, const double *a, int lda,
                             const double *b, int ldb, double beta, double *cmat, int ldc, int round_mode,
                             hipStream_t st, GemmPlan *plan);
hipError_t exgemm_i8_rows(const GemmPlan &plan, int row0, int row1, hipStream_t st);
hipError_t exgemm_crt_prepare(Ctx &c, char transa, char transb, int m, int n, int k, double alpha, const double *a, int lda,
                              const double *b, int ldb, double beta, double *cmat, int ldc, int round_mode,
                              hipStream_t st, GemmPlan *plan);
hipError_t exgemm_crt_rows(const GemmPlan &plan, int row0, int row1, hipStream_t st);
hipError_t crt_tables_upload();  // into the current device's tables; context creation only
constexpr int CRT_MIN_EDGE = 192;  // gemm_path 0: the residue path serves products with min(m, n) >= this

// Row chunks of one exgemm call: the rows [bound[i], bound[i+1]) of C are finished (on the stream) when hook(user, i)
// is called; bound[0] = 0, bound[n] = m, inner bounds multiples of 64.  Used by the row-sharded GEMM (comm.hip) to
// ship finished rows while the next chunk is computed.
struct GemmChunks {
    int n = 1;
    int bound[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int (*hook)(void *user, int chunk, hipStream_t st) = nullptr;
    void *user = nullptr;
};
int exgemm_chunked_dev(char transa, char transb, int m, int n, int k, double alpha, const double *d_a, int lda,
                       const double *d_b, int ldb, double beta, double *d_c, int ldc, int fpe, int early_exit,
                       hipStream_t st, const GemmChunks *chunks);
// blas3_mfma.hip: the fp64-slice path; *slices = the slice count it ran with (0: it did not)
bool exgemm_try_mfma(Ctx &c, char transa, char transb, int m, int n, int k, double alpha, const double *a, int lda,
                     const double *b, int ldb, double beta, double *cmat, int ldc, hipStream_t st, hipError_t *err,
                     int *slices);

int round_mode();

}  // namespace exb
