/*
 * exblas_hip.h -- C ABI of libexblas.so, the MI355X (gfx950) replacement for the reference's
 * OpenCL backend (src/gpu of nikolovjovan/exblas).  Plain pointers and sizes only.
 *
 * Two layers:
 *  (1) host-pointer entry points with exactly the argument meaning of the reference's public C++
 *      API (include/blas1.hpp:48,74; blas2.hpp:57,95; blas3.hpp:56) -- what its tests and examples call;
 *      the C++ overloads themselves (exsum/exdot/extrsv/exgemv/exgemm, global namespace) are declared in
 *      include/blas1.hpp, blas2.hpp, blas3.hpp of this repository and exported by the same library.
 *  (2) device-pointer, stream-ordered entry points underneath: what the reference's launcher layer
 *      (extern "C" initEx* / Ex* / closeEx* on cl_mem, src/gpu/blas/blas1/ExSUM.Launcher.hpp,
 *      ExDOT.Launcher.hpp, blas2/ExGEMV.Launcher.hpp, blas3/ExGEMM.Launcher.hpp) is to OpenCL.
 *      These keep data resident in HBM and are what bench.py and the multi-GPU path drive.
 *
 * Error behaviour mirrors the reference: no error channel in the BLAS-style calls;
 * fpe < 0 or a HIP failure prints to stderr and exit(EXIT_FAILURE)s (cpu:ExSUM.cpp:25-28,
 * gpu:ExSUM.cpp:111-115); Ng <= 0 returns 0.0 (ExDOT.cpp:70-71).  The *_dev functions return a
 * hipError_t-compatible int instead of exiting (0 = success).
 *
 * Concurrency: the host-pointer layer may be called from any number of threads (calls on one device are
 * serialised; the reference's GPU library is not re-entrant at all, ExSUM.Launcher.cpp:16-36).  It owns a PRIVATE
 * context per device -- its own group accumulators, flags, workspace, staging buffers and stream -- so a host call
 * never touches state an in-flight *_dev call uses, and vice versa: the two layers may be mixed freely.
 * The *_dev layer keeps ONE set of group accumulators and ONE workspace per device (two accumulator slots, see
 * exblas_set_accumulator_slot): its calls may come from any thread, but the work they enqueue must be ordered on
 * the device -- one stream, or streams chained by events -- exactly like kernels sharing a scratch buffer.
 * Callers with several independent streams create one CONTEXT HANDLE per stream (exblas_ctx_create) and use the *_ctx
 * entry points: every handle owns its accumulators, flags and workspace, so work enqueued through different handles
 * may run concurrently in any order.
 * Workspace and hipGraphs: exgemv / exgemm / extrsv use a context workspace whose size depends on the problem.  It
 * only grows; a block it outgrows is parked (not freed) so that graphs captured earlier stay valid until
 * exblas_release_retired_workspaces().  Growth needs hipMalloc, which is illegal while a stream is being captured:
 * a call that would have to grow during capture fails with hipErrorStreamCaptureUnsupported (900) -- make the same
 * call once before capturing, or exblas_reserve_workspace().  Every *_dev entry point is a pure sequence of
 * stream-ordered launches: no host synchronisation, no device-to-host read, capturable.
 *
 * Rounding: EXBLAS_ROUND=exact (default; correctly rounded = the MPFR oracle of
 * tests/test.exsum.gpu.cpp:23-38) or EXBLAS_ROUND=reference (bug-compatible with
 * Superaccumulator::Round, superaccumulator.cpp:80-134).  The limbs are identical in both.
 */
#ifndef EXBLAS_HIP_H_
#define EXBLAS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* result record written by every *_dev reduction: EXBLAS_OUT_WORDS int64 words */
#define EXBLAS_OUT_WORDS 128
#define EXBLAS_OUT_EXACT 0    /* bit pattern of the correctly rounded double */
#define EXBLAS_OUT_REFMODE 1  /* bit pattern of the reference-compatible rounding */
#define EXBLAS_OUT_FLAGS 2    /* bit0 +inf, bit1 -inf, bit2 NaN seen in the input.  ExDOT also:
                               * bit3 (PRODUCT_UNDERFLOW) = a product of two non-zero operands was below 2^-968, i.e. had bits
                               *   below 2^-1074, the last place of the double-range accumulator;
                               * bit4 (PRODUCT_OVERFLOW) = a product of two FINITE operands was 2^1024 or more (+-Inf as a double);
                               * bit5 (PRODUCT_LOW_EXACT, with bit3) / bit6 (PRODUCT_HIGH_EXACT, with bit4) = those products lost
                               *   nothing: each was formed again at a scaled exponent (error-free) and summed in a second (LOW)
                               *   resp. third (HIGH) accumulator that the finalize kernel folded back -- the high one exactly,
                               *   1216 bits up; the low one exactly where it reaches 2^-1074 and as the half / sticky bits of
                               *   the rounding below -- so the result is the correctly rounded EXACT dot product: finite where
                               *   overflowing products cancel (IEEE arithmetic and the reference's kernels give Inf - Inf =
                               *   NaN there), +-Inf where the exact sum is beyond the double range (if it is also beyond the
                               *   record's digits, 2^1101, bit0 / bit1 is set as for an infinity in the input and the digit
                               *   fields are meaningless).  The library's multi-rank calls all-reduce the low and high digit
                               *   sets beside the main one (a host-pointer exdot spread over several devices adds them on the
                               *   host), so this holds for every rank / device count.  Bit3 / bit4 WITHOUT bit5 / bit6 only
                               *   arises from exblas_finalize_dev on user-held digit sets, which has no such sets, and means:
                               *   the correctly rounded sum of the sets' values, each truncated at 2^-1074 resp. saturated.
                               * Whatever the bits (3..6), a result of a single call or of the library's multi-rank calls is
                               * the MPFR-4196 value of tests/test.exdot.gpu.cpp:24-46.  The reference's kernels have both
                               * limits, silently. */
#define EXBLAS_FLAG_PRODUCT_UNDERFLOW 8
#define EXBLAS_FLAG_PRODUCT_OVERFLOW 16
#define EXBLAS_FLAG_PRODUCT_LOW_EXACT 32
#define EXBLAS_FLAG_PRODUCT_HIGH_EXACT 64
#define EXBLAS_OUT_CANON 4    /* 41 canonical limbs (52-bit, reference geometry) */
#define EXBLAS_OUT_DIGITS 48  /* 68 normalised 32-bit digits, then 3 flag indicators + 1 pad word: */
#define EXBLAS_SET_WORDS 72   /* words [48,120) = one "digit set", the int64-sum all-reduce payload */
#define EXBLAS_NDIGITS 68
#define EXBLAS_NCANON 41

/* generator kinds for exblas_gen_dev (restating the distributions of src/common/common.cpp) */
#define EXBLAS_GEN_NAIVE 0
#define EXBLAS_GEN_FPUNIFORM 1
#define EXBLAS_GEN_LOGNORMAL 2
#define EXBLAS_GEN_ILLCOND 3
#define EXBLAS_GEN_CANCEL 4
#define EXBLAS_GEN_FPUNIFORM_SIGNED 5

/* ---- context ------------------------------------------------------------------------------ */
/* Lazily creates the per-device context (workspace, CU count).  device < 0: current device.
 * Replaces the per-call OpenCL platform/context/queue/JIT of gpu:ExSUM.cpp:86-209. */
int exblas_hip_init(int device);
int exblas_hip_device_count(void);
const char *exblas_hip_version(void);
/* Launch-geometry knobs for A/B measurements (<= 0 leaves a value unchanged): resident blocks per CU of the
 * streaming kernels, number of global group accumulators.  variant must be -1 or 0 (the library builds one kernel
 * per configuration; candidates are A/B'd as separate builds); any other value returns hipErrorInvalidValue and
 * changes nothing. */
int exblas_set_tuning(int blocks_per_cu, int ngroups, int variant);
/* ExGEMM implementation.  0 (default): error-free integer arithmetic on the int8 matrix cores
 * (v_mfma_i32_32x32x32_i8) for every (fpe, early_exit) variant and both rounding modes whenever the data qualifies --
 * decided on the device, the scalar kernel runs otherwise.  Products with min(m, n) >= 192 use residues modulo
 * pairwise coprime 8-bit moduli (one int8 GEMM per modulus, Chinese-remainder reconstruction: blas3_crt.hip), smaller
 * ones base-256 digit slices (all digit pairs: blas3_i8.hip); 4 = residues always, 2 = digit slices always;
 * 1 = scalar kernel only (TwoProd + expansions + one superaccumulator per output, the reference's own scheme);
 * 3 = error-free 21-bit slices on MFMA-F64 (v_mfma_f64_16x16x4_f64; host-decided: synchronises the stream,
 * exact-rounding mode only).  Same bits on every path. */
void exblas_set_gemm_path(int mode);
/* digits per operand the digit-slice path may use (workspace: that many bytes per matrix entry); 0 = default 16 */
void exblas_set_gemm_max_slices(int s);
/* moduli the residue path may use (workspace: that many bytes per entry of B and of a 2048-row chunk of A and C);
 * 0 = default 39 = every input the path accepts (126 bits per operand).  When the reservation fails the call retries with
 * 24, 18 and 12 moduli (data that needs more then takes the scalar kernel), then with the digit-slice workspace. */
void exblas_set_gemm_max_moduli(int l);
/* Which implementation the last exgemm on this device used: out[0] = 0 scalar kernel / 1 fp64 slices / 2 int8 digit
 * slices / 4 int8 residues.  Slices: out[1], out[2] = slices of A, B (out[1]*out[2] matrix multiply-adds per element
 * pair).  Residues: out[1], out[2] = bits of the fixed-point entries of A, B; out[3] = moduli (= matrix multiply-adds
 * per element pair); out[4] = moduli the workspace was reserved for (39, fewer after an out-of-memory retry).  Synchronises the device when the decision was taken there.  exblas_last_gemm_slices() =
 * max(out[1], out[2]) for the slice paths, out[3] for residues, 0 for the scalar kernel. */
int exblas_last_gemm_info(int *out8);
/* The most recent streaming ExSUM / ExDOT launch of this device's default context (the *_dev entry points and
 * exblas_*_ctx with a NULL handle): out[0] = kernel (1 contiguous ExSUM, 2 strided ExSUM, 3 contiguous 16-byte-aligned
 * ExDOT, 4 strided or misaligned ExDOT; the narrow-input kernels: 5 contiguous ExSUM, 6 strided ExSUM, 7 vector ExDOT
 * (both operands equally misaligned modulo 16 bytes), 8 strided or unequally misaligned ExDOT; 0 nothing launched
 * yet), out[1] = workgroups launched, out[2] = group
 * accumulators (EXBLAS_NGROUPS / exblas_set_tuning), out[3] = compute units the geometry is sized for, out[4..7] = 0.
 * Recorded on the host at launch: no synchronisation, nothing read from the device.  For tests and tuning tools that
 * must know which launch geometry a size took.  Returns 0 or hipErrorInvalidValue (out8 NULL). */
int exblas_last_blas1_info(int *out8);
/* CPU-only self-test of the residue path's constant tables and reconstruction formulas: `cases` random integers per
 * modulus count through a host mirror of the device arithmetic; returns the number of failures (0 = pass). */
int exblas_crt_selftest(int cases, unsigned seed);
int exblas_last_gemm_slices(void);
/* Makes the *_dev layer's workspace at least `bytes` large (see "Workspace and hipGraphs" above).  A request that cannot
 * be met returns the hipError_t and leaves the current workspace (and the parked blocks) exactly as they were. */
int exblas_reserve_workspace(size_t bytes);
/* Bytes the *_dev layer's workspace holds right now on the current device (the parked blocks not included).  Footprint of
 * the residue path of exgemm: 39 bytes per entry of B, of a 2048-row chunk of A and of a 2048-row chunk of C --
 * 8192^3: 3.7 GiB, 16384^3: 12.2 GiB; the digit-slice path: 16 bytes per entry of A and B (+ 40 per entry of C when more
 * than one pass can be needed).  ExSpMM: 1024 + 4 m + 8 ceil(m / r) t + 12 L + 576 k L bytes (each term rounded up to 256),
 * r = 64 / min(64, k rounded up to a power of two) rows per wave, t = ceil(k / 64) column tiles (one bitmap word per 64
 * outputs), L = min(m, floor(32 MiB / (576 k))) accumulator slots for split rows: at most 32 MiB whatever k is; rows
 * past L run whole.  ExSpTRSV: 256 + 8 m bytes (the header and the mailbox of m doubles).  ExSpTRSM: 256 + 8 m min(k, P)
 * bytes (the header and the mailbox of one column panel), P = max(64, 64 floor(EXBLAS_SPTRSM_MAILBOX_BYTES / (8 m) / 64))
 * columns per panel: at most 64 MiB (EXBLAS_SPTRSM_MAILBOX_BYTES) unless 512 m exceeds it.  ExTRSM: 256 + 8 n min(k, P)
 * bytes likewise, P = max(64, 64 floor(EXBLAS_TRSM_MAILBOX_BYTES / (8 n) / 64)) (the same 64 MiB).  ExBDOT:
 * EXBLAS_BDOT_WORKSPACE_BYTES (2.25 MiB: 4096 accumulator sets of 576 bytes) whatever n, p and q are. */
size_t exblas_workspace_bytes(void);
/* Frees the workspace blocks that later, larger calls replaced.  Synchronises the device; only call it when no graph
 * captured before the growth will be replayed again. */
int exblas_release_retired_workspaces(void);
/* Frees the current workspace as well (a large exgemm leaves gigabytes reserved: 39 bytes per entry of A, B and
 * 4-row group of C for the residue path).  Synchronises the device; graphs captured so far must not be replayed. */
int exblas_release_workspace(void);
/* 0 = exact, 1 = reference; overrides EXBLAS_ROUND for the host-pointer API */
void exblas_set_round_mode(int mode);
int exblas_get_round_mode(void);

/* ---- (2) device-pointer layer -------------------------------------------------------------- */
/* ExSUM over d_a[i*inca], i < n (offset already applied to the pointer).  Replaces
 * initExSUM/ExSUM/closeExSUM (ExSUM.Launcher.hpp) = kernels ExSUM + ExSUMComplete
 * (ExSUM.Superacc.cl:211-356, ExSUM.FPE.cl:230-388).  fpe/early_exit select the variant exactly
 * as gpu:ExSUM.cpp:64-84.  d_out: EXBLAS_OUT_WORDS int64 in device memory. */
int exblas_exsum_dev(const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                     void *stream, int64_t *d_out);
/* ExDOT.  Replaces initExDOT/ExDOT/closeExDOT (ExDOT.Launcher.hpp) = kernels ExDOT +
 * ExDOTComplete (ExDOT.Superacc.cl:217-359, ExDOT.FPE.cl:201-345); variants as ExDOT.cpp:69-98. */
int exblas_exdot_dev(const double *d_a, int64_t inca, const double *d_b, int64_t incb, int64_t n,
                     int fpe, int early_exit, void *stream, int64_t *d_out);
/* Segmented (batched) ExSUM: d_out[s] = correctly rounded sum of d_values[d_offsets[s] .. d_offsets[s+1]) for
 * s < nseg, all in one launch (one wavefront per segment).  The batched form of what the reference's examples do
 * with one exsum() call per CSR row (src/cpu/examples/spmv (Parboil)/StrongReproducibility/main.cpp:85).
 * Rounding mode as set by exblas_set_round_mode / EXBLAS_ROUND. */
int exblas_exsum_segmented_dev(const double *d_values, const int64_t *d_offsets, int64_t nseg, int fpe,
                               int early_exit, void *stream, double *d_out);
/* The two phases of the calls above, separately: *_accumulate_dev launches only the streaming kernel
 * and adds its result into the context's (zero-initialised) accumulators, so several arrays can be
 * folded into ONE exact sum; exblas_finish_dev carry-propagates, rounds, writes the record and
 * leaves the accumulators zero again.  bench.py brackets the streaming kernel with events this way.
 * Capacity: one reduction (everything between two exblas_finish_dev calls) may hold up to 2^36 values (each of the
 * 32 group accumulators takes 2^31 adds; the finalize sums them carry-safely); a single call takes n < 2^31 like
 * the reference API's `int Ng` -- larger n is rejected with an error. */
int exblas_exsum_accumulate_dev(const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                                void *stream);
int exblas_exdot_accumulate_dev(const double *d_a, int64_t inca, const double *d_b, int64_t incb,
                                int64_t n, int fpe, int early_exit, void *stream);
int exblas_finish_dev(void *stream, int64_t *d_out);
/* ---- narrow inputs: ExSUM / ExDOT on float32, float16 and bfloat16 arrays, and one rounding into a narrow format ----
 * dtype names the element type of d_a (and d_b: both operands of ExDOT have the same type); bfloat16 is the raw 16-bit
 * word (the upper half of a float32).  Every such value widens to a double exactly and the product of two of them is
 * an exact double, so these entries compute the same exact total as the fp64 entries on the widened data -- the same
 * 128-word record, every field with the same meaning, EXBLAS_OUT_EXACT still the correctly rounded DOUBLE -- while
 * reading the data at its own width, with no temporary.  Flag bits 3 to 6 are never set: a product of two narrow
 * values lies in [2^-298, 2^256) or is zero.  The kernels add into the same context accumulators as the fp64 ones: narrow
 * and fp64 *_accumulate calls between two exblas_finish_dev calls fold into ONE exact reduction, and the multi-rank
 * finish (exblas_allreduce_finish_dev) serves them unchanged.
 * fpe: 0 to 8.  0 and 1 run the superaccumulators alone, 2 to 4 an expansion of 4 and 5 to 8 an expansion of 8, both
 * with the per-tile early exit; early_exit is accepted for symmetry and changes nothing (the bits cannot depend on
 * either).  EXBLAS_DT_F64 forwards to the fp64 entry: the same record.  Refused with hipErrorInvalidValue (1) before the
 * device is touched: an unknown dtype, fpe outside 0..8, an increment < 1, n < 0, n >= 2^31, a pointer that is not a
 * multiple of the element size.  n == 0 launches nothing and yields the zero record.  The pointers need only be
 * element-aligned; ExDOT streams 16-byte vectors when d_a and d_b are equally misaligned modulo 16 bytes and takes
 * the (slower) strided kernel otherwise. */
#define EXBLAS_DT_F64 0
#define EXBLAS_DT_F32 1
#define EXBLAS_DT_F16 2
#define EXBLAS_DT_BF16 3
int exblas_exsum_lp_dev(int dtype, const void *d_a, int64_t n, int64_t inca, int fpe, int early_exit, void *stream,
                        int64_t *d_out);
int exblas_exdot_lp_dev(int dtype, const void *d_a, int64_t inca, const void *d_b, int64_t incb, int64_t n, int fpe,
                        int early_exit, void *stream, int64_t *d_out);
int exblas_exsum_lp_accumulate_dev(int dtype, const void *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                                   void *stream);
int exblas_exdot_lp_accumulate_dev(int dtype, const void *d_a, int64_t inca, const void *d_b, int64_t incb, int64_t n,
                                   int fpe, int early_exit, void *stream);
/* d_out[i] = the exact total of record i, rounded ONCE (to nearest, ties to even) into `dtype`: one element of that
 * format per record (8, 4 or 2 bytes), i < count; record i is the EXBLAS_OUT_WORDS words at d_records +
 * i * stride_words (stride_words >= EXBLAS_OUT_WORDS when count > 1).  A record whose flags word has one of bits 0 to 2
 * set yields its EXBLAS_OUT_EXACT double converted to the format (+-Inf and NaN convert exactly); every other record
 * yields the rounding of its 68 digits (words [48, 116)): subnormal results, the carry into the next binade and the
 * overflow to +-Inf (float16 from 65520 on, float32 / bfloat16 from 2^128 - 2^103 / 2^128 - 2^119 on) included; an
 * exact zero gives +0.  Rounding the record's double instead would round twice and go wrong on near-ties.  With
 * EXBLAS_DT_F64 the output equals word EXBLAS_OUT_EXACT.  Limit: a record that carries
 * EXBLAS_FLAG_PRODUCT_UNDERFLOW (an fp64 ExDOT) has a fraction below 2^-1074 that the digits do not hold; this routine
 * rounds the value of the digits.  Narrow-input reductions never set that bit.  Refused with hipErrorInvalidValue: an
 * unknown dtype, count < 0, a stride below EXBLAS_OUT_WORDS with count > 1, a NULL pointer with count > 0. */
int exblas_round_records_dev(const int64_t *d_records, int64_t count, int64_t stride_words, int dtype, void *d_out,
                             void *stream);
/* The same rounding of ONE digit set (68 normalised digits: digits 0..66 in [0, 2^32), the top one signed) on the CPU;
 * no device is touched.  *bits receives the pattern in its low 64 / 32 / 16 bits.  hipErrorInvalidValue for an unknown
 * dtype or a NULL pointer. */
int exblas_round_digits_host(const int64_t *digits68, int dtype, uint64_t *bits);
/* The context owns TWO accumulator sets.  *_accumulate_dev and exblas_finish_dev act on the selected one
 * (0 by default).  A caller that pipelines independent reductions alternates the slot per reduction and runs
 * exblas_finish_dev on a second stream (ordered by events), so that the finalize of reduction i overlaps the
 * streaming kernel of reduction i+1 (bench.py does).  Returns 0, or an error for a slot other than 0 / 1. */
int exblas_set_accumulator_slot(int slot);
/* Timing without packets of its own: the NEXT exblas_exsum_accumulate_dev / exblas_exdot_accumulate_dev on the current
 * device's default context attaches these hipEvent_t (either may be NULL) to the dispatch packet of its streaming kernel
 * (hipExtLaunchKernelGGL): they then carry the kernel's own start / stop timestamps -- what rocprofv3 reports for that
 * dispatch -- and no hipEventRecord barrier sits in the queue around the kernel.  Consumed by that one launch; a call that
 * launches nothing leaves them unrecorded and cleared.  bench.py's kernel_ms. */
int exblas_set_launch_events(void *ev_start, void *ev_stop);
/* Sum `nsets` digit sets (EXBLAS_SET_WORDS int64 each = words [48,120) of a record, e.g. the
 * all-reduced payloads of several GPUs), carry-propagate once and round: the "single global
 * carry-propagated normalise".  The sets need not be normalised: any words below 2^63 in magnitude are
 * accepted (it is the kernel that reads the raw group accumulators) as long as the sum of the top words
 * does and the total fits the 68 digits.  d_out may alias d_digit_sets - EXBLAS_OUT_DIGITS (in-place).
 * Plays the role of MPI_Reduce + Round in cpu:ExSUM.cpp:142-156. flags_or: OR of the ranks' flags. */
int exblas_finalize_dev(const int64_t *d_digit_sets, int nsets, uint32_t flags_or, void *stream,
                        int64_t *d_out);
/* ExGEMV on device pointers, column-major A (ExGEMV.Launcher.hpp; kernels gemv/gemvT,
 * ExGEMV.Superacc.cl:192-392).  y is updated in place. */
int exblas_exgemv_dev(char transa, int m, int n, double alpha, const double *d_a, int lda,
                      const double *d_x, int incx, double beta, double *d_y, int incy, int fpe,
                      int early_exit, void *stream);
/* ExTRSV on device pointers, column-major A (ExTRSV.Launcher.hpp; kernels trsv_init/trsv,
 * ExTRSV.lnn.Superacc.cl:241-348, ExTRSV.unn.Superacc.cl:249-355).  d_x holds b on entry and the solution on
 * return: x_i = fl(Round(b_i - sum_j A(i,j) x_j) / A(i,i)), the sum exact.  uplo 'L'/'U', transa 'N'/'T',
 * diag 'N'/'U' (unit diagonal: not read).  fpe as ExTRSV.cpp:70-123: 0 superaccumulators, 1 plain DTRSV,
 * 2..8 expansions (early_exit: buckets 4/6/8); returns EXBLAS_UNSUPPORTED (-1) for fpe >= 9, the
 * iterative-refinement variants whose kernel files the reference does not ship.  Other non-zero: a hipError_t. */
#define EXBLAS_UNSUPPORTED (-1)
int exblas_extrsv_dev(char uplo, char transa, char diag, int n, const double *d_a, int lda, double *d_x,
                      int incx, int fpe, int early_exit, void *stream);
/* Diagnostics: how many rows of the most recent exact ExTRSV on this device were rounded by the integer
 * (superaccumulator) path instead of the register expansion -- near-ties, heavy cancellation, huge/tiny/non-finite
 * values.  Synchronises the device; valid until the next exgemv/exgemm/extrsv call; -1 when unknown. */
int exblas_extrsv_last_slow_rows(void);
/* ExSpMV: exact, reproducible y = alpha A x + beta y for an m x n CSR matrix A on device pointers.  row_ptr[m+1] and
 * col_idx[nnz] are int32 (index_bits 32) or int64 (64), both the same width; val, x, y contiguous fp64.  Row i, with its
 * stored entries p in [row_ptr[i], row_ptr[i+1]), is exactly what ExGEMV 'N' computes for the 1 x k_i matrix of those
 * values against the gathered x:
 *     y_i = Round( sum_p val[p] * fl(alpha * x[col_idx[p]])  (+)  beta * y_i )
 * in both rounding modes (exblas_set_round_mode), with ExGEMV's rules: alpha is folded into x by a rounded multiply;
 * beta = 0 ignores y (NaN included), beta = 1 adds y exactly, any other beta adds the error-free product; ExGEMV's
 * product domain and non-finite rules.  The order of a row's entries does not matter and duplicate columns each
 * count; an empty row (or row_ptr[i+1] <= row_ptr[i]) gives Round(0 (+) beta y_i), +0.0 for beta = 0.  A column index
 * outside [0, n) is never dereferenced: that row's result is NaN.  row_ptr entries must lie in [0, nnz].  The bits do
 * not depend on fpe (>= 2, or 0), early_exit, the internal path, the grid, the index width or the row order.  fpe == 1
 * is the plain, non-reproducible fp64 CSR SpMV.  Stream-ordered launches only (classification on the device, the
 * context workspace): capturable into a hipGraph after exblas_reserve_workspace or one call of the same m.
 * Returns 0 or a hipError_t; invalid m, n, index_bits or fpe < 0 give hipErrorInvalidValue. */
int exblas_exspmv_csr_dev(int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                          const double *d_val, double alpha, const double *d_x, double beta, double *d_y, int fpe,
                          int early_exit, void *stream);
/* Test hook for ExSpMV (same bits on every path): 0 automatic, 1 every row rounded from its integer accumulator,
 * 2 rows rounded in registers wherever the rounding test certifies it (no row is split), 3 every row split into
 * chunks of 16 entries across waves. */
void exblas_set_spmv_path(int mode);
/* The most recent ExSpMV on this device: out[0] rows rounded in registers, out[1] rows rounded from their integer
 * accumulator (fallback), out[2] rows split across workgroups, out[3] chunks of those rows (all 0 for fpe == 1).
 * Synchronises the device; valid until the next call that uses the workspace; -1 when unknown. */
int exblas_last_spmv_info(int64_t *out4);
/* ExSpMM: exact, reproducible Y = alpha A X + beta Y for an m x n CSR matrix A (as for ExSpMV) and dense ROW-MAJOR blocks
 * X (at least n rows, k columns, leading dimension ldx >= k) and Y (m x k, ldy >= k, updated in place) on device
 * pointers.  Column j of Y is, bit for bit, what exblas_exspmv_csr_dev gives for (A, X[:, j], alpha, beta, Y[:, j]):
 *     Y[i, j] = Round( sum_p val[p] * fl(alpha * X[col_idx[p], j])  (+)  beta * Y[i, j] )
 * with everything said there: both rounding modes, alpha folded into X by a rounded multiply, beta = 0 ignores Y (NaN
 * included), beta = 1 adds it exactly, any other beta adds the error-free product, ExGEMV's product domain and
 * non-finite rules, empty rows, duplicate columns count, the entry order is irrelevant.  A column index outside [0, n)
 * is never dereferenced and makes that whole row of Y NaN (all k entries).  The bits depend on the data only: not on k,
 * the column tiling, ldx / ldy, fpe (0 or >= 2), early_exit, the internal path, the grid, the index width or the order
 * of the rows.  fpe == 1 is the plain, non-reproducible fp64 product on the same structure.  The padding between k and
 * ldy in Y is never written.  X and Y must not overlap.  All offsets (row * ld) are 64-bit.
 * m == 0 or k == 0: success, nothing is launched.  m, n, k < 0, ldx < k, ldy < k, index_bits other than 32 / 64 or
 * fpe < 0: hipErrorInvalidValue.  Stream-ordered launches only (classification on the device, no host synchronisation,
 * the context workspace): capturable into a hipGraph after exblas_reserve_workspace or one call with the same (m, k).
 * Returns 0 or a hipError_t. */
int exblas_exspmm_csr_dev(int m, int n, int k, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                          const double *d_val, double alpha, const double *d_x, int64_t ldx, double beta, double *d_y,
                          int64_t ldy, int fpe, int early_exit, void *stream);
/* Test hook for ExSpMM (same bits on every path): 0 automatic, 1 every output rounded from an integer accumulator,
 * 2 outputs rounded in registers wherever the rounding test certifies it (no row is split), 3 every row split into
 * small chunks (16 entries per group of lanes) across waves, as long as the accumulator budget has a slot for it (see
 * exblas_workspace_bytes). */
void exblas_set_spmm_path(int mode);
/* The most recent ExSpMM on this device: out[0] outputs (i, j) rounded in registers, out[1] outputs rounded from an
 * integer accumulator after the main kernel deferred them, out[2] rows split across workgroups, out[3] chunks of those
 * rows.  Synchronises the device; valid until the next call that uses the workspace; -1 when unknown. */
int exblas_last_spmm_info(int64_t *out4);
/* Narrow ExSpMV / ExSpMM: the matrix values in float32, float16 or bfloat16 (val_dtype, an EXBLAS_DT_* code) read at
 * their own width, the vectors x and y (the blocks X and Y) in float64 or in the type of the values (vec_dtype).  With W
 * the exact widening to double,
 *     y_i = RoundTo_vec_dtype( sum_p W(val[p]) * fl64(alpha * W(x[col_idx[p]]))  (+)  beta * W(y_i) )
 * where the sum is the one exblas_exspmv_csr_dev forms on the widened operands, with every rule stated there (alpha folded
 * into x by one rounded fp64 multiply, the three cases of beta, the product domain and non-finite rules, empty rows,
 * duplicate columns, a column outside [0, n) makes the row NaN unread), and RoundTo is ONE rounding of that exact sum:
 *   vec_dtype = EXBLAS_DT_F64: the rounding of the fp64 entry, in both modes of exblas_set_round_mode: the result is bit for
 *     bit exblas_exspmv_csr_dev / exblas_exspmm_csr_dev on the values converted to double;
 *   vec_dtype = val_dtype: to nearest, ties to even, whatever the mode, straight into the narrow format as
 *     exblas_round_records_dev does (subnormal results, the carry into the next binade, overflow to +-Inf at the format's
 *     threshold, -0 for a negative sum that rounds to zero; +-Inf and NaN convert exactly).  The double of the fp64 entry
 *     cast afterwards would round twice.
 * ExSpMM: column j of Y is bit for bit the narrow ExSpMV on (A, X[:, j], Y[:, j]); ldx and ldy count elements; the padding
 * of Y is never written.  The bits depend on the data only (not on the index width, fpe, early_exit, the path, the grid,
 * k, the column tile, ldx / ldy or the alignment).  Pointers need the alignment of their element only.
 * (EXBLAS_DT_F64, EXBLAS_DT_F64) forwards to the fp64 entry.  fpe: 0 and 2..8; fpe == 1 returns EXBLAS_UNSUPPORTED (there
 * is no plain narrow kernel).  hipErrorInvalidValue, before a device is touched: an unknown dtype, float64 values with
 * narrow vectors, two different narrow types, a pointer that is no multiple of its element size, any other fpe, and
 * whatever the fp64 entries refuse.  exblas_set_spmv_path / exblas_set_spmm_path and exblas_last_spmv_info /
 * exblas_last_spmm_info apply with their meanings; workspace and graph capture as for the fp64 entries. */
int exblas_exspmv_csr_lp_dev(int m, int n, int index_bits, const void *d_row_ptr, const void *d_col_idx, int val_dtype,
                             const void *d_val, double alpha, int vec_dtype, const void *d_x, double beta, void *d_y, int fpe,
                             int early_exit, void *stream);
int exblas_exspmm_csr_lp_dev(int m, int n, int k, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                             int val_dtype, const void *d_val, double alpha, int vec_dtype, const void *d_x, int64_t ldx,
                             double beta, void *d_y, int64_t ldy, int fpe, int early_exit, void *stream);
/* The certificate behind the narrow products' rounding in registers, on the CPU; no device is touched.  Returns 1 and in
 * *bits the pattern (low 64 / 32 / 16 bits) of the one `dtype` value that EVERY real number of [res - bound, res + bound]
 * rounds to (to nearest, ties to even), or 0 (and *bits = 0) when the interval reaches a rounding boundary of the format,
 * so that the value cannot be decided from (res, bound).  bound == 0 declares res exact: ties are then decided, to even.
 * Sound for every input; it certifies whenever res lies more than 4 * bound from every boundary.  A negative value for
 * an unknown dtype or a NULL pointer. */
int exblas_round_interval_host(double res, double bound, int dtype, uint64_t *bits);
/* The narrow sparse products' rounding of an accumulator, on the CPU; no device is touched.  The same contract as
 * exblas_round_digits_host (68 normalised digits in, the pattern out), computed the way the kernels do it: from the
 * leading bit, the 64 bits below it and a sticky for the rest.  It equals exblas_round_digits_host bit for bit for all
 * four dtypes. */
int exblas_round_window_host(const int64_t *digits68, int dtype, uint64_t *bits);
/* ExSpTRSV: exact, reproducible sparse triangular solve A x = b for a square m x m CSR matrix A on device pointers
 * (row_ptr[m+1], col_idx[nnz] int32 or int64, both the same width; val and x contiguous fp64).  d_x holds b on entry and
 * the solution on return, as in exblas_extrsv_dev.  uplo 'L': forward, rows 0 .. m-1,
 *     T_i = b_i - sum over the stored p of row i with col_idx[p] < i of val[p] * x[col_idx[p]]
 * exactly over the already fixed doubles x_j (every TwoProd pair goes in; duplicates of an off-diagonal column all
 * count; the order of a row's entries does not matter), then x_i = Round(T_i) / d_i as one IEEE fp64 quotient for diag
 * 'N' and x_i = Round(T_i) for diag 'U'.  Round is the superaccumulator rounding of the current rounding mode
 * (exblas_set_round_mode).  uplo 'U' is the mirror image: rows m-1 .. 0, entries with col_idx[p] > i.  For the same
 * logical system the bits are those of exblas_extrsv_dev on the densified matrix.
 * d_i is the FIRST stored entry of row i with col_idx[p] == i, in storage order; later diagonal duplicates are skipped.
 * A row without one divides by +0.0 (Inf or NaN, as exblas_extrsv_dev gives for a zero diagonal).  Under diag 'U' stored
 * diagonal entries are skipped.  Entries of the other triangle are skipped and their values never used (a NaN there
 * changes nothing), so a full matrix can be passed for a Gauss-Seidel sweep.  A column index outside [0, m) is never
 * dereferenced and makes x_i NaN.  Product domain and Inf / NaN propagation: those of ExTRSV / ExSpMV (an explicit zero
 * times an infinite x_j is NaN).  row_ptr entries must lie in [0, nnz].
 * The bits depend on the data and (uplo, diag, rounding mode) only: not on the grid, the index width, the entry order
 * inside a row, the path (exblas_set_sptrsv_path), fpe (0 or >= 2), early_exit, the context or the stream.  fpe == 0
 * rounds every row from its integer accumulator; fpe == 1 is the plain fp64 solve on the same structure (not exact;
 * its order of operations is fixed, so it is deterministic).
 * One stream-ordered chain (a preset kernel and the solve kernel, the context workspace: 256 + 8 m bytes), no host
 * synchronisation and no analysis phase: capturable into a hipGraph after exblas_reserve_workspace or one call of the same
 * m.  m == 0: success, nothing is launched.  A uplo other than L/U, a diag other than N/U, m < 0, index_bits other than
 * 32 / 64 or fpe < 0: hipErrorInvalidValue.  Returns 0 or a hipError_t.
 * Several right-hand sides: exblas_exsptrsm_csr_dev.  Not provided: A^T solves (pass the transposed CSR), other storage
 * formats. */
int exblas_exsptrsv_csr_dev(char uplo, char diag, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                            const double *d_val, double *d_x, int fpe, int early_exit, void *stream);
/* Test hook for ExSpTRSV (same bits on every path): 0 automatic, 1 every row rounded from its integer accumulator,
 * 2 every row in the one-row-per-wave form (64 lanes stride the row, one row per work item). */
void exblas_set_sptrsv_path(int mode);
/* The most recent ExSpTRSV on this device: out[0] rows rounded in registers, out[1] rows rounded from their integer
 * accumulator, out[2] rows without a stored diagonal under diag 'N', out[3] stored entries skipped (other triangle,
 * diagonal under 'U', duplicate diagonals); all 0 after a call that launched nothing, out[0] = out[1] = 0 for fpe == 1.
 * Synchronises the device; valid until the next call that uses the workspace.  Returns 0, a hipError_t, or
 * EXBLAS_SPTRSV_STALLED when a wave of that call waited for one solved value for more than 2 s and gave up (the values
 * behind it are NaN): a fault of the library, which no valid input causes. */
#define EXBLAS_SPTRSV_STALLED (-3)
int exblas_last_sptrsv_info(int64_t *out4);
/* ExSpTRSM: ExSpTRSV with k right-hand sides.  d_x is an m x k ROW-MAJOR block with leading dimension ldx >= k that holds
 * B on entry and the solution on return.  For every column j, X[:, j] afterwards is bit for bit what
 * exblas_exsptrsv_csr_dev writes for (uplo, diag, A, B[:, j]), with everything said there: per row, in substitution order,
 *     x_ij = Round(b_ij - sum_p val[p] * x[col_idx[p], j]) / d_i
 * the sum exact over the already fixed doubles and rounded once in the current rounding mode, then one IEEE division (none
 * for diag 'U'); the first stored diagonal entry is the divisor; the other triangle and later diagonal entries are
 * skipped unread; a column index outside [0, m) makes that row NaN in every column.  The bits depend on the data and
 * (uplo, diag, rounding mode) only: not on k, ldx, the grid, the column panel, the index width, the entry order inside a
 * row, the path (exblas_set_sptrsm_path), fpe (0 or >= 2), early_exit, the context or the stream.  fpe == 0 rounds every
 * output from an integer accumulator; fpe == 1 is the plain fp64 solve on the same structure (deterministic, not exact).
 * Columns are independent: a NaN or Inf in column j of B changes no bit of another column.  The padding of a row of X
 * beyond column k - 1 is neither read nor written.  All offsets (row * ldx) are 64-bit.
 * The matrix is paid for once per row, not once per row and column: lanes own columns, so the wait for a solved row, the
 * loads of its indices and values and the work ticket serve all columns of a tile of 64.  Columns are solved in panels
 * of min(k, P) columns, one after the other in stream order (each a preset kernel and a solve kernel), P the largest
 * multiple of 64 with 8 m P <= EXBLAS_SPTRSM_MAILBOX_BYTES, at least 64 (see exblas_workspace_bytes).  No host
 * synchronisation, no analysis phase: capturable into a hipGraph after exblas_reserve_workspace or one call with the
 * same (m, k).  m == 0 or k == 0: success, nothing is launched; k == 1 is valid.  The argument errors of
 * exblas_exsptrsv_csr_dev, k < 0 or ldx < k: hipErrorInvalidValue.  Returns 0 or a hipError_t.
 * Not provided: A^T solves, a column-major X, other storage formats. */
#define EXBLAS_SPTRSM_MAILBOX_BYTES ((size_t)64 << 20)
int exblas_exsptrsm_csr_dev(char uplo, char diag, int m, int k, int index_bits, const void *d_row_ptr,
                            const void *d_col_idx, const double *d_val, double *d_x, int64_t ldx, int fpe, int early_exit,
                            void *stream);
/* Test hook for ExSpTRSM (same bits on every path): 0 automatic, 1 every output rounded from the integer accumulator,
 * 2 one row per work item, 3 column panels of 4 columns and column tiles of 4 (the seams between panels and tiles then
 * occur at small k). */
void exblas_set_sptrsm_path(int mode);
/* The most recent ExSpTRSM on this device: out[0] outputs (i, j) rounded in registers, out[1] outputs rounded from the
 * integer accumulator, out[2] rows without a stored diagonal under diag 'N', out[3] stored entries skipped.  out[2] and
 * out[3] count the structure once: they equal exblas_last_sptrsv_info's for the same A whatever k and the panel width;
 * out[0] + out[1] == m * k for fpe != 1 (both 0 for fpe == 1); all 0 after a call that launched nothing.  Synchronises
 * the device; valid until the next call that uses the workspace.  Returns 0, a hipError_t, or EXBLAS_SPTRSV_STALLED as
 * exblas_last_sptrsv_info does. */
int exblas_last_sptrsm_info(int64_t *out4);
/* ExSpILU0: the exact-sum ILU(0) factor of a square m x m CSR matrix A on device pointers (row_ptr[m+1], col_idx[nnz]
 * int32 or int64, both the same width; val and lu contiguous fp64 of nnz entries).  Every row must have strictly ascending
 * column indices and a stored diagonal; S is the set of stored positions and the factor has the same pattern.  For every
 * stored (i, j), rows in ascending order,
 *     c_ij = Round(a_ij - sum over k of l_ik * u_kj)      k < min(i, j), (i, k) in S, (k, j) in S
 *     j <  i:  l_ij = c_ij / u_jj   (one IEEE fp64 quotient)          j >= i:  u_ij = c_ij
 * the sum exact over the already fixed doubles (every TwoProd pair goes in) and rounded once, Round being the
 * superaccumulator rounding of the current rounding mode (exblas_set_round_mode).  This is the step of
 * exblas_exgetrf_batched_dev without the pivot search: on a dense pattern where partial pivoting never swaps, lu holds the
 * bits that routine gives with batch = 1.  L has a unit diagonal and is stored strictly below it, U on and above it, both
 * in ONE value array d_lu on A's own row_ptr / col_idx: exblas_exsptrsv_csr_dev('L', 'U', ..., d_lu, x) followed by
 * exblas_exsptrsv_csr_dev('U', 'N', ..., d_lu, x) (or the ExSpTRSM pair) applies the factor as it is, each solve skipping
 * the other triangle unread.  Non-finite operands and zero pivots follow IEEE arithmetic (Inf - Inf and 0 * Inf are NaN,
 * c / 0 is what the division gives); the factorisation does not stop.  d_lu may be d_val (a_ij is read once, by the wave
 * that writes lu_ij): same bits.
 * d_info is int64[2] on the device, written in stream order.  info[0]: 0, or r + 1 for the smallest row r with a
 * structural defect -- row_ptr decreasing (or a row outside [0, row_ptr[m]]), a column outside [0, m), columns not
 * strictly ascending, no stored diagonal, more than EXBLAS_SPILU0_MAX_ROW entries -- and then d_lu is not written at all.
 * info[1]: 0, or r + 1 for the smallest row whose pivot u_rr is zero or NaN (LAPACK's first zero pivot; an Inf pivot is
 * not reported).  Both are order-independent minima.
 * The bits depend on the data and the rounding mode only: not on the grid, the index width, the path
 * (exblas_set_spilu0_path), fpe (0 or >= 2), early_exit, the context or the stream.  fpe == 0 rounds every entry from the
 * integer accumulator; fpe == 1 is the plain fp64 form s = a_ij, then s -= l_ik * u_kj for k ascending (deterministic,
 * not exact).
 * One stream-ordered chain of three kernels (preset, structure check, one persistent factor kernel), no analysis phase.
 * Context workspace: 256 + 8 m (rounded up to 256) + 8 nnz bytes (header, the diagonal position of every row, a mailbox of
 * one double per stored entry).  The signature carries no nnz: a call outside a stream capture reads row_ptr[m] back (one
 * word, one wait on the stream) to size the mailbox; info and lu are written without a host synchronisation.  A call that
 * is being captured reads nothing back: it is capturable after exblas_reserve_workspace of that many bytes or one call of
 * the same m and pattern, and on replay serves any values on a pattern of at most the nnz it was captured with (a row
 * that does not fit the mailbox is reported in info[0]).  m == 0: info is zeroed, nothing else is launched.  m < 0,
 * index_bits other than 32 / 64, fpe < 0 or d_info null: hipErrorInvalidValue.  Returns 0 or a hipError_t.
 * Not provided: fill (ILU(k), ILUT), modified ILU, pivoting, unsorted rows, BSR / CSC.  The symmetric form is ExSpIC0. */
#define EXBLAS_SPILU0_MAX_ROW 512
int exblas_exspilu0_csr_dev(int m, int index_bits, const void *d_row_ptr, const void *d_col_idx, const double *d_val,
                            double *d_lu, int64_t *d_info, int fpe, int early_exit, void *stream);
/* Test hook for ExSpILU0 (same bits on every path): 0 automatic, 1 every rounding through the wave's integer accumulator,
 * 2 every row in the several-entries-per-lane form (8 lanes share a row of at most 64 entries). */
void exblas_set_spilu0_path(int mode);
/* The most recent ExSpILU0 on this device: out[0] entries rounded in registers, out[1] entries rounded from the integer
 * accumulator (out[0] + out[1] == nnz on a sound, completed call with fpe != 1; both 0 for fpe == 1), out[2] product terms
 * l_ik * u_kj summed (the triples (i, k, j) of the definition), out[3] rows in the several-entries-per-lane form; all 0
 * after a call that launched nothing or met a structural defect.  Synchronises the device; valid until the next call
 * that uses the workspace.  Returns 0, a hipError_t, or EXBLAS_SPTRSV_STALLED as exblas_last_sptrsv_info does. */
int exblas_last_spilu0_info(int64_t *out4);
/* ExSpIC0: the exact-sum IC(0) factor of a symmetric square m x m CSR matrix A on device pointers (row_ptr[m+1], col_idx[nnz]
 * int32 or int64, both the same width; val and ll contiguous fp64 of nnz entries).  Every row must have strictly ascending
 * column indices and a stored diagonal, and the pattern S must be structurally symmetric: (i, j) is stored exactly when
 * (j, i) is (the full matrix a CG caller holds for ExSpMV).  Only the entries on and below the diagonal are read: values
 * above it are never read, so a NaN there changes nothing.  For every stored (i, j) with j <= i, rows in ascending order,
 *     c_ij = Round(a_ij - sum over k of l_ik * l_jk)      k < j, (i, k) in S, (j, k) in S   (for j = i: the l_ik^2)
 *     j <  i:  l_ij = c_ij / l_jj   (one IEEE fp64 quotient)
 *     j == i:  l_ii = sqrt(c_ii)    (one correctly rounded fp64 square root, as in exblas_expotrf_dev)
 * the sum exact over the already fixed doubles (every TwoProd pair goes in) and rounded once, Round being the
 * superaccumulator rounding of the current rounding mode (exblas_set_round_mode).  The output is ONE value array d_ll on
 * A's own row_ptr / col_idx: L on and below the diagonal, and every stored upper position (j, i) holds the same double as
 * l_ij (L^T written as a mirror), so exblas_exsptrsv_csr_dev('L', 'N', ..., d_ll, x) followed by
 * exblas_exsptrsv_csr_dev('U', 'N', ..., d_ll, x) (or the ExSpTRSM pair) applies (L L^T)^-1 as it is.  On a sound call
 * every stored position of d_ll is written.  d_ll may be d_val (same bits).  On a dense pattern with no breakdown the lower
 * triangle is bit for bit exblas_expotrf_dev(G, 'L'); on a block-diagonal pattern of dense blocks, each block is what
 * ExPOTRF gives on that block.
 * Breakdown: ExSpILU0's rule, NOT ExPOTRF's (which stops at the first radicand that is not > 0 and leaves the rest).  A
 * radicand c_ii that is not > 0 (zero, negative or NaN) gives l_ii = sqrt(c_ii) by IEEE arithmetic, and every later entry
 * follows IEEE arithmetic (c / 0, Inf - Inf, 0 * Inf); the factorisation never stops.
 * d_info is int64[2] on the device, written in stream order.  info[0]: 0, or r + 1 for the smallest row r with a
 * structural defect, in two phases.  Phase 1: ExSpILU0's defects -- row_ptr decreasing (or a row outside [0, row_ptr[m]]),
 * a column outside [0, m), columns not strictly ascending, no stored diagonal, more than EXBLAS_SPIC0_MAX_ROW entries.
 * Phase 2, only when phase 1 found nothing: the smallest row r that stores some (r, j) with no stored (j, r).  On any
 * structural defect d_ll is not written at all.  info[1]: 0, or r + 1 for the smallest row whose radicand c_rr is not > 0
 * ("not positive definite on the pattern").  Both are order-independent minima.
 * The bits depend on the data and the rounding mode only: not on the grid, the index width, the path
 * (exblas_set_spic0_path), fpe (0 or >= 2), early_exit, the context or the stream.  fpe == 0 rounds every entry from the
 * integer accumulator; fpe == 1 is the plain fp64 form s = a_ij, then s -= l_ik * l_jk for k ascending, then the division
 * or the square root (deterministic, not exact).
 * One stream-ordered chain of four kernels (preset, the two phases of the structure check, one persistent factor kernel),
 * no analysis phase.  Context workspace: 256 + 8 m (rounded up to 256) + 8 nnz bytes, and the rules of a captured call,
 * as for ExSpILU0: a call outside a stream capture reads row_ptr[m] back; a call that is being captured is capturable
 * after exblas_reserve_workspace of that many bytes or one call of the same m and pattern, and on replay a row that does
 * not fit the captured nnz is reported in info[0].  m == 0: info is zeroed, nothing else is launched.  m < 0, index_bits
 * other than 32 / 64, fpe < 0 or d_info null: hipErrorInvalidValue.  Returns 0 or a hipError_t.
 * Not provided: fill (IC(k), ICT), modified IC, shifts on breakdown, a stored upper triangle alone, unsorted rows. */
#define EXBLAS_SPIC0_MAX_ROW EXBLAS_SPILU0_MAX_ROW
int exblas_exspic0_csr_dev(int m, int index_bits, const void *d_row_ptr, const void *d_col_idx, const double *d_val,
                           double *d_ll, int64_t *d_info, int fpe, int early_exit, void *stream);
/* Test hook for ExSpIC0 (same bits on every path): 0 automatic, 1 every rounding through the wave's integer accumulator,
 * 2 every row in the several-entries-per-lane form (8 lanes share an owned part of at most 64 entries). */
void exblas_set_spic0_path(int mode);
/* The most recent ExSpIC0 on this device: out[0] entries rounded in registers, out[1] entries rounded from the integer
 * accumulator (out[0] + out[1] == the stored entries on and below the diagonal on a sound, completed call with fpe != 1;
 * both 0 for fpe == 1), out[2] product terms summed (the triples (i, k, j) with j <= i of the definition), out[3] rows whose
 * owned part (the entries on and below the diagonal) is in the several-entries-per-lane form; all 0 after a call that
 * launched nothing or met a structural defect.  Synchronises the device; valid until the next call that uses the
 * workspace.  Returns 0, a hipError_t, or EXBLAS_SPTRSV_STALLED as exblas_last_sptrsv_info does. */
int exblas_last_spic0_info(int64_t *out4);
/* ExTRSM: ExTRSV with k right-hand sides.  A is the n x n column-major triangle of exblas_extrsv_dev (lda >= max(1, n),
 * uplo 'L'/'U', transa 'N'/'T', diag 'N'/'U'); d_x is an n x k ROW-MAJOR block with leading dimension ldx >= k, as in
 * ExSpTRSM and ExBDOT, that holds B on entry and the solution on return.  For every column j, X[:, j] afterwards holds
 * exactly the bits that exblas_extrsv_dev(uplo, transa, diag, n, A, lda, X + j, incx = ldx, fpe', early_exit', stream)
 * writes for B[:, j], for any fpe' that is 0 or in 2..8, in the current rounding mode:
 *     x_ij = fl( Round( b_ij - sum_{c before i} op(A)(i,c) * x_cj ) / op(A)(i,i) )
 * in substitution order, the sum exact over the already fixed doubles and rounded once by the superaccumulator rounding
 * of exblas_set_round_mode, then one IEEE division (none for diag 'U').  Product domain and Inf / NaN rules: ExTRSV's;
 * every stored entry of the strict triangle counts, so a zero times an infinite x_cj is NaN.  The other triangle, the
 * lda padding and, under diag 'U', the stored diagonal are never read.
 * The bits depend on the data and (uplo, transa, diag, rounding mode) only: not on k, ldx, the column panel or tile, the
 * row grouping, the grid, the path (exblas_set_trsm_path), fpe (0 or 2..8), early_exit, the context or the stream.
 * Columns are independent: a NaN or Inf in column j of B changes no bit of another column.  The padding of a row of X
 * beyond column k - 1 is neither read nor written.  All offsets (row * ldx, column * lda) are 64-bit.
 * fpe == 0 rounds every output from an integer accumulator; fpe == 1 is the plain fp64 solve on the same structure
 * (deterministic, not exact); fpe >= 9 returns EXBLAS_UNSUPPORTED and touches nothing, as exblas_extrsv_dev does.
 * The chain of n rounded divisions is walked once for all columns and A is read once per tile of 64 columns, not once
 * per column: lanes own columns, so the wait for a solved row and the entries of A serve every column of a tile.
 * Columns are solved in panels of min(k, P) columns, one after the other in stream order (each a preset kernel and a
 * solve kernel), P the largest multiple of 64 with 8 n P <= EXBLAS_TRSM_MAILBOX_BYTES, at least 64 (see
 * exblas_workspace_bytes).  No host synchronisation: capturable into a hipGraph after exblas_reserve_workspace or one
 * call with the same (n, k).  n == 0 or k == 0: success, nothing is launched; k == 1 is valid.  n < 0, k < 0,
 * lda < max(1, n), ldx < k, a uplo, transa or diag outside L/U, N/T, N/U (either case) or fpe < 0: hipErrorInvalidValue.
 * Returns 0, EXBLAS_UNSUPPORTED or a hipError_t.
 * Not provided: a scaling alpha, the right-side solve X op(A) = B, a column-major X, conjugation. */
#define EXBLAS_TRSM_MAILBOX_BYTES ((size_t)64 << 20)
int exblas_extrsm_dev(char uplo, char transa, char diag, int n, int k, const double *d_a, int lda, double *d_x,
                      int64_t ldx, int fpe, int early_exit, void *stream);
/* Test hook for ExTRSM (same bits on every path): 0 automatic, 1 every output rounded from the integer accumulator,
 * 2 the smallest row group (one row per work item), 3 column panels of 4 columns and column tiles of 4 (the seams between
 * panels and tiles then occur at small k). */
void exblas_set_trsm_path(int mode);
/* The most recent ExTRSM on this device: out[0] outputs (i, j) rounded in registers, out[1] outputs rounded from the
 * integer accumulator, out[2] = out[3] = 0.  out[0] + out[1] == n * k for fpe != 1 (both 0 for fpe == 1); all 0 after a
 * call that launched nothing.  Synchronises the device; valid until the next call that uses the workspace.  Returns 0, a
 * hipError_t, or EXBLAS_SPTRSV_STALLED as exblas_last_sptrsv_info does. */
int exblas_last_trsm_info(int64_t *out4);
/* ExBDOT: exact, reproducible inner products of two dense ROW-MAJOR blocks on device pointers, both read once.  X is
 * n x p with leading dimension ldx >= p, Y is n x q with ldy >= q.
 *   mode 'G' (Gram):      C[i * ldc + j] = Round( sum_r X[r, i] * Y[r, j] ),  C p x q row-major, ldc >= q
 *   mode 'D' (diagonal):  c[j] = Round( sum_r X[r, j] * Y[r, j] ),  p == q, c a contiguous vector of p doubles (ldc ignored)
 * The sum is exact and rounded once: to nearest even, or by the reference rule under exblas_set_round_mode(1).  Every
 * output is, bit for bit, the `exact` word (rounding mode 0) or the `refmode` word (mode 1) of the record that
 * exblas_exdot_dev(X + i, ldx, Y + j, ldy, n, ...) returns, whenever that record carries none of the product-domain flag
 * bits 3..6: the domain is ExGEMV's product domain with its non-finite rules, as for the sparse routines (the outputs
 * are plain doubles without a flag channel; products below 2^-968 or beyond the double range are outside it).
 * The bits depend on the data only: not on p, q, the column panel or output tile, ldx / ldy / ldc, the alignment of X and
 * Y, fpe (0 or >= 2), early_exit, the grid, the row slab or the internal path (exblas_set_bdot_path).  fpe == 1 is the
 * plain, non-reproducible fp64 computation on the same structure.  early_exit with fpe > 8 is ExGEMV's (the reference's)
 * silent return: nothing is launched and the outputs keep their values.
 * Columns are independent: a NaN or Inf in column i of X changes only row i of C ('G') or c[i] ('D'), and likewise for Y
 * and the columns of C; 0 * Inf is NaN, as in ExDOT.  X and Y are only read and may be the same block or overlap; with
 * X == Y in 'G', C is bit for bit symmetric.  C must not overlap X or Y.  The padding between q and ldc is never
 * written; the padding of X and Y is never read.  All offsets (r * ld) are 64-bit.  Any p and q are served (outputs
 * beyond 4096, or a Gram matrix beyond 64 x 64, in batches that each read their columns again); the design range is up to
 * 64 each.
 * n == 0 writes +0.0 to every output; p == 0 or q == 0: success, nothing is launched.  n < 0 or n > INT_MAX, p < 0,
 * q < 0, ldx < p, ldy < q, ldc < q in 'G', p != q in 'D', a mode other than G/g/D/d or fpe < 0: hipErrorInvalidValue.
 * Stream-ordered launches only (per batch a zeroing kernel, the accumulate kernel and the finalize kernel; no host
 * synchronisation): the accumulators -- one 68-limb set of 576 bytes per output and accumulator group -- live in the
 * context workspace, EXBLAS_BDOT_WORKSPACE_BYTES whatever the sizes, are zeroed before use (other routines leave scratch
 * in the workspace) and are left zeroed.  Capturable into a hipGraph after exblas_reserve_workspace or one call.
 * Returns 0 or a hipError_t.
 * Not provided: products outside the domain (no per-output low / high accumulators), column-major blocks, fp32,
 * alpha / beta.  Rows sharded over ranks or calls: exblas_exbdot_export_dev / _round_dev / _allreduce_dev below. */
#define EXBLAS_BDOT_WORKSPACE_BYTES ((size_t)4096 * 576)
int exblas_exbdot_dev(char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y, int64_t ldy,
                      double *d_c, int64_t ldc, int fpe, int early_exit, void *stream);
/* Row-sharded ExBDOT, first half: the rows of one shard go through the accumulate kernel as in exblas_exbdot_dev, and
 * instead of a double every output leaves its NORMALISED DIGIT SET: EXBLAS_SET_WORDS int64 -- words 0..67 the exact sum
 * of the shard's products in base 2^32 (67 digits in [0, 2^32) under a signed top digit: a negative total is -1 over a
 * run of 0xffffffff digits), words 68 / 69 / 70 are 1 where a +Inf / -Inf / NaN product was seen and 0 otherwise, word 71
 * is 0.  d_sets is [outputs][EXBLAS_SET_WORDS] in output order -- 'G': output i * q + j, p * q sets; 'D': output j, p sets
 * -- whatever the batches: every word of every set is written, nothing beyond them.  Sets add as plain int64 (digits
 * below 2^32: 2^31 of them cannot overflow), which is what an all-reduce of them does.
 * The set of an output depends on the data of the shard only: not on the path, the tile, the grid, fpe (0 or >= 2) or
 * early_exit.  n == 0 writes all-zero sets; p == 0 or q == 0 launches nothing.  fpe == 1 (plain fp64 sums have no digit
 * sets) and early_exit with fpe > 8 (a silent return would leave the sets undefined) are hipErrorInvalidValue; every
 * other argument rule is exblas_exbdot_dev's (d_sets in C's place, no ldc).  Workspace, launches and capture as
 * exblas_exbdot_dev (the export kernel in the finalize kernel's place); the context's accumulators are left zero. */
int exblas_exbdot_export_dev(char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx, const double *d_y,
                             int64_t ldy, int64_t *d_sets, int fpe, int early_exit, void *stream);
/* Second half: d_sets is [nsets][outputs][EXBLAS_SET_WORDS] (nsets >= 1, else hipErrorInvalidValue), e.g. the exports
 * of nsets shards stacked, or one set per output that an int64-sum all-reduce has already added.  One wave per output
 * adds the nsets copies (low and high halves of the words apart: no overflow up to 2^31 sets of normalised digits or of
 * sums of them), ORs the indicators (a non-zero word 68 / 69 / 70 counts: +Inf on one shard and -Inf on another give
 * NaN), propagates the carries and stores the double of the current rounding mode at C's position (ldc in 'G', a
 * contiguous vector in 'D').  d_sets is only read; the padding of C is never written.  One launch, no workspace,
 * capturable.
 * CONTRACT of export + round, and of exblas_exbdot_allreduce_dev: the result is bit for bit what exblas_exbdot_dev gives
 * on the blocks of all shards stacked in any order -- for any number of shards, any shard sizes (empty ones included) and
 * any mix of paths and fpe between them -- inside ExGEMV's product domain (there are still no per-output low / high
 * sets).  A shard's PARTIAL total may be negative under a positive total, or beyond 2^1024 under a finite one. */
int exblas_exbdot_round_dev(char mode, int p, int q, const int64_t *d_sets, int nsets, double *d_c, int64_t ldc,
                            void *stream);
/* Test hook for ExBDOT (same bits on every path): 0 automatic, 1 the row slab of a workgroup forced to the smallest the
 * kernel supports (4 waves x 64 / T rows, T the outputs of a tile: a few hundred rows are already merged from many
 * workgroups per output), 2 column panels ('D') and output tiles ('G') of width 4 (p, q = 5 then cross an edge). */
void exblas_set_bdot_path(int mode);
/* ExBGEMM: exact, reproducible block update Y = alpha X C + beta Y for dense ROW-MAJOR blocks on device pointers: X tall
 * (n x p, leading dimension ldx >= p), C small (p x q, ldc >= q), Y tall (n x q, ldy >= q, updated in place) -- the last
 * step of a block-Krylov iteration (X += P a, R -= Q a, P = Z + P b, W -= V (V^T W)).
 *     Y[r, j] = Round( sum_{i<p} X[r, i] * fl(alpha * C[i, j])  (+)  beta * Y[r, j] )
 * Every output is, bit for bit, what exblas_exspmm_csr_dev writes for the CSR matrix that stores X densely
 * (row_ptr[r] = r p, col_idx = 0 .. p-1, values = the row of X) against C as its dense block, with everything said there:
 * both rounding modes (exblas_set_round_mode), alpha folded into C by one rounded multiply, beta = 0 ignores Y (NaN
 * included), beta = 1 adds it exactly, any other beta adds the error-free product, ExGEMV's product domain and non-finite
 * rules.  Every entry of X counts, so a zero in X times an Inf in C is NaN.  p == 0 gives Round(0 (+) beta Y), +0.0 for
 * beta = 0.  The sum and the beta term are rounded ONCE (exblas_exgemm_dev rounds the sum, then adds beta * C in fp64).
 * The bits depend on the data and the rounding mode only: not on n, q, ldx / ldc / ldy, the row block, the column tile,
 * the chunk of C, the grid, fpe (0 or >= 2), early_exit (also with fpe > 8, as in exblas_exspmm_csr_dev), the path
 * (exblas_set_bgemm_path), the context or the stream.  fpe == 0 rounds every output from an integer accumulator; fpe == 1
 * is the plain fp64 product on the same structure (deterministic, not exact).
 * Rows are independent: a NaN or Inf in row r of X changes only row r of Y, one in column j of C only column j.  The
 * padding of X and C is never read, the padding of Y never written.  X and C must not overlap Y.  All offsets (row * ld)
 * are 64-bit.  With C replicated, a row-sharded caller needs no communication: each rank updates its own rows.
 * Any p and q are served (q beyond 64 in column tiles of 64, p beyond 64 in chunks of 64 rows of C, staged again per row
 * block); the design range is up to 64 each.  n == 0 or q == 0: success, nothing is launched.  n, p or q < 0,
 * n > INT_MAX, ldx < p, ldc < q, ldy < q or fpe < 0: hipErrorInvalidValue.
 * ONE stream-ordered kernel launch and nothing else: no memset, no host synchronisation.  The only workspace is that of
 * the info counters: 16 bytes per workgroup, at most 128 bytes per compute unit, which the kernel stores without needing
 * them cleared and exblas_last_bgemm_info adds up.  Capturable into a hipGraph after exblas_reserve_workspace or one call.
 * Returns 0 or a hipError_t.
 * Not provided: transposes of X or C, column-major blocks, fp32, p or q far beyond 64 (served, not designed for). */
int exblas_exbgemm_dev(int64_t n, int p, int q, double alpha, const double *d_x, int64_t ldx, const double *d_c,
                       int64_t ldc, double beta, double *d_y, int64_t ldy, int fpe, int early_exit, void *stream);
/* Test hook for ExBGEMM (same bits on every path): 0 automatic, 1 every output rounded from the integer accumulator,
 * 2 a register block of one row (one row per lane), 3 column tiles of 4 and chunks of 4 rows of C (the seams between
 * tiles and chunks then occur at small p and q). */
void exblas_set_bgemm_path(int mode);
/* The most recent ExBGEMM on this device: out[0] outputs (r, j) rounded in registers, out[1] outputs rounded from the
 * integer accumulator, out[2] = out[3] = 0.  out[0] + out[1] == n * q for fpe != 1 (both 0 for fpe == 1); all 0 after a
 * call that launched nothing.  Synchronises the device; valid until the next call that uses the workspace.  Returns 0 or
 * a hipError_t. */
int exblas_last_bgemm_info(int64_t *out4);
/* ExBTRSM: exact, reproducible triangular solve FROM THE RIGHT on a tall block, X op(T) = alpha B, on device pointers: T is
 * ExTRSV's p x p COLUMN-MAJOR triangle (ldt >= max(1, p); uplo, transt, diag as there), X is n x p ROW-MAJOR (ldx >= p, all
 * offsets 64-bit), holds B on entry and the solution on return -- Q = X R^-1 of CholQR, the P (P^T A P)^-1 of a block CG
 * through its Cholesky factor, the normalisation of block Gram-Schmidt.  Per row r, in substitution order over the columns
 * (forward when op(T) is upper: 'U','N' or 'L','T'; backward otherwise):
 *     x_rj = fl( Round( alpha * b_rj - sum_{i before j} x_ri * op(T)(i, j) ) / op(T)(j, j) )
 * the sum exact over the already fixed doubles and rounded ONCE in the current rounding mode (exblas_set_round_mode), then
 * one IEEE division (none under diag 'U', never a multiplication by a reciprocal).  With alpha = 1, row r is bit for bit
 * what exblas_extrsv_dev(uplo, the other trans, diag, p, T, ldt, X + r ldx, 1) writes for B[r, :], i.e. column r of
 * exblas_extrsm_dev on the transposed block.  The alpha term follows ExBGEMM's beta term: alpha = 1 adds b_rj exactly, any
 * other non-zero alpha adds the error-free product alpha * b_rj (both parts: alpha * b is NOT rounded before the sum),
 * alpha = 0 does not read B (NaN there is ignored) and solves the zero right-hand side.  Every entry of the strict triangle
 * counts (a zero times an infinite x_ri is NaN); the other triangle, the ldt padding and the diagonal under 'U' are never
 * read; the padding of X beyond column p - 1 is neither read nor written.  Rows are independent: a NaN in row r of B
 * changes row r only; a row-sharded caller with T replicated needs no communication.
 * The bits depend on the data, (uplo, transt, diag, alpha) and the rounding mode only: not on n, ldx, the rows of a wave, the
 * column block, the chunk of T, the grid, the path (exblas_set_btrsm_path), fpe (0 or 2..8), early_exit, the context or the
 * stream.  fpe == 0 rounds every output from an integer accumulator; fpe == 1 is the plain fp64 solve on the same structure
 * (deterministic, not exact; counters 0); fpe >= 9: EXBLAS_UNSUPPORTED, nothing is touched (as exblas_extrsm_dev).
 * The design range is p <= 64 (the triangle is staged once per workgroup); p up to EXBLAS_BTRSM_MAX_P is served with the
 * same bits (chunks of T staged again per item).  p > EXBLAS_BTRSM_MAX_P is REFUSED with hipErrorInvalidValue before the
 * device is touched: the rows of a wave must fit its share of the LDS.  n == 0 or p == 0: success, nothing is launched.
 * Bad flags, n or p < 0, ldt < max(1, p), ldx < p or fpe < 0: hipErrorInvalidValue, also before the device is touched.
 * ONE stream-ordered kernel launch and nothing else: no preset kernel, no memset, no mailbox, no host synchronisation.  The
 * only workspace is that of the info counters, 16 bytes per workgroup (ExBGEMM's scheme).  Capturable into a hipGraph
 * after one call on the device (the first one raises the kernel's dynamic LDS limit) and, for a context without
 * workspace, exblas_reserve_workspace or one call on it.  Returns 0, EXBLAS_UNSUPPORTED or a hipError_t.
 * Not provided: the left-side solve (exblas_extrsm_dev), column-major X, conjugation, fp32. */
#define EXBLAS_BTRSM_MAX_P 512
int exblas_exbtrsm_dev(char uplo, char transt, char diag, int64_t n, int p, double alpha, const double *d_t, int ldt,
                       double *d_x, int64_t ldx, int fpe, int early_exit, void *stream);
/* Test hook for ExBTRSM (same bits on every path): 0 automatic, 1 every output rounded from the integer accumulator,
 * 2 a register block of one column, 3 four rows per wave item and chunks of 4 rows x 4 columns of T (the seams between
 * items, slices and chunks then occur at small n and p). */
void exblas_set_btrsm_path(int mode);
/* The most recent ExBTRSM on this device: out[0] outputs (r, j) rounded in registers, out[1] outputs rounded from the
 * integer accumulator, out[2] = out[3] = 0.  out[0] + out[1] == n * p for fpe != 1 (both 0 for fpe == 1); all 0 after a
 * call that launched nothing.  Synchronises the device; valid until the next call that uses the workspace.  Returns 0 or
 * a hipError_t. */
int exblas_last_btrsm_info(int64_t *out4);
/* ExPOTRF: exact-sum Cholesky factorisation of a small symmetric positive definite matrix (the Gram matrix X^T X of CholQR,
 * the P^T A P of a block CG), on device pointers, IN PLACE on ExTRSV's p x p COLUMN-MAJOR triangle (ldg >= max(1, p)): what
 * it leaves is what exblas_extrsm_dev and exblas_exbtrsm_dev take, with no conversion.  For uplo = 'U', G = R^T R with R
 * upper.  Row by row, j = 0 .. p-1:
 *     r_jj = sqrt( Round( g_jj - sum_{k<j} r_kj^2 ) )
 *     r_ji = fl( Round( g_ji - sum_{k<j} r_kj * r_ki ) / r_jj )      for i > j
 * every sum exact over the already fixed doubles (both parts of every TwoProd and every entry count, zeros included: a zero
 * times an infinite entry is NaN) and rounded ONCE in the current rounding mode (exblas_set_round_mode), then ONE IEEE
 * correctly rounded square root or ONE IEEE division (never a multiplication by a reciprocal).  The diagonal of R is
 * positive.  uplo = 'L' is G = L L^T with L = R^T: the same numbers in the other triangle.
 * The bits depend on the data, uplo and the rounding mode only: not on the path (exblas_set_potrf_path), the row block, the
 * column tile, the slices, the number of waves, fpe (0 or 2..8), early_exit, ldg, the context or the stream.  Two identities
 * follow: the strict part of column i of R is bit for bit what exblas_extrsv_dev('U', 'T', 'N', i, R, ldg, .) writes for
 * g[0:i, i]; the radicand of r_ii is bit for bit ExBGEMM's Round(-1 * r[0:i, i]^T r[0:i, i] + 1 * g_ii) on a 1 x i block.
 * BREAKDOWN (LAPACK's rule): at the first j whose rounded radicand v is not > 0 (zero, negative, NaN) the routine stores v
 * itself at (j, j), leaves every entry of row j beyond the diagonal and all later rows as they were on entry, and writes
 * j + 1 to the int32 word d_info; otherwise it writes 0.  +Inf passes, as in LAPACK.  The word is written by every call
 * that launches, with a plain store: nothing has to be cleared, and it is valid after every graph replay.  The routine
 * never synchronises; the caller reads the word when it wants to.
 * The other triangle is neither read nor written; the padding of a column beyond row p - 1 is not touched.
 * fpe == 0 rounds every output from an integer accumulator; fpe == 1 is the plain fp64 factorisation on the same structure
 * (deterministic, not exact; counters 0); fpe >= 9: EXBLAS_UNSUPPORTED, nothing is touched.
 * The design range is p <= 64 (the triangle is factored in LDS); p up to EXBLAS_BTRSM_MAX_P, every triangle ExBTRSM accepts,
 * is served with the same bits (in place in global memory).  A larger p is REFUSED with hipErrorInvalidValue before the
 * device is touched; so are a bad uplo, p < 0, ldg < max(1, p), fpe < 0 and a null d_info with p > 0.  p == 0: success,
 * nothing is launched, d_info is not written.
 * ONE stream-ordered launch of ONE workgroup and nothing else: no memset, no mailbox, no ticket, no host synchronisation.
 * The only workspace is that of the two counters (16 bytes).  Capturable into a hipGraph after one call on the context (or
 * exblas_reserve_workspace).  Returns 0, EXBLAS_UNSUPPORTED or a hipError_t.
 * Not provided: pivoting, a shifted CholQR, LDL^T, fp32, more than one workgroup, p > 512. */
int exblas_expotrf_dev(char uplo, int p, double *d_g, int ldg, int *d_info, int fpe, int early_exit, void *stream);
/* Test hook for ExPOTRF (same bits on every path): 0 automatic, 1 every output rounded from the integer accumulator,
 * 2 a register block of one row, 3 column tiles of 4 and no staging in LDS (the seams between tiles, slices and row
 * blocks, and the in-place form of p > 64, then occur at small p). */
void exblas_set_potrf_path(int mode);
/* The most recent ExPOTRF on this device: out[0] outputs rounded in registers, out[1] outputs rounded from the integer
 * accumulator, out[2] = out[3] = 0.  out[0] + out[1] is the number of entries the call fixed for fpe != 1 (both 0 for
 * fpe == 1): p (p + 1) / 2 on success, j (2p - j + 1) / 2 + 1 after a breakdown at pivot j (0-based); all 0 after a call
 * that launched nothing.  The workgroup stores them with plain stores: valid after each graph replay.  Synchronises the
 * device; valid until the next call that uses the workspace.  Returns 0 or a hipError_t. */
int exblas_last_potrf_info(int64_t *out4);
/* Batched ExPOTRF: the exact-sum Cholesky factorisation of `batch` independent small matrices (the diagonal blocks of a
 * block-Jacobi preconditioner) in ONE launch, on device pointers.  Matrix b is the p x p COLUMN-MAJOR triangle at
 * d_g + b * stride (ldg >= max(1, p); stride >= ldg * p when batch > 1; all offsets 64-bit) and is factored IN PLACE exactly
 * as exblas_expotrf_dev(uplo, p, d_g + b * stride, ldg, d_info + b, ...) defines: the same row-by-row contract, one rounding
 * per exact sum, then ONE correctly rounded square root or ONE IEEE division per entry, and LAPACK's breakdown rule PER
 * MATRIX (the radicand that is not > 0 is stored at its pivot, the rest of that matrix stays as it was, d_info[b] = j + 1,
 * else 0).  d_info[b] is written for every b by every call that launches, with plain stores.  Bit for bit, every matrix is
 * what the single routine gives.
 * The bits of a matrix depend on its data, uplo and the rounding mode only: not on batch, its position in the batch, its
 * neighbours, ldg, stride, the path (exblas_set_potrf_batched_path), fpe (0 or 2..8), early_exit, the context or the
 * stream.  Matrices are independent: a NaN matrix or a breakdown changes no bit of another one.  The other triangle, the
 * ldg padding of a column and the gap between matrices (stride > ldg * p) are neither read nor written.
 * fpe == 0 rounds every output from an integer accumulator; fpe == 1 is the plain fp64 factorisation (s = g_ji, then
 * s -= r_kj r_ki for k ascending; deterministic, not exact; counters 0); fpe >= 9: EXBLAS_UNSUPPORTED, nothing is touched.
 * REFUSED with hipErrorInvalidValue before the device is touched: p > EXBLAS_POTRF_BATCHED_MAX_P, a bad uplo, p < 0,
 * batch < 0, ldg < max(1, p), batch > 1 with stride < ldg * p, fpe < 0, and a null d_g or d_info when anything would be
 * launched.  p == 0 or batch == 0: success, nothing is launched, d_info is not written.
 * ONE stream-ordered kernel launch and nothing else: no memset, no mailbox, no ticket, no host synchronisation.  One wave
 * walks a matrix (no workgroup barrier in the pivot chain); for p <= 32 a wave carries 64 / pw matrices, pw = p rounded up
 * to a power of two, its lanes being (matrix, column) pairs.  The only workspace is that of the counters (16 bytes per
 * workgroup).  Capturable into a hipGraph after one call on the context (the first call raises the kernel's dynamic-LDS
 * limit).  Returns 0, EXBLAS_UNSUPPORTED or a hipError_t.
 * Not provided: variable block sizes, p > 64, LDL^T, fp32.  General (nonsymmetric or indefinite) blocks: the batched
 * ExGETRF below, an LU with partial pivoting. */
#define EXBLAS_POTRF_BATCHED_MAX_P 64
int exblas_expotrf_batched_dev(char uplo, int p, int64_t batch, double *d_g, int ldg, int64_t stride, int *d_info, int fpe,
                               int early_exit, void *stream);
/* Test hook for the batched ExPOTRF (same bits on every path): 0 automatic, 1 every output rounded from the integer
 * accumulator, 2 no packing (one matrix per wave), 3 one matrix per workgroup item on a handful of workgroups (the seams
 * between the items of a workgroup then occur at a small batch). */
void exblas_set_potrf_batched_path(int mode);
/* The most recent batched ExPOTRF on this device: out[0] entries rounded in registers, out[1] entries rounded from the
 * integer accumulator, out[2] = out[3] = 0.  For fpe != 1, out[0] + out[1] is the sum over the batch of the entries each
 * matrix fixed (as exblas_last_potrf_info counts them); both 0 for fpe == 1; all 0 after a call that launched nothing.
 * Synchronises the device; valid until the next call that uses the workspace.  Returns 0 or a hipError_t. */
int exblas_last_potrf_batched_info(int64_t *out4);
/* Batched ExPOTRS, the apply of a block-Jacobi preconditioner, on device pointers: d_x is an n x k ROW-MAJOR block
 * (ldx >= k), solved IN PLACE.  Block b covers the rows b p .. min(n, (b + 1) p) - 1 (batch = ceil(n / p)); its factor is the
 * p x p column-major triangle at d_r + b * stride exactly as the batched ExPOTRF leaves it (ldr >= max(1, p); stride >=
 * ldr * p with more than one block).  A last block of pl = n - (batch - 1) p < p rows uses the leading pl x pl part of its
 * triangle (the factor of a leading submatrix is the leading part of the factor); the rest of that triangle is not read.
 * With G_b = F^T F, F = R for uplo 'U' and F = L^T for 'L':
 *     sweep '1'  F^T Y = B  by substitution, rows ascending
 *     sweep '2'  F Z = Y    rows descending
 *     sweep 'B'  '1' then '2' in one launch (X read and written once, the triangle read once); bit for bit '1', then '2'.
 * Every output follows ExTRSV's row step, x_ij = fl( Round( b_ij - sum_{c before i} op(F)(i, c) x_cj ) / F(i, i) ): the sum
 * exact over the already fixed doubles and rounded ONCE in the current rounding mode, then ONE IEEE division (never a
 * multiplication by a reciprocal).  Column j of block b is bit for bit what exblas_extrsv_dev writes for (uplo, diag 'N',
 * the block's row count, the block's triangle, ldr) on the vector at X + b p ldx + j with incx = ldx, sweep '1' being trans
 * 'T' for 'U' and 'N' for 'L', sweep '2' the other trans; so is what exblas_extrsm_dev gives on the block.  Every stored
 * entry of the strict triangle counts: zero times Inf is NaN.
 * Never touched: the other triangle, the padding of R (ldr, stride), the padding of a row of X, the unused trailing part of
 * the last block's triangle.  Columns and blocks are independent.  The bits do not depend on k, ldx, the column tile, the
 * number of blocks a wave carries, the grid, the path, fpe (0 or 2..8), early_exit, the context or the stream.
 * The info word of the factorisation is NOT consulted: solving with a block whose factorisation broke down is the
 * caller's concern (read the batched ExPOTRF's d_info first).
 * fpe == 0 / 1 / >= 9 as for the batched ExPOTRF (fpe == 1: s = b_i, then s -= F x over the solved rows ascending).
 * REFUSED with hipErrorInvalidValue before the device is touched: p > 64, p < 1 with n > 0, a bad uplo or sweep (1, 2, B or
 * b), negative sizes, ldr < max(1, p), stride < ldr * p with more than one block, ldx < k, fpe < 0, null pointers when
 * anything would be launched.  n == 0 or k == 0: success, nothing is launched.
 * ONE launch, no mailbox; capturable after one call.  Lanes own (block, column) pairs: with the column tile kc = min(k, 64)
 * rounded up to a power of two a wave carries 64 / kc consecutive blocks, fewer where its share of LDS does not hold their
 * triangles and its panel of X.  Returns 0, EXBLAS_UNSUPPORTED or a hipError_t.
 * Not provided: variable block sizes, p > 64, fusing the apply into ExSpMM, a device-side check of the factor's info. */
int exblas_expotrs_batched_dev(char uplo, char sweep, int p, int64_t n, int k, const double *d_r, int ldr, int64_t stride,
                               double *d_x, int64_t ldx, int fpe, int early_exit, void *stream);
/* Test hook for the batched ExPOTRS (same bits on every path): 0 automatic, 1 every output rounded from the integer
 * accumulator, 2 one block per wave, 3 column tiles of 4 (the seams between tiles then occur at small k). */
void exblas_set_potrs_batched_path(int mode);
/* The most recent batched ExPOTRS on this device: out[0] outputs rounded in registers, out[1] outputs rounded from the
 * integer accumulator, out[2] = out[3] = 0.  out[0] + out[1] == n * k for one sweep and 2 n k for 'B' (both 0 for
 * fpe == 1); all 0 after a call that launched nothing.  Synchronises the device.  Returns 0 or a hipError_t. */
int exblas_last_potrs_batched_info(int64_t *out4);
/* Batched ExGETRF: the exact-sum LU factorisation with partial pivoting of `batch` independent small GENERAL matrices (the
 * diagonal blocks of a block-Jacobi preconditioner of a nonsymmetric or indefinite operator) in ONE launch, on device
 * pointers, IN PLACE.  order 'C': element (i, j) of matrix b is at d_a[b * stride + i + j * lda]; order 'R': at
 * d_a[b * stride + i * lda + j] (lda >= max(1, p); stride >= lda * p when batch > 1; all offsets 64-bit).  The LU of A^T is
 * not the LU of A: `order` says which of the two is meant.  Storage follows LAPACK: the unit-lower L strictly below the
 * diagonal, U on and above it, d_ipiv[b * p + j] the 1-based row that step j exchanged with row j (int32, batch * p words,
 * contiguous), d_info[b] = 0 or the breakdown step + 1.
 * The definition is the compact (Doolittle) LU, every entry ONE exact sum over already fixed doubles, rounded once in the
 * current rounding mode.  Step j = 0 .. p - 1 on the working matrix W (A on entry, rows swapped as the steps go):
 *   1. candidates  c_i = Round( w_ij - sum_{k<j} l_ik u_kj )  for every i >= j
 *   2. pivot       piv = the smallest i >= j at which |c_i| is largest (a NaN ranks above +Inf); d_ipiv[j] = piv + 1
 *   3. breakdown   c_piv is 0 (either sign) or NaN: the candidates are stored in column j, rows j .. p - 1, with no swap at
 *                  this step, d_ipiv[i] = i + 1 for i >= j, d_info[b] = j + 1, the rest of the matrix stays as it is (the
 *                  original entries in the row order reached so far).  An infinite pivot is no breakdown: IEEE goes on.
 *   4. column of L rows j and piv of W are swapped whole; u_jj = c_piv; l_ij = fl( c_i / u_jj ), ONE IEEE division, i > j
 *   5. row of U    u_ji = Round( w_ji - sum_{k<j} l_jk u_ki )  for i > j
 * Every stored entry counts (0 * Inf is NaN).  d_ipiv and d_info are written for every matrix by every call that launches,
 * with plain stores.  The bits of a matrix depend on its data and the rounding mode only: not on batch, its position, its
 * neighbours, order, lda, stride, the path (exblas_set_getrf_batched_path), fpe (0 or 2..8), early_exit, the context or the
 * stream.  A NaN matrix or a breakdown changes no bit of another matrix.  The lda padding and the gap between matrices are
 * neither read nor written.
 * fpe == 0 rounds every output from an integer accumulator; fpe == 1 is the plain fp64 factorisation of the same structure
 * (s = w, then s -= l * u for k ascending; deterministic, not exact; counters 0); fpe >= 9: EXBLAS_UNSUPPORTED.
 * REFUSED with hipErrorInvalidValue before the device is touched: p > EXBLAS_GETRF_BATCHED_MAX_P, an order other than C, c,
 * R, r, p < 0, batch < 0, lda < max(1, p), batch > 1 with stride < lda * p, fpe < 0, and a null d_a, d_ipiv or d_info when
 * anything would be launched.  p == 0 or batch == 0: success, nothing is launched, nothing is written.
 * ONE stream-ordered kernel launch and nothing else: no memset, no mailbox, no spin-wait, no host synchronisation.  One wave
 * walks a matrix; for p <= 32 a wave carries 64 / pw matrices, pw = p rounded up to a power of two.  The only workspace is
 * that of the counters (16 bytes per workgroup).  Capturable into a hipGraph after one call on the context.  Returns 0,
 * EXBLAS_UNSUPPORTED or a hipError_t.
 * Not provided: A^T solves, p > 64, variable block sizes, complete or rook pivoting, LAPACK's continue-after-zero-pivot
 * rule, a non-batched entry (batch = 1 serves), fp32. */
#define EXBLAS_GETRF_BATCHED_MAX_P 64
int exblas_exgetrf_batched_dev(char order, int p, int64_t batch, double *d_a, int lda, int64_t stride, int *d_ipiv, int *d_info,
                               int fpe, int early_exit, void *stream);
/* Test hook for the batched ExGETRF (same bits on every path): 0 automatic, 1 every output rounded from the integer
 * accumulator, 2 no packing (one matrix per wave), 3 one matrix per workgroup item on a handful of workgroups. */
void exblas_set_getrf_batched_path(int mode);
/* The most recent batched ExGETRF on this device: out[0] roundings done in registers, out[1] roundings done from the
 * integer accumulator, out[2] = out[3] = 0.  For fpe != 1, out[0] + out[1] is the number of roundings: p^2 for a complete
 * matrix, sum_{s<j} (2 (p - s) - 1) + (p - j) for a breakdown at step j; both 0 for fpe == 1; all 0 after a call that
 * launched nothing.  Synchronises the device; valid until the next call that uses the workspace. */
int exblas_last_getrf_batched_info(int64_t *out4);
/* Batched ExGETRS, the apply of a block-Jacobi preconditioner with general blocks, on device pointers: d_x is an n x k
 * ROW-MAJOR block (ldx >= k), solved IN PLACE, X_b := A_b^-1 X_b for every block b of p rows (batch = ceil(n / p)).  d_lu,
 * ldlu, stride, order and d_ipiv are what the batched ExGETRF left.  A last block of rows = n - (batch - 1) p < p rows uses
 * the leading rows x rows part of its factors and its first `rows` pivots.
 *   1. interchanges  for j = 0 .. rows - 1 in order, rows j and d_ipiv[b * p + j] - 1 of the block are swapped.  An index
 *                    outside 1 .. rows is skipped and never dereferenced: garbage pivots read and write nothing out of bounds.
 *   2. forward       y_i = Round( b_i - sum_{c<i} l_ic y_c ), unit diagonal, no division
 *   3. backward      z_i = fl( Round( y_i - sum_{c>i} u_ic z_c ) / u_ii ), ONE IEEE division
 * This is ExTRSV's row step: column j of block b is bit for bit what exblas_extrsv_dev ('L', 'N', 'U') followed by ('U', 'N',
 * 'N') gives on the permuted column.  The info words of the factorisation are NOT consulted.  The bits do not depend on k,
 * ldx, order, the column tile, the grid, the path, fpe (0 or 2..8), early_exit, the context or the stream.
 * REFUSED with hipErrorInvalidValue before the device is touched: p > 64, p < 1 with n > 0, a bad order, negative sizes,
 * ldlu < max(1, p), stride < ldlu * p with more than one block, ldx < k, fpe < 0, null pointers when anything would be
 * launched.  n == 0 or k == 0: success, nothing is launched.  fpe >= 9: EXBLAS_UNSUPPORTED.
 * ONE launch, no mailbox; capturable after one call.  Returns 0, EXBLAS_UNSUPPORTED or a hipError_t.
 * Not provided: A^T solves, variable block sizes, p > 64, fusing the apply into ExSpMM. */
int exblas_exgetrs_batched_dev(char order, int p, int64_t n, int k, const double *d_lu, int ldlu, int64_t stride,
                               const int *d_ipiv, double *d_x, int64_t ldx, int fpe, int early_exit, void *stream);
/* Test hook for the batched ExGETRS (same bits on every path): 0 automatic, 1 every output rounded from the integer
 * accumulator, 2 one block per wave, 3 column tiles of 4. */
void exblas_set_getrs_batched_path(int mode);
/* The most recent batched ExGETRS on this device: out[0] outputs rounded in registers, out[1] outputs rounded from the
 * integer accumulator, out[2] = out[3] = 0.  out[0] + out[1] == 2 n k (both 0 for fpe == 1); all 0 after a call that
 * launched nothing.  Synchronises the device.  Returns 0 or a hipError_t. */
int exblas_last_getrs_batched_info(int64_t *out4);
/* ExGEMM on device pointers, row-major (ExGEMM.Launcher.hpp; kernel gemm, ExGEMM.Superacc.cl:200-283). */
int exblas_exgemm_dev(char transa, char transb, int m, int n, int k, double alpha,
                      const double *d_a, int lda, const double *d_b, int ldb, double beta,
                      double *d_c, int ldc, int fpe, int early_exit, void *stream);
/* Deterministic counter-based input generators, bit-identical to oracle/exblas_oracle.c:orc_gen_ctr;
 * element index range [first, first+count) of a vector of n_total elements. */
int exblas_gen_dev(int kind, uint64_t seed, int64_t first, int64_t count, int64_t n_total,
                   double p0, double p1, double *d_out, void *stream);
/* Plain streaming read (sum of doubles, not exact): measures the box's achievable read bandwidth,
 * the second roofline denominator of BASELINE.md section 3. */
int exblas_stream_read_dev(const double *d_a, int64_t n, void *stream, double *d_sink);
/* the same for the two-stream (ExDOT) access pattern: plain fp64 dot, blocks_per_cu <= 0 uses the ExDOT geometry */
int exblas_stream_read2_dev(const double *d_a, const double *d_b, int64_t n, int blocks_per_cu, void *stream,
                            double *d_sink);

/* ---- (2a) context handles ---------------------------------------------------------------------- */
/* The reference launchers keep their kernels and buffers in file-static globals (src/gpu/blas/blas1/ExSUM.Launcher.cpp:
 * 16-36): one call at a time per process.  The *_dev layer above relaxes that to "one ordered sequence per device"; a
 * handle relaxes it completely: exblas_ctx_create (on the current device) allocates private group accumulators (both
 * slots), flag words and -- on first use -- a private workspace; the *_ctx functions are the *_dev functions on that
 * state (handle NULL = the device's default context = exactly the *_dev call).  Calls on ONE handle must still be
 * ordered on the device; calls on different handles need no ordering at all.  A handle belongs to the device it was
 * created on: using it while another device is current returns hipErrorInvalidDevice (101).  exblas_ctx_destroy
 * synchronises the device and frees everything the handle owns (graphs captured through it must not be replayed
 * afterwards).  Tuning knobs (exblas_set_tuning, exblas_set_gemm_path, ...) are inherited at creation. */
typedef struct exblas_ctx exblas_ctx_t;
int exblas_ctx_create(exblas_ctx_t **ctx);
int exblas_ctx_destroy(exblas_ctx_t *ctx);
int exblas_exsum_ctx(exblas_ctx_t *ctx, const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                     void *stream, int64_t *d_out);
int exblas_exdot_ctx(exblas_ctx_t *ctx, const double *d_a, int64_t inca, const double *d_b, int64_t incb, int64_t n,
                     int fpe, int early_exit, void *stream, int64_t *d_out);
int exblas_exsum_accumulate_ctx(exblas_ctx_t *ctx, const double *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                                void *stream);
int exblas_exdot_accumulate_ctx(exblas_ctx_t *ctx, const double *d_a, int64_t inca, const double *d_b, int64_t incb,
                                int64_t n, int fpe, int early_exit, void *stream);
int exblas_finish_ctx(exblas_ctx_t *ctx, void *stream, int64_t *d_out);
/* the narrow-input entries (see exblas_exsum_lp_dev) on a handle */
int exblas_exsum_lp_ctx(exblas_ctx_t *ctx, int dtype, const void *d_a, int64_t n, int64_t inca, int fpe, int early_exit,
                        void *stream, int64_t *d_out);
int exblas_exdot_lp_ctx(exblas_ctx_t *ctx, int dtype, const void *d_a, int64_t inca, const void *d_b, int64_t incb,
                        int64_t n, int fpe, int early_exit, void *stream, int64_t *d_out);
int exblas_exsum_lp_accumulate_ctx(exblas_ctx_t *ctx, int dtype, const void *d_a, int64_t n, int64_t inca, int fpe,
                                   int early_exit, void *stream);
int exblas_exdot_lp_accumulate_ctx(exblas_ctx_t *ctx, int dtype, const void *d_a, int64_t inca, const void *d_b,
                                   int64_t incb, int64_t n, int fpe, int early_exit, void *stream);
int exblas_round_records_ctx(exblas_ctx_t *ctx, const int64_t *d_records, int64_t count, int64_t stride_words, int dtype,
                             void *d_out, void *stream);
int exblas_exgemv_ctx(exblas_ctx_t *ctx, char transa, int m, int n, double alpha, const double *d_a, int lda,
                      const double *d_x, int incx, double beta, double *d_y, int incy, int fpe, int early_exit,
                      void *stream);
int exblas_extrsv_ctx(exblas_ctx_t *ctx, char uplo, char transa, char diag, int n, const double *d_a, int lda,
                      double *d_x, int incx, int fpe, int early_exit, void *stream);
int exblas_extrsm_ctx(exblas_ctx_t *ctx, char uplo, char transa, char diag, int n, int k, const double *d_a, int lda,
                      double *d_x, int64_t ldx, int fpe, int early_exit, void *stream);
int exblas_exgemm_ctx(exblas_ctx_t *ctx, char transa, char transb, int m, int n, int k, double alpha,
                      const double *d_a, int lda, const double *d_b, int ldb, double beta, double *d_c, int ldc,
                      int fpe, int early_exit, void *stream);
int exblas_exspmv_csr_ctx(exblas_ctx_t *ctx, int m, int n, int index_bits, const void *d_row_ptr,
                          const void *d_col_idx, const double *d_val, double alpha, const double *d_x, double beta,
                          double *d_y, int fpe, int early_exit, void *stream);
int exblas_exspilu0_csr_ctx(exblas_ctx_t *ctx, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                            const double *d_val, double *d_lu, int64_t *d_info, int fpe, int early_exit, void *stream);
int exblas_exspic0_csr_ctx(exblas_ctx_t *ctx, int m, int index_bits, const void *d_row_ptr, const void *d_col_idx,
                           const double *d_val, double *d_ll, int64_t *d_info, int fpe, int early_exit, void *stream);
int exblas_exsptrsv_csr_ctx(exblas_ctx_t *ctx, char uplo, char diag, int m, int index_bits, const void *d_row_ptr,
                            const void *d_col_idx, const double *d_val, double *d_x, int fpe, int early_exit, void *stream);
int exblas_exsptrsm_csr_ctx(exblas_ctx_t *ctx, char uplo, char diag, int m, int k, int index_bits, const void *d_row_ptr,
                            const void *d_col_idx, const double *d_val, double *d_x, int64_t ldx, int fpe, int early_exit,
                            void *stream);
int exblas_exspmm_csr_ctx(exblas_ctx_t *ctx, int m, int n, int k, int index_bits, const void *d_row_ptr,
                          const void *d_col_idx, const double *d_val, double alpha, const double *d_x, int64_t ldx,
                          double beta, double *d_y, int64_t ldy, int fpe, int early_exit, void *stream);
int exblas_exspmv_csr_lp_ctx(exblas_ctx_t *ctx, int m, int n, int index_bits, const void *d_row_ptr,
                             const void *d_col_idx, int val_dtype, const void *d_val, double alpha, int vec_dtype,
                             const void *d_x, double beta, void *d_y, int fpe, int early_exit, void *stream);
int exblas_exspmm_csr_lp_ctx(exblas_ctx_t *ctx, int m, int n, int k, int index_bits, const void *d_row_ptr,
                             const void *d_col_idx, int val_dtype, const void *d_val, double alpha, int vec_dtype,
                             const void *d_x, int64_t ldx, double beta, void *d_y, int64_t ldy, int fpe, int early_exit,
                             void *stream);
int exblas_exbdot_ctx(exblas_ctx_t *ctx, char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx,
                      const double *d_y, int64_t ldy, double *d_c, int64_t ldc, int fpe, int early_exit, void *stream);
int exblas_exbgemm_ctx(exblas_ctx_t *ctx, int64_t n, int p, int q, double alpha, const double *d_x, int64_t ldx,
                       const double *d_c, int64_t ldc, double beta, double *d_y, int64_t ldy, int fpe, int early_exit,
                       void *stream);
int exblas_exbtrsm_ctx(exblas_ctx_t *ctx, char uplo, char transt, char diag, int64_t n, int p, double alpha,
                       const double *d_t, int ldt, double *d_x, int64_t ldx, int fpe, int early_exit, void *stream);
int exblas_expotrf_ctx(exblas_ctx_t *ctx, char uplo, int p, double *d_g, int ldg, int *d_info, int fpe, int early_exit,
                       void *stream);
int exblas_expotrf_batched_ctx(exblas_ctx_t *ctx, char uplo, int p, int64_t batch, double *d_g, int ldg, int64_t stride,
                               int *d_info, int fpe, int early_exit, void *stream);
int exblas_expotrs_batched_ctx(exblas_ctx_t *ctx, char uplo, char sweep, int p, int64_t n, int k, const double *d_r, int ldr,
                               int64_t stride, double *d_x, int64_t ldx, int fpe, int early_exit, void *stream);
int exblas_exgetrf_batched_ctx(exblas_ctx_t *ctx, char order, int p, int64_t batch, double *d_a, int lda, int64_t stride,
                               int *d_ipiv, int *d_info, int fpe, int early_exit, void *stream);
int exblas_exgetrs_batched_ctx(exblas_ctx_t *ctx, char order, int p, int64_t n, int k, const double *d_lu, int ldlu,
                               int64_t stride, const int *d_ipiv, double *d_x, int64_t ldx, int fpe, int early_exit,
                               void *stream);
int exblas_exbdot_export_ctx(exblas_ctx_t *ctx, char mode, int64_t n, int p, int q, const double *d_x, int64_t ldx,
                             const double *d_y, int64_t ldy, int64_t *d_sets, int fpe, int early_exit, void *stream);
int exblas_exbdot_round_ctx(exblas_ctx_t *ctx, char mode, int p, int q, const int64_t *d_sets, int nsets, double *d_c,
                            int64_t ldc, void *stream);
int exblas_reserve_workspace_ctx(exblas_ctx_t *ctx, size_t bytes);
size_t exblas_workspace_bytes_ctx(exblas_ctx_t *ctx);
int exblas_last_gemm_info_ctx(exblas_ctx_t *ctx, int *out8);

/* ---- (2b) multi-GPU: one process per GPU ----------------------------------------------------- */
/* The reference reduces across processes inside the library call: local reduction, MPI_Reduce(MPI_LONG, MPI_SUM) of
 * the normalised limbs, Round on the root (src/cpu/blas/blas1/ExSUM.cpp:142-152, :266-273; scatter :33-63).  Here:
 * local reduction on each GPU, ONE int64-sum all-reduce launch over the 576-byte main digit set and the two extension sets
 * of the same size (low / high digits = ExDOT products below 2^-968 / beyond the double range, all zero otherwise), the
 * same carry-propagation +
 * rounding kernel on every rank.  Integer addition is order-free, so the result is bit-identical for any number of
 * ranks and any shard boundaries.  ExGEMV / ExGEMM shard the outputs (no reduction collective): x resp. B is
 * replicated by one broadcast, y resp. C completed by an all-gather that overlaps the remaining compute.
 *
 * A communicator wraps a transport: RCCL (resolved at run time with dlopen("librccl.so.1"); collectives are
 * enqueued on the caller's stream, nothing synchronises) or three host callbacks (what an MPI program passes to keep
 * MPI_Allreduce / MPI_Bcast / MPI_Allgatherv as the transport, and what lets several ranks share one GPU in tests;
 * this transport synchronises the stream around each callback).  All functions return 0, a hipError_t value, or
 * EXBLAS_COMM_ERROR for a transport failure (message on stderr). */
typedef struct exblas_comm exblas_comm_t;
#define EXBLAS_UNIQUE_ID_BYTES 128
#define EXBLAS_COMM_ERROR (-2)
/* rank 0: make an id (ncclGetUniqueId) and hand the 128 bytes to every rank by any means (MPI_Bcast, a file, a store) */
int exblas_comm_unique_id(void *id128);
/* every rank, current device = its GPU: ncclCommInitRank */
int exblas_comm_init_rccl(exblas_comm_t **comm, int nranks, int rank, const void *id128);
/* wrap an ncclComm_t the application already has (not destroyed by exblas_comm_destroy) */
int exblas_comm_adopt_rccl(exblas_comm_t **comm, void *nccl_comm, int nranks, int rank);
/* host transport; the callbacks operate in place on host memory and return 0 on success:
 *   allreduce: buf[0..count) := element-wise int64 sum over all ranks
 *   bcast:     the root's `bytes` bytes of buf reach every rank
 *   allgatherv: rank r owns bytes [off[r], off[r+1]) of buf (off has nranks+1 entries, off[0] == 0); afterwards every
 *               rank holds all off[nranks] bytes */
typedef int (*exblas_host_allreduce_i64_fn)(void *user, int64_t *buf, int64_t count);
typedef int (*exblas_host_bcast_fn)(void *user, void *buf, int64_t bytes, int root);
typedef int (*exblas_host_allgatherv_fn)(void *user, void *buf, const int64_t *off);
int exblas_comm_init_host(exblas_comm_t **comm, int nranks, int rank, exblas_host_allreduce_i64_fn allreduce,
                          exblas_host_bcast_fn bcast, exblas_host_allgatherv_fn allgatherv, void *user);
int exblas_comm_destroy(exblas_comm_t *comm);
int exblas_comm_rank(const exblas_comm_t *comm);
int exblas_comm_size(const exblas_comm_t *comm);
/* [first, last) of rank's contiguous shard of n items; boundaries are even, so fp64 shards stay 16-byte aligned */
void exblas_shard_range(int64_t n, int rank, int nranks, int64_t *first, int64_t *last);
/* ExSUM / ExDOT of the concatenation of every rank's local array(s): d_out (EXBLAS_OUT_WORDS int64, device) holds
 * the SAME record on every rank.  = exblas_ex*_accumulate_dev + exblas_allreduce_finish_dev. */
int exblas_exsum_allreduce_dev(exblas_comm_t *comm, const double *d_a_local, int64_t n_local, int64_t inca, int fpe,
                               int early_exit, void *stream, int64_t *d_out);
int exblas_exdot_allreduce_dev(exblas_comm_t *comm, const double *d_a_local, int64_t inca, const double *d_b_local,
                               int64_t incb, int64_t n_local, int fpe, int early_exit, void *stream, int64_t *d_out);
/* The second half alone: normalise the selected accumulator slot (exblas_finish_dev), all-reduce the digit set,
 * carry-propagate + round.  A caller that pipelines reductions runs this on a second stream while the next streaming
 * kernel fills the other slot (bench.py). */
int exblas_allreduce_finish_dev(exblas_comm_t *comm, void *stream, int64_t *d_out);
/* Throughput form for a caller that runs reduction after reduction (bench.py's step loop): ONE call per reduction.  The
 * streaming kernel runs on `stream` into the accumulator slot the communicator alternates (0, 1, 0, ...); the second half
 * -- normalise, all-reduce, carry-propagate + round into d_out -- is enqueued on the communicator's own side stream behind
 * an event, so it overlaps the NEXT call's streaming kernel (a slot is reused only after its second half has left it
 * zero: the call waits for that -- on the HOST, for at most EXBLAS_PIPE_SPIN_US microseconds (default 500; the host
 * then runs at most two reductions ahead of the device), after that by making `stream` wait; a wait packet in front of
 * the streaming kernel would expose its launch latency on every call).  d_out of call i is complete once work ordered after
 * exblas_pipeline_drain_dev(comm, stream) runs (which also re-selects slot 0); use distinct d_out buffers for reductions
 * in flight (two).  ev_kernel_start / ev_kernel_end: optional hipEvent_t that bracket the streaming kernel (attached to
 * its dispatch packet: they carry the kernel's own start / stop timestamps; bench.py times the kernel with them), NULL
 * otherwise.  Uses the device's default context: do not interleave with
 * exblas_*_accumulate_dev / exblas_finish_dev on it before draining. */
int exblas_exsum_allreduce_pipelined_dev(exblas_comm_t *comm, const double *d_a_local, int64_t n_local, int64_t inca,
                                         int fpe, int early_exit, void *stream, int64_t *d_out, void *ev_kernel_start,
                                         void *ev_kernel_end);
int exblas_exdot_allreduce_pipelined_dev(exblas_comm_t *comm, const double *d_a_local, int64_t inca,
                                         const double *d_b_local, int64_t incb, int64_t n_local, int fpe, int early_exit,
                                         void *stream, int64_t *d_out, void *ev_kernel_start, void *ev_kernel_end);
int exblas_pipeline_drain_dev(exblas_comm_t *comm, void *stream);
/* Row-sharded ExBDOT: every rank holds n_local rows of X and Y (any split of the rows, n_local == 0 included; p, q, mode
 * the same on every rank) and receives the same C -- bit for bit exblas_exbdot_dev on the blocks of all ranks stacked in
 * any order (the contract at exblas_exbdot_round_dev).  Per batch of outputs (one up to 4096 outputs in 'D' or 64 x 64 in
 * 'G'): the rank's normalised sets (exblas_exbdot_export_dev, in the workspace), ONE int64-sum all-reduce over
 * outputs_of_batch * EXBLAS_SET_WORDS words, the round.  Number, order and length of the collectives depend on
 * (mode, p, q) only -- never on n_local, the path or fpe.  Decided before the first collective, the same way on every
 * rank: the argument rules of exblas_exbdot_dev, fpe == 1 (hipErrorInvalidValue: nothing to all-reduce), and early_exit
 * with fpe > 8 (returns 0: no collective, C untouched, as exblas_exgemv_sharded_dev).  A one-rank host communicator
 * without callbacks skips the collective.  Uses the device's default context. */
int exblas_exbdot_allreduce_dev(exblas_comm_t *comm, char mode, int64_t n_local, int p, int q, const double *d_x_local,
                                int64_t ldx, const double *d_y_local, int64_t ldy, double *d_c, int64_t ldc, int fpe,
                                int early_exit, void *stream);
/* Row-sharded ExGEMV.  transa 'N': rank r owns rows [first, last) = exblas_shard_range(m, r, size) of A and y;
 * d_a_local is that row block (column-major, leading dimension lda >= last - first).  transa 'T': rank r owns the
 * OUTPUTS [first, last) of n, i.e. columns first..last-1 of A; d_a_local points at column `first`.  d_x is the full
 * vector on every rank; x_root >= 0 broadcasts it from that rank first, x_root < 0 says it is already replicated.
 * d_y is the full vector on every rank: on entry a rank's own part holds its input (beta != 0); gather != 0: on return
 * every rank holds all of y (in-place all-gather); gather == 0: only the rank's own part is written and NO collective
 * is issued after the product (y stays sharded: what a caller that keeps iterating on row blocks wants).
 * early_exit with fpe > 8 is the reference's silent no-op: nothing is computed or communicated, on any rank. */
int exblas_exgemv_sharded_dev(exblas_comm_t *comm, char transa, int m, int n, double alpha, const double *d_a_local,
                              int lda, double *d_x, int incx, int x_root, double beta, double *d_y, int incy, int gather,
                              int fpe, int early_exit, void *stream);
/* Row-sharded ExGEMM (row-major): rank r owns rows [first, last) = exblas_shard_range(m, r, size) of op(A) and C;
 * d_a_local points at the rank's first row of op(A) (for transa 'T': column `first` of the stored k x m matrix).
 * d_b: all of op(B)'s storage on every rank, broadcast from b_root first when b_root >= 0.  d_c: the full m x ldc
 * matrix on every rank; a rank's own rows hold its input (beta != 0).  gather != 0: on return every rank holds all of C
 * (with the RCCL transport the all-gather of a finished row chunk overlaps the computation of the next one);
 * gather == 0: only the rank's own rows are written, no collective follows the product -- with b_root < 0 the call
 * then issues no collective at all (rows of C are independent units; the reference has no distributed GEMM to imitate,
 * and an m x n all-gather costs more than the product itself from 4 GPUs up). */
int exblas_exgemm_sharded_dev(exblas_comm_t *comm, char transa, char transb, int m, int n, int k, double alpha,
                              const double *d_a_local, int lda, double *d_b, int ldb, int b_root, double beta,
                              double *d_c, int ldc, int gather, int fpe, int early_exit, void *stream);

/* ---- (1) host-pointer layer (reference semantics; copies H2D per call like gpu:ExSUM.cpp:126) -- */
/* exsum / exdot of host vectors spread one call over several GPUs of the node (each streams its contiguous part in
 * 64 MiB chunks through its own PCIe link; the 576-byte digit sets of the parts are added and rounded once): the
 * reference's rank-0 scatter (cpu:ExSUM.cpp:33-63) inside one process.  Default: every visible device for inputs of
 * 256 MiB or more in a stand-alone process; always the current device only in a one-process-per-GPU job (a launcher's
 * WORLD_SIZE / OMPI_COMM_WORLD_SIZE / PMI_SIZE / SLURM_NTASKS > 1 in the environment, or a communicator of
 * more than one rank created through exblas_comm_*), where every rank sees its peers' devices;
 * `EXBLAS_HOST_DEVICES=all|current|0,1,...` or this call override it
 * (count == 0 restores the default; a device may be listed twice -- two independent parts on one GPU).  The result
 * does not depend on the choice.  exgemv / exgemm / extrsv always use the current device. */
int exblas_set_host_devices(int count, const int *devices);
double exblas_exsum(int Ng, const double *ag, int inca, int offset, int fpe, int early_exit);
double exblas_exdot(int Ng, const double *ag, int inca, int offseta, const double *bg, int incb,
                    int offsetb, int fpe, int early_exit);
int exblas_exgemv(char transa, int m, int n, double alpha, const double *a, int lda, int offseta,
                  const double *x, int incx, int offsetx, double beta, double *y, int incy,
                  int offsety, int fpe, int early_exit);
/* blas2.hpp:57 extrsv; returns 0, or -1 (message on stderr, x untouched) for fpe >= 9 */
int exblas_extrsv(char uplo, char transa, char diag, int n, const double *a, int lda, int offseta, double *x,
                  int incx, int offsetx, int fpe, int early_exit);
int exblas_exgemm(char transa, char transb, int m, int n, int k, double alpha, const double *a,
                  int lda, const double *b, int ldb, double beta, double *c, int ldc, int fpe,
                  int early_exit);
/* exblas_exspmv_csr_dev on host arrays (row_ptr, col_idx, val, x, y; y updated in place): staged through the device,
 * synchronous.  Returns 0 or hipErrorInvalidValue (also for a negative row_ptr entry). */
int exblas_exspmv_csr(int m, int n, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                      double alpha, const double *x, double beta, double *y, int fpe, int early_exit);
/* exblas_exspmv_csr_lp_dev / exblas_exspmm_csr_lp_dev on host arrays, staged through the current device */
int exblas_exspmv_csr_lp(int m, int n, int index_bits, const void *row_ptr, const void *col_idx, int val_dtype,
                         const void *val, double alpha, int vec_dtype, const void *x, double beta, void *y, int fpe,
                         int early_exit);
int exblas_exspmm_csr_lp(int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx, int val_dtype,
                         const void *val, double alpha, int vec_dtype, const void *x, int64_t ldx, double beta, void *y,
                         int64_t ldy, int fpe, int early_exit);
/* exblas_exspmm_csr_dev on host arrays (X: n rows of ldx, Y: m rows of ldy, updated in place; the padding of Y keeps
 * its values): staged through the device, synchronous.  Returns 0 or hipErrorInvalidValue (also for a negative row_ptr
 * entry). */
int exblas_exspmm_csr(int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                      double alpha, const double *x, int64_t ldx, double beta, double *y, int64_t ldy, int fpe,
                      int early_exit);
/* exblas_exspilu0_csr_dev on host arrays (lu: nnz values out, left as they are on a structural defect; info: two words):
 * staged through the device, synchronous.  Returns 0, hipErrorInvalidValue (also for a negative row_ptr entry) or
 * EXBLAS_SPTRSV_STALLED (see exblas_last_spilu0_info). */
int exblas_exspilu0_csr(int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val, double *lu,
                        int64_t *info, int fpe, int early_exit);
/* exblas_exspic0_csr_dev on host arrays (ll: nnz values out, left as they are on a structural defect; info: two words):
 * staged through the device, synchronous.  Returns 0, hipErrorInvalidValue (also for a negative row_ptr entry) or
 * EXBLAS_SPTRSV_STALLED (see exblas_last_spic0_info). */
int exblas_exspic0_csr(int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val, double *ll,
                       int64_t *info, int fpe, int early_exit);
/* exblas_exsptrsv_csr_dev on host arrays (x: b on entry, the solution on return): staged through the device, synchronous.
 * Returns 0, hipErrorInvalidValue (also for a negative row_ptr entry) or EXBLAS_SPTRSV_STALLED (see
 * exblas_last_sptrsv_info). */
int exblas_exsptrsv_csr(char uplo, char diag, int m, int index_bits, const void *row_ptr, const void *col_idx,
                        const double *val, double *x, int fpe, int early_exit);
/* exblas_exsptrsm_csr_dev on host arrays (x: the m x k row-major block with leading dimension ldx, B on entry, the solution
 * on return; its padding comes back as it went): staged through the device, synchronous.  Returns 0, hipErrorInvalidValue
 * (also for a negative row_ptr entry) or EXBLAS_SPTRSV_STALLED (see exblas_last_sptrsm_info). */
int exblas_exsptrsm_csr(char uplo, char diag, int m, int k, int index_bits, const void *row_ptr, const void *col_idx,
                        const double *val, double *x, int64_t ldx, int fpe, int early_exit);
/* exblas_extrsm_dev on host arrays (a: the n columns of lda; x: the n x k row-major block with leading dimension ldx, B on
 * entry, the solution on return; its padding comes back as it went): staged through the device, synchronous.  Returns 0,
 * hipErrorInvalidValue, EXBLAS_UNSUPPORTED (fpe >= 9: nothing is touched) or EXBLAS_SPTRSV_STALLED (see
 * exblas_last_trsm_info). */
int exblas_extrsm(char uplo, char transa, char diag, int n, int k, const double *a, int lda, double *x, int64_t ldx,
                  int fpe, int early_exit);
/* exblas_exbdot_dev on host arrays (X: n rows of ldx, Y: n rows of ldy, C: p rows of ldc in 'G', p doubles in 'D'; the
 * padding of C keeps its values): staged through the device, synchronous.  Returns 0 or hipErrorInvalidValue. */
int exblas_exbdot(char mode, int64_t n, int p, int q, const double *x, int64_t ldx, const double *y, int64_t ldy,
                  double *c, int64_t ldc, int fpe, int early_exit);
/* exblas_exbgemm_dev on host arrays (X: n rows of ldx, C: p rows of ldc, Y: n rows of ldy, updated in place; the padding
 * of Y keeps its values): staged through the device, synchronous.  Returns 0 or hipErrorInvalidValue. */
int exblas_exbgemm(int64_t n, int p, int q, double alpha, const double *x, int64_t ldx, const double *c, int64_t ldc,
                   double beta, double *y, int64_t ldy, int fpe, int early_exit);
/* exblas_exbtrsm_dev on host arrays (t: the p columns of ldt; x: the n x p row-major block with leading dimension ldx, B on
 * entry, the solution on return; its padding comes back as it went): staged through the device, synchronous.  Returns 0,
 * hipErrorInvalidValue or EXBLAS_UNSUPPORTED (fpe >= 9: nothing is touched). */
int exblas_exbtrsm(char uplo, char transt, char diag, int64_t n, int p, double alpha, const double *t, int ldt, double *x,
                   int64_t ldx, int fpe, int early_exit);
/* exblas_expotrf_dev on a host array (g: the p columns of ldg, factored in place; its padding and the other triangle come
 * back as they went); *info (may be NULL) receives the info word: staged through the device, synchronous.  Returns 0,
 * hipErrorInvalidValue or EXBLAS_UNSUPPORTED (fpe >= 9: nothing is touched). */
int exblas_expotrf(char uplo, int p, double *g, int ldg, int *info, int fpe, int early_exit);
/* exblas_expotrf_batched_dev on host arrays (g: the batch matrices, stride apart, factored in place; padding, gaps and the
 * other triangles come back as they went); info (may be NULL) receives the batch info words: staged through the device,
 * synchronous.  Returns 0, hipErrorInvalidValue or EXBLAS_UNSUPPORTED (fpe >= 9: nothing is touched). */
int exblas_expotrf_batched(char uplo, int p, int64_t batch, double *g, int ldg, int64_t stride, int *info, int fpe,
                           int early_exit);
/* exblas_expotrs_batched_dev on host arrays (r: the ceil(n / p) triangles, stride apart; x: the n x k row-major block with
 * leading dimension ldx, B on entry, the solution on return; its padding comes back as it went): staged through the
 * device, synchronous.  Returns 0, hipErrorInvalidValue or EXBLAS_UNSUPPORTED (fpe >= 9: nothing is touched). */
int exblas_expotrs_batched(char uplo, char sweep, int p, int64_t n, int k, const double *r, int ldr, int64_t stride, double *x,
                           int64_t ldx, int fpe, int early_exit);
/* exblas_exgetrf_batched_dev on host arrays (a: the batch matrices, stride apart, factored in place; padding and gaps come
 * back as they went); ipiv (batch * p words) and info (batch words) may each be NULL: staged through the device,
 * synchronous.  Returns 0, hipErrorInvalidValue or EXBLAS_UNSUPPORTED (fpe >= 9: nothing is touched). */
int exblas_exgetrf_batched(char order, int p, int64_t batch, double *a, int lda, int64_t stride, int *ipiv, int *info, int fpe,
                           int early_exit);
/* exblas_exgetrs_batched_dev on host arrays (lu, ipiv: the ceil(n / p) factored blocks and their pivots; x: the n x k
 * row-major block with leading dimension ldx, B on entry, the solution on return; its padding comes back as it went):
 * staged through the device, synchronous.  Returns 0, hipErrorInvalidValue or EXBLAS_UNSUPPORTED. */
int exblas_exgetrs_batched(char order, int p, int64_t n, int k, const double *lu, int ldlu, int64_t stride, const int *ipiv,
                           double *x, int64_t ldx, int fpe, int early_exit);
/* as exblas_exsum / exblas_exdot, additionally returning the full record (limbs, both roundings) */
int exblas_exsum_record(int Ng, const double *ag, int inca, int offset, int fpe, int early_exit,
                        int64_t *out_words);
int exblas_exdot_record(int Ng, const double *ag, int inca, int offseta, const double *bg, int incb,
                        int offsetb, int fpe, int early_exit, int64_t *out_words);

/* Narrow ExSUM / ExDOT on HOST arrays (see exblas_exsum_lp_dev): the arrays are staged to the current device and the
 * same routine runs there; out_words receives the record.  One device (the fp64 host entries spread over several).
 * The argument refusals of the device entries apply, before the device is touched. */
int exblas_exsum_lp(int dtype, const void *a, int64_t n, int64_t inca, int fpe, int early_exit, int64_t *out_words);
int exblas_exdot_lp(int dtype, const void *a, int64_t inca, const void *b, int64_t incb, int64_t n, int fpe,
                    int early_exit, int64_t *out_words);
#ifdef __cplusplus
}
#endif
#endif /* EXBLAS_HIP_H_ */
