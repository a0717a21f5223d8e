// blas3.hip -- ExGEMM for gfx950, row-major (the reference's layout, tests/test.exgemm.gpu.cpp:183-184).
//
// Replaces the reference's OpenCL kernel gemm (src/gpu/blas/blas3/ExGEMM.Superacc.cl:200-283, ExGEMM.FPE.cl:209-341):
//   C_ij := beta*C_ij + Round( sum_l fl(alpha*A_il) * B_lj ),   every dot product correctly rounded.
// (The reference kernel ignores alpha/beta/trans/ld* and computes C += Round(A*B) for square matrices,
// ExGEMM.Superacc.cl:197-198,:280; with alpha = beta = 1, 'N','N' this is the same value.  The final
// beta*C + s is a plain fp64 multiply-add pair, like the reference's "+=".)
//
// Kernel k_gemm (all variants): 16x16 outputs per workgroup, one output per thread like the reference, but the
// thread's private superaccumulator is a column of an LDS array [limb][thread] (bank = f(lane) only, no
// conflicts, no scratch spills -- the reference's 39 private longs per thread live in scratch memory); A and B
// stream through LDS in 16x32 / 32x16 tiles; products are made exact with TwoProductFMA and pushed, four at a
// time, through the thread's register expansion (or straight into the column for fpe < 3).
#include "superacc.hip.h"
#include "fpe.hip.h"
#include "exblas_internal.h"

namespace exb {

constexpr int GM_T = 16;   // outputs per workgroup edge
constexpr int GM_KB = 32;  // k-depth of one LDS tile
constexpr int GM_THREADS = GM_T * GM_T;

template <int N, bool EE>
__global__ void __launch_bounds__(GM_THREADS) k_gemm(int ta, int tb, int m, int n, int k, double alpha,
                                                     const double *__restrict__ a, long long lda,
                                                     const double *__restrict__ b, long long ldb, double beta,
                                                     double *__restrict__ c, long long ldc, int round_mode,
                                                     const int *__restrict__ gate)
{
    __shared__ long long acc[NL * GM_THREADS];          // 139,264 B: private column per thread
    // Predicated launch: the int8 path (blas3_i8.hip) decides ON THE DEVICE whether the data qualifies for it; this
    // kernel is enqueued behind it either way and does the work only when *gate says "scalar" (0).
    if (gate && *gate != 0) return;
    __shared__ double As[GM_T][GM_KB + 1], Bs[GM_KB][GM_T + 1];
    const int tid = threadIdx.x, tx = tid & (GM_T - 1), ty = tid >> 4;
    // The grid is capped (gemm_variant): a workgroup walks over tiles, so that a predicated launch that has nothing to
    // do costs a few thousand empty workgroups instead of one per 16 x 16 outputs (0.11 ms at 8192 x 8192).
    const int tiles_x = (n + GM_T - 1) / GM_T, tiles_y = (m + GM_T - 1) / GM_T;
    for (long long tile = blockIdx.x; tile < (long long)tiles_x * tiles_y; tile += gridDim.x) {
    const int i0 = (int)(tile / tiles_x) * GM_T, j0 = (int)(tile % tiles_x) * GM_T;
    __syncthreads();  // the previous tile's last reads of As / Bs / acc
    for (int t = tid; t < NL * GM_THREADS; t += GM_THREADS) acc[t] = 0;
    unsigned flags = 0;
    LdsSink<GM_THREADS> sink{acc + tid, flags};
    double f[N > 0 ? N : 1];
#pragma unroll
    for (int q = 0; q < (N > 0 ? N : 1); ++q) f[q] = 0.0;

    Bypass bypass;
    for (int l0 = 0; l0 < k; l0 += GM_KB) {
        __syncthreads();
        // A tile: rows i0..i0+15, depth l0..l0+31 ; B tile: depth x cols j0..j0+15
        for (int t = tid; t < GM_T * GM_KB; t += GM_THREADS) {
            const int r = t / GM_KB, l = t % GM_KB;
            const int gi = i0 + r, gl = l0 + l;
            double v = 0.0;
            if (gi < m && gl < k) v = alpha * (ta ? a[(long long)gl * lda + gi] : a[(long long)gi * lda + gl]);
            As[r][l] = v;
        }
        for (int t = tid; t < GM_KB * GM_T; t += GM_THREADS) {
            const int l = t / GM_T, cc = t % GM_T;
            const int gl = l0 + l, gj = j0 + cc;
            double v = 0.0;
            if (gl < k && gj < n) v = tb ? b[(long long)gj * ldb + gl] : b[(long long)gl * ldb + gj];
            Bs[l][cc] = v;
        }
        __syncthreads();
#pragma unroll 2
        for (int l = 0; l < GM_KB; l += 4) {
            double p[4], e[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) p[u] = two_prod(As[ty][l + u], Bs[l + u][tx], e[u]);
            fpe_absorb_prod_adaptive<N, EE, 4>(f, p, e, sink, bypass);
        }
    }
    fpe_flush_sink<N>(f, sink);
    // finish: every thread normalises and rounds its own column (private, no barrier needed)
    const int gi = i0 + ty, gj = j0 + tx;
    long long loc[NL];
    for (int q = 0; q < NL; ++q) loc[q] = acc[q * GM_THREADS + tid];
    normalize_digits(loc);
    double s;
    if (flags) {
        const bool nan = (flags & FLAG_NAN) || ((flags & FLAG_PINF) && (flags & FLAG_NINF));
        s = nan ? __longlong_as_double(0x7ff8000000000000ll)
                : __longlong_as_double((flags & FLAG_NINF) ? (long long)0xfff0000000000000ull : 0x7ff0000000000000ll);
    } else if (round_mode) {
        long long canon[CANON];
        digits_to_canon(loc, canon);
        s = round_reference(canon);
    } else {
        s = __longlong_as_double((long long)round_exact_bits(loc));
    }
    if (gi < m && gj < n) {
        double *cij = c + (long long)gi * ldc + gj;
        *cij = (beta == 0.0) ? s : beta * (*cij) + s;
    }
    }  // tile loop
}

template <int N, bool EE>
static hipError_t gemm_variant(char transa, char transb, int m, int n, int k, double alpha, const double *a, int lda,
                               const double *b, int ldb, double beta, double *c, int ldc, int round_mode,
                               hipStream_t st, const int *gate)
{
    const int ta = (transa == 'T' || transa == 't'), tb = (transb == 'T' || transb == 't');
    const long long tiles = (long long)((n + GM_T - 1) / GM_T) * ((m + GM_T - 1) / GM_T);
    dim3 grid((unsigned)(tiles < 8192 ? tiles : 8192));  // 1 workgroup per CU (139 KiB of LDS): 32 rounds of 256
    hipLaunchKernelGGL((k_gemm<N, EE>), grid, dim3(GM_THREADS), 0, st, ta, tb, m, n, k, alpha, a, (long long)lda, b,
                       (long long)ldb, beta, c, (long long)ldc, round_mode, gate);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// the operand scan of the three matrix-core paths (blas3_mfma.hip: 21-bit fp64 slices; blas3_i8.hip: base-256 digit
// slices; blas3_crt.hip: residues).  Per vector (row of A' = fl(alpha*A), column of B): the scale exponent (|x| < 2^ea)
// and the lowest set bit; globally: how many bits a vector spans at most (-> slice count), the exponent range, and
// whether anything is non-finite or subnormal (-> scalar kernel).
// ---------------------------------------------------------------------------------------------
struct ScanAcc {
    int emax, lsbmin;
    unsigned bad;
    __device__ __forceinline__ void init() { emax = -100000; lsbmin = 100000; bad = 0; }
    __device__ __forceinline__ void add(double x)
    {
        const unsigned long long u = (unsigned long long)__double_as_longlong(x);
        const unsigned be = (unsigned)(u >> 52) & 0x7ffu;
        const unsigned long long frac = u & 0x000fffffffffffffull;
        if (be == 0) {
            if (frac) bad = 1;  // subnormal input: scalar path
            return;             // zero
        }
        if (be == 0x7ffu) { bad = 1; return; }
        const int e = (int)be - 1023;
        const unsigned long long mant = frac | 0x0010000000000000ull;
        const int lsb = e - 52 + __builtin_ctzll(mant);
        emax = max(emax, e);
        lsbmin = min(lsbmin, lsb);
    }
    __device__ __forceinline__ void merge(const ScanAcc &o)
    {
        emax = max(emax, o.emax);
        lsbmin = min(lsbmin, o.lsbmin);
        bad |= o.bad;
    }
};

// Both scan kernels only fold their part of a vector into vmax[v] / vlsb[v] (atomicMax / atomicMin), so the
// reduction dimension can be split over workgroups; k_scan_finish then derives the scale and the global needs.
__device__ __forceinline__ void scan_publish(const ScanAcc &s, int *vmax, int *vlsb, int *info)
{
    if (s.emax > -50000) {
        atomicMax(vmax, s.emax);
        atomicMin(vlsb, s.lsbmin);
    }
    if (s.bad) atomicOr((unsigned *)&info[INFO_FLAGS], 1u);
}

// vectors whose elements are contiguous (stride 1 along the reduction): one workgroup per vector
static __global__ void __launch_bounds__(256) k_scan_contig(const double *__restrict__ p, long long ldv, int nvec, int len,
                                                     double scale, int *vmax, int *vlsb, int *info)
{
    __shared__ ScanAcc red[256];
    const int v = blockIdx.x;
    if (v >= nvec) return;
    ScanAcc s;
    s.init();
    const double *q = p + (long long)v * ldv;
    for (int i = threadIdx.x; i < len; i += 1024) {  // four loads in flight per thread
        double w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = i + 256 * u < len ? q[i + 256 * u] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s.add(scale * w[u]);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x].merge(red[threadIdx.x + o]);
        __syncthreads();
    }
    if (threadIdx.x == 0) scan_publish(red[0], &vmax[v], &vlsb[v], info);
}

// vectors whose elements are strided by ldv (adjacent vectors are contiguous): one thread per vector and
// per slice of the reduction dimension (blockIdx.y)
static __global__ void __launch_bounds__(256) k_scan_strided(const double *__restrict__ p, long long ldv, int nvec, int len,
                                                      double scale, int *vmax, int *vlsb, int *info)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nvec) return;
    const int per = (len + gridDim.y - 1) / gridDim.y;
    const int i0 = blockIdx.y * per, i1 = min(len, i0 + per);
    ScanAcc s;
    s.init();
    for (int i = i0; i < i1; i += 4) {  // four loads in flight per thread
        double w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = i + u < i1 ? p[(long long)(i + u) * ldv + v] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; ++u) s.add(scale * w[u]);
    }
    scan_publish(s, &vmax[v], &vlsb[v], info);
}

// also resets the info block (first thread), so the whole scan is kernels only: capturable, no host memory involved
static __global__ void __launch_bounds__(256) k_scan_init(int nvec, int *vmax, int *vlsb, int *info)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < nvec) {
        vmax[v] = -100000;
        vlsb[v] = 100000;
    }
    if (v < INFO_WORDS) info[v] = v == INFO_EMIN ? 100000 : (v == INFO_EMAX ? -100000 : 0);
}

// vmax -> scale ea = emax + 1 (in place), and the global slice need / exponent range
static __global__ void __launch_bounds__(256) k_scan_finish(int nvec, int *vmax, const int *vlsb, int *info, int need_slot)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= nvec) return;
    const int e = vmax[v];
    if (e < -50000) {
        vmax[v] = 0;
        return;
    }
    vmax[v] = e + 1;
    atomicMax(&info[need_slot], e + 1 - vlsb[v]);
    atomicMin(&info[INFO_EMIN], e);
    atomicMax(&info[INFO_EMAX], e);
}

void gemm_scan(hipStream_t st, int ta, int tb, int m, int n, int k, double alpha, const double *a, int lda, const double *b,
               int ldb, int *info, int *EA)
{
    int *EB = EA + m, *LA = EB + n, *LB = LA + m;
    hipLaunchKernelGGL(k_scan_init, dim3((m + n + 255) / 256), dim3(256), 0, st, m + n, EA, LA, info);
    const int ysplit = k >= 2048 ? 32 : (k >= 256 ? 8 : 1);
    // rows of A' (reduction over l)
    if (!ta)
        hipLaunchKernelGGL(k_scan_contig, dim3(m), dim3(256), 0, st, a, (long long)lda, m, k, alpha, EA, LA, info);
    else
        hipLaunchKernelGGL(k_scan_strided, dim3((m + 255) / 256, ysplit), dim3(256), 0, st, a, (long long)lda, m, k, alpha,
                           EA, LA, info);
    // columns of B (reduction over l)
    if (!tb)
        hipLaunchKernelGGL(k_scan_strided, dim3((n + 255) / 256, ysplit), dim3(256), 0, st, b, (long long)ldb, n, k, 1.0,
                           EB, LB, info);
    else
        hipLaunchKernelGGL(k_scan_contig, dim3(n), dim3(256), 0, st, b, (long long)ldb, n, k, 1.0, EB, LB, info);
    hipLaunchKernelGGL(k_scan_finish, dim3((m + 255) / 256), dim3(256), 0, st, m, EA, LA, info, INFO_NEED_A);
    hipLaunchKernelGGL(k_scan_finish, dim3((n + 255) / 256), dim3(256), 0, st, n, EB, LB, info, INFO_NEED_B);
}

// one (fpe, early_exit) variant of the scalar kernel on a row block; fpe < 3: superaccumulators only (ExGEMM.cpp:78-87)
static hipError_t gemm_scalar(char transa, char transb, int m, int n, int k, double alpha, const double *a, int lda,
                              const double *b, int ldb, double beta, double *cmat, int ldc, int fpe, int early_exit,
                              int round_mode, hipStream_t st, const int *gate)
{
    hipError_t e = hipSuccess;
    auto go = [&](auto N, auto EE) {
        e = gemm_variant<N(), EE()>(transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, cmat, ldc, round_mode, st, gate);
    };
    if (fpe < 3) go(std::integral_constant<int, 0>(), std::false_type());
    else select_variant<3>(fpe, early_exit, go);  // early exit with fpe > 8 never gets here (exgemm_dispatch)
    return e;
}

// The path table (exblas_set_gemm_path): 0 residues (blas3_crt.hip) for min(m, n) >= CRT_MIN_EDGE, digit slices
// (blas3_i8.hip) below and when the residue workspace cannot be had even for 12 moduli; 4 residues only; 1 the scalar
// kernel; 3 fp64 slices on MFMA-F64 (blas3_mfma.hip, host-decided) in exact-rounding mode, the scalar kernel in
// reference mode; 2 and any other value digit slices.  The int8 paths serve every variant and both rounding modes: the
// result is the correctly rounded exact dot product whichever expansion size the caller names.  The scalar kernel is
// enqueued behind them, predicated on their device-side decision; it runs unconditionally when no path was enqueued.
static hipError_t gemm_paths(Ctx &c, char transa, char transb, int m, int n, int k, double alpha, const double *a, int lda,
                             const double *b, int ldb, double beta, double *cmat, int ldc, int fpe, int early_exit,
                             int round_mode, hipStream_t st, const GemmChunks *chunks, GemmPlan &plan, int &slices)
{
    if (early_exit && fpe > 8) return hipSuccess;  // the reference's silent no-op (ExGEMM.cpp:88-99), on every path
    const bool ta = (transa == 'T' || transa == 't');
    GemmChunks whole;
    whole.n = 1;
    whole.bound[0] = 0;
    whole.bound[1] = m;
    const GemmChunks &ch = chunks ? *chunks : whole;
    const int knob = c.gemm_path;
    if (k > 0 && knob != 1 && knob != 3) {
        hipError_t e = hipSuccess;
        if (knob == 4 || (knob == 0 && m >= CRT_MIN_EDGE && n >= CRT_MIN_EDGE))
            e = exgemm_crt_prepare(c, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, cmat, ldc, round_mode, st,
                                   &plan);
        if (e == hipSuccess && plan.path == PATH_SCALAR && knob != 4)
            e = exgemm_i8_prepare(c, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, cmat, ldc, round_mode, st,
                                  &plan);
        if (e != hipSuccess) return e;
    }
    const int *gate = plan.info ? plan.info + INFO_PATH : nullptr;
    for (int i = 0; i < ch.n; ++i) {
        const int row0 = ch.bound[i], row1 = ch.bound[i + 1];
        if (row1 > row0) {
            const double *ar = ta ? a + row0 : a + (size_t)row0 * lda;
            double *cr = cmat + (size_t)row0 * ldc;
            bool done = false;
            if (plan.path != PATH_SCALAR) {
                hipError_t e = plan.path == PATH_CRT ? exgemm_crt_rows(plan, row0, row1, st)
                                                     : exgemm_i8_rows(plan, row0, row1, st);
                if (e != hipSuccess) return e;
            } else if (knob == 3 && round_mode == 0) {
                hipError_t e = hipSuccess;
                done = exgemm_try_mfma(c, transa, transb, row1 - row0, n, k, alpha, ar, lda, b, ldb, beta, cr, ldc, st, &e,
                                       &slices);
                if (done && e != hipSuccess) return e;
            }
            if (!done) {
                hipError_t e = gemm_scalar(transa, transb, row1 - row0, n, k, alpha, ar, lda, b, ldb, beta, cr, ldc, fpe,
                                           early_exit, round_mode, st, gate);
                if (e != hipSuccess) return e;
            }
        }
        if (ch.hook) {
            const int rc = ch.hook(ch.user, i, st);
            if (rc) return (hipError_t)rc;
        }
    }
    return hipSuccess;
}

// chunks != nullptr: the rows of C are produced chunk by chunk and chunks->hook runs after each (row-sharded GEMM).
hipError_t exgemm_dispatch(Ctx &c, char transa, char transb, int m, int n, int k, double alpha, const double *a,
                           int lda, const double *b, int ldb, double beta, double *cmat, int ldc, int fpe,
                           int early_exit, int round_mode, hipStream_t st, const GemmChunks *chunks)
{
    if (m <= 0 || n <= 0) return hipSuccess;
    GemmPlan plan;
    int slices = 0;
    const hipError_t e = gemm_paths(c, transa, transb, m, n, k, alpha, a, lda, b, ldb, beta, cmat, ldc, fpe, early_exit,
                                    round_mode, st, chunks, plan, slices);
    // what exblas_last_gemm_info reports: the info block of a device-decided path, or the host-decided slice count
    c.gemm_info_dev = plan.info;
    c.last_gemm_slices = slices;
    return e;
}

}  // namespace exb
