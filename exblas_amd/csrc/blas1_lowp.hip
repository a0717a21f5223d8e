// blas1_lowp.hip -- ExSUM / ExDOT on float32, float16 and bfloat16 inputs, and the rounding of records into a narrow format.
//
// Every value of the three types widens to a double exactly, and the product of two of them is an exact double (at most
// 48 significand bits, magnitude in [2^-298, 2^256) or zero).  So the narrow kernels are the fp64 streaming kernels of
// blas1.hip with another front end and LESS behind it: ExDOT needs no TwoProd error term, no range divert and no low /
// high accumulators -- it is ExSUM's cascade fed with products, and flag bits 3 to 6 are never set here.
//   * a lane's 16-byte non-temporal load carries 4 float32 or 8 16-bit elements; U = 4 loads per lane, stream and tile
//     (4096 float32 / 8192 16-bit elements per workgroup tile), two explicit register sets filled alternately with
//     unconditional clamped loads, LDS zeroed after the first loads are in flight -- k_exsum / k_exdot's loop;
//   * a tile is widened and absorbed in chunks of 8 doubles (what the fp64 kernels hold per tile and set), each through
//     fpe_absorb_adaptive into the wave's LDS superaccumulator columns;
//   * the pointer is only element-aligned: up to 3 (float32) / 7 (16-bit) head elements before the first 16-byte boundary
//     and as many tail elements go straight into the accumulator, one lane each.  ExDOT streams vectors when both
//     operands have the SAME misalignment modulo 16 bytes (their heads coincide); otherwise the strided kernel runs;
//   * block_epilogue adds into the context's group accumulators: narrow and fp64 accumulate calls fold into one exact
//     reduction, finished by the one k_finalize.
// Widening: v_cvt_f32_f16 / v_cvt_f64_f32 obey the wave's denormal mode; the library is built without
// -fgpu-flush-denormals-to-zero (build.py: FLAGS), which leaves both modes at "keep" (float_denorm_mode_32 = 3,
// _16_64 = 3 in every kernel descriptor), and the tests feed subnormals of all three types.  bfloat16 is bits << 16 read
// as a float32.  Inf and NaN widen to Inf and NaN and take the range guard's flag path (fpe_guard, lds_add).
#include "blas1_common.hip.h"
#include "round_lowp.hip.h"

namespace exb {

typedef unsigned u4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u4_t ld16(const u4_t *p) { return __builtin_nontemporal_load(p); }

constexpr int ULP = 4;    // 16-byte loads per lane and stream in one tile
constexpr int CHUNK = 8;  // doubles fed to the cascade at once

// element types: `elem` as it lies in memory, VEC elements per 16 bytes, element j of a loaded vector as a double
struct LpF32 {
    typedef float elem;
    static constexpr int VEC = 4;
    static __device__ __forceinline__ double widen(elem v) { return (double)v; }
    static __device__ __forceinline__ double at(const u4_t &r, int j) { return (double)__uint_as_float(r[j]); }
};
struct LpF16 {
    typedef _Float16 elem;
    static constexpr int VEC = 8;
    static __device__ __forceinline__ double widen(elem v) { return (double)(float)v; }
    static __device__ __forceinline__ double at(const u4_t &r, int j)
    {
        const unsigned w = r[j >> 1];
        return widen(__builtin_bit_cast(_Float16, (unsigned short)((j & 1) ? (w >> 16) : (w & 0xffffu))));
    }
};
struct LpBF16 {
    typedef unsigned short elem;   // raw words
    static constexpr int VEC = 8;
    static __device__ __forceinline__ double widen(elem v) { return (double)__uint_as_float((unsigned)v << 16); }
    static __device__ __forceinline__ double at(const u4_t &r, int j)
    {
        const unsigned w = r[j >> 1];
        return (double)__uint_as_float((j & 1) ? (w & 0xffff0000u) : (w << 16));
    }
};

// elements before the first 16-byte boundary (at most n)
template <class T>
__device__ __forceinline__ long long head_of(const typename T::elem *a, long long n)
{
    const long long h = (long long)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) / sizeof(typename T::elem));
    return h < n ? h : n;
}

// chunk `c` (CHUNK consecutive elements of this lane) of a register set as doubles; PROD: times the other stream's
template <class T, bool PROD>
__device__ __forceinline__ void widen_chunk(const u4_t (&ra)[ULP], const u4_t (&rb)[ULP], int c, double (&x)[CHUNK])
{
#pragma unroll
    for (int j = 0; j < CHUNK; ++j) {
        const int e = c * CHUNK + j, u = e / T::VEC, k = e % T::VEC;
        x[j] = PROD ? T::at(ra[u], k) * T::at(rb[u], k) : T::at(ra[u], k);   // (the product is exact)
    }
}

// ---------------------------------------------------------------------------------------------
// contiguous ExSUM (PROD = false, b unused) and vector ExDOT (PROD = true; a and b equally misaligned)
// ---------------------------------------------------------------------------------------------
template <class T, bool PROD, int N, bool EE, int COPIES, int ZM>
__global__ void __launch_bounds__(BLOCK) k_lp_stream(const typename T::elem *__restrict__ a,
                                                     const typename T::elem *__restrict__ b, long long n,
                                                     long long *__restrict__ gacc, unsigned *__restrict__ gflags,
                                                     int ngroups)
{
    constexpr int VEC = T::VEC;
    __shared__ long long s_acc[WAVES * NL * COPIES];
    auto zero_lds = [&]() {   // (after the first tile's loads are in flight, see k_exdot)
        for (int i = threadIdx.x; i < WAVES * NL * COPIES; i += BLOCK) s_acc[i] = 0;
        __syncthreads();
    };
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long *col = s_acc + wave * NL * COPIES + (lane & (COPIES - 1));
    unsigned flags = 0;
    double fpe[N > 0 ? N : 1];
#pragma unroll
    for (int i = 0; i < (N > 0 ? N : 1); ++i) fpe[i] = 0.0;

    const long long head = head_of<T>(a, n);
    const u4_t *va = (const u4_t *)(a + head), *vb = (const u4_t *)((PROD ? b : a) + head);
    const long long nv = (n - head) / VEC;
    const long long tail = (n - head) - nv * VEC;
    constexpr long long TILE = (long long)BLOCK * ULP;
    const long long ntiles = nv / TILE;
    LdsSink<COPIES> sinkm{col, flags};
    Bypass bypass;

    long long t = blockIdx.x;
    if (t < ntiles) {
        // two explicit register sets per stream, filled alternately with unconditional loads (past the end: the last
        // tile again)
        u4_t a0[ULP], a1[ULP], b0[PROD ? ULP : 1], b1[PROD ? ULP : 1];
        auto fill = [&](long long tile, u4_t (&pa)[ULP], u4_t (&pb)[PROD ? ULP : 1]) {
            const long long base = (tile < ntiles ? tile : ntiles - 1) * TILE + threadIdx.x;
#pragma unroll
            for (int u = 0; u < ULP; ++u) {
                pa[u] = ld16(va + base + u * BLOCK);
                if constexpr (PROD) pb[u] = ld16(vb + base + u * BLOCK);
            }
        };
        auto absorb = [&](u4_t (&pa)[ULP], u4_t (&pb)[PROD ? ULP : 1]) {
#pragma unroll
            for (int c = 0; c < ULP * VEC / CHUNK; ++c) {
                double x[CHUNK];
                if constexpr (PROD) widen_chunk<T, true>(pa, pb, c, x);
                else widen_chunk<T, false>(pa, pa, c, x);
                fpe_absorb_adaptive<N, EE, CHUNK, LdsSink<COPIES>, ZM>(fpe, x, sinkm, bypass);
            }
        };
        fill(t, a0, b0);
        zero_lds();
        for (;;) {
            fill(t + gridDim.x, a1, b1);
            absorb(a0, b0);
            t += gridDim.x;
            if (t >= ntiles) break;
            fill(t + gridDim.x, a0, b0);
            absorb(a1, b1);
            t += gridDim.x;
            if (t >= ntiles) break;
        }
    } else {
        zero_lds();
    }
    // remainder vectors, grid-strided one 16-byte vector at a time
    for (long long i = ntiles * TILE + (long long)blockIdx.x * BLOCK + threadIdx.x; i < nv;
         i += (long long)gridDim.x * BLOCK) {
        const u4_t ra = va[i], rb = PROD ? vb[i] : ra;
        double x[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) x[j] = PROD ? T::at(ra, j) * T::at(rb, j) : T::at(ra, j);
        fpe_absorb<N, false, COPIES, VEC>(fpe, x, 0, col, flags);
    }
    // scalar head / tail straight into the superaccumulator, one lane each
    if (blockIdx.x == 0 && (long long)threadIdx.x < head + tail) {
        const long long i = (long long)threadIdx.x < head ? threadIdx.x : n - tail + (threadIdx.x - head);
        lds_add<COPIES>(col, PROD ? T::widen(a[i]) * T::widen(b[i]) : T::widen(a[i]), flags);
    }
    fpe_flush<N, COPIES>(fpe, col, flags);
    block_epilogue<COPIES>(s_acc, flags, gacc, gflags, ngroups);
}

// strided forms a[i inca] (b[i incb]); also ExDOT on contiguous operands of unequal misalignment
template <class T, bool PROD, int N, bool EE, int COPIES>
__global__ void __launch_bounds__(BLOCK) k_lp_strided(const typename T::elem *__restrict__ a, long long inca,
                                                      const typename T::elem *__restrict__ b, long long incb,
                                                      long long n, long long *__restrict__ gacc,
                                                      unsigned *__restrict__ gflags, int ngroups)
{
    __shared__ long long s_acc[WAVES * NL * COPIES];
    for (int i = threadIdx.x; i < WAVES * NL * COPIES; i += BLOCK) s_acc[i] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    long long *col = s_acc + wave * NL * COPIES + (lane & (COPIES - 1));
    unsigned flags = 0;
    double fpe[N > 0 ? N : 1];
#pragma unroll
    for (int i = 0; i < (N > 0 ? N : 1); ++i) fpe[i] = 0.0;
    // four independent loads in flight per lane and stream
    const long long S = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += 4 * S) {
        double x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = i + u * S < n;
            const double xa = in ? T::widen(a[(i + u * S) * inca]) : 0.0;
            if constexpr (PROD) x[u] = in ? xa * T::widen(b[(i + u * S) * incb]) : 0.0;
            else x[u] = xa;
        }
        fpe_absorb<N, false, COPIES, 4>(fpe, x, 0, col, flags);
    }
    fpe_flush<N, COPIES>(fpe, col, flags);
    block_epilogue<COPIES>(s_acc, flags, gacc, gflags, ngroups);
}

// ---------------------------------------------------------------------------------------------
// records -> narrow values.  One lane per record (the rounding is a scalar walk over 68 digits).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_round_records(const long long *__restrict__ rec, long long count,
                                                      long long stride_words, int dtype, void *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const long long *r = rec + i * stride_words;
    const NarrowFormat f = format_of(dtype);
    unsigned long long bits;
    if (r[OUT_FLAGS] & FLAG_NONFINITE) {   // the record's double is +-Inf or NaN: both convert exactly
        const unsigned long long ex = (unsigned long long)r[OUT_EXACT];
        const unsigned long long inf = (unsigned long long)(2 * f.emax + 1) << (f.prec - 1);
        if (ex & 0x000fffffffffffffull) bits = inf | (1ull << (f.prec - 2));   // the quiet NaN
        else bits = inf | ((ex >> 63) << (f.bits - 1));
    } else {
        bits = round_digits_to(r + OUT_DIGITS, dtype);
    }
    if (f.bits == 64) ((unsigned long long *)out)[i] = bits;
    else if (f.bits == 32) ((unsigned *)out)[i] = (unsigned)bits;
    else ((unsigned short *)out)[i] = (unsigned short)bits;
}

hipError_t round_records_dispatch(const long long *d_records, long long count, long long stride_words, int dtype,
                                  void *d_out, hipStream_t st)
{
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_round_records, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, st, d_records, count,
                       stride_words, dtype, d_out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
template <class T, int N, bool EE>
static hipError_t launch_exsum_lp(Ctx &c, const void *pa, long long n, long long inca, hipStream_t st)
{
    typedef typename T::elem E;
    constexpr int COPIES = (N == 0) ? 16 : 8;
    const E *a = (const E *)pa;
    if (inca == 1) {
        const int bpc = c.bpc_lp_sum;   // (the superaccumulator-only kernel too: 0.268 ms at 3 per CU, 0.23 to 0.24 at 8 to 32)
        int grid = grid_for(c, n, (long long)BLOCK * ULP * T::VEC, bpc);
        if (grid == c.num_cu * bpc && grid > 1 && !(grid & 1)) grid -= 1;   // an odd grid, as run_exsum
        c.last_blas1_kernel = BLAS1_K_EXSUM_LP, c.last_blas1_grid = grid;
        EXB_LAUNCH_STREAMING(c, (k_lp_stream<T, false, N, EE, COPIES, 0>), grid, st, a, a, n, c.gacc, c.gflags, c.ngroups);
    } else {
        const int grid = grid_for(c, n, BLOCK, c.blocks_per_cu);
        c.last_blas1_kernel = BLAS1_K_EXSUM_LP_STRIDED, c.last_blas1_grid = grid;
        EXB_LAUNCH_STREAMING(c, (k_lp_strided<T, false, N, EE, COPIES>), grid, st, a, inca, a, inca, n, c.gacc, c.gflags,
                             c.ngroups);
    }
    return hipGetLastError();
}

template <class T, int N, bool EE>
static hipError_t launch_exdot_lp(Ctx &c, const void *pa, long long inca, const void *pb, long long incb, long long n,
                                  hipStream_t st)
{
    typedef typename T::elem E;
    constexpr int COPIES = (N == 0) ? 16 : 8;
    const E *a = (const E *)pa, *b = (const E *)pb;
    if (inca == 1 && incb == 1 && (((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0) {
        // a workgroup should stream about five tiles or more, and the grid is odd: run_exdot's two rules
        const long long tiles = n / ((long long)BLOCK * ULP * T::VEC);
        const int bpc = (int)min((long long)c.bpc_lp_dot, max(4ll, tiles / (5ll * c.num_cu)));
        int grid = grid_for(c, n, (long long)BLOCK * ULP * T::VEC, bpc);
        if (grid > c.num_cu && !(grid & 1)) grid += 1;
        c.last_blas1_kernel = BLAS1_K_EXDOT_LP, c.last_blas1_grid = grid;
        EXB_LAUNCH_STREAMING(c, (k_lp_stream<T, true, N, EE, COPIES, 1>), grid, st, a, b, n, c.gacc, c.gflags, c.ngroups);
    } else {
        const int grid = grid_for(c, n, BLOCK, c.blocks_per_cu);
        c.last_blas1_kernel = BLAS1_K_EXDOT_LP_STRIDED, c.last_blas1_grid = grid;
        EXB_LAUNCH_STREAMING(c, (k_lp_strided<T, true, N, EE, COPIES>), grid, st, a, inca, b, incb, n, c.gacc, c.gflags,
                             c.ngroups);
    }
    return hipGetLastError();
}

// The bits cannot depend on the variant, so three instantiations serve every fpe: superaccumulators only below 2,
// an expansion of 4 up to fpe = 4 and of 8 above, both with the per-tile early exit (whatever early_exit says: without
// it the fp64 kernels take the same shortcut, fpe.hip.h: SKIP_ZERO_LEVELS).  The caller has checked fpe and dtype.
template <class F>
static void lp_variant(int fpe, F &&f)
{
    using std::integral_constant;
    if (fpe < 2) f(integral_constant<int, 0>(), std::false_type());
    else if (fpe <= 4) f(integral_constant<int, 4>(), std::true_type());
    else f(integral_constant<int, 8>(), std::true_type());
}

template <class F>
static void lp_type(int dtype, F &&f)
{
    if (dtype == DT_F32) f(LpF32());
    else if (dtype == DT_F16) f(LpF16());
    else f(LpBF16());
}

hipError_t exsum_lp_dispatch(Ctx &c, int dtype, const void *a, long long n, long long inca, int fpe, hipStream_t st)
{
    hipError_t e = hipSuccess;
    lp_type(dtype, [&](auto T) {
        lp_variant(fpe, [&](auto N, auto EE) { e = launch_exsum_lp<decltype(T), N(), EE()>(c, a, n, inca, st); });
    });
    return e;
}

hipError_t exdot_lp_dispatch(Ctx &c, int dtype, const void *a, long long inca, const void *b, long long incb, long long n,
                             int fpe, hipStream_t st)
{
    hipError_t e = hipSuccess;
    lp_type(dtype, [&](auto T) {
        lp_variant(fpe, [&](auto N, auto EE) { e = launch_exdot_lp<decltype(T), N(), EE()>(c, a, inca, b, incb, n, st); });
    });
    return e;
}

}  // namespace exb
