// blas1_lowp.hip -- ExSUM / ExDOT on float32, float16 and bfloat16 inputs, and the rounding of records into a narrow format.
//
// Every value of the three types widens to a double exactly, and the product of two of them is an exact double (at most
// 48 significand bits, magnitude in [2^-298, 2^256) or zero).  So the narrow kernels are k_blas1_stream / k_blas1_strided
// (blas1_common.hip.h), the kernels of the fp64 routines, with another front end and LESS behind it: ExDOT needs no
// TwoProd error term, no range divert and no low / high accumulators -- it is ExSUM's cascade fed with products
// (ExactOp), and flag bits 3 to 6 are never set here.
//   * a lane's 16-byte non-temporal load carries 4 float32 or 8 16-bit elements; U = 4 loads per lane, stream and tile
//     (4096 float32 / 8192 16-bit elements per workgroup tile), two explicit register sets filled alternately with
//     unconditional clamped loads, LDS zeroed after the first loads are in flight;
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
#include "lowp_types.hip.h"

namespace exb {

// the element types LpF32 / LpF16 / LpBF16: lowp_types.hip.h

// the narrow front ends of k_blas1_stream / k_blas1_strided (blas1_common.hip.h): exact doubles in, exact products
template <class T>
struct SumLp : ExactOp<T, 1> {
    static constexpr int COPIES = 8, K_STREAM = BLAS1_K_EXSUM_LP, K_STRIDED = BLAS1_K_EXSUM_LP_STRIDED;
    // (the superaccumulator-only kernel too: 0.268 ms at 3 per CU, 0.23 to 0.24 at 8 to 32)
    template <int N, bool EE>
    static int bpc(const Ctx &c) { return c.bpc_lp_sum; }
};
template <class T>
struct DotLp : ExactOp<T, 2> {
    static constexpr int COPIES = 8, K_STREAM = BLAS1_K_EXDOT_LP, K_STRIDED = BLAS1_K_EXDOT_LP_STRIDED;
    template <int N, bool EE>
    static int bpc(const Ctx &c) { return c.bpc_lp_dot; }
};

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
        lp_variant(fpe, [&](auto N, auto EE) { e = launch_blas1<SumLp<decltype(T)>, N(), EE()>(c, a, inca, a, inca, n, st); });
    });
    return e;
}

hipError_t exdot_lp_dispatch(Ctx &c, int dtype, const void *a, long long inca, const void *b, long long incb, long long n,
                             int fpe, hipStream_t st)
{
    hipError_t e = hipSuccess;
    lp_type(dtype, [&](auto T) {
        lp_variant(fpe, [&](auto N, auto EE) { e = launch_blas1<DotLp<decltype(T)>, N(), EE()>(c, a, inca, b, incb, n, st); });
    });
    return e;
}

}  // namespace exb
