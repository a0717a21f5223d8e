// blas1.hip -- ExSUM / ExDOT for gfx950: streaming FPE front-end + per-wavefront LDS superaccumulators.
//
// Replaces the reference's OpenCL kernels ExSUM/ExSUMComplete (src/gpu/blas/blas1/ExSUM.Superacc.cl:211-356,
// ExSUM.FPE.cl:230-388, ExSUM.FPE.EX.{4,6,8}.cl) and ExDOT/ExDOTComplete (ExDOT.Superacc.cl:217-359,
// ExDOT.FPE.cl:201-345) -- behaviour only; the structure is ours.  This file holds the fp64 front ends (SumF64, DotF64),
// the finalize and the segmented ExSUM.  The loop itself is k_blas1_stream / k_blas1_strided of blas1_common.hip.h,
// and with these front ends it works like this:
//   * every lane streams 16-byte (double2) coalesced, non-temporal loads, U of them in flight per tile, and the
//     next tile is already on its way into a second register set while the current one is absorbed;
//   * a register-resident floating-point expansion of NFPE doubles absorbs the elements with Knuth
//     TwoSum; the early-exit test is one wave-uniform branch per level per *tile* (not per element); a tile
//     whose residues outlive all levels switches the wave to the direct path for the next 63 tiles
//     (fpe_absorb_adaptive), a tile with |x| >= 2^1000 / Inf / NaN takes the range guard (fpe_guard);
//   * what survives the expansion is split by integer shifts and added with ds_add_u64 to a
//     per-wavefront superaccumulator in LDS (COPIES columns per wave, limb-major, see superacc.hip.h);
//   * block epilogue: merge the columns, add the non-zero limbs to one of NGROUPS global accumulators
//     with int64 atomics (exact, order-free); the finalize kernel sums the groups, carry-propagates
//     ONCE, re-cuts into the reference's canonical limbs and rounds.  No inter-workgroup reads inside a
//     launch (the reference's ExSUMComplete races on that).
#include "blas1_common.hip.h"

namespace exb {

#ifndef EXBLAS_SUM_COPIES
#define EXBLAS_SUM_COPIES 8
#endif
#ifndef EXBLAS_DOT_COPIES
#define EXBLAS_DOT_COPIES 8
#endif

// ---------------------------------------------------------------------------------------------
// the fp64 front ends of k_blas1_stream / k_blas1_strided (blas1_common.hip.h)
// ---------------------------------------------------------------------------------------------
// a lane's 16-byte load is a double2 (loaded through a generic 4 x 32-bit vector and rebuilt from halves, the doubles
// cost 9 more VGPRs)
struct F64 {
    typedef double elem;
    typedef d2_t vec;
    static constexpr int VEC = 2;
    static __device__ __forceinline__ double widen(elem v) { return v; }
    static __device__ __forceinline__ double at(const vec &r, int j) { return j ? r.y : r.x; }
};

struct SumF64 : ExactOp<F64, 1> {
    static constexpr int COPIES = EXBLAS_SUM_COPIES, K_STREAM = BLAS1_K_EXSUM, K_STRIDED = BLAS1_K_EXSUM_STRIDED;
    // resident blocks per CU: the HBM-bound kernels want few fat blocks; the variants that run the full N-level cascade
    // on every element (no early exit, N >= 5: 30-48 dependent fp64 adds per element) are VALU-latency-bound and want
    // more waves per SIMD to hide it
    template <int N, bool EE>
    static int bpc(const Ctx &c)
    {
        return N == 0 ? c.bpc_sa : ((!SKIP_ZERO_LEVELS<EE> && N >= 5) ? c.bpc_heavy : c.bpc_sum);
    }
};

// ExDOT: TwoProductFMA front-end (ExDOT.Superacc.cl:25-29, :244-253); the rounding error of the product enters the
// expansion at slot max(N-3,0) like ExDOT.FPE.cl:254.  Products below 2^-968 / beyond the double range have their exact
// homes in the context's low / high accumulators (prod_range_divert, which replaces the range guard: GUARD = false).
struct DotF64 : F64 {
    static constexpr int STREAMS = 2;
    static constexpr int COPIES = EXBLAS_DOT_COPIES, K_STREAM = BLAS1_K_EXDOT, K_STRIDED = BLAS1_K_EXDOT_STRIDED;
    template <int N, bool EE>
    static int bpc(const Ctx &c) { return c.bpc_dot; }
    // vectors only when BOTH streams are 16-byte aligned
    static bool can_stream(const double *a, const double *b) { return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0; }
    // x becomes the products, e their TwoProd errors; true: the group was diverted as a whole (prod_range_divert)
    template <int N, int COPIES, int CNT>
    static __device__ __forceinline__ bool divert(double (&fpe)[N > 0 ? N : 1], Lane<COPIES> &L, double (&x)[CNT],
                                                  const double (&y)[CNT], double (&e)[CNT])
    {
        LdsSink<COPIES> sink = L.sink();
        double a[CNT];
#pragma unroll
        for (int j = 0; j < CNT; ++j) a[j] = x[j], x[j] = two_prod(a[j], y[j], e[j]);
        return prod_range_divert<CNT>(fpe[0], x, e, sink, low_acc_of(L.gflags), high_acc_of(L.gflags),
                                      [&](int j) { return a[j]; }, [&](int j) { return y[j]; });
    }
    template <Feed M, int N, bool EE, int COPIES, int ZM, int CNT>
    static __device__ __forceinline__ void absorb(double (&fpe)[N > 0 ? N : 1], Lane<COPIES> &L, double (&p)[CNT],
                                                  double (&e)[CNT])
    {
        LdsSink<COPIES> sink = L.sink();
        if constexpr (M == ONE) sink_product(sink, p[0], e[0]);
        else if constexpr (M == HOT) fpe_absorb_prod_adaptive<N, EE, CNT, LdsSink<COPIES>, ZM, false>(fpe, p, e, sink, L.bypass);
        else fpe_absorb_prod<N, false, CNT, LdsSink<COPIES>, 0, false>(fpe, p, e, sink);
    }
};

// ---------------------------------------------------------------------------------------------
// finalize: sum `nsets` limb vectors, ONE carry propagation, canonical limbs, rounding.
// zero_sets: the input is the context's group accumulators -> leave them zeroed for the next call.
// ---------------------------------------------------------------------------------------------
// ext_out (with gflags): EXPORT the context's low and high accumulators (ExDOT products beyond the accumulator's range,
// fpe.hip.h: prod_range_divert) as two normalised digit sets [low | high] instead of folding them (the multi-rank path
// all-reduces them beside the main digit set); ext_in: fold THESE digit sets (the all-reduced ones).
__global__ void __launch_bounds__(64) k_finalize(long long *sets, int nsets, int set_stride, unsigned *gflags,
                                                 unsigned flags_or, int zero_sets, long long *out,
                                                 const long long *ext_in, long long *ext_out)
{
    // one wavefront: lane l owns limb l and (l < 4) limb 64+l
    const int lane = threadIdx.x;
    unsigned flags = flags_or;
    if (gflags) flags |= *gflags;
    if (set_stride >= SET_WORDS) {  // record-style sets carry their own flag indicators
        for (int g = 0; g < nsets; ++g)
        {
            for (int k = 0; k < 3; ++k)
                if (sets[(size_t)g * set_stride + NL + k] != 0) flags |= (1u << k);
            const long long pw = sets[(size_t)g * set_stride + NL + 3];  // product flags: low 16 bits / the rest
            if (pw & 0xffff) flags |= FLAG_PUNDER;
            if (pw >> 16) flags |= FLAG_POVER;
        }
    }
    // all loads of a batch are issued before the first use (the words were last touched by other CUs' atomics,
    // so each load is a full memory round trip: 32 dependent ones cost ~20 us)
    // The low 32 bits and the (signed) high parts of the sets are summed separately and the high parts enter one
    // limb up, so this sum cannot overflow however many adds the sets hold (each set alone stays below 2^63 as long
    // as it received fewer than 2^31 adds: with 32 group accumulators that is 2^36 values per reduction).
    long long lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    for (int g0 = 0; g0 < nsets; g0 += 16) {
        long long t0[16], t1[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool ok = g0 + k < nsets;
            const long long *p = sets + (size_t)(ok ? g0 + k : 0) * set_stride;
            t0[k] = ok ? __builtin_nontemporal_load(p + lane) : 0;
            t1[k] = (ok && lane < NL - 64) ? __builtin_nontemporal_load(p + 64 + lane) : 0;
        }
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            lo0 += t0[k] & 0xffffffffll;
            hi0 += t0[k] >> 32;
            if (lane == NL - 65) {  // the top limb is never split
                lo1 += t1[k];
            } else {
                lo1 += t1[k] & 0xffffffffll;
                hi1 += t1[k] >> 32;
            }
        }
    }
    long long in0 = __shfl_up(hi0, 1), in1 = __shfl_up(hi1, 1);
    const long long h63 = __shfl(hi0, 63);
    if (lane == 0) { in0 = 0; in1 = h63; }
    long long v0 = lo0 + in0, v1 = (lane < NL - 64) ? lo1 + in1 : 0;
    if (zero_sets) {
        for (int i = lane; i < nsets * set_stride; i += 64) sets[i] = 0;
        if (lane == 0 && gflags) *gflags = 0;
    }
    // ExDOT with products below 2^-968 (FLAG_PUNDER) or beyond the double range (FLAG_POVER): fold the LOW / HIGH
    // accumulator in.  The high digits are added to the main digits exactly, EXT_SHIFT_DIGITS digits up (a sum that does
    // not fit the main geometry is beyond the double range whatever follows: +-Inf); the low accumulator's digits at or
    // above 2^-1074 are added exactly, what lies below becomes the half / sticky bits of the rounding.  Rare, so one lane
    // does it with the scalar routines (carry passes over 68 / 106 digits + one rounding).
    __shared__ long long s_v[NL], s_lo[NL], s_hi[NL], s_c[NL + EXT_SHIFT_DIGITS];
    __shared__ unsigned long long s_ex;
    __shared__ int s_over;
    bool low_folded = false;
    const bool have_low = (flags & FLAG_PUNDER) && (ext_in || gflags);   // wave-uniform
    const bool have_high = (flags & FLAG_POVER) && (ext_in || gflags);
    if (ext_out) {   // export mode: all-zero sets for the accumulators nothing was added to
        if (!have_low) {
            ext_out[lane] = 0;
            if (lane < SET_WORDS - 64) ext_out[64 + lane] = 0;
        }
        if (!have_high) {
            ext_out[SET_WORDS + lane] = 0;
            if (lane < SET_WORDS - 64) ext_out[SET_WORDS + 64 + lane] = 0;
        }
    }
    if (have_low || have_high) {
        const long long *lsrc = ext_in ? ext_in : low_acc_of(gflags);
        const long long *hsrc = ext_in ? ext_in + SET_WORDS : high_acc_of(gflags);
        s_lo[lane] = have_low ? lsrc[lane] : 0;
        s_hi[lane] = have_high ? hsrc[lane] : 0;
        s_v[lane] = v0;
        if (lane < NL - 64) {
            s_lo[64 + lane] = have_low ? lsrc[64 + lane] : 0;
            s_hi[64 + lane] = have_high ? hsrc[64 + lane] : 0;
            s_v[64 + lane] = v1;
        }
        if (!ext_in && zero_sets) {
            long long *lo = low_acc_of(gflags), *hi = high_acc_of(gflags);
            if (have_low) {
                lo[lane] = 0;
                if (lane < NL - 64) lo[64 + lane] = 0;
            }
            if (have_high) {
                hi[lane] = 0;
                if (lane < NL - 64) hi[64 + lane] = 0;
            }
        }
        __syncthreads();
        if (lane == 0) {
            s_over = 0;
            if (have_low) normalize_digits(s_lo);
            if (have_high) normalize_digits(s_hi);
            if (!ext_out) {
                if (have_high) s_over = fold_high_digits(s_v, s_hi, s_c);
                if (have_low && !s_over) {
                    for (int j = LOW_SHIFT_DIGITS; j < NL; ++j) s_v[j - LOW_SHIFT_DIGITS] += s_lo[j];
                    normalize_digits(s_v);
                    const bool half = (s_lo[LOW_SHIFT_DIGITS - 1] >> 31) & 1ll;
                    bool sticky = (s_lo[LOW_SHIFT_DIGITS - 1] & 0x7fffffffll) != 0;
                    for (int j = 0; j < LOW_SHIFT_DIGITS - 1; ++j) sticky = sticky || s_lo[j] != 0;
                    s_ex = round_exact_bits_frac(s_v, half, sticky);
                }
            }
        }
        __syncthreads();
        if (ext_out) {   // digits < 2^32 (the top one signed and small): sums over 2^31 ranks cannot overflow
            if (have_low) {
                ext_out[lane] = s_lo[lane];
                if (lane < SET_WORDS - 64) ext_out[64 + lane] = lane < NL - 64 ? s_lo[64 + lane] : 0;
            }
            if (have_high) {
                ext_out[SET_WORDS + lane] = s_hi[lane];
                if (lane < SET_WORDS - 64) ext_out[SET_WORDS + 64 + lane] = lane < NL - 64 ? s_hi[64 + lane] : 0;
            }
        } else {
            const int over = s_over;   // wave-uniform
            if (over) {
                // the exact sum is beyond the double range: it rounds to +-Inf, reported like an infinity in the input
                flags |= over > 0 ? FLAG_PINF : FLAG_NINF;
            } else {
                v0 = s_v[lane];
                v1 = lane < NL - 64 ? s_v[64 + lane] : 0;
                low_folded = have_low;
            }
            if (have_low) flags |= FLAG_PLOW_EXACT;
            if (have_high) flags |= FLAG_PHIGH_EXACT;
        }
    }
    // every input word has been read (into registers) before the first output word is written: out may alias sets
    WaveFinish r = finish_wave(v0, v1, flags);
    if (low_folded && !(flags & FLAG_NONFINITE)) r.ex = s_ex;
    write_record_wave(r, flags, out);
}

// ---------------------------------------------------------------------------------------------
// Segmented ExSUM: out[s] = Round(sum values[offsets[s] .. offsets[s+1])), one wave per segment, four
// segments per workgroup.  This is the batched form of the call pattern of the reference's SpMV example, which
// runs one exsum per matrix row on a short vector of products (src/cpu/examples/spmv (Parboil)/
// StrongReproducibility/main.cpp:85): thousands of tiny reductions cost one launch instead of one each.
// ---------------------------------------------------------------------------------------------
template <int N, bool EE>
__global__ void __launch_bounds__(BLOCK) k_exsum_segmented(const double *__restrict__ values,
                                                           const long long *__restrict__ offsets, long long nseg,
                                                           int round_mode, double *__restrict__ out)
{
    __shared__ long long acc[WAVES][NL];
    __shared__ unsigned fl[WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long seg = (long long)blockIdx.x * WAVES + w;
    const bool valid = seg < nseg;
    for (int t = lane; t < NL; t += 64) acc[w][t] = 0;
    if (lane == 0) fl[w] = 0;
    __syncthreads();
    if (valid) {
        unsigned flags = 0;
        LdsSink<1> sink{acc[w], flags};
        double fpe[N > 0 ? N : 1];
#pragma unroll
        for (int i = 0; i < (N > 0 ? N : 1); ++i) fpe[i] = 0.0;
        const long long b = offsets[seg], e = offsets[seg + 1];
        // all lanes run the same number of iterations (the early-exit vote is wave-wide); lanes past the end add 0
        for (long long i0 = b; i0 < e; i0 += 64) {
            const long long i = i0 + lane;
            double x[1] = {i < e ? values[i] : 0.0};
            fpe_absorb_sink<N, EE, 1>(fpe, x, 0, sink);
        }
        fpe_flush_sink<N>(fpe, sink);
        if (flags) atomicOr(&fl[w], flags);
    }
    __syncthreads();
    const WaveFinish r = finish_wave(acc[w][lane], lane < NL - 64 ? acc[w][64 + lane] : 0, fl[w]);
    if (valid && lane == 0) out[seg] = round_mode ? r.rf : __longlong_as_double((long long)r.ex);
}

// every segment reads 0.0: an unsupported variant (a kernel, not a memset: a captured memset node of a few MiB does not
// replay reliably on this stack, see k_bdot_zero and k_gemv_zero)
__global__ void __launch_bounds__(BLOCK) k_exsum_segmented_zero(long long nseg, double *__restrict__ out)
{
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < nseg; i += (long long)gridDim.x * BLOCK) out[i] = 0.0;
}

// ---------------------------------------------------------------------------------------------
// launchers (launch_blas1, EXB_LAUNCH_STREAMING and grid_for: blas1_common.hip.h)
// ---------------------------------------------------------------------------------------------

// d_ext_out == nullptr: the context's low / high accumulators (ExDOT products below 2^-968 / beyond the double range) are
// folded into the record; otherwise they are exported as two digit sets (EXT_WORDS int64: [low | high]) and the record
// holds the main digits alone
hipError_t finalize_groups(Ctx &c, hipStream_t st, long long *d_out, long long *d_ext_out)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, st, c.gacc, c.ngroups, NL, c.gflags, 0u, 1, d_out,
                       (const long long *)nullptr, d_ext_out);
    return hipGetLastError();
}

// d_ext_sets: the sums of the ranks' exported [low | high] digit sets (folded when the flags say products left the range), or nullptr
hipError_t finalize_sets(const long long *d_sets, int nsets, unsigned flags_or, hipStream_t st, long long *d_out,
                         const long long *d_ext_sets)
{
    hipLaunchKernelGGL(k_finalize, dim3(1), dim3(64), 0, st, const_cast<long long *>(d_sets), nsets, SET_WORDS,
                       (unsigned *)nullptr, flags_or, 0, d_out, d_ext_sets, (long long *)nullptr);
    return hipGetLastError();
}

// fpe < 2: superaccumulators only (gpu:ExSUM.cpp:64-71).  Early exit with fpe > 8: nothing is launched, the
// accumulators stay zero and the caller reads 0.0, the reference's silent return.
hipError_t exsum_dispatch(Ctx &c, const double *a, long long n, long long inca, int fpe, int early_exit,
                          hipStream_t st)
{
    if (fpe < 2) return launch_blas1<SumF64, 0, false>(c, a, inca, a, inca, n, st);
    hipError_t e = hipSuccess;
    select_variant<2>(fpe, early_exit, [&](auto N, auto EE) { e = launch_blas1<SumF64, N(), EE()>(c, a, inca, a, inca, n, st); });
    return e;
}

// same variant rules as exsum; an unsupported combination yields 0.0 for every segment
hipError_t exsum_segmented_dispatch(const double *values, const long long *offsets, long long nseg, int fpe,
                                    int early_exit, int round_mode, hipStream_t st, double *out)
{
    if (nseg <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nseg + WAVES - 1) / WAVES)), block(BLOCK);
    auto go = [&](auto N, auto EE) {
        hipLaunchKernelGGL((k_exsum_segmented<N(), EE()>), grid, block, 0, st, values, offsets, nseg, round_mode, out);
    };
    if (fpe < 2) go(std::integral_constant<int, 0>(), std::false_type());
    else if (!select_variant<2>(fpe, early_exit, go))
        hipLaunchKernelGGL(k_exsum_segmented_zero, dim3((unsigned)min(4096ll, (nseg + BLOCK - 1) / BLOCK)), block, 0, st, nseg,
                           out);
    return hipGetLastError();
}

// fpe < 3: superaccumulators only (ExDOT.cpp:69-76); early exit with fpe > 8 as in exsum_dispatch
hipError_t exdot_dispatch(Ctx &c, const double *a, long long inca, const double *b, long long incb, long long n,
                          int fpe, int early_exit, hipStream_t st)
{
    if (fpe < 3) return launch_blas1<DotF64, 0, false>(c, a, inca, b, incb, n, st);
    hipError_t e = hipSuccess;
    select_variant<3>(fpe, early_exit,
                      [&](auto N, auto EE) { e = launch_blas1<DotF64, N(), EE()>(c, a, inca, b, incb, n, st); });
    return e;
}

}  // namespace exb
