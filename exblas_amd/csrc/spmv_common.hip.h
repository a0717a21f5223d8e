// spmv_common.hip.h -- what the four sparse routines (spmv.hip: ExSpMV, spmm.hip: ExSpMM, sptrsv.hip: ExSpTRSV, sptrsm.hip:
// ExSpTRSM) share.  The row step: the guarded gather of x, the row sink, the beta * y term, one step of the exact merge of
// lane expansions (sp_cascade_step), the certified in-register rounding test (spmv_round_fast) and the leader's use of it
// with the spill into the row's accumulator behind it (sp_certify_or_spill), the rounding of an LDS integer accumulator
// (sp_acc_round, with sp_pick and sp_acc_clear), the union of a lane group's non-finite flags (NonFiniteLanes) and the
// wave's LDS hand-over (sp_wave_sync).  Split rows: the chunk-base scan and the chunk-owner search.  Host side: geometry
// constants, the choice of index type and plain / exact kernels, the split thresholds.  For the routines built on these
// pieces (sptrs_common.hip.h, block_common.hip.h) also the sink of a lane's expansion without an accumulator (SpLaneSink)
// and the rule for fpe, path and rounding mode (st_rule).
// The narrow products (exspmv_lp / exspmm_lp) run the same row step with typed front ends (lowp_types.hip.h): gather_x,
// sp_absorb_beta and sp_wave_add_beta widen an element of the vector's type, sp_round_fast_to certifies a rounding into that
// type against ITS rounding boundaries, and sp_pick_to / sp_acc_round_to round an accumulator's digits once into it.  With
// LpF64 (the default) every one of them is the fp64 code above it.
#pragma once
#include "superacc.hip.h"
#include "fpe.hip.h"
#include "exblas_internal.h"
#include "lowp_types.hip.h"

namespace exb {

constexpr int SP_BLOCK = 256;
constexpr int SP_WAVES = SP_BLOCK / 64;
constexpr int SP_N = 4;              // expansion size of every fpe >= 2 (and 0): the bits do not depend on it
constexpr int SP_G_SHORT = 8;        // lanes per short row
constexpr long long SP_SHORT_MAX = 64;     // entries of a short row (<= 8 per lane)
constexpr long long SP_LONG_MIN = 16384;   // rows longer than this are split
constexpr long long SP_CHUNK = 4096;       // entries per wave of a split row
constexpr long long SP_CHUNK_SMALL = 16;   // path 3: split every row at this chunk
constexpr long long SP_LCAP = 16384;       // long-row accumulator slots (beyond: the row runs as a medium row)
constexpr unsigned SP_SPILL = 128u;        // row flag: something went to the row's integer accumulator
constexpr int SP_HDR = 8;                  // header words: [0] medium rows [1] long rows [2] chunks, [4..7] info
constexpr int SP_ACC_FLAGS = NL + 3;       // word of a long row's accumulator that holds its flags

template <class I>
__device__ __forceinline__ I ld_nt(const I *p) { return __builtin_nontemporal_load(p); }

// fl(alpha * W(x[c])) for an in-range column; a column outside [0, n) is never read and makes the row NaN.  XT: the
// element type of x (lowp_types.hip.h), W its exact widening
template <class XT = LpF64, class I>
__device__ __forceinline__ double gather_x(const typename XT::elem *__restrict__ x, I c, int n, double alpha,
                                           unsigned &flags)
{
    if ((unsigned long long)(long long)c < (unsigned long long)n) return alpha * XT::widen(x[c]);
    flags |= FLAG_NAN | SP_SPILL;
    return 0.0;
}

// what an expansion cannot hold goes to the row's integer accumulator in LDS; the row then rounds from it
struct RowSink {
    long long *col;   // the row's 68 limbs in LDS
    unsigned &flags;
    __device__ __forceinline__ void add(double x)
    {
        lds_add<1>(col, x, flags);
        flags |= SP_SPILL;
    }
    __device__ __forceinline__ void note(unsigned bits) { flags |= bits | SP_SPILL; }
};

// the sink of a lane's expansion that has no accumulator behind it (the block solves, block_common.hip.h): whatever
// would spill only raises SP_SPILL, which sends the output to the routine's fall-back
struct SpLaneSink {
    unsigned &flags;
    __device__ __forceinline__ void add(double) { flags |= SP_SPILL; }
    __device__ __forceinline__ void note(unsigned) { flags |= SP_SPILL; }
};

// Certified round-to-nearest-even of the exact value of an expansion f (any N terms, finite, |f| < 2^1012).
// Two error-free VecSum passes leave S = f0 + f1 + sum_{i>=2} f_i exactly; res + q = f0 + f1 exactly (TwoSum).  Then
// |S - res| <= |q| + sum_{i>=2} |f_i|.  When that is below half the spacing of the doubles next to res (a quarter of
// ulp(res) when |res| is a power of two: the spacing below it is halved), res is the unique nearest double, so
// RN(S) = res: no tie is possible.  The bound on the tail is taken twice over (fp rounding of the |f_i| sum, and the
// absolute error of subnormal partials, are far below that margin for |res| >= 2^-960).  Returns false whenever it
// cannot decide (near-ties, ties, |res| < 2^-960 or >= 2^1020, a zero head over non-zero terms): the caller then rounds
// the exact accumulator.  Sound, not complete.
template <int N>
__device__ __forceinline__ bool spmv_round_fast(double (&f)[N], double &out)
{
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int i = N - 1; i >= 1; --i) {
            double s;
            f[i - 1] = two_sum(f[i - 1], f[i], s);
            f[i] = s;
        }
    }
    double q;
    const double res = two_sum(f[0], f[1], q);
    double tail = 0.0;
    bool any = f[0] != 0.0 || f[1] != 0.0;
#pragma unroll
    for (int i = 2; i < N; ++i) {
        tail += __builtin_fabs(f[i]);
        any |= f[i] != 0.0;
    }
    if (!any) {
        out = 0.0;   // the exact sum is zero: +0.0, as the accumulator rounds it
        return true;
    }
    const unsigned ef = expo_field(res);
    if (ef < 1023u - 960u || ef >= 1023u + 1020u) return false;
    const bool pow2 = (((unsigned long long)__double_as_longlong(res)) & 0x000fffffffffffffull) == 0;
    // half = ulp(res) / 2 = 2^(E - 53), a quarter ulp for a power of two
    const double half = __longlong_as_double((long long)((unsigned long long)(ef - (pow2 ? 54u : 53u)) << 52));
    if (!(tail <= half * 0x1p-32)) return false;
    if (!(__builtin_fabs(q) < half - half * 0x1p-30)) return false;
    out = res;
    return true;
}

// (The typed forms below -- sp_round_fast_to, sp_certify_or_spill_to, sp_pick_to, sp_acc_round_to -- stand BESIDE
// spmv_round_fast, sp_certify_or_spill, sp_pick and sp_acc_round and repeat some of their lines on purpose: the fp64
// functions, and finish_wave under them, are shared with the solves, the factors and the block routines, and are left
// exactly as they were so that the code generated for every fp64 kernel stays what it was.  With LpF64 the typed forms
// only call them.)
// The same certificate for an output of the type XT, as the bit pattern to store.  float64: spmv_round_fast.  A narrow XT:
// the same two VecSum passes, res and the bound |q| + tail on |S - res| -- the tail taken twice over and the whole with a
// margin of 2^-30, the safety factors of spmv_round_fast -- and round_interval_to (round_lowp.hip.h), which certifies
// against the rounding boundaries of XT: the value is returned only if every real number within the bound of res rounds
// to it.  A bound of zero says that res is the exact sum, and then a tie of XT is decided here.
template <class XT, int N>
__device__ __forceinline__ bool sp_round_fast_to(double (&f)[N], unsigned long long &bits)
{
    if constexpr (XT::DT == DT_F64) {
        double out = 0.0;
        const bool ok = spmv_round_fast<N>(f, out);
        bits = (unsigned long long)__double_as_longlong(out);
        return ok;
    } else {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
            for (int i = N - 1; i >= 1; --i) {
                double s;
                f[i - 1] = two_sum(f[i - 1], f[i], s);
                f[i] = s;
            }
        }
        double q;
        const double res = two_sum(f[0], f[1], q);
        double tail = 0.0;
        bool any = f[0] != 0.0 || f[1] != 0.0;
#pragma unroll
        for (int i = 2; i < N; ++i) {
            tail += __builtin_fabs(f[i]);
            any |= f[i] != 0.0;
        }
        bits = 0ull;   // the exact sum is zero: +0, as the accumulator rounds it
        if (!any) return true;
        const unsigned ef = expo_field(res);
        if (ef < 1023u - 960u || ef >= 1023u + 1020u) return false;
        const double b = __builtin_fabs(q) + 2.0 * tail;
        return round_interval_to(res, b + b * 0x1p-30, XT::DT, &bits) != 0;
    }
}

// between a wave's lanes writing LDS and other lanes of it reading (or overwriting) the same words
__device__ __forceinline__ void sp_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One step of the exact merge of lane expansions: a lane where `take` holds absorbs the expansion and the flags of the lane
// `stride` above it.  SKIP leaves the cascade out when no lane of the wave took a non-zero term (wave-uniform).
template <bool SKIP = false, class Sink>
__device__ __forceinline__ void sp_cascade_step(double (&f)[SP_N], unsigned &flags, int stride, bool take, Sink &sink)
{
    double q[SP_N];
#pragma unroll
    for (int i = 0; i < SP_N; ++i) {
        const double t = __shfl_down(f[i], stride, 64);
        q[i] = take ? t : 0.0;
    }
    const unsigned fo = __shfl_down(flags, stride, 64);
    if (take) flags |= fo;
    if (!SKIP || __any(any_nonzero<SP_N>(q))) fpe_cascade<SP_N, true, SP_N>(f, q, 0, sink);
}

// A row's leader rounds its merged expansion: true with the certified value in `out`, or false after adding the non-zero
// terms to the row's accumulator `acc`, which the wave then rounds (sp_acc_round)
__device__ __forceinline__ bool sp_certify_or_spill(double (&f)[SP_N], unsigned &flags, int force_fb, long long *acc,
                                                    double &out)
{
    if (!force_fb && flags == 0 && spmv_round_fast<SP_N>(f, out)) return true;
#pragma unroll
    for (int i = 0; i < SP_N; ++i)
        if (f[i] != 0.0) lds_add<1>(acc, f[i], flags);
    return false;
}

// the same with the output of the type XT, as the bit pattern to store (sp_round_fast_to)
template <class XT>
__device__ __forceinline__ bool sp_certify_or_spill_to(double (&f)[SP_N], unsigned &flags, int force_fb, long long *acc,
                                                       unsigned long long &bits)
{
    if (!force_fb && flags == 0 && sp_round_fast_to<XT, SP_N>(f, bits)) return true;
#pragma unroll
    for (int i = 0; i < SP_N; ++i)
        if (f[i] != 0.0) lds_add<1>(acc, f[i], flags);
    return false;
}

// the value of a finished accumulator under the rounding mode (0: nearest even, else the reference's)
__device__ __forceinline__ double sp_pick(const WaveFinish &r, int round_mode)
{
    return round_mode ? r.rf : __longlong_as_double((long long)r.ex);
}

// The pattern to store for an output of the type XT from a finished accumulator.  float64: sp_pick.  A narrow XT is rounded
// ONCE, to nearest even whatever the mode, from the normalised digits the wave holds in r.d0 / r.d1 -- never from r.ex,
// which is rounded already.  The wave forms the magnitude and its leading 64 bits as finish_wave does for the double;
// round_window_to (round_lowp.hip.h) is round_digits_to on them.  Every lane gets the pattern.
template <class XT>
__device__ __forceinline__ unsigned long long sp_pick_to(const WaveFinish &r, unsigned nonfinite, int round_mode)
{
    if constexpr (XT::DT == DT_F64) {
        return (unsigned long long)__double_as_longlong(sp_pick(r, round_mode));
    } else {
        if (nonfinite & FLAG_NONFINITE) return nonfinite_to(r.ex, XT::DT);
        const int lane = (int)(threadIdx.x & 63u);
        constexpr int HI = NL - 64;
        const bool neg = lane_bcast(r.d1, HI - 1) < 0;
        const unsigned d0 = (unsigned)r.d0, d1 = (unsigned)r.d1;
        const unsigned long long nz0 = __ballot(d0 != 0), nz1 = __ballot(lane < HI && d1 != 0);
        const int z = nz0 ? __builtin_ctzll(nz0) : (nz1 ? 64 + __builtin_ctzll(nz1) : NL);
        const int i1 = 64 + lane;
        const unsigned m0 = !neg ? d0 : (lane < z ? 0u : (lane == z ? (0u - d0) : ~d0));
        const unsigned m1 = (lane >= HI) ? 0u : (!neg ? d1 : (i1 < z ? 0u : (i1 == z ? (0u - d1) : ~d1)));
        const unsigned long long mz0 = __ballot(m0 != 0), mz1 = __ballot(m1 != 0);
        const int tp = mz1 ? 64 + (63 - __builtin_clzll(mz1)) : (mz0 ? 63 - __builtin_clzll(mz0) : -1);
        if (tp < 0) return 0ull;
        auto mag = [&](int i) -> unsigned {   // i uniform
            const unsigned a = lane_bcast(m0, i & 63), b = lane_bcast(m1, (i - 64) & 63);
            return i < 0 ? 0u : (i < 64 ? a : b);
        };
        const unsigned mt = mag(tp), ma = mag(tp - 1), mb = mag(tp - 2);
        const int lz = __builtin_clz(mt | 1u);
        unsigned long long w = ((unsigned long long)mt << 32) | ma;
        unsigned rest = mb;
        if (lz) {
            w = (w << lz) | (unsigned long long)(mb >> (32 - lz));
            rest = mb << lz;
        }
        return round_window_to(neg, 32 * tp + 31 - lz, w, rest != 0 || z < tp - 2, XT::DT);
    }
}

__device__ __forceinline__ void sp_acc_clear(long long *a)
{
    const int lane = threadIdx.x & 63;
    a[lane] = 0;
    if (lane < NL - 64) a[64 + lane] = 0;
}

// Rounds the NL limbs of an LDS accumulator that the whole wave runs through (every lane gets the value) and leaves them
// zero; `nonfinite` is wave-uniform.  The caller separates it from the lanes' adds, and from the next ones, by sp_wave_sync.
__device__ __forceinline__ double sp_acc_round(long long *a, unsigned nonfinite, int round_mode)
{
    const int lane = threadIdx.x & 63;
    const long long v0 = a[lane], v1 = lane < NL - 64 ? a[64 + lane] : 0;
    const WaveFinish r = finish_wave(v0, v1, nonfinite);
    sp_acc_clear(a);
    return sp_pick(r, round_mode);
}

// the same for an output of the type XT, as the bit pattern to store (sp_pick_to)
template <class XT>
__device__ __forceinline__ unsigned long long sp_acc_round_to(long long *a, unsigned nonfinite, int round_mode)
{
    const int lane = threadIdx.x & 63;
    const long long v0 = a[lane], v1 = lane < NL - 64 ? a[64 + lane] : 0;
    const WaveFinish r = finish_wave(v0, v1, nonfinite);
    sp_acc_clear(a);
    return sp_pick_to<XT>(r, nonfinite, round_mode);
}

// which lanes of the wave hold which non-finite flag; of(group): the union over the lanes of a mask
struct NonFiniteLanes {
    unsigned long long pinf, ninf, nan;
    __device__ __forceinline__ explicit NonFiniteLanes(unsigned flags)
        : pinf(__ballot((flags & FLAG_PINF) != 0)), ninf(__ballot((flags & FLAG_NINF) != 0)),
          nan(__ballot((flags & FLAG_NAN) != 0))
    {
    }
    __device__ __forceinline__ unsigned of(unsigned long long group) const
    {
        return ((pinf & group) ? FLAG_PINF : 0u) | ((ninf & group) ? FLAG_NINF : 0u) | ((nan & group) ? FLAG_NAN : 0u);
    }
};

// beta * y under ExGEMV's rules (beta = 0 ignores y, 1 adds it exactly, else the error-free product), absorbed into a
// lane's expansion; `take` says whether this lane carries the term (y[at] is read by no other).  XT: the element type of y
template <class XT = LpF64, class Sink>
__device__ __forceinline__ void sp_absorb_beta(double (&f)[SP_N], bool take, double beta, const typename XT::elem *y,
                                               long long at, Sink &sink)
{
    double p[1] = {0.0}, er[1] = {0.0};
    if (take && beta != 0.0) {
        const double yv = XT::widen(y[at]);
        if (beta == 1.0) p[0] = yv;
        else p[0] = two_prod(beta, yv, er[0]);
    }
    fpe_absorb_prod<SP_N, true, 1>(f, p, er, sink);
}

// the same term added into the accumulator a wave holds in (v0, v1)
template <class XT = LpF64>
__device__ __forceinline__ void sp_wave_add_beta(long long &v0, long long &v1, double beta, const typename XT::elem *y,
                                                 long long at, unsigned &flags)
{
    if (beta == 0.0) return;
    const double yv = XT::widen(y[at]);
    if (beta == 1.0) {
        wave_add_double(v0, v1, yv, flags);
    } else {
        double e;
        const double p = two_prod_safe(beta, yv, e);
        wave_add_double(v0, v1, p, flags);
        if (e != 0.0) wave_add_double(v0, v1, e, flags);
    }
}

// split rows: which of the nl rows owns chunk t, i.e. the last idx with lbase[idx] <= t (bases are non-decreasing)
__device__ __forceinline__ long long sp_chunk_owner(const long long *__restrict__ lbase, long long nl, long long t)
{
    long long lo = 0, hi = nl;
    while (hi - lo > 1) {
        const long long mid = (lo + hi) >> 1;
        if (lbase[mid] <= t) lo = mid;
        else hi = mid;
    }
    return lo;
}

// the header of an ExSpMV / ExSpMM call before its first kernel counts into it (one small kernel, not a memset node: a
// captured graph with memset nodes does not replay reliably on this stack, see sptrs_common.hip.h's preset)
static __global__ void __launch_bounds__(64) k_sp_zero_header(long long *__restrict__ hdr, int words)
{
    for (int i = threadIdx.x; i < words; i += 64) hdr[i] = 0;
}

// split rows: chunk counts of the rows in lrows[0 .. min(hdr[1], lcap)) -> exclusive scan (lbase), total in hdr[2]
template <class I>
__global__ void __launch_bounds__(1024) k_spmv_long_prep(const I *__restrict__ rp, const int *__restrict__ lrows,
                                                         int lcap, long long chunk, long long *__restrict__ hdr,
                                                         long long *__restrict__ lbase)
{
    __shared__ long long part[1024];
    __shared__ long long carry;
    const int tid = threadIdx.x;
    const long long nl = min(hdr[1], (long long)lcap);
    if (tid == 0) carry = 0;
    __syncthreads();
    for (long long b = 0; b < nl; b += 1024) {
        const long long i = b + tid;
        long long k = 0;
        if (i < nl) {
            const int r = lrows[i];
            const long long len = max(0ll, (long long)rp[r + 1] - (long long)rp[r]);
            k = (len + chunk - 1) / chunk;
        }
        part[tid] = k;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {   // inclusive Hillis-Steele scan
            const long long t = tid >= o ? part[tid - o] : 0;
            __syncthreads();
            part[tid] += t;
            __syncthreads();
        }
        if (i < nl) lbase[i] = carry + part[tid] - k;
        __syncthreads();
        if (tid == 0) carry += part[1023];
        __syncthreads();
    }
    if (tid == 0) {
        lbase[nl] = carry;
        hdr[2] = carry;
    }
}

static inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// The rule of the solves and the block routines (sptrs_common.hip.h, block_common.hip.h) for fpe, path and rounding mode.
// fpe: 0 every output from the integer accumulator, 1 the plain sums, 2..8 the expansions; path 1 and the reference
// rounding mode send every output through the accumulator as well; the path it was made for travels with it
struct StRule {
    int force_fb, round_mode, path;
};
static inline StRule st_rule(int fpe, int path, int round_mode)
{
    return {(fpe != 1 && (fpe == 0 || path == 1 || round_mode)) ? 1 : 0, fpe == 1 ? 0 : round_mode, path};
}

// exblas_set_spmv_path / exblas_set_spmm_path -> which rows are split and at what chunk: 3 splits every row at the small
// chunk, 2 splits none, the others keep the routine's own threshold and chunk
struct SplitRule {
    long long long_min, chunk;
};
static inline SplitRule sp_split_rule(int path, long long long_min, long long chunk)
{
    if (path == 3) return {-1, SP_CHUNK_SMALL};
    return {path == 2 ? 0x7fffffffffffffffll : long_min, chunk};
}

// the four host-side instantiations of a sparse routine: f(std::bool_constant<PLAIN>, rp, ci) with the index arrays
// typed (int32 or int64) and PLAIN set for fpe == 1, the plain fp64 sums
template <class F>
static hipError_t sp_dispatch(int index_bits, int fpe, const void *row_ptr, const void *col_idx, F &&f)
{
    if (index_bits == 32) {
        const int *rp = (const int *)row_ptr, *ci = (const int *)col_idx;
        return fpe == 1 ? f(std::true_type(), rp, ci) : f(std::false_type(), rp, ci);
    }
    const long long *rp = (const long long *)row_ptr, *ci = (const long long *)col_idx;
    return fpe == 1 ? f(std::true_type(), rp, ci) : f(std::false_type(), rp, ci);
}

}  // namespace exb
