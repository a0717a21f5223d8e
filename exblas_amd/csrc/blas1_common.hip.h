// blas1_common.hip.h -- the ExSUM / ExDOT frame that blas1.hip (fp64) and blas1_lowp.hip (float32, float16, bfloat16)
// instantiate: the workgroup shape, the LDS sink wrappers, the ONE streaming kernel k_blas1_stream and the ONE strided
// kernel k_blas1_strided with their launchers, the block epilogue into the context's group accumulators and the launch
// plumbing.  Both files add into the same accumulators, so their calls fold into one exact reduction.
//
// The kernels never test the element type or the operation.  What differs sits in a FRONT END type F:
//   element side    F::elem as it lies in memory, F::vec the 16-byte vector a lane loads, F::VEC elements in it,
//                   F::at(vec, j) element j as a double, F::widen(elem)
//   operation side  F::STREAMS (1: ExSUM, 2: ExDOT) and the two steps by which CNT values, or operand pairs, enter the
//                   expansion: F::divert<N>(fpe, lane, x, y, e) turns x into what is summed (x itself, or the products
//                   with their error terms e) and says whether it has already dealt with the group (the fp64 ExDOT's
//                   range divert); if not, F::absorb<MODE, ...>(fpe, lane, x, e) adds it (Feed below).  The kernels
//                   write `if (!divert) absorb` themselves: behind one more inlined call the fp64 strided ExDOT
//                   allocates two more VGPRs and loses a wave per SIMD at N = 3
//   launch rules    F::COPIES, F::bpc<N, EE>(ctx), F::can_stream(a, b), F::K_STREAM / F::K_STRIDED (BLAS1_K_* ids)
#pragma once
#include "superacc.hip.h"
#include "fpe.hip.h"
#include "exblas_internal.h"
#include <hip/hip_ext.h>

namespace exb {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int U = 4;       // 16-byte loads per lane and stream in one tile
constexpr int CHUNK = 8;   // values fed to the expansion at once: one chunk per fp64 tile, two per float32, four per 16-bit

template <class V>
__device__ __forceinline__ V ld16(const V *p) { return __builtin_nontemporal_load(p); }

// What a lane accumulates into beside its expansion: its column of the wave's LDS superaccumulator (limb stride COPIES),
// the flags it raises and its bypass state.  (The expansion stays a plain array of the kernel, as the cascade routines
// take it; the sink is made where it is used: stored here it would point into the struct and pin it to scratch memory.)
template <int COPIES>
struct Lane {
    long long *col;
    unsigned flags = 0;
    Bypass bypass;
    unsigned *gflags;   // (the ExDOT low / high accumulators live behind it: low_acc_of, high_acc_of)
    __device__ __forceinline__ Lane(long long *s_acc, unsigned *gf)
        : col(s_acc + (threadIdx.x >> 6) * NL * COPIES + ((threadIdx.x & 63) & (COPIES - 1))), gflags(gf)
    {
    }
    __device__ __forceinline__ LdsSink<COPIES> sink() { return {col, flags}; }
};

// How absorb takes a group of values into the expansion.  HOT: a chunk of the tile loop, adaptive and with the per-chunk early
// exit; LOOSE: a group of the remainder or strided loop, the plain cascade; ONE: a head or tail element, straight into
// the accumulator (one lane each: the votes of a divert are then votes of the few active lanes).
enum Feed { HOT, LOOSE, ONE };

// Front end of every stream of exact doubles: ExSUM of any type, and ExDOT of the narrow types, whose widened products
// are exact doubles -- no TwoProd error term, no range divert, no low / high accumulators, flag bits 3 to 6 never set.
template <class T, int STREAMS_>
struct ExactOp : T {
    static constexpr int STREAMS = STREAMS_;
    // exact doubles need no range divert: the products are formed in place and nothing is handled here
    template <int N, int COPIES, int CNT>
    static __device__ __forceinline__ bool divert(double (&)[N > 0 ? N : 1], Lane<COPIES> &, double (&x)[CNT],
                                                  const double (&y)[CNT], double (&)[CNT])
    {
        if constexpr (STREAMS == 2) {
#pragma unroll
            for (int j = 0; j < CNT; ++j) x[j] *= y[j];   // (the product is exact)
        }
        return false;
    }
    template <Feed M, int N, bool EE, int COPIES, int ZM, int CNT>
    static __device__ __forceinline__ void absorb(double (&fpe)[N > 0 ? N : 1], Lane<COPIES> &L, double (&x)[CNT],
                                                  double (&)[CNT])
    {
        LdsSink<COPIES> sink = L.sink();
        if constexpr (M == ONE) sink.add(x[0]);
        else if constexpr (M == HOT) fpe_absorb_adaptive<N, EE, CNT, LdsSink<COPIES>, ZM>(fpe, x, sink, L.bypass);
        else fpe_absorb_sink<N, false, CNT>(fpe, x, 0, sink);
    }
    // two operands stream as vectors when their heads coincide (ExSUM passes its one operand twice)
    static bool can_stream(const typename T::elem *a, const typename T::elem *b)
    {
        return (((uintptr_t)a ^ (uintptr_t)b) & 15u) == 0;
    }
};

// elements before the first 16-byte boundary (at most n)
template <class F>
__device__ __forceinline__ long long head_of(const typename F::elem *a, long long n)
{
    const long long h = (long long)(((16u - (unsigned)((uintptr_t)a & 15u)) & 15u) / sizeof(typename F::elem));
    return h < n ? h : n;
}

// block epilogue: columns -> one limb vector -> global group accumulator
template <int COPIES>
__device__ __forceinline__ void block_epilogue(long long *s_acc, unsigned flags, long long *gacc,
                                               unsigned *gflags, int ngroups)
{
    __shared__ unsigned s_flags;
    if (threadIdx.x == 0) s_flags = 0;
    __syncthreads();  // also orders every wave's LDS atomics before the merge
    if (flags) atomicOr(&s_flags, flags);
    long long *g = gacc + (size_t)(blockIdx.x % ngroups) * NL;
    for (int l = threadIdx.x; l < NL; l += BLOCK) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w)
#pragma unroll
            for (int c = 0; c < COPIES; ++c) sum += s_acc[(w * NL + l) * COPIES + c];
        if (sum != 0) atomicAdd((unsigned long long *)&g[l], (unsigned long long)sum);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_flags) atomicOr(gflags, s_flags);
}

// ---------------------------------------------------------------------------------------------
// The streaming kernel: contiguous ExSUM (b unused), and ExDOT on operands whose heads coincide (F::can_stream).
// The pointers are only element-aligned: the elements before the first 16-byte boundary and those after the last whole
// vector go straight into the accumulator, one lane each.  ZM: how the early exit votes (any_nonzero).
// ---------------------------------------------------------------------------------------------
template <class F, int N, bool EE, int COPIES, int ZM>
__global__ void __launch_bounds__(BLOCK) k_blas1_stream(const typename F::elem *__restrict__ a,
                                                        const typename F::elem *__restrict__ b, long long n,
                                                        long long *__restrict__ gacc, unsigned *__restrict__ gflags,
                                                        int ngroups)
{
    typedef typename F::vec vec;
    constexpr int VEC = F::VEC;
    constexpr bool TWO = F::STREAMS == 2;
    constexpr int UB = TWO ? U : 1;
    __shared__ long long s_acc[WAVES * NL * COPIES];
    // (zeroed AFTER the first tile's loads are in flight: a microsecond of every workgroup's life, which counts for the
    // short shards of a multi-GPU job -- 2^25 doubles are 16 us of HBM time per stream)
    auto zero_lds = [&]() {
        for (int i = threadIdx.x; i < WAVES * NL * COPIES; i += BLOCK) s_acc[i] = 0;
        __syncthreads();
    };
    Lane<COPIES> L(s_acc, gflags);
    double fpe[N > 0 ? N : 1];
#pragma unroll
    for (int i = 0; i < (N > 0 ? N : 1); ++i) fpe[i] = 0.0;

    const long long head = head_of<F>(a, n);
    const vec *va = (const vec *)(a + head), *vb = (const vec *)((TWO ? b : a) + head);
    const long long nv = (n - head) / VEC;
    const long long tail = (n - head) - nv * VEC;
    constexpr long long TILE = (long long)BLOCK * U;
    const long long ntiles = nv / TILE;

    // register double-buffering: the next tile's loads are in flight while this one is absorbed.  Tile t goes to
    // workgroup t mod grid: the grid sweeps one compact window of addresses.
    long long t = blockIdx.x;
    if (t < ntiles) {
        // Two explicit register sets per stream, filled alternately; the loads are unconditional (past the end they
        // fetch the last tile again), so the compiler has no reason to copy one set into the other each trip
        // (16 v_mov_b64 per tile with a conditional reload) and both sets stay in flight.
        vec a0[U], a1[U], b0[UB], b1[UB];
        auto fill = [&](long long tile, vec (&pa)[U], vec (&pb)[UB]) {
            const long long base = (tile < ntiles ? tile : ntiles - 1) * TILE + threadIdx.x;
#pragma unroll
            for (int u = 0; u < U; ++u) {
                pa[u] = ld16(va + base + u * BLOCK);
                if constexpr (TWO) pb[u] = ld16(vb + base + u * BLOCK);
            }
        };
        auto absorb = [&](vec (&pa)[U], vec (&pb)[UB]) {
#pragma unroll
            for (int c = 0; c < U * VEC / CHUNK; ++c) {   // chunk c: CHUNK consecutive elements of this lane
                double x[CHUNK], y[CHUNK];
#pragma unroll
                for (int j = 0; j < CHUNK; ++j) {
                    const int e = c * CHUNK + j, u = e / VEC, k = e % VEC;
                    x[j] = F::at(pa[u], k);
                    if constexpr (TWO) y[j] = F::at(pb[u], k);
                }
                double e[CHUNK];
                if (!F::template divert<N>(fpe, L, x, TWO ? y : x, e)) F::template absorb<HOT, N, EE, COPIES, ZM>(fpe, L, x, e);
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
        const vec ra = va[i], rb = TWO ? vb[i] : ra;
        double x[VEC], y[VEC];
#pragma unroll
        for (int j = 0; j < VEC; ++j) x[j] = F::at(ra, j), y[j] = F::at(rb, j);
        double e[VEC];
        if (!F::template divert<N>(fpe, L, x, y, e)) F::template absorb<LOOSE, N, EE, COPIES, 0>(fpe, L, x, e);
    }
    // head / tail elements, one lane each
    if (blockIdx.x == 0 && (long long)threadIdx.x < head + tail) {
        const long long i = (long long)threadIdx.x < head ? threadIdx.x : n - tail + (threadIdx.x - head);
        double x[1] = {F::widen(a[i])}, y[1] = {F::widen((TWO ? b : a)[i])};
        double e[1];
        if (!F::template divert<N>(fpe, L, x, y, e)) F::template absorb<ONE, N, EE, COPIES, 0>(fpe, L, x, e);
    }
    LdsSink<COPIES> sink = L.sink();
    fpe_flush_sink<N>(fpe, sink);
    block_epilogue<COPIES>(s_acc, L.flags, gacc, gflags, ngroups);
}

// The strided kernel: a[i inca] (b[i incb]), and ExDOT on contiguous operands that may not stream as vectors
// (ExSUM.Superacc.cl:248-264 takes the same slow path)
template <class F, int N, bool EE, int COPIES>
__global__ void __launch_bounds__(BLOCK) k_blas1_strided(const typename F::elem *__restrict__ a, long long inca,
                                                         const typename F::elem *__restrict__ b, long long incb,
                                                         long long n, long long *__restrict__ gacc,
                                                         unsigned *__restrict__ gflags, int ngroups)
{
    constexpr bool TWO = F::STREAMS == 2;
    __shared__ long long s_acc[WAVES * NL * COPIES];
    for (int i = threadIdx.x; i < WAVES * NL * COPIES; i += BLOCK) s_acc[i] = 0;
    __syncthreads();
    Lane<COPIES> L(s_acc, gflags);
    double fpe[N > 0 ? N : 1];
#pragma unroll
    for (int i = 0; i < (N > 0 ? N : 1); ++i) fpe[i] = 0.0;
    // four independent loads in flight per lane and stream (a strided element is its own cache line: latency, not
    // bandwidth)
    const long long S = (long long)gridDim.x * BLOCK;
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += 4 * S) {
        double x[4], y[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const bool in = i + u * S < n;
            x[u] = in ? F::widen(a[(i + u * S) * inca]) : 0.0;
            if constexpr (TWO) y[u] = in ? F::widen(b[(i + u * S) * incb]) : 0.0;
        }
        double e[4];
        if (!F::template divert<N>(fpe, L, x, TWO ? y : x, e)) F::template absorb<LOOSE, N, EE, COPIES, 0>(fpe, L, x, e);
    }
    LdsSink<COPIES> sink = L.sink();
    fpe_flush_sink<N>(fpe, sink);
    block_epilogue<COPIES>(s_acc, L.flags, gacc, gflags, ngroups);
}

// streaming-kernel launch: plain, or -- when the context holds events for it -- with the events attached to the
// dispatch packet itself (exblas_internal.h: launch_stop_event)
#define EXB_LAUNCH_STREAMING(c, kernel, grid, st, ...)                                                                \
    do {                                                                                                               \
        if ((c).launch_stop_event || (c).launch_start_event) {                                                         \
            hipEvent_t ev0_ = (c).launch_start_event, ev1_ = (c).launch_stop_event;                                    \
            (c).launch_start_event = (c).launch_stop_event = nullptr;                                                  \
            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, st, ev0_, ev1_, 0, __VA_ARGS__);                 \
        } else {                                                                                                       \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, st, __VA_ARGS__);                                   \
        }                                                                                                              \
    } while (0)

static inline int grid_for(const Ctx &c, long long work_items, long long per_block, int blocks_per_cu)
{
    long long want = (work_items + per_block - 1) / per_block;
    long long cap = (long long)c.num_cu * blocks_per_cu;
    if (want < 1) want = 1;
    if (want >= cap) return (int)max(1ll, cap + c.grid_adj);
    return (int)want;
}

// ---------------------------------------------------------------------------------------------
// launchers, one per kernel; what a rule needs to know of the type or the operation comes from the front end
// ---------------------------------------------------------------------------------------------
template <class F, int N, bool EE, int COPIES>
static void run_stream(Ctx &c, const typename F::elem *a, const typename F::elem *b, long long n, hipStream_t st)
{
    constexpr bool DOT = F::STREAMS == 2;
    constexpr long long PER = (long long)BLOCK * U * F::VEC;   // elements of a tile
    int bpc = F::template bpc<N, EE>(c);
    // ExDOT, workgroups per CU: 48 at n = 2^28 (placement probe, round 2), but a workgroup should stream about five
    // tiles or more: at n = 2^25 -- a rank's shard of ONE 2^28 vector over 8 GPUs -- 48 per CU leave 1.3 tiles per
    // workgroup (some stream two, most one: 108 us with the finalize), 12 per CU 5.3 (93 us); 2^26: 179 -> 174 us with
    // 24 (tools/tune_shard.py).  An explicit smaller setting (exblas_set_tuning / EXBLAS_BPC_DOT) is kept.
    if (DOT) bpc = (int)min((long long)bpc, max(4ll, n / PER / (5ll * c.num_cu)));
    int grid = grid_for(c, n, PER, bpc);
    // An ODD number of workgroups.  ExSUM at the cap leaves one resident slot idle: the tiles a workgroup has in flight
    // are grid x 16 KiB apart, and with an even grid they compete for the same HBM channels -- 865 against 855 Gelem/s
    // at n = 2^28.  ExDOT adds one: a workgroup's successive tiles then walk through the 32 KiB period with which the
    // two streams' addresses compete for HBM channels, whatever b - a is.  With the even grid (32 x 256) the step time
    // at n = 2^28 depended on the relative placement of the two vectors, 0.625 ms (b - a = 16 KiB mod 32 KiB) to
    // 0.667 ms (0 mod 32 KiB); odd: 0.625-0.635 ms for every placement (tools/dot_align.py,
    // profiles/r02_exdot_placement.log).
    if (!(grid & 1) && (DOT ? grid > c.num_cu : grid == c.num_cu * bpc && grid > 1)) grid += DOT ? 1 : -1;
    // early-exit votes of the two-stream kernels by one fp64 compare per residue (ZM = 1): median 0.658 ms against
    // 0.699 by integer ORs at n = 2^28 (tools/tune.py, same box)
    c.last_blas1_kernel = F::K_STREAM, c.last_blas1_grid = grid;   // (exblas_last_blas1_info)
    EXB_LAUNCH_STREAMING(c, (k_blas1_stream<F, N, EE, COPIES, DOT && SKIP_ZERO_LEVELS<EE> ? 1 : 0>), grid, st, a, b, n,
                         c.gacc, c.gflags, c.ngroups);
}

template <class F, int N, bool EE, int COPIES>
static void run_strided(Ctx &c, const typename F::elem *a, long long inca, const typename F::elem *b, long long incb,
                        long long n, hipStream_t st)
{
    const int grid = grid_for(c, n, BLOCK, c.blocks_per_cu);
    c.last_blas1_kernel = F::K_STRIDED, c.last_blas1_grid = grid;
    EXB_LAUNCH_STREAMING(c, (k_blas1_strided<F, N, EE, COPIES>), grid, st, a, inca, b, incb, n, c.gacc, c.gflags,
                         c.ngroups);
}

// ExSUM passes its one operand and increment twice
template <class F, int N, bool EE>
static hipError_t launch_blas1(Ctx &c, const void *pa, long long inca, const void *pb, long long incb, long long n,
                               hipStream_t st)
{
    constexpr int COPIES = (N == 0) ? 16 : F::COPIES;
    const typename F::elem *a = (const typename F::elem *)pa, *b = (const typename F::elem *)pb;
    if (inca == 1 && incb == 1 && F::can_stream(a, b)) run_stream<F, N, EE, COPIES>(c, a, b, n, st);
    else run_strided<F, N, EE, COPIES>(c, a, inca, b, incb, n, st);
    return hipGetLastError();
}

}  // namespace exb
