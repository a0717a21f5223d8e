// spmm.hip -- ExSpMM for gfx950: exact, reproducible Y = alpha A X + beta Y, A in CSR (int32 or int64 indices), X and Y
// dense row-major blocks of k columns.
//
// Contract: column j of Y is, bit for bit, what ExSpMV (spmv.hip) gives for (A, X[:, j], alpha, beta, Y[:, j]):
//   Y[i, j] = Round( sum_p val[p] * fl(alpha * X[col[p], j])  (+)  beta * Y[i, j] )
// Every path below sums the multiset {p, e} of ExSpMV (TwoProd of every stored product, the beta terms) exactly and
// rounds it once, so the bits depend on nothing but the data.
//
// Structure (classification on the device, no host synchronisation, workspace from the context):
//   k_spmm_hist       one thread per row: rows longer than the split threshold, counted by floor(log2(length))
//   k_spmm_classify   one thread per row: rows longer than the threshold get k global accumulators (zeroed here); when
//                     the slots do not suffice, the longest rows have them (the threshold is raised to a power of two,
//                     from the counts).  lslot[row] says which slot (-1: the row runs whole)
//   k_spmm_main       LANES OWN COLUMNS.  An item is 64 outputs: one row x a tile of 64 columns (k > 32, the row and
//                     its entries are wave-uniform: scalar loads), or 64 / G consecutive rows x G columns (G = k rounded
//                     up to a power of two).  Per stored entry the X row is one contiguous read across the lanes; TwoProd
//                     and the FPE cascade run in the lane's own expansion, so no cross-lane merge exists.  An output
//                     whose expansion spilled, whose rounding spmv_round_fast cannot certify, or that is forced is NOT
//                     written: its bit is set in the item's 64-bit word of the deferral bitmap (one plain store per item)
//   k_spmm_deferred   scans the bitmap; every listed output is summed straight into an integer accumulator in LDS (8
//                     outputs of 8 lanes each per wave when the rows are short, one output per wave otherwise) and
//                     rounded by finish_wave.  Y[i, j] is still the caller's value when it is read for the beta term
//   k_spmv_long_prep  chunk bases of the split rows (shared with ExSpMV)
//   k_spmm_long       one wave per (chunk, column tile): lane expansions -> integer atomics into the row's global
//                     accumulators (order-free)
//   k_spmm_long_finish one wave per (split row, column): beta term, finish_wave, store
// fpe == 1 runs the same structure with plain fp64 sums (nothing is deferred).
// Narrow entries (exspmm_lp_dispatch): as in spmv.hip, the kernels are templates on the element types VT (values) and XT
// (X and Y); <LpF64, LpF64> is the fp64 routine, ldx and ldy count elements.
#include "spmv_common.hip.h"

namespace exb {

constexpr int SM_U = 4;                         // stored entries per step of the main loop (loads in flight)
constexpr long long SM_LONG_MIN = 1024;         // rows longer than this are split (one wave walks a row serially)
constexpr long long SM_CHUNK = 1024;            // entries per lane group (64 / G of them in a wave) and chunk of a split row
constexpr int SM_HIST = 16;                     // header words [16, 80): split candidates by floor(log2(length))
constexpr int SM_HDR_WORDS = SM_HIST + 64;
constexpr size_t SM_LACC_BYTES = (size_t)32 << 20;   // budget of the split rows' accumulators (k * 576 bytes a row)
constexpr int SM_DEF_G = 8;                     // lanes per deferred output when every row of the item is short
constexpr long long SM_DEF_SHORT = 64;

// the lane's expansion has no accumulator behind it: whatever would spill defers the output
struct DeferSink {
    unsigned &flags;
    __device__ __forceinline__ void add(double) { flags |= SP_SPILL; }
    __device__ __forceinline__ void note(unsigned) { flags |= SP_SPILL; }
};

struct AccSink {
    long long *acc;   // 68 limbs in LDS
    unsigned &flags;
    __device__ __forceinline__ void add(double x) { lds_add<1>(acc, x, flags); }
    __device__ __forceinline__ void note(unsigned) {}
};

// fl(alpha * W(X[c, j])) for an in-range column; a column outside [0, n) is never read and makes the row NaN
template <class XT, class I>
__device__ __forceinline__ double gather_xj(const typename XT::elem *__restrict__ xj, I c, long long ldx, int n,
                                            double alpha, unsigned &flags)
{
    if ((unsigned long long)(long long)c < (unsigned long long)n) return alpha * XT::widen(xj[(long long)c * ldx]);
    flags |= FLAG_NAN | SP_SPILL;
    return 0.0;
}

__device__ __forceinline__ long long uniform(long long v)
{
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}

struct ItemGeom {
    int lg;            // log2 of the lanes per row (G = 1 << lg)
    long long tiles;   // column tiles per row (1 unless G == 64)
    __device__ __forceinline__ long long row(long long item, int bit) const
    {
        return (item / tiles) * (64 >> lg) + (bit >> lg);
    }
    __device__ __forceinline__ long long col(long long item, int bit) const
    {
        return (item % tiles) * 64 + (bit & ((1 << lg) - 1));
    }
};

// ---------------------------------------------------------------------------------------------
// classification: slots of the split rows
// ---------------------------------------------------------------------------------------------
// Which rows are split must not depend on which thread comes first, and when the slots do not suffice for every row above
// the threshold the LONGEST rows must have them (a row that runs whole is walked by one wave).  So the rows above the
// threshold are counted by floor(log2(length)) first, and the threshold is raised to the smallest power of two (minus
// one) above which the slots suffice.
__device__ __forceinline__ int spmm_len_bucket(long long len)
{
    return len > 0 ? 63 - __builtin_clzll((unsigned long long)len) : 0;
}

template <class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmm_hist(int m, const I *__restrict__ rp, long long long_min,
                                                       long long *__restrict__ hdr)
{
    __shared__ unsigned cnt[64];   // per workgroup first: a matrix of equal rows would send every atomic to one word
    if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i < m) {
        const long long len = max(0ll, (long long)rp[i + 1] - (long long)rp[i]);
        if (len > long_min) atomicAdd(&cnt[spmm_len_bucket(len)], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 64 && cnt[threadIdx.x])
        atomicAdd((unsigned long long *)&hdr[SM_HIST + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

template <class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmm_classify(int m, int k, const I *__restrict__ rp, long long long_min,
                                                           int lcap, long long *__restrict__ hdr,
                                                           int *__restrict__ lslot, int *__restrict__ lrows,
                                                           long long *__restrict__ lacc)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= m) return;
    const long long len = max(0ll, (long long)rp[i + 1] - (long long)rp[i]);
    if (len <= long_min) return;   // lslot is only read for rows longer than long_min
    int b = 63;
    for (long long cum = 0; b >= 0 && cum + hdr[SM_HIST + b] <= (long long)lcap; --b) cum += hdr[SM_HIST + b];
    // the buckets above b fit; b < 0: every counted row does
    int s = -1;
    if (b < 0 || spmm_len_bucket(len) > b) {
        const long long slot = (long long)atomicAdd((unsigned long long *)&hdr[1], 1ull);
        if (slot < lcap) {
            s = (int)slot;
            lrows[slot] = i;
            long long *a = lacc + slot * (long long)k * SET_WORDS;
            for (long long t = 0; t < (long long)k * SET_WORDS; ++t) a[t] = 0;
        }
    }
    lslot[i] = s;   // no slot: the row runs whole (same bits)
}

// ---------------------------------------------------------------------------------------------
// main kernel: lanes own columns
// ---------------------------------------------------------------------------------------------
template <bool WIDE, bool PLAIN, class VT, class XT, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmm_main(int m, int n, int k, ItemGeom geo, const I *__restrict__ rp,
                                                       const I *__restrict__ ci, const typename VT::elem *__restrict__ val,
                                                       double alpha, const typename XT::elem *__restrict__ x, long long ldx,
                                                       double beta, typename XT::elem *__restrict__ y, long long ldy,
                                                       long long long_min, const int *__restrict__ lslot,
                                                       unsigned long long *__restrict__ bm, long long nitems,
                                                       long long *__restrict__ hdr, int force_defer)
{
    const int lane = threadIdx.x & 63;
    const long long w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const long long wave0 = (long long)blockIdx.x * SP_WAVES + w, nwaves = (long long)gridDim.x * SP_WAVES;
    unsigned long long n_reg = 0, n_def = 0;
    for (long long item = wave0; item < nitems; item += nwaves) {
        long long row = geo.row(item, lane);
        const long long j = geo.col(item, lane);
        if constexpr (WIDE) row = uniform(row);
        long long p0 = 0, p1 = 0;
        bool active = row < m && j < k;
        if (row < m) {
            p0 = (long long)rp[row];
            p1 = max(p0, (long long)rp[row + 1]);
            if (p1 - p0 > long_min && lslot[row] >= 0) active = false;   // split row: other kernels
        }
        if (!active || force_defer) p1 = p0;   // forced: k_spmm_deferred does all the work
        const typename XT::elem *xj = x + j;
        typename XT::elem *yp = y + row * ldy + j;
        unsigned flags = 0;
        if constexpr (PLAIN) {
            double s = 0.0;
            for (long long p = p0; __any(p < p1); ++p) {
                if (p < p1) s += val[p] * gather_xj<XT>(xj, ci[p], ldx, n, alpha, flags);
            }
            if (flags & FLAG_NAN) s = __builtin_nan("");
            if (active) *yp = (beta == 0.0) ? s : s + beta * *yp;
        } else {
            DeferSink sink{flags};
            double f[SP_N];
#pragma unroll
            for (int i = 0; i < SP_N; ++i) f[i] = 0.0;
            for (long long q0 = p0; __any(q0 < p1); q0 += SM_U) {
                double a[SM_U], xv[SM_U], p[SM_U], er[SM_U];
                I c[SM_U];
#pragma unroll
                for (int u = 0; u < SM_U; ++u) {
                    const long long q = q0 + u;
                    c[u] = 0;
                    a[u] = 0.0;
                    if (q < p1) {
                        c[u] = ci[q];
                        a[u] = VT::widen(val[q]);
                    }
                }
#pragma unroll
                for (int u = 0; u < SM_U; ++u) {
                    xv[u] = 0.0;
                    if (q0 + u < p1) xv[u] = gather_xj<XT>(xj, c[u], ldx, n, alpha, flags);
                }
#pragma unroll
                for (int u = 0; u < SM_U; ++u) p[u] = two_prod(a[u], xv[u], er[u]);
                fpe_absorb_prod<SP_N, true, SM_U>(f, p, er, sink);
                if (!__any(active && flags == 0)) break;   // every output of the item is deferred already
            }
            sp_absorb_beta<XT>(f, active, beta, yp, 0, sink);
            bool defer = false;
            if (active) {
                if constexpr (XT::DT == DT_F64) {   // (the fp64 kernel's own lines: its code stays what it was)
                    double r;
                    if (!force_defer && flags == 0 && spmv_round_fast<SP_N>(f, r)) *yp = r;
                    else defer = true;
                } else {
                    unsigned long long r;
                    if (!force_defer && flags == 0 && sp_round_fast_to<XT, SP_N>(f, r)) XT::store(yp, r);
                    else defer = true;
                }
            }
            const unsigned long long dm = __ballot(defer);
            if (lane == 0) bm[item] = dm;
            n_def += __popcll(dm);
            n_reg += __popcll(__ballot(active && !defer));
        }
    }
    if constexpr (!PLAIN) {
        if (lane == 0 && n_reg) atomicAdd((unsigned long long *)&hdr[4], n_reg);
        if (lane == 0 && n_def) atomicAdd((unsigned long long *)&hdr[5], n_def);
    }
}

// ---------------------------------------------------------------------------------------------
// deferred outputs: integer accumulator in LDS, finish_wave
// ---------------------------------------------------------------------------------------------
// up to 64 / G2 of the outputs listed in `bits` (an item's bitmap word), one per group of G2 lanes; returns the rest
template <int G2, class VT, class XT, class I>
__device__ __forceinline__ unsigned long long spmm_finish_some(unsigned long long bits, long long item, ItemGeom geo,
                                                               int n, const I *__restrict__ rp, const I *__restrict__ ci,
                                                               const typename VT::elem *__restrict__ val, double alpha,
                                                               const typename XT::elem *__restrict__ x, long long ldx,
                                                               double beta, typename XT::elem *__restrict__ y,
                                                               long long ldy,
                                                               long long (*acc)[NL], int round_mode)
{
    constexpr int NOUT = 64 / G2;
    const int lane = threadIdx.x & 63, grp = lane / G2, sub = lane % G2;
    int bit = -1, count = 0;
#pragma unroll
    for (int s = 0; s < NOUT; ++s) {
        if (bits) {
            const int b = __builtin_ctzll(bits);
            bits &= bits - 1ull;
            if (grp == s) bit = b;
            ++count;
        }
    }
    unsigned flags = 0;
    long long row = 0, j = 0;
    if (bit >= 0) {
        row = geo.row(item, bit);
        j = geo.col(item, bit);
        const long long p0 = (long long)rp[row], p1 = max(p0, (long long)rp[row + 1]);
        AccSink sink{acc[grp], flags};
        const typename XT::elem *xj = x + j;
        for (long long p = p0 + sub; p < p1; p += G2) {
            double e;
            const double a = VT::widen(ld_nt(val + p));
            const double pr = two_prod(a, gather_xj<XT>(xj, ld_nt(ci + p), ldx, n, alpha, flags), e);
            sink_product(sink, pr, e);
        }
        if (sub == 0 && beta != 0.0) {
            const double yv = XT::widen(y[row * ldy + j]);
            if (beta == 1.0) {
                sink.add(yv);
            } else {
                double e;
                const double pr = two_prod(beta, yv, e);
                sink_product(sink, pr, e);
            }
        }
    }
    sp_wave_sync();
    const NonFiniteLanes nf(flags);
    for (int s = 0; s < count; ++s) {   // wave-uniform: every lane runs the finish of each output
        const unsigned long long gm = G2 == 64 ? ~0ull : (((1ull << (G2 & 63)) - 1ull) << (s * (G2 & 63)));
        if constexpr (XT::DT == DT_F64) {   // (the fp64 kernel's own lines: its code stays what it was)
            const double v = sp_acc_round(acc[s], nf.of(gm), round_mode);
            const long long o_row = __shfl(row, s * G2, 64), o_j = __shfl(j, s * G2, 64);
            if (lane == 0) y[o_row * ldy + o_j] = v;
        } else {
            const unsigned long long v = sp_acc_round_to<XT>(acc[s], nf.of(gm), round_mode);
            const long long o_row = __shfl(row, s * G2, 64), o_j = __shfl(j, s * G2, 64);
            if (lane == 0) XT::store(y + (o_row * ldy + o_j), v);
        }
    }
    sp_wave_sync();
    return bits;
}

template <class VT, class XT, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmm_deferred(int m, int n, ItemGeom geo, const I *__restrict__ rp,
                                                           const I *__restrict__ ci,
                                                           const typename VT::elem *__restrict__ val, double alpha,
                                                           const typename XT::elem *__restrict__ x, long long ldx,
                                                           double beta, typename XT::elem *__restrict__ y, long long ldy,
                                                           const unsigned long long *__restrict__ bm, long long nitems,
                                                           int span, int round_mode)
{
    constexpr int NACC = 64 / SM_DEF_G;
    __shared__ long long acc[SP_WAVES][NACC][NL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int t = lane; t < NACC * NL; t += 64) (&acc[w][0][0])[t] = 0;
    sp_wave_sync();
    const long long wave0 = (long long)blockIdx.x * SP_WAVES + w, nwaves = (long long)gridDim.x * SP_WAVES;
    // a wave looks at `span` (<= 64) bitmap words per step: 64 when there are items enough for every wave, fewer when not
    for (long long base = wave0 * span; base < nitems; base += nwaves * span) {
        unsigned long long mine = 0;
        if (lane < span && base + lane < nitems) mine = bm[base + lane];
        unsigned long long todo = __ballot(mine != 0);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const long long item = base + l;
            unsigned long long bits = (unsigned long long)lane_bcast((long long)mine, l);
            // are all rows of the item short?  (lane r looks at the item's r-th row)
            bool is_long = false;
            {
                const long long r = geo.row(item, 0) + lane;
                if (lane < (64 >> geo.lg) && r < m)
                    is_long = max(0ll, (long long)rp[r + 1] - (long long)rp[r]) > SM_DEF_SHORT;
            }
            if (__any(is_long)) {
                while (bits)
                    bits = spmm_finish_some<64, VT, XT>(bits, item, geo, n, rp, ci, val, alpha, x, ldx, beta, y, ldy, acc[w],
                                                round_mode);
            } else {
                while (bits)
                    bits = spmm_finish_some<SM_DEF_G, VT, XT>(bits, item, geo, n, rp, ci, val, alpha, x, ldx, beta, y,
                                                              ldy, acc[w], round_mode);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// split rows: chunks into the row's k global accumulators, finish
// ---------------------------------------------------------------------------------------------
template <bool PLAIN, class VT, class XT, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmm_long(int n, int k, ItemGeom geo, const I *__restrict__ rp,
                                                       const I *__restrict__ ci, const typename VT::elem *__restrict__ val,
                                                       double alpha, const typename XT::elem *__restrict__ x, long long ldx,
                                                       const int *__restrict__ lrows, const long long *__restrict__ lbase,
                                                       int lcap, long long chunk, long long *__restrict__ hdr,
                                                       long long *__restrict__ lacc)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int G = 1 << geo.lg, part = lane >> geo.lg, nparts = 64 >> geo.lg;   // the chunk's entries go round the parts
    const long long nl = min(hdr[1], (long long)lcap), total = hdr[2] * geo.tiles;
    const long long wave0 = (long long)blockIdx.x * SP_WAVES + w, nwaves = (long long)gridDim.x * SP_WAVES;
    unsigned long long n_chunks = 0;
    for (long long u = wave0; u < total; u += nwaves) {
        const long long t = u / geo.tiles;
        const long long j = (u % geo.tiles) * 64 + (lane & (G - 1));
        const long long lo = sp_chunk_owner(lbase, nl, t);
        const int row = lrows[lo];
        const long long r0 = (long long)rp[row], r1 = max(r0, (long long)rp[row + 1]);
        const long long p0 = r0 + (t - lbase[lo]) * chunk, p1 = min(r1, p0 + chunk);
        const bool active = j < k;
        long long *g = lacc + (lo * (long long)k + (active ? j : 0)) * SET_WORDS;
        const typename XT::elem *xj = x + j;
        unsigned flags = 0;
        if (u % geo.tiles == 0) ++n_chunks;
        if constexpr (PLAIN) {
            double s = 0.0;
            if (active)
                for (long long p = p0 + part; p < p1; p += nparts)
                    s += ld_nt(val + p) * gather_xj<XT>(xj, ld_nt(ci + p), ldx, n, alpha, flags);
            if (flags & FLAG_NAN) s = __builtin_nan("");
            if (active) atomicAdd((double *)g, s);
        } else {
            GlobalSink sink{g};
            double f[SP_N];
#pragma unroll
            for (int i = 0; i < SP_N; ++i) f[i] = 0.0;
            for (long long q0 = p0 + part; __any(q0 < p1); q0 += (long long)nparts * SM_U) {
                double p[SM_U], er[SM_U];
#pragma unroll
                for (int v = 0; v < SM_U; ++v) {
                    const long long q = q0 + (long long)v * nparts;
                    double a = 0.0, xv = 0.0;
                    if (active && q < p1) {
                        a = VT::widen(ld_nt(val + q));
                        xv = gather_xj<XT>(xj, ld_nt(ci + q), ldx, n, alpha, flags);
                    }
                    p[v] = two_prod(a, xv, er[v]);
                }
                fpe_absorb_prod<SP_N, true, SM_U>(f, p, er, sink);
            }
            fpe_flush_sink<SP_N>(f, sink);
            if (flags & FLAG_NAN) atomicAdd((unsigned long long *)&g[NL + 2], 1ull);   // a column outside [0, n)
        }
    }
    if (lane == 0 && n_chunks) atomicAdd((unsigned long long *)&hdr[7], n_chunks);
}

template <bool PLAIN, class XT>
__global__ void __launch_bounds__(SP_BLOCK) k_spmm_long_finish(int k, const int *__restrict__ lrows, int lcap,
                                                              double beta, typename XT::elem *__restrict__ y, long long ldy,
                                                              long long *__restrict__ hdr,
                                                              const long long *__restrict__ lacc, int round_mode)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long nl = min(hdr[1], (long long)lcap);
    const long long wave0 = (long long)blockIdx.x * SP_WAVES + w, nwaves = (long long)gridDim.x * SP_WAVES;
    for (long long o = wave0; o < nl * k; o += nwaves) {
        const long long i = o / k, j = o % k;
        typename XT::elem *yp = y + (long long)lrows[i] * ldy + j;
        const long long *g = lacc + o * SET_WORDS;
        if constexpr (PLAIN) {
            const double s = __longlong_as_double(g[0]);
            if (lane == 0) *yp = (beta == 0.0) ? s : s + beta * *yp;
        } else {
            long long v0 = g[lane], v1 = lane < NL - 64 ? g[64 + lane] : 0;
            unsigned flags = (g[NL] ? FLAG_PINF : 0u) | (g[NL + 1] ? FLAG_NINF : 0u) | (g[NL + 2] ? FLAG_NAN : 0u);
            sp_wave_add_beta<XT>(v0, v1, beta, yp, 0, flags);
            const WaveFinish r = finish_wave(v0, v1, flags);
            const unsigned long long v = sp_pick_to<XT>(r, flags, round_mode);
            if (lane == 0) XT::store(yp, v);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) hdr[6] = nl;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
template <bool PLAIN, class VT, class XT, class I>
static hipError_t spmm_launch(Ctx &c, int m, int n, int k, const I *rp, const I *ci, const typename VT::elem *val,
                              double alpha, const typename XT::elem *x, long long ldx, double beta, typename XT::elem *y,
                              long long ldy, int force_defer, int round_mode, hipStream_t st)
{
    const SplitRule split = sp_split_rule(c.spmm_path, SM_LONG_MIN, SM_CHUNK);
    const long long long_min = split.long_min;
    const int lcap = (int)min((long long)m, (long long)(SM_LACC_BYTES / ((size_t)k * SET_WORDS * 8)));
    ItemGeom geo;
    geo.lg = 0;
    while (geo.lg < 6 && (1 << geo.lg) < k) ++geo.lg;
    geo.tiles = geo.lg == 6 ? ((long long)k + 63) / 64 : 1;
    // a wave's lane groups share a chunk's entries round-robin: the chunk grows with their number, so that a column of a
    // split row sees the same number of atomic flushes whatever k is
    const long long chunk = split.chunk * (64 >> geo.lg);
    const long long rpw = 64 >> geo.lg, nitems = (((long long)m + rpw - 1) / rpw) * geo.tiles;
    const size_t b_hdr = 1024, b_lslot = align256((size_t)m * 4), b_lrows = align256((size_t)lcap * 4),
                 b_lbase = align256((size_t)(lcap + 1) * 8), b_bm = align256((size_t)nitems * 8),
                 b_lacc = (size_t)lcap * (size_t)k * SET_WORDS * 8;
    hipError_t e;
    char *base = (char *)workspace(c, b_hdr + b_lslot + b_lrows + b_lbase + b_bm + b_lacc, st, &e);
    if (!base) return e;
    long long *hdr = (long long *)base;
    int *lslot = (int *)(base + b_hdr);
    int *lrows = (int *)(base + b_hdr + b_lslot);
    long long *lbase = (long long *)(base + b_hdr + b_lslot + b_lrows);
    unsigned long long *bm = (unsigned long long *)(base + b_hdr + b_lslot + b_lrows + b_lbase);
    long long *lacc = (long long *)(base + b_hdr + b_lslot + b_lrows + b_lbase + b_bm);
    c.spmm_info_dev = hdr;
    hipLaunchKernelGGL(k_sp_zero_header, dim3(1), dim3(64), 0, st, hdr, SM_HDR_WORDS);
    const int cap = c.num_cu * 8;
    hipLaunchKernelGGL((k_spmm_hist<I>), dim3((m + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, st, m, rp, long_min, hdr);
    hipLaunchKernelGGL((k_spmm_classify<I>), dim3((m + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, st, m, k, rp, long_min,
                       lcap, hdr, lslot, lrows, lacc);
    const int grid = (int)min((long long)cap, (nitems + SP_WAVES - 1) / SP_WAVES);
    if (geo.lg == 6)
        hipLaunchKernelGGL((k_spmm_main<true, PLAIN, VT, XT, I>), dim3(grid), dim3(SP_BLOCK), 0, st, m, n, k, geo, rp, ci, val,
                           alpha, x, ldx, beta, y, ldy, long_min, (const int *)lslot, bm, nitems, hdr, force_defer);
    else
        hipLaunchKernelGGL((k_spmm_main<false, PLAIN, VT, XT, I>), dim3(grid), dim3(SP_BLOCK), 0, st, m, n, k, geo, rp, ci, val,
                           alpha, x, ldx, beta, y, ldy, long_min, (const int *)lslot, bm, nitems, hdr, force_defer);
    if constexpr (!PLAIN) {
        const long long span = max(1ll, min(64ll, nitems / ((long long)cap * SP_WAVES)));
        const int gd = (int)min((long long)cap, (nitems + span * SP_WAVES - 1) / (span * SP_WAVES));
        hipLaunchKernelGGL((k_spmm_deferred<VT, XT, I>), dim3(gd), dim3(SP_BLOCK), 0, st, m, n, geo, rp, ci, val, alpha, x, ldx,
                           beta, y, ldy, (const unsigned long long *)bm, nitems, (int)span, round_mode);
    }
    hipLaunchKernelGGL((k_spmv_long_prep<I>), dim3(1), dim3(1024), 0, st, rp, (const int *)lrows, lcap, chunk, hdr, lbase);
    hipLaunchKernelGGL((k_spmm_long<PLAIN, VT, XT, I>), dim3(cap), dim3(SP_BLOCK), 0, st, n, k, geo, rp, ci, val, alpha, x, ldx,
                       (const int *)lrows, (const long long *)lbase, lcap, chunk, hdr, lacc);
    {
        const int gl = (int)min((long long)c.num_cu * 2, ((long long)lcap * k + SP_WAVES - 1) / SP_WAVES);
        hipLaunchKernelGGL((k_spmm_long_finish<PLAIN, XT>), dim3(max(gl, 1)), dim3(SP_BLOCK), 0, st, k, (const int *)lrows,
                           lcap, beta, y, ldy, hdr, (const long long *)lacc, round_mode);
    }
    return hipGetLastError();
}

hipError_t exspmm_dispatch(Ctx &c, int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx,
                           const double *val, double alpha, const double *x, long long ldx, double beta, double *y,
                           long long ldy, int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    if (m == 0 || k == 0) return hipSuccess;
    // fpe == 0, the accumulator test path and the reference rounding mode round every output from an integer accumulator
    const int force_defer = (fpe == 0 || c.spmm_path == 1 || round_mode) ? 1 : 0;
    return sp_dispatch(index_bits, fpe, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
        constexpr bool PLAIN = decltype(plain)::value;   // the plain kernels neither defer nor round
        return spmm_launch<PLAIN, LpF64, LpF64>(c, m, n, k, rp, ci, val, alpha, x, ldx, beta, y, ldy,
                                                PLAIN ? 0 : force_defer, PLAIN ? 0 : round_mode, st);
    });
}

// The narrow entry, as exspmv_lp_dispatch (spmv.hip): values of val_dtype, X and Y of vec_dtype (float64 or val_dtype; the
// caller has checked the pair and that fpe != 1); ldx and ldy in elements
template <class VT, class XT>
static hipError_t spmm_lp_typed(Ctx &c, int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx,
                                const void *val, double alpha, const void *x, long long ldx, double beta, void *y,
                                long long ldy, int force_defer, int round_mode, hipStream_t st)
{
    return sp_dispatch(index_bits, 0, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
        if constexpr (decltype(plain)::value) return hipErrorInvalidValue;   // (fpe = 0 was passed: never taken)
        else
            return spmm_launch<false, VT, XT>(c, m, n, k, rp, ci, (const typename VT::elem *)val, alpha,
                                              (const typename XT::elem *)x, ldx, beta, (typename XT::elem *)y, ldy,
                                              force_defer, round_mode, st);
    });
}

hipError_t exspmm_lp_dispatch(Ctx &c, int m, int n, int k, int index_bits, const void *row_ptr, const void *col_idx,
                              int val_dtype, const void *val, double alpha, int vec_dtype, const void *x, long long ldx,
                              double beta, void *y, long long ldy, int fpe, int round_mode, hipStream_t st)
{
    if (m == 0 || k == 0) return hipSuccess;
    const int force_defer = (fpe == 0 || c.spmm_path == 1 || round_mode) ? 1 : 0;
    hipError_t e = hipErrorInvalidValue;
    auto run = [&](auto vt, auto xt) {
        e = spmm_lp_typed<decltype(vt), decltype(xt)>(c, m, n, k, index_bits, row_ptr, col_idx, val, alpha, x, ldx, beta,
                                                      y, ldy, force_defer, round_mode, st);
    };
    auto by_value = [&](auto vt) {
        if (vec_dtype == DT_F64) run(vt, LpF64());
        else run(vt, vt);
    };
    if (val_dtype == DT_F32) by_value(LpF32());
    else if (val_dtype == DT_F16) by_value(LpF16());
    else if (val_dtype == DT_BF16) by_value(LpBF16());
    return e;
}

}  // namespace exb
