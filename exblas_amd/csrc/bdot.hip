// bdot.hip -- ExBDOT for gfx950: exact, reproducible inner products of two dense row-major blocks, read once.
//   'G' (Gram):     C[i, j] = Round( sum_r X[r, i] * Y[r, j] )       X: n x p (ldx), Y: n x q (ldy), C: p x q (ldc)
//   'D' (diagonal): c[j]    = Round( sum_r X[r, j] * Y[r, j] )       p == q
//
// Contract: every output is, bit for bit, the value ExDOT returns for the two columns (the `exact` word, or the `refmode`
// word under the reference rounding mode) inside ExGEMV's product domain: every product is split by TwoProd, the
// multiset {p, e} is summed exactly and rounded once, so the bits depend on nothing but the data.
//
// Structure (two kernels, the normalisable digit sets of the outputs between them; workspace from the context):
//   k_bdot_acc       LANES OWN OUTPUTS.  A workgroup owns a tile of T <= 64 outputs and a slab of rows; a wave covers
//                    64 / T consecutive rows per step (lane = row-in-step * T + output), the four waves take the steps
//                    round-robin.  'D': output c of the tile is column c of a panel of T columns -- with ld == k the loads
//                    of a wave are one contiguous run.  'G': output c is (i, j) = (c / TJ, c % TJ) of a TI x TJ tile; the
//                    TI + TJ values of a row are read by the 64 lanes as broadcasts out of two cache lines.  Each lane
//                    keeps ONE expansion for its output (TwoProd, fpe_absorb_prod with the range guard); whatever spills,
//                    and the expansion at the end of the slab, goes to the output's 68 limbs in LDS (ds_add_u64, shared
//                    by the waves).  Epilogue: the non-zero limbs are added to the output's set of one of `ngroups` group
//                    accumulators with int64 atomics (exact, order-free); non-finite products count in words 68..70
//   k_bdot_finalize  one wave per output: sums the copies of its set (the groups; or the sets of several shards, read
//                    only) with low and high halves apart, so that the sum cannot overflow, finish_wave, stores the
//                    double of the rounding mode, leaves the groups zero
//   k_bdot_export    the row-sharded form's first half: the same sum of the groups, finish_wave<false>, and the normalised
//                    digits (67 in [0, 2^32) under a signed top digit, three non-finite indicators) go out instead of the
//                    double -- 72 int64 per output that add across ranks as plain integers; k_bdot_finalize rounds the sum
// Outputs beyond 4096 (more than 64 x 64 in 'G') are served batch by batch with the same workspace.
// fpe == 1 runs the same structure on plain fp64 sums (fp64 atomics: not reproducible).
#include "superacc.hip.h"
#include "fpe.hip.h"
#include "exblas_internal.h"

namespace exb {

constexpr int BD_BLOCK = 256;
constexpr int BD_WAVES = BD_BLOCK / 64;
constexpr int BD_U = 4;                 // row steps per lane in flight
constexpr int BD_COLS = 64;             // LDS accumulators of a workgroup (outputs of a tile)
constexpr int BD_EDGE = 64;             // 'G': a batch is at most BD_EDGE x BD_EDGE outputs
constexpr int BD_BATCH = BD_EDGE * BD_EDGE;   // outputs per accumulate / finalize pair
constexpr int BD_MAX_GROUPS = 32;
constexpr int BD_GROUP_SETS = 256;      // group accumulators are kept while ngroups * outputs stays within this
constexpr long long BD_MIN_STEPS = 16;  // automatic path: steps of a slab (a workgroup's epilogue costs about one step per limb)
constexpr long long BD_MAX_SLABS = 1 << 20;

struct BdotGeom {
    int diag;          // 'D'
    int T, TJ;         // outputs per tile; 'G': columns of Y in a tile (T = TI * TJ)
    int rpw;           // rows of a wave step: 64 / T
    int i0, j0;        // the batch: first column of X and of Y
    int ni, nj;        // the batch: columns of X and of Y ('D': nj == 1, the outputs are ni)
    int ntj, ntiles;   // tiles along j, tiles of the batch
    long long steps;   // steps of every wave in a slab: a slab is steps * BD_WAVES * rpw rows
    int ngroups;
};

// output c of a tile: its columns of X and Y and its index among the batch's outputs; false beyond the batch's edge
__device__ __forceinline__ bool bd_output(const BdotGeom &g, int tile, int c, int &xi, int &yj, int &o)
{
    if (g.diag) {
        xi = yj = tile * g.T + c;
        o = xi;
        return xi < g.ni;
    }
    const int TI = g.T / g.TJ;
    xi = (tile / g.ntj) * TI + c / g.TJ;
    yj = (tile % g.ntj) * g.TJ + c % g.TJ;
    o = xi * g.nj + yj;
    return xi < g.ni && yj < g.nj;
}

template <int N, bool EE, bool PLAIN>
__global__ void __launch_bounds__(BD_BLOCK) k_bdot_acc(BdotGeom g, long long n, const double *__restrict__ x,
                                                      long long ldx, const double *__restrict__ y, long long ldy,
                                                      long long *__restrict__ sets)
{
    __shared__ long long s_acc[NL * BD_COLS];   // limb-major: the bank of an access depends on the output only
    __shared__ unsigned s_flags[BD_COLS];
    for (int i = threadIdx.x; i < NL * BD_COLS; i += BD_BLOCK) s_acc[i] = 0;
    if (threadIdx.x < BD_COLS) s_flags[threadIdx.x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int tile = (int)(blockIdx.x % (unsigned)g.ntiles);
    const long long slab = blockIdx.x / (unsigned)g.ntiles;
    const int c = lane % g.T, r = lane / g.T;
    int xi, yj, o;
    const bool active = bd_output(g, tile, c, xi, yj, o) && r < g.rpw;
    const double *xp = x + g.i0 + xi, *yp = y + g.j0 + yj;
    const long long row0 = slab * g.steps * BD_WAVES * g.rpw;
    unsigned flags = 0;
    LdsSink<BD_COLS> sink{s_acc + c, flags};
    double f[N > 0 ? N : 1];
#pragma unroll
    for (int i = 0; i < (N > 0 ? N : 1); ++i) f[i] = 0.0;
    double plain = 0.0;
    // every lane of the workgroup runs the same steps (the votes of the cascade are wave-wide); lanes without a row add 0
    for (long long s0 = 0; s0 < g.steps && row0 + s0 * BD_WAVES * g.rpw < n; s0 += BD_U) {
        double a[BD_U], b[BD_U];
#pragma unroll
        for (int u = 0; u < BD_U; ++u) {
            const long long row = row0 + ((s0 + u) * BD_WAVES + w) * g.rpw + r;
            a[u] = b[u] = 0.0;
            if (active && s0 + u < g.steps && row < n) {
                if (g.diag) {   // read once
                    a[u] = __builtin_nontemporal_load(xp + row * ldx);
                    b[u] = __builtin_nontemporal_load(yp + row * ldy);
                } else {        // read again by the other tiles of the slab
                    a[u] = xp[row * ldx];
                    b[u] = yp[row * ldy];
                }
            }
        }
        if constexpr (PLAIN) {
#pragma unroll
            for (int u = 0; u < BD_U; ++u) plain += a[u] * b[u];
        } else {
            double p[BD_U], e[BD_U];
#pragma unroll
            for (int u = 0; u < BD_U; ++u) p[u] = two_prod(a[u], b[u], e[u]);
            fpe_absorb_prod<N, EE, BD_U>(f, p, e, sink);
        }
    }
    if constexpr (PLAIN) {
        if (active) atomicAdd((double *)&s_acc[c], plain);
    } else {
        fpe_flush_sink<N>(f, sink);
        if (flags & FLAG_NONFINITE) atomicOr(&s_flags[c], flags & FLAG_NONFINITE);
    }
    __syncthreads();
    long long *gs = sets + (long long)(slab % g.ngroups) * ((long long)g.ni * g.nj) * SET_WORDS;
    if constexpr (PLAIN) {
        const int cc = threadIdx.x;
        if (cc < g.T && bd_output(g, tile, cc, xi, yj, o))
            atomicAdd((double *)&gs[(long long)o * SET_WORDS], __longlong_as_double(s_acc[cc]));
    } else {
        for (int t = threadIdx.x; t < g.T * (NL + 3); t += BD_BLOCK) {
            const int cc = t % g.T, l = t / g.T;
            if (!bd_output(g, tile, cc, xi, yj, o)) continue;
            // limbs, then the three non-finite indicators
            const long long v = l < NL ? s_acc[l * BD_COLS + cc] : (long long)((s_flags[cc] >> (l - NL)) & 1u);
            if (v != 0) atomicAdd((unsigned long long *)&gs[(long long)o * SET_WORDS + l], (unsigned long long)v);
        }
    }
}

// the group sets before a batch accumulates into them (a kernel, not a memset: a captured memset node of this size did
// not survive a second replay of the graph)
__global__ void __launch_bounds__(BD_BLOCK) k_bdot_zero(long long *__restrict__ sets, long long count)
{
    for (long long i = (long long)blockIdx.x * BD_BLOCK + threadIdx.x; i < count; i += (long long)gridDim.x * BD_BLOCK)
        sets[i] = 0;
}

// One wave sums the `ncopies` copies of an output's set, `stride` words apart (the accumulator groups, or the exported
// sets of the shards): the low 32 bits and the signed high parts of the limbs are summed apart and the high parts enter
// one limb up (as in k_finalize), so the sum cannot overflow however many adds the copies hold -- nor can 2^31 copies of
// normalised digits.  ZERO: the copies are left zero.  v0: limb `lane`, v1: limb 64 + lane (lane < 4); a non-zero word
// 68 / 69 / 70 in any copy raises FLAG_PINF / FLAG_NINF / FLAG_NAN.
template <bool ZERO>
__device__ __forceinline__ void bd_sum_copies(std::conditional_t<ZERO, long long, const long long> *p, long long stride,
                                              int ncopies, long long &v0, long long &v1, unsigned &flags)
{
    const int lane = threadIdx.x & 63;
    long long lo0 = 0, hi0 = 0, lo1 = 0, hi1 = 0;
    flags = 0;
    for (int k = 0; k < ncopies; ++k, p += stride) {
        const long long t0 = p[lane], t1 = lane < SET_WORDS - 64 ? p[64 + lane] : 0;
        if constexpr (ZERO) {
            p[lane] = 0;
            if (lane < SET_WORDS - 64) p[64 + lane] = 0;
        }
        lo0 += t0 & 0xffffffffll;
        hi0 += t0 >> 32;
        if (lane < NL - 65) {
            lo1 += t1 & 0xffffffffll;
            hi1 += t1 >> 32;
        } else if (lane == NL - 65) {   // the top limb is never split
            lo1 += t1;
        } else if (lane < NL - 64 + 3 && t1 != 0) {   // words 68..70: +Inf, -Inf, NaN seen
            flags |= 1u << (lane - (NL - 64));
        }
    }
    flags = (__ballot(flags & FLAG_PINF) ? FLAG_PINF : 0u) | (__ballot(flags & FLAG_NINF) ? FLAG_NINF : 0u) |
            (__ballot(flags & FLAG_NAN) ? FLAG_NAN : 0u);
    long long in0 = __shfl_up(hi0, 1), in1 = __shfl_up(hi1, 1);
    const long long h63 = __shfl(hi0, 63);
    if (lane == 0) {
        in0 = 0;
        in1 = h63;
    }
    v0 = lo0 + in0;
    v1 = lane < NL - 64 ? lo1 + in1 : 0;
}

// output o of the batch rounds the copies at sets + o * SET_WORDS + k * stride, k < ncopies
template <bool PLAIN, bool ZERO>
__global__ void __launch_bounds__(BD_BLOCK) k_bdot_finalize(BdotGeom g,
                                                           std::conditional_t<ZERO, long long, const long long> *__restrict__ sets,
                                                           long long stride, int ncopies, double *__restrict__ out,
                                                           long long ldc, int round_mode)
{
    const int lane = threadIdx.x & 63;
    const long long nout = (long long)g.ni * g.nj;
    const long long o = (long long)blockIdx.x * BD_WAVES + (threadIdx.x >> 6);
    if (o >= nout) return;   // (the whole wave)
    double *dst = g.diag ? out + g.i0 + o : out + (g.i0 + o / g.nj) * ldc + g.j0 + o % g.nj;
    if constexpr (PLAIN) {
        static_assert(ZERO, "the plain sums live in the groups only");
        if (lane == 0) {
            double s = 0.0;
            for (int k = 0; k < ncopies; ++k) {
                long long *p = sets + k * stride + o * SET_WORDS;
                s += __longlong_as_double(p[0]);
                p[0] = 0;
            }
            *dst = s;
        }
    } else {
        long long v0, v1;
        unsigned flags;
        bd_sum_copies<ZERO>(sets + o * SET_WORDS, stride, ncopies, v0, v1, flags);
        const WaveFinish r = finish_wave(v0, v1, flags);
        if (lane == 0) *dst = round_mode ? r.rf : __longlong_as_double((long long)r.ex);
    }
}

// output o of the batch: the groups summed and left zero, the normalised set stored at dst + (row * dst_ld + column) *
// SET_WORDS, row and column those of the output in the whole result (dst_i0, dst_j0: the batch's corner there; 'D': the
// output's index).  dst may be the groups' own block with the batch's outputs in order (dst_ld == g.nj, corner 0): a wave
// has read, and zeroed, all it owns in every group before it stores into group 0's set of its own output.
__global__ void __launch_bounds__(BD_BLOCK) k_bdot_export(BdotGeom g, long long *sets, long long *dst, long long dst_i0,
                                                         long long dst_j0, long long dst_ld)
{
    const int lane = threadIdx.x & 63;
    const long long nout = (long long)g.ni * g.nj;
    const long long o = (long long)blockIdx.x * BD_WAVES + (threadIdx.x >> 6);
    if (o >= nout) return;   // (the whole wave)
    long long v0, v1;
    unsigned flags;
    bd_sum_copies<true>(sets + o * SET_WORDS, nout * SET_WORDS, g.ngroups, v0, v1, flags);
    const WaveFinish r = finish_wave<false>(v0, v1, flags);
    long long *d = dst + (g.diag ? dst_i0 + o : (dst_i0 + o / g.nj) * dst_ld + dst_j0 + o % g.nj) * SET_WORDS;
    d[lane] = r.d0;
    // limbs 64..67, then +Inf / -Inf / NaN seen as 0 or 1, then a zero word
    if (lane < SET_WORDS - 64) d[64 + lane] = lane < NL - 64 ? r.d1 : (lane < NL - 64 + 3 ? (long long)((flags >> (lane - (NL - 64))) & 1u) : 0ll);
}

// where the outputs of a launch go: doubles (`sets_out` and `merge` null), the exported sets of the whole result in output
// order (`sets_out`), or doubles rounded from the sets that `merge` has summed over the ranks, batch by batch
struct BdotSink {
    double *out = nullptr;
    long long ldc = 0;
    int round_mode = 0;
    long long *sets_out = nullptr;
    const BdotMerge *merge = nullptr;
};

template <int N, bool EE, bool PLAIN>
static int bdot_launch(Ctx &c, bool diag, long long n, int p, int q, const double *x, long long ldx, const double *y,
                       long long ldy, const BdotSink &sink, hipStream_t st)
{
    hipError_t err;
    // the footprint depends on nothing: a captured call replays into the block any earlier call (or a reservation) left
    long long *sets = (long long *)workspace(c, (size_t)BD_BATCH * SET_WORDS * 8, st, &err);
    if (!sets) return (int)err;
    const int narrow = c.bdot_path == 2;
    const int bi = diag ? BD_BATCH : BD_EDGE;
    for (int i0 = 0; i0 < p; i0 += bi) {
        for (int j0 = 0; j0 < (diag ? 1 : q); j0 += BD_EDGE) {
            BdotGeom g;
            g.diag = diag;
            g.i0 = i0;
            g.j0 = diag ? i0 : j0;
            g.ni = min(bi, p - i0);
            g.nj = diag ? 1 : min(BD_EDGE, q - j0);
            if (diag) {
                g.TJ = 1;
                g.T = min(g.ni, narrow ? 4 : BD_COLS);
                g.ntj = 1;
                g.ntiles = (g.ni + g.T - 1) / g.T;
            } else {
                g.TJ = min(g.nj, narrow ? 4 : 8);
                const int TI = min(g.ni, narrow ? 4 : BD_COLS / g.TJ);
                g.T = TI * g.TJ;
                g.ntj = (g.nj + g.TJ - 1) / g.TJ;
                g.ntiles = ((g.ni + TI - 1) / TI) * g.ntj;
            }
            g.rpw = 64 / g.T;
            const long long nout = (long long)g.ni * g.nj;
            g.ngroups = (int)max(1ll, min((long long)BD_MAX_GROUPS, BD_GROUP_SETS / nout));
            // the row slab: workgroups enough to fill the chip a few times over, every slab a whole number of BD_U steps
            const long long total = (n + (long long)BD_WAVES * g.rpw - 1) / (BD_WAVES * g.rpw);
            const long long want = max(1ll, (long long)c.num_cu * 8 / g.ntiles);
            g.steps = c.bdot_path == 1 ? 1 : max(BD_MIN_STEPS, (total + want - 1) / want);
            g.steps = max(g.steps, (total + BD_MAX_SLABS - 1) / BD_MAX_SLABS);
            if (c.bdot_path != 1) g.steps = (g.steps + BD_U - 1) / BD_U * BD_U;
            const long long nslabs = max(1ll, (total + g.steps - 1) / g.steps);
            // the workspace is shared with routines that leave scratch in it: the sets are zeroed here as well
            const long long nzero = (long long)g.ngroups * nout * SET_WORDS;
            hipLaunchKernelGGL(k_bdot_zero, dim3((unsigned)min(4096ll, (nzero + BD_BLOCK - 1) / BD_BLOCK)), dim3(BD_BLOCK), 0,
                               st, sets, nzero);
            hipLaunchKernelGGL((k_bdot_acc<N, EE, PLAIN>), dim3((unsigned)(nslabs * g.ntiles)), dim3(BD_BLOCK), 0, st, g, n,
                               x, ldx, y, ldy, sets);
            const dim3 waves((unsigned)((nout + BD_WAVES - 1) / BD_WAVES));
            if constexpr (!PLAIN) {
                if (sink.sets_out) {
                    hipLaunchKernelGGL(k_bdot_export, waves, dim3(BD_BLOCK), 0, st, g, sets, sink.sets_out, (long long)g.i0,
                                       (long long)g.j0, (long long)q);
                    continue;
                }
                if (sink.merge) {
                    // in place: the batch's normalised sets land in group 0's block, contiguous over the batch; ONE
                    // all-reduce over them, and the sum is rounded as one copy (and left zero)
                    hipLaunchKernelGGL(k_bdot_export, waves, dim3(BD_BLOCK), 0, st, g, sets, sets, 0ll, 0ll, (long long)g.nj);
                    if ((err = hipGetLastError()) != hipSuccess) return (int)err;
                    if (int rc = sink.merge->allreduce(sink.merge->user, sets, (size_t)nout * SET_WORDS, st)) return rc;
                    hipLaunchKernelGGL((k_bdot_finalize<false, true>), waves, dim3(BD_BLOCK), 0, st, g, sets, 0ll, 1, sink.out,
                                       sink.ldc, sink.round_mode);
                    continue;
                }
            }
            hipLaunchKernelGGL((k_bdot_finalize<PLAIN, true>), waves, dim3(BD_BLOCK), 0, st, g, sets, nout * SET_WORDS,
                               g.ngroups, sink.out, sink.ldc, sink.round_mode);
        }
    }
    return (int)hipGetLastError();
}

template <bool PLAIN_OK>
static int bdot_variant(Ctx &c, char mode, long long n, int p, int q, const double *x, long long ldx, const double *y,
                        long long ldy, const BdotSink &sink, int fpe, int early_exit, hipStream_t st)
{
    const bool diag = mode == 'D' || mode == 'd';
    if (p == 0 || q == 0) return 0;
    if constexpr (PLAIN_OK) {
        if (fpe == 1) {
            BdotSink plain = sink;
            plain.round_mode = 0;
            return bdot_launch<0, false, true>(c, diag, n, p, q, x, ldx, y, ldy, plain, st);
        }
    }
    if (fpe < 3) return bdot_launch<0, false, false>(c, diag, n, p, q, x, ldx, y, ldy, sink, st);
    int e = 0;
    select_variant<3>(fpe, early_exit, [&](auto N, auto EE) {
        e = bdot_launch<N(), EE(), false>(c, diag, n, p, q, x, ldx, y, ldy, sink, st);
    });
    return e;
}

// fpe == 1: plain fp64; fpe < 3: superaccumulators only, as ExDOT; early exit with fpe > 8: nothing is launched and the
// outputs keep their values, ExGEMV's (and the reference's) silent return
hipError_t exbdot_dispatch(Ctx &c, char mode, long long n, int p, int q, const double *x, long long ldx, const double *y,
                           long long ldy, double *out, long long ldc, int fpe, int early_exit, int round_mode,
                           hipStream_t st)
{
    BdotSink sink;
    sink.out = out;
    sink.ldc = ldc;
    sink.round_mode = round_mode;
    return (hipError_t)bdot_variant<true>(c, mode, n, p, q, x, ldx, y, ldy, sink, fpe, early_exit, st);
}

// The row-sharded forms: fpe == 1 (no digit sets) and early exit with fpe > 8 (no variant) are the caller's to refuse.
// d_sets: the [outputs][SET_WORDS] sets of the whole result in output order.
int exbdot_export_dispatch(Ctx &c, char mode, long long n, int p, int q, const double *x, long long ldx, const double *y,
                           long long ldy, long long *d_sets, int fpe, int early_exit, hipStream_t st)
{
    BdotSink sink;
    sink.sets_out = d_sets;
    return bdot_variant<false>(c, mode, n, p, q, x, ldx, y, ldy, sink, fpe, early_exit, st);
}

// per batch: export in place, merge->allreduce over the batch's outputs * SET_WORDS words, round.  The calls of
// merge->allreduce depend on (mode, p, q) only.
int exbdot_merge_dispatch(Ctx &c, char mode, long long n, int p, int q, const double *x, long long ldx, const double *y,
                          long long ldy, double *out, long long ldc, int fpe, int early_exit, int round_mode,
                          const BdotMerge *merge, hipStream_t st)
{
    BdotSink sink;
    sink.out = out;
    sink.ldc = ldc;
    sink.round_mode = round_mode;
    sink.merge = merge;
    return bdot_variant<false>(c, mode, n, p, q, x, ldx, y, ldy, sink, fpe, early_exit, st);
}

// d_sets: [nsets][outputs][SET_WORDS], read only; no workspace, one launch over the whole result
hipError_t exbdot_round_dispatch(char mode, int p, int q, const long long *d_sets, int nsets, double *out, long long ldc,
                                 int round_mode, hipStream_t st)
{
    BdotGeom g = {};
    g.diag = mode == 'D' || mode == 'd';
    g.ni = p;
    g.nj = g.diag ? 1 : q;
    const long long nout = (long long)g.ni * g.nj;
    if (nout == 0) return hipSuccess;
    if (nout > (long long)0x7fffffff * BD_WAVES) return hipErrorInvalidValue;   // (beyond any memory: a grid of 2^31 workgroups)
    hipLaunchKernelGGL((k_bdot_finalize<false, false>), dim3((unsigned)((nout + BD_WAVES - 1) / BD_WAVES)), dim3(BD_BLOCK), 0,
                       st, g, d_sets, nout * SET_WORDS, nsets, out, ldc, round_mode);
    return hipGetLastError();
}

}  // namespace exb
