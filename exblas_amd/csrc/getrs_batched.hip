// getrs_batched.hip -- batched ExGETRS for gfx950: the apply of a block-Jacobi preconditioner with general blocks.  X (n x k,
// row-major, row stride ldx) is solved in place; block b covers the rows b p .. min(n, (b + 1) p) - 1, its factors are the
// p x p matrix at lu + b * stride (column- or row-major by `order`) and its pivots the p words at ipiv + b * p, as the batched
// ExGETRF leaves them (a last block of rows < p rows uses the leading rows x rows part and the first `rows` pivots).
//   interchanges  for j = 0 .. rows - 1 in order: rows j and ipiv[j] - 1 of the block are swapped; an index outside 1 .. rows
//                 is skipped and never used as an address
//   forward       y_i = Round( b_i - sum_{c<i} l_ic y_c ), unit diagonal, no division
//   backward      z_i = fl( Round( y_i - sum_{c>i} u_ic z_c ) / u_ii )
// Every sum is exact over the already fixed doubles (every stored entry counts: zero times Inf is NaN) and rounded once:
// ExTRSV's row step, so column j of block b is what exblas_extrsv_dev ('L', 'N', 'U') and then ('U', 'N', 'N') write on the
// permuted column.  The info words of the factorisation are not consulted.
//
// Structure: the frame of block_common.hip.h, on the pattern of potrs_batched.hip.  What is this routine's own:
//   * Lanes own (block, column) pairs: with the column tile kc = min(k, 64) rounded up to a power of two (4 on path 3) a wave
//     carries NB = 64 / kc CONSECUTIVE blocks (1 on path 2), fewer where the wave's share of LDS does not hold them (then kc
//     shrinks too).  A column is independent of every other: no shuffle and no barrier in the substitution.
//   * The wave stages its NB whole LU blocks row-wise (row pitch p | 1), their pivots and its panel of X in its own LDS, does
//     the interchanges there (each lane on its own column), walks the forward and the backward sweep in place, a row at a
//     time, and stores the panel once.  Both sweeps read row i of the staged block: the part left of the diagonal, then the
//     part right of it.
//   * Certify in registers, or settle one output at a time through the wave's accumulator (blk_resolve).
//   * k > kc runs in column tiles; a wave item is (block group, column tile), a workgroup item four of them.
//   * fpe == 1: s = b_i, then s -= a * x over c ascending, in fp64.
#include <atomic>

#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int GS_U = 4;   // solved rows per step of the inner loop
constexpr size_t GS_LDS = 152 * 1024;   // dynamic LDS of a workgroup (160 KiB less the accumulators and counters)

struct GsArgs {
    long long n, ldx, stride, nblocks, ngroups, ntiles, nitems, per;   // nitems workgroup items, `per` to a workgroup
    int p, k, ldlu, rowmajor, lgkc, NB, tsz, force, round_mode;
};

// the geometry of a staged block: LU(i, c) at T[i * pitch + c]; x(r, col) at X[r * kc + col]
struct GsBlock {
    const double *T;
    double *X;
    int pitch, kc, rows;
};

// Round(x_i - sum a x) of row i, column col of a block through the wave's accumulator.  UP: the backward sweep (the solved
// rows lie below i).  x(i, col) still holds the right-hand side.  Wave-uniform; every lane gets the value.
template <bool UP>
__device__ double gs_resolve(const GsBlock &B, int i, int col, int round_mode, long long *acc)
{
    const int n = UP ? B.rows - 1 - i : i;
    const double v = blk_resolve(
        acc, n, round_mode,
        [&](int t, double &a, double &b) {
            const int c = UP ? i + 1 + t : t;
            a = B.T[i * B.pitch + c];
            b = -B.X[c * B.kc + col];
        },
        [&](RowSink &sink) { sink.add(B.X[i * B.kc + col]); });
    sp_wave_sync();
    return v;
}

// one sweep over the wave's blocks: lane (gi, col) walks the rows of its column; `act`: the lane owns a column
template <bool PLAIN, bool UP>
__device__ __forceinline__ void gs_sweep(const GsArgs &A, const double *lus, double *xs, int msz, int xbs, bool act, int rows,
                                         int maxrows, long long *acc, unsigned long long &n_reg, unsigned long long &n_fb)
{
    const int lane = threadIdx.x & 63, kc = 1 << A.lgkc, gi = lane >> A.lgkc, col = lane & (kc - 1), pitch = A.p | 1;
    const double *T = lus + gi * msz;
    double *X = xs + gi * xbs;
    for (int s = 0; s < maxrows; ++s) {   // wave-uniform
        // row i of a block of `rows` rows: ascending, or descending from its own last row
        const int i = UP ? rows - 1 - s : s;
        const bool on = act && s < rows;
        double f[SP_N], ps = on ? X[i * kc + col] : 0.0;
        unsigned flags = 0;
#pragma unroll
        for (int t4 = 0; t4 < SP_N; ++t4) f[t4] = 0.0;
        const int c0 = UP ? i + 1 : 0, c1 = UP ? rows : i;   // the solved rows
        const int steps = s;   // s products for every lane that is on (wave-uniform bound)
        for (int k0 = 0; k0 < steps; k0 += GS_U) {
            double pr[GS_U], er[GS_U];
#pragma unroll
            for (int u = 0; u < GS_U; ++u) {
                const int c = c0 + k0 + u;
                const bool ok = on && c < c1;
                const double tv = ok ? T[i * pitch + c] : 0.0, x = ok ? X[c * kc + col] : 0.0;
                if constexpr (PLAIN) {
                    ps -= tv * x;
                    pr[u] = er[u] = 0.0;
                } else {
                    pr[u] = two_prod(tv, -x, er[u]);
                }
            }
            if constexpr (!PLAIN) {
                SpLaneSink sink{flags};
                fpe_absorb_prod<SP_N, true, GS_U>(f, pr, er, sink);
            }
        }
        double v = ps;
        if constexpr (!PLAIN) {
            double pr[1] = {ps}, er[1] = {0.0};   // the right-hand side joins the lane's sum
            SpLaneSink sink{flags};
            fpe_absorb_prod<SP_N, true, 1>(f, pr, er, sink);
            bool fb = false;
            v = 0.0;
            if (on) {
                double rr;
                if (!A.force && flags == 0 && spmv_round_fast<SP_N>(f, rr)) v = rr;
                else fb = true;
            }
            const unsigned long long om = __ballot(on);
            unsigned long long fbm = __ballot(fb);
            n_reg += __popcll(om & ~fbm);
            n_fb += __popcll(fbm);
            while (fbm) {   // wave-uniform
                const int l = __builtin_ctzll(fbm);
                fbm &= fbm - 1ull;
                const int lg = l >> A.lgkc;
                // the rows of lane l's block: every lane of its group knows them
                const int lrows = __shfl(rows, l, 64), li = UP ? lrows - 1 - s : s;
                const GsBlock B{lus + lg * msz, xs + lg * xbs, pitch, kc, lrows};
                const double tt = gs_resolve<UP>(B, li, l & (kc - 1), A.round_mode, acc);
                if (lane == l) v = tt;
            }
        }
        if (on) X[i * kc + col] = UP ? v / T[i * pitch + i] : v;   // the unit diagonal of L divides nothing
        sp_wave_sync();   // the row is in the panel before gs_resolve reads it
    }
}

template <bool PLAIN>
__global__ void __launch_bounds__(SP_BLOCK)
    k_getrs_batched(GsArgs A, const double *__restrict__ lu, const int *__restrict__ ipiv, double *x, long long *slots)
{
    extern __shared__ double gs_lds[];   // SP_WAVES x tsz: [NB blocks of LU] [NB panels of X] [NB x p pivots]
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = A.p, pitch = p | 1, msz = (p * pitch) | 1;
    const int kc = 1 << A.lgkc, xbs = pitch * kc, gi = lane >> A.lgkc, col = lane & (kc - 1);
    double *lus = gs_lds + (size_t)w * A.tsz, *xs = lus + A.NB * msz;
    int *pvs = (int *)(xs + A.NB * xbs);
    if constexpr (!PLAIN) {
        for (int k = lane; k < NL; k += 64) acc[w][k] = 0;
    }
    unsigned long long n_reg = 0, n_fb = 0;
    const long long t1 = min(((long long)blockIdx.x + 1) * A.per, A.nitems);
    for (long long t = (long long)blockIdx.x * A.per; t < t1; ++t) {   // workgroup-uniform
        const long long it = t * SP_WAVES + w;   // the wave item: (block group, column tile)
        if (it >= A.ngroups * A.ntiles) continue;   // wave-uniform
        const long long grp = it / A.ntiles, b0 = grp * A.NB;
        const int ct = (int)(it - grp * A.ntiles), col0 = ct * kc, kw = min(kc, A.k - col0);
        const int nbl = (int)min((long long)A.NB, A.nblocks - b0);            // blocks of the wave
        const long long row0 = b0 * p;
        const int nrows = (int)min((long long)nbl * p, A.n - row0);          // rows of its panel
        // ---- stage: the blocks along their unit stride, their pivots, the panel along the rows of X ----
        const int pp = p * p;
        for (int e = lane; e < nbl * pp; e += 64) {
            const int gg = e / pp, q = e - gg * pp, hi = q / p, lo = q - hi * p;
            const int r = A.rowmajor ? hi : lo, c = A.rowmajor ? lo : hi;
            const int rows = (int)min((long long)p, A.n - (b0 + gg) * p);
            if (r < rows && c < rows) lus[gg * msz + r * pitch + c] = lu[(b0 + gg) * A.stride + (long long)hi * A.ldlu + lo];
        }
        for (int e = lane; e < nrows; e += 64) pvs[e] = ipiv[row0 + e];   // block gg, pivot j at gg * p + j
        for (int e = lane; e < nrows * kw; e += 64) {
            const int rr = e / kw, cc = e - rr * kw, gg = rr / p, ri = rr - gg * p;
            xs[gg * xbs + ri * kc + cc] = x[(row0 + rr) * A.ldx + col0 + cc];
        }
        sp_wave_sync();
        const bool act = gi < nbl && col < kw;
        const int rows = gi < nbl ? (int)min((long long)p, A.n - (b0 + gi) * p) : 0;
        const int maxrows = min(p, nrows);   // of the wave's first block: the longest
        // ---- the interchanges, in order, each lane on its own column; an index out of range moves nothing ----
        if (act) {
            double *X = xs + gi * xbs;
            for (int j = 0; j < rows; ++j) {
                const int pv = pvs[gi * p + j] - 1;
                if (pv >= 0 && pv < rows && pv != j) {
                    const double tj = X[j * kc + col], tp = X[pv * kc + col];
                    X[j * kc + col] = tp, X[pv * kc + col] = tj;
                }
            }
        }
        sp_wave_sync();
        gs_sweep<PLAIN, false>(A, lus, xs, msz, xbs, act, rows, maxrows, acc[w], n_reg, n_fb);
        gs_sweep<PLAIN, true>(A, lus, xs, msz, xbs, act, rows, maxrows, acc[w], n_reg, n_fb);
        for (int e = lane; e < nrows * kw; e += 64) {
            const int rr = e / kw, cc = e - rr * kw, gg = rr / p, ri = rr - gg * p;
            x[(row0 + rr) * A.ldx + col0 + cc] = xs[gg * xbs + ri * kc + cc];
        }
        sp_wave_sync();   // the panel is out before the next item's comes in
    }
    blk_store_counters(cnt, n_reg, n_fb, slots, blockIdx.x);
}

// more than 64 KiB of dynamic LDS has to be asked for, once per device and instantiation (no stream operation)
hipError_t gs_lds_optin(int device)
{
    static std::atomic<unsigned long long> done{0};
    const unsigned long long bit = 1ull << (device & 63);
    if (done.load() & bit) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void *)k_getrs_batched<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GS_LDS);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_getrs_batched<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GS_LDS);
    if (e == hipSuccess) done.fetch_or(bit);
    return e;
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain substitution, 2..8 the expansions (the caller refused the
// rest, p > 64 and the bad flags)
hipError_t exgetrs_batched_dispatch(Ctx &c, char order, int p, long long n, int k, const double *lu, int ldlu, long long stride,
                                    const int *ipiv, double *x, long long ldx, int fpe, int early_exit, int round_mode,
                                    hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.getrs_batched_slots = SlotInfo();
    if (n == 0 || k == 0) return hipSuccess;
    const int path = c.getrs_batched_path;
    GsArgs A;
    A.p = p, A.k = k, A.ldlu = ldlu, A.n = n, A.ldx = ldx, A.stride = stride;
    A.rowmajor = (order == 'R' || order == 'r') ? 1 : 0;
    A.nblocks = (n + p - 1) / p;
    A.lgkc = 0;
    while ((1 << A.lgkc) < min(k, path == 3 ? 4 : 64)) ++A.lgkc;
    A.NB = path == 2 ? 1 : 64 >> A.lgkc;
    const int pitch = p | 1, msz = (p * pitch) | 1, pvd = (p + 1) / 2;   // pvd: doubles that hold a block's p pivots
    // the wave's share of LDS: fewer blocks first, then a narrower column tile
    auto per_wave = [&]() { return (size_t)A.NB * (msz + pitch * (1 << A.lgkc) + pvd); };
    while ((size_t)SP_WAVES * per_wave() * sizeof(double) > GS_LDS) {
        if (A.NB > 1) A.NB >>= 1;
        else --A.lgkc;
    }
    A.tsz = (int)per_wave();
    const StRule rule = st_rule(fpe, path, round_mode);
    A.force = rule.force_fb, A.round_mode = rule.round_mode;
    A.ngroups = (A.nblocks + A.NB - 1) / A.NB;
    A.ntiles = (k + (1 << A.lgkc) - 1) >> A.lgkc;
    const long long witems = A.ngroups * A.ntiles;
    A.nitems = (witems + SP_WAVES - 1) / SP_WAVES;
    const BlkPartition P = blk_partition(c, A.nitems);
    A.per = P.per;
    hipError_t e = gs_lds_optin(c.device);
    if (e != hipSuccess) return e;
    long long *slots = blk_reserve_slots(c, c.getrs_batched_slots, P.grid, st, &e);
    if (!slots) return e;
    const size_t lds = (size_t)SP_WAVES * A.tsz * sizeof(double);
    if (fpe == 1) hipLaunchKernelGGL((k_getrs_batched<true>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, lu, ipiv, x, slots);
    else hipLaunchKernelGGL((k_getrs_batched<false>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, lu, ipiv, x, slots);
    return hipGetLastError();
}

}  // namespace exb
