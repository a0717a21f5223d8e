// bjacobi_apply.hip -- the apply of a block-Jacobi preconditioner for gfx950: the batched ExPOTRS (Cholesky factors) and the
// batched ExGETRS (pivoted LU factors), ONE kernel in four instances (plain / exact, Cholesky / LU).  X (n x k, row-major,
// row stride ldx) is solved in place; block b covers the rows b p .. min(n, (b + 1) p) - 1 and its factor is the p x p array
// at f + b * stride, as the batched ExPOTRF / ExGETRF leaves it (a last block of rows < p rows uses the leading rows x rows
// part).  Either way a block is two sweeps of ExTRSV's row step: every sum exact over the already fixed doubles (every
// stored entry counts: zero times Inf is NaN) and rounded once, then at most ONE IEEE division.  The info words of the
// factorisation are not consulted.
//
// Cholesky (batched ExPOTRS): the factor is a column-major triangle, G_b = F^T F (F = R for 'U', F = L^T for 'L').
//   sweep '1'  F^T Y = B, rows ascending:   y_i = fl( Round( b_i - sum_{c<i} F(c, i) y_c ) / F(i, i) )
//   sweep '2'  F Z = Y,  rows descending:   z_i = fl( Round( y_i - sum_{c>i} F(i, c) z_c ) / F(i, i) )
//   sweep 'B'  both, in one launch, bit for bit '1' followed by '2'.
//   Column j of block b is what exblas_extrsv_dev (and exblas_extrsm_dev) writes on the same data.
// LU (batched ExGETRS): the factor is the whole matrix, column- or row-major by `order`, with the block's pivots the p words
// at ipiv + b * p (a last block uses the first `rows` of them).
//   interchanges  for j = 0 .. rows - 1 in order: rows j and ipiv[j] - 1 of the block are swapped; an index outside 1 .. rows
//                 is skipped and never used as an address
//   forward       y_i = Round( b_i - sum_{c<i} l_ic y_c ), unit diagonal, no division
//   backward      z_i = fl( Round( y_i - sum_{c>i} u_ic z_c ) / u_ii )
//   Column j of block b is what exblas_extrsv_dev ('L', 'N', 'U') and then ('U', 'N', 'N') write on the permuted column.
//
// Structure: the frame of block_common.hip.h.  What is this file's own:
//   * Lanes own (block, column) pairs: with the column tile kc = min(k, 64) rounded up to a power of two (4 on path 3) a wave
//     carries NB = 64 / kc CONSECUTIVE blocks (1 on path 2), fewer where the wave's share of LDS does not hold them (then kc
//     shrinks too).  A column is independent of every other, so the substitution needs no shuffle and no barrier.
//   * The wave stages its NB factors along their unit stride (row pitch p | 1) and its panel of X (NB p consecutive rows,
//     coalesced) in its own LDS, walks the first sweep and then the second in place there, a row at a time, and stores the
//     panel once.  The staged image T holds F(c, i), c <= i, at T[c * pitch + i], or LU(i, c) at T[i * pitch + c]: the second
//     sweep reads row i of T right of the diagonal in both.
//   * Certify in registers, or settle one output at a time through the wave's accumulator (blk_resolve reads the factor
//     and the solved values from LDS), over the ballot across all lanes.
//   * k > kc runs in column tiles; a wave item is (block group, column tile), a workgroup item four of them.
//   * fpe == 1: s = b_i, then s -= F * x over c ascending, in fp64.
// LU alone (under `if constexpr (LU)`, or picked by LU in an expression): the whole block is staged, not the triangle; the
// first sweep walks ROW i of T and does not divide; the pivots are staged beside the panel (their doubles count in the
// wave's share of LDS) and the interchanges are done there, each lane on its own column.  Cholesky alone: the `sweeps` mask.
#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int BA_U = 4;   // solved rows per step of the inner loop
constexpr size_t BA_LDS = 152 * 1024;   // dynamic LDS of a workgroup (160 KiB less the accumulators and counters)

struct BaArgs {
    long long n, ldx, stride, nblocks, ngroups, ntiles, nitems, per;   // nitems workgroup items, `per` to a workgroup
    // hirow: the slow index of a stored factor is the row of its staged image ('L' of a triangle, 'R' of an LU block);
    // sweeps (Cholesky): bit 0 sweep 1, bit 1 sweep 2
    int p, k, ldf, hirow, lgkc, NB, sweeps, tsz, force, round_mode;
};

// the geometry of a staged block: the factor at T (row pitch `pitch`, see above); x(r, col) at X[r * kc + col]
struct BaBlock {
    const double *T;
    double *X;
    int pitch, kc, rows;
};

// Round(x_i - sum t x) of row i, column col of a block through the wave's accumulator.  UP: the second sweep (the solved
// rows lie past i).  x(i, col) still holds the right-hand side.  Wave-uniform; every lane gets the value.
template <bool UP, bool LU>
__device__ double ba_resolve(const BaBlock &B, int i, int col, int round_mode, long long *acc)
{
    const int n = UP ? B.rows - 1 - i : i;
    const double v = blk_resolve(
        acc, n, round_mode,
        [&](int t, double &a, double &b) {
            const int c = UP ? i + 1 + t : t;
            a = (UP || LU) ? B.T[i * B.pitch + c] : B.T[c * B.pitch + i];
            b = -B.X[c * B.kc + col];
        },
        [&](RowSink &sink) { sink.add(B.X[i * B.kc + col]); });
    sp_wave_sync();
    return v;
}

// one sweep over the wave's blocks: lane (gi, col) walks the rows of its column; `act`: the lane owns a column
template <bool PLAIN, bool UP, bool LU>
__device__ __forceinline__ void ba_sweep(const BaArgs &A, const double *fs, double *xs, int msz, int xbs, bool act, int rows,
                                         int maxrows, long long *acc, unsigned long long &n_reg, unsigned long long &n_fb)
{
    const int lane = threadIdx.x & 63, kc = 1 << A.lgkc, gi = lane >> A.lgkc, col = lane & (kc - 1), pitch = A.p | 1;
    const double *T = fs + gi * msz;
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
        for (int k0 = 0; k0 < steps; k0 += BA_U) {
            double pr[BA_U], er[BA_U];
#pragma unroll
            for (int u = 0; u < BA_U; ++u) {
                const int c = c0 + k0 + u;
                const bool ok = on && c < c1;
                const double tv = ok ? ((UP || LU) ? T[i * pitch + c] : T[c * pitch + i]) : 0.0, x = ok ? X[c * kc + col] : 0.0;
                if constexpr (PLAIN) {
                    ps -= tv * x;
                    pr[u] = er[u] = 0.0;
                } else {
                    pr[u] = two_prod(tv, -x, er[u]);
                }
            }
            if constexpr (!PLAIN) {
                SpLaneSink sink{flags};
                fpe_absorb_prod<SP_N, true, BA_U>(f, pr, er, sink);
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
                const BaBlock B{fs + lg * msz, xs + lg * xbs, pitch, kc, lrows};
                const double tt = ba_resolve<UP, LU>(B, li, l & (kc - 1), A.round_mode, acc);
                if (lane == l) v = tt;
            }
        }
        if (on) X[i * kc + col] = (UP || !LU) ? v / T[i * pitch + i] : v;   // the unit diagonal of L divides nothing
        sp_wave_sync();   // the row is in the panel before ba_resolve reads it
    }
}

template <bool PLAIN, bool LU>
__global__ void __launch_bounds__(SP_BLOCK)
    k_bjacobi_apply(BaArgs A, const double *__restrict__ fac, const int *__restrict__ ipiv, double *x, long long *slots)
{
    extern __shared__ double ba_lds[];   // SP_WAVES x tsz: [NB factors] [NB panels of X] [LU: NB x p pivots]
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = A.p, pitch = p | 1, msz = (p * pitch) | 1;
    const int kc = 1 << A.lgkc, xbs = pitch * kc, gi = lane >> A.lgkc, col = lane & (kc - 1);
    double *fs = ba_lds + (size_t)w * A.tsz, *xs = fs + A.NB * msz;
    int *pvs = (int *)(xs + A.NB * xbs);   // LU
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
        // ---- stage: the factors along their unit stride, (LU) their pivots, the panel along the rows of X ----
        const int pp = p * p;
        for (int e = lane; e < nbl * pp; e += 64) {
            const int gg = e / pp, q = e - gg * pp, hi = q / p, lo = q - hi * p;
            const int r = A.hirow ? hi : lo, c = A.hirow ? lo : hi;   // T[r * pitch + c]
            const int rows = (int)min((long long)p, A.n - (b0 + gg) * p);
            if (LU ? (r < rows && c < rows) : (r <= c && c < rows))
                fs[gg * msz + r * pitch + c] = fac[(b0 + gg) * A.stride + (long long)hi * A.ldf + lo];
        }
        if constexpr (LU) {
            for (int e = lane; e < nrows; e += 64) pvs[e] = ipiv[row0 + e];   // block gg, pivot j at gg * p + j
        }
        for (int e = lane; e < nrows * kw; e += 64) {
            const int rr = e / kw, cc = e - rr * kw, gg = rr / p, ri = rr - gg * p;
            xs[gg * xbs + ri * kc + cc] = x[(row0 + rr) * A.ldx + col0 + cc];
        }
        sp_wave_sync();
        const bool act = gi < nbl && col < kw;
        const int rows = gi < nbl ? (int)min((long long)p, A.n - (b0 + gi) * p) : 0;
        const int maxrows = min(p, nrows);   // of the wave's first block: the longest
        if constexpr (LU) {
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
        }
        if (LU || (A.sweeps & 1)) ba_sweep<PLAIN, false, LU>(A, fs, xs, msz, xbs, act, rows, maxrows, acc[w], n_reg, n_fb);
        if (LU || (A.sweeps & 2)) ba_sweep<PLAIN, true, LU>(A, fs, xs, msz, xbs, act, rows, maxrows, acc[w], n_reg, n_fb);
        for (int e = lane; e < nrows * kw; e += 64) {
            const int rr = e / kw, cc = e - rr * kw, gg = rr / p, ri = rr - gg * p;
            x[(row0 + rr) * A.ldx + col0 + cc] = xs[gg * xbs + ri * kc + cc];
        }
        sp_wave_sync();   // the panel is out before the next item's comes in
    }
    blk_store_counters(cnt, n_reg, n_fb, slots, blockIdx.x);
}

// The plan and the launch of both routines.  lu: ExGETRS (ipiv is read), else ExPOTRS (ipiv is null, `sweeps` counts).
// `info`: the caller's counter slots, already emptied.
hipError_t ba_launch(Ctx &c, SlotInfo &info, int path, bool lu, bool hirow, int sweeps, int p, long long n, int k,
                     const double *fac, int ldf, long long stride, const int *ipiv, double *x, long long ldx, int fpe,
                     int round_mode, hipStream_t st)
{
    BaArgs A;
    A.p = p, A.k = k, A.ldf = ldf, A.n = n, A.ldx = ldx, A.stride = stride, A.hirow = hirow ? 1 : 0, A.sweeps = sweeps;
    A.nblocks = (n + p - 1) / p;
    A.lgkc = 0;
    while ((1 << A.lgkc) < min(k, path == 3 ? 4 : 64)) ++A.lgkc;
    A.NB = path == 2 ? 1 : 64 >> A.lgkc;
    const int pitch = p | 1, msz = (p * pitch) | 1, pvd = lu ? (p + 1) / 2 : 0;   // pvd: doubles that hold a block's p pivots
    // the wave's share of LDS: fewer blocks first, then a narrower column tile
    auto per_wave = [&]() { return (size_t)A.NB * (msz + pitch * (1 << A.lgkc) + pvd); };
    while ((size_t)SP_WAVES * per_wave() * sizeof(double) > BA_LDS) {
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
    static std::atomic<unsigned long long> optin{0};
    hipError_t e = blk_lds_optin(optin, c.device, BA_LDS,
                                 {(const void *)k_bjacobi_apply<true, false>, (const void *)k_bjacobi_apply<false, false>,
                                  (const void *)k_bjacobi_apply<true, true>, (const void *)k_bjacobi_apply<false, true>});
    if (e != hipSuccess) return e;
    long long *slots = blk_reserve_slots(c, info, P.grid, st, &e);
    if (!slots) return e;
    const size_t lds = (size_t)SP_WAVES * A.tsz * sizeof(double);
    const dim3 grid(P.grid), block(SP_BLOCK);
    if (lu && fpe == 1) hipLaunchKernelGGL((k_bjacobi_apply<true, true>), grid, block, lds, st, A, fac, ipiv, x, slots);
    else if (lu) hipLaunchKernelGGL((k_bjacobi_apply<false, true>), grid, block, lds, st, A, fac, ipiv, x, slots);
    else if (fpe == 1) hipLaunchKernelGGL((k_bjacobi_apply<true, false>), grid, block, lds, st, A, fac, ipiv, x, slots);
    else hipLaunchKernelGGL((k_bjacobi_apply<false, false>), grid, block, lds, st, A, fac, ipiv, x, slots);
    return hipGetLastError();
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain substitution, 2..8 the expansions (the caller refused the
// rest, p > 64 and the bad flags)
hipError_t expotrs_batched_dispatch(Ctx &c, char uplo, char sweep, int p, long long n, int k, const double *r, int ldr,
                                    long long stride, double *x, long long ldx, int fpe, int early_exit, int round_mode,
                                    hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.potrs_batched_slots = SlotInfo();
    if (n == 0 || k == 0) return hipSuccess;
    return ba_launch(c, c.potrs_batched_slots, c.potrs_batched_path, false, uplo == 'L' || uplo == 'l',
                     sweep == '1' ? 1 : sweep == '2' ? 2 : 3, p, n, k, r, ldr, stride, nullptr, x, ldx, fpe, round_mode, st);
}

hipError_t exgetrs_batched_dispatch(Ctx &c, char order, int p, long long n, int k, const double *lu, int ldlu, long long stride,
                                    const int *ipiv, double *x, long long ldx, int fpe, int early_exit, int round_mode,
                                    hipStream_t st)
{
    (void)early_exit;   // as above
    c.getrs_batched_slots = SlotInfo();
    if (n == 0 || k == 0) return hipSuccess;
    return ba_launch(c, c.getrs_batched_slots, c.getrs_batched_path, true, order == 'R' || order == 'r', 3, p, n, k, lu, ldlu,
                     stride, ipiv, x, ldx, fpe, round_mode, st);
}

}  // namespace exb
