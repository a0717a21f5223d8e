// potrs_batched.hip -- batched ExPOTRS for gfx950: the apply of a block-Jacobi preconditioner.  X (n x k, row-major, row
// stride ldx) is solved in place; block b covers the rows b p .. min(n, (b + 1) p) - 1 and its factor is the p x p
// column-major triangle at r + b * stride, as the batched ExPOTRF leaves it (a last block of pl < p rows uses the leading
// pl x pl part).  With G_b = F^T F (F = R for 'U', F = L^T for 'L'):
//   sweep '1'  F^T Y = B, rows ascending:   y_i = fl( Round( b_i - sum_{c<i} F(c, i) y_c ) / F(i, i) )
//   sweep '2'  F Z = Y,  rows descending:   z_i = fl( Round( y_i - sum_{c>i} F(i, c) z_c ) / F(i, i) )
//   sweep 'B'  both, in one launch, bit for bit '1' followed by '2'.
// Every sum is exact over the already fixed doubles (every stored entry of the strict triangle counts: zero times Inf is
// NaN) and rounded once, then ONE IEEE division: ExTRSV's row step, so column j of block b is what exblas_extrsv_dev (and
// exblas_extrsm_dev) writes on the same data.  The info word of the factorisation is not consulted.
//
// Structure: the frame of block_common.hip.h.  What is this routine's own:
//   * Lanes own (block, column) pairs: with the column tile kc = min(k, 64) rounded up to a power of two (4 on path 3) a wave
//     carries NB = 64 / kc CONSECUTIVE blocks (1 on path 2), fewer where the wave's share of LDS does not hold them (then kc
//     shrinks too).  A column is independent of every other, so the substitution needs no shuffle and no barrier.
//   * The wave stages its NB triangles along their unit stride (row pitch p | 1) and its panel of X (NB p consecutive rows,
//     coalesced) in its own LDS, walks sweep 1 and then sweep 2 in place there, a row at a time, and stores the panel once.
//   * Certify in registers, or settle one output at a time through the wave's accumulator (blk_resolve reads the factor
//     and the solved values from LDS), over the ballot across all lanes.
//   * k > kc runs in column tiles; a wave item is (block group, column tile), a workgroup item four of them.
//   * fpe == 1: s = b_i, then s -= F * x over c ascending, in fp64.
#include <atomic>

#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int PS_U = 4;   // solved rows per step of the inner loop
constexpr size_t PS_LDS = 152 * 1024;   // dynamic LDS of a workgroup (160 KiB less the accumulators and counters)

struct PsArgs {
    long long n, ldx, stride, nblocks, ngroups, ntiles, nitems, per;   // nitems workgroup items, `per` to a workgroup
    int p, k, ldr, lower, lgkc, NB, sweeps, tsz, force, round_mode;    // sweeps: bit 0 sweep 1, bit 1 sweep 2
};

// the geometry of a staged block: F(c, i), c <= i, at T[c * pitch + i]; x(r, col) at X[r * kc + col]
struct PsBlock {
    const double *T;
    double *X;
    int pitch, kc, rows;
};

// Round(x_i - sum F x) of row i, column col of a block through the wave's accumulator.  UP: sweep 2 (the solved rows lie
// above i).  x(i, col) still holds the right-hand side.  Wave-uniform; every lane gets the value.
template <bool UP>
__device__ double ps_resolve(const PsBlock &B, int i, int col, int round_mode, long long *acc)
{
    const int n = UP ? B.rows - 1 - i : i;
    const double v = blk_resolve(
        acc, n, round_mode,
        [&](int t, double &a, double &b) {
            const int c = UP ? i + 1 + t : t;
            a = UP ? B.T[i * B.pitch + c] : B.T[c * B.pitch + i];
            b = -B.X[c * B.kc + col];
        },
        [&](RowSink &sink) { sink.add(B.X[i * B.kc + col]); });
    sp_wave_sync();
    return v;
}

// one sweep over the wave's blocks: lane (gi, col) walks the rows of its column; `act`: the lane owns a column
template <bool PLAIN, bool UP>
__device__ __forceinline__ void ps_sweep(const PsArgs &A, const double *tri, double *xs, int msz, int xbs, bool act, int rows,
                                         int maxrows, long long *acc, unsigned long long &n_reg, unsigned long long &n_fb)
{
    const int lane = threadIdx.x & 63, kc = 1 << A.lgkc, gi = lane >> A.lgkc, col = lane & (kc - 1), pitch = A.p | 1;
    const double *T = tri + gi * msz;
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
        for (int k0 = 0; k0 < steps; k0 += PS_U) {
            double pr[PS_U], er[PS_U];
#pragma unroll
            for (int u = 0; u < PS_U; ++u) {
                const int c = c0 + k0 + u;
                const bool ok = on && c < c1;
                const double tv = ok ? (UP ? T[i * pitch + c] : T[c * pitch + i]) : 0.0, x = ok ? X[c * kc + col] : 0.0;
                if constexpr (PLAIN) {
                    ps -= tv * x;
                    pr[u] = er[u] = 0.0;
                } else {
                    pr[u] = two_prod(tv, -x, er[u]);
                }
            }
            if constexpr (!PLAIN) {
                SpLaneSink sink{flags};
                fpe_absorb_prod<SP_N, true, PS_U>(f, pr, er, sink);
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
                const PsBlock B{tri + lg * msz, xs + lg * xbs, pitch, kc, lrows};
                const double tt = ps_resolve<UP>(B, li, l & (kc - 1), A.round_mode, acc);
                if (lane == l) v = tt;
            }
        }
        if (on) X[i * kc + col] = v / T[i * pitch + i];
        sp_wave_sync();   // the row is in the panel before ps_resolve reads it
    }
}

template <bool PLAIN>
__global__ void __launch_bounds__(SP_BLOCK) k_potrs_batched(PsArgs A, const double *__restrict__ r, double *x, long long *slots)
{
    extern __shared__ double ps_lds[];   // SP_WAVES x tsz: [NB triangles] [NB panels of X]
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = A.p, pitch = p | 1, msz = (p * pitch) | 1;
    const int kc = 1 << A.lgkc, xbs = pitch * kc, gi = lane >> A.lgkc, col = lane & (kc - 1);
    double *tri = ps_lds + (size_t)w * A.tsz, *xs = tri + A.NB * msz;
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
        // ---- stage: the triangles along their unit stride, the panel along the rows of X ----
        const int pp = p * p;
        for (int e = lane; e < nbl * pp; e += 64) {
            const int gg = e / pp, q = e - gg * pp, a = q / p, b = q - a * p;
            const int c = A.lower ? a : b, i = A.lower ? b : a;   // F(c, i), c <= i
            const int rows = (int)min((long long)p, A.n - (b0 + gg) * p);
            if (c <= i && i < rows) tri[gg * msz + c * pitch + i] = r[(b0 + gg) * A.stride + (long long)a * A.ldr + b];
        }
        for (int e = lane; e < nrows * kw; e += 64) {
            const int rr = e / kw, cc = e - rr * kw, gg = rr / p, ri = rr - gg * p;
            xs[gg * xbs + ri * kc + cc] = x[(row0 + rr) * A.ldx + col0 + cc];
        }
        sp_wave_sync();
        const bool act = gi < nbl && col < kw;
        const int rows = gi < nbl ? (int)min((long long)p, A.n - (b0 + gi) * p) : 0;
        const int maxrows = min(p, nrows);   // of the wave's first block: the longest
        if (A.sweeps & 1) ps_sweep<PLAIN, false>(A, tri, xs, msz, xbs, act, rows, maxrows, acc[w], n_reg, n_fb);
        if (A.sweeps & 2) ps_sweep<PLAIN, true>(A, tri, xs, msz, xbs, act, rows, maxrows, acc[w], n_reg, n_fb);
        for (int e = lane; e < nrows * kw; e += 64) {
            const int rr = e / kw, cc = e - rr * kw, gg = rr / p, ri = rr - gg * p;
            x[(row0 + rr) * A.ldx + col0 + cc] = xs[gg * xbs + ri * kc + cc];
        }
        sp_wave_sync();   // the panel is out before the next item's comes in
    }
    blk_store_counters(cnt, n_reg, n_fb, slots, blockIdx.x);
}

// more than 64 KiB of dynamic LDS has to be asked for, once per device and instantiation (no stream operation)
hipError_t ps_lds_optin(int device)
{
    static std::atomic<unsigned long long> done{0};
    const unsigned long long bit = 1ull << (device & 63);
    if (done.load() & bit) return hipSuccess;
    hipError_t e = hipFuncSetAttribute((const void *)k_potrs_batched<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PS_LDS);
    if (e == hipSuccess)
        e = hipFuncSetAttribute((const void *)k_potrs_batched<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)PS_LDS);
    if (e == hipSuccess) done.fetch_or(bit);
    return e;
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
    const int path = c.potrs_batched_path;
    PsArgs A;
    A.p = p, A.k = k, A.ldr = ldr, A.n = n, A.ldx = ldx, A.stride = stride;
    A.lower = (uplo == 'L' || uplo == 'l') ? 1 : 0;
    A.sweeps = sweep == '1' ? 1 : sweep == '2' ? 2 : 3;
    A.nblocks = (n + p - 1) / p;
    A.lgkc = 0;
    while ((1 << A.lgkc) < min(k, path == 3 ? 4 : 64)) ++A.lgkc;
    A.NB = path == 2 ? 1 : 64 >> A.lgkc;
    const int pitch = p | 1, msz = (p * pitch) | 1;
    // the wave's share of LDS: fewer blocks first, then a narrower column tile
    auto need = [&]() { return (size_t)SP_WAVES * A.NB * (msz + pitch * (1 << A.lgkc)) * sizeof(double); };
    while (need() > PS_LDS) {
        if (A.NB > 1) A.NB >>= 1;
        else --A.lgkc;
    }
    A.tsz = A.NB * (msz + pitch * (1 << A.lgkc));
    const StRule rule = st_rule(fpe, path, round_mode);
    A.force = rule.force_fb, A.round_mode = rule.round_mode;
    A.ngroups = (A.nblocks + A.NB - 1) / A.NB;
    A.ntiles = (k + (1 << A.lgkc) - 1) >> A.lgkc;
    const long long witems = A.ngroups * A.ntiles;
    A.nitems = (witems + SP_WAVES - 1) / SP_WAVES;
    const BlkPartition P = blk_partition(c, A.nitems);
    A.per = P.per;
    hipError_t e = ps_lds_optin(c.device);
    if (e != hipSuccess) return e;
    long long *slots = blk_reserve_slots(c, c.potrs_batched_slots, P.grid, st, &e);
    if (!slots) return e;
    const size_t lds = (size_t)SP_WAVES * A.tsz * sizeof(double);
    if (fpe == 1) hipLaunchKernelGGL((k_potrs_batched<true>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, r, x, slots);
    else hipLaunchKernelGGL((k_potrs_batched<false>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, r, x, slots);
    return hipGetLastError();
}

}  // namespace exb
