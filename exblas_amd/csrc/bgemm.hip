// bgemm.hip -- ExBGEMM for gfx950: exact, reproducible block update Y = alpha X C + beta Y with row-major blocks: X tall
// (n x p, ldx), C small (p x q, ldc), Y tall (n x q, ldy), updated in place.  The design range is p, q <= 64.
//
// Contract: every output is, bit for bit, what ExSpMM (spmm.hip) writes for the CSR matrix that stores X densely
// (row_ptr[r] = r p, col_idx = 0 .. p-1, values = the row of X) against C as its dense block:
//   Y[r, j] = Round( sum_{i<p} X[r, i] * fl(alpha * C[i, j])  (+)  beta * Y[r, j] )
// Every path below sums ExSpMM's multiset of TwoProd pairs (every entry of X counts: a zero times an infinite C is NaN;
// the beta terms under ExGEMV's rules) exactly and rounds it once, so the bits depend on the data and the rounding mode
// only.
//
// Structure: the frame of block_common.hip.h (one kernel, certify in registers or settle through the wave's accumulator,
// a counter slot per workgroup, the plain kernel of fpe == 1); what is this routine's own:
//   * LANES OWN COLUMNS.  G is the tile width (q rounded up to a power of two, at most 64; 4 on path 3), a wave holds
//     S = 64 / G row slices, and each lane keeps BG_R (4; 1 on path 2) 4-term expansions: the register block.  A wave's
//     item is S * R consecutive rows times one tile; slice s owns the rows r * S + s of it, so that for every r the wave
//     stores S consecutive rows of Y.  One C[i, j] read from LDS serves the R rows of the block, one X[r, i] serves the G
//     lanes of its slice.
//   * fl(alpha * C) is staged into LDS once per workgroup and (tile, chunk): a chunk is at most 64 rows of C (4 on path
//     3) times G columns, at most 32 KiB.  A workgroup takes a contiguous range of items, tile major, so for p <= 64 the
//     chunk is staged once per tile, and with one tile once per workgroup; a larger p stages per item.
//   * The wave's rows of X go through the wave's LDS in steps of xc columns (S * R * xc <= 512 doubles, xc >= 4), read
//     with coalesced loads along the unit stride.  The pitch of a staged row is xc + 1 doubles, odd: the S slices'
//     broadcast reads of one column meet 32 different banks per half wave (ds_read_b64 takes the bank from the address in
//     units of 4 bytes modulo 64).
//   * Rounding.  The beta term goes into the lane's expansion (sp_absorb_beta) before the certificate.  The fall-back
//     (bg_resolve) strides the p products of the output straight from memory, lane 0 adds the beta term.  Y[r, j] is the
//     caller's value until its one store.
// The plain sums of fpe == 1 run in the order of i.
// Rows are independent and nothing crosses lanes: a row-sharded caller with C replicated needs no communication.
#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int BG_R = 4;          // rows per lane: four 4-term expansions
constexpr int BG_U = 4;          // entries of a row of X per step of the inner loop
constexpr int BG_CH = 64;        // rows of C in a staged chunk ...
constexpr int BG_TILE = 64;      // ... and columns of a tile
constexpr int BG_SMALL = 4;      // both on path 3
constexpr int BG_XS = 512;       // doubles of X a wave stages per step (more when S * R * 4 exceeds it)

struct BgArgs {
    long long n, ldx, ldc, ldy, nrb, nitems, per;   // nrb: row blocks (of SP_WAVES * S * R rows); per: items per workgroup
    int p, q, lg, R, ch, lgxc, force, round_mode;
    double alpha, beta;
};

// What no lane could certify: output (row, col) through the wave's integer accumulator, every operand from memory.
// Wave-uniform.
__device__ void bg_resolve(const BgArgs &A, const double *__restrict__ x, const double *__restrict__ c, double *y,
                           long long row, long long col, long long *acc)
{
    const double *xr = x + row * A.ldx, *cj = c + col;
    double *yp = y + row * A.ldy + col;
    const double v = blk_resolve(
        acc, A.p, A.round_mode, [&](int i, double &a, double &b) { a = xr[i], b = A.alpha * cj[(long long)i * A.ldc]; },
        [&](RowSink &sink) {
            if (A.beta != 0.0) blk_sink_term(sink, A.beta, *yp);
        });
    if ((threadIdx.x & 63) == 0) *yp = v;
    sp_wave_sync();
}

template <bool PLAIN>
__global__ void __launch_bounds__(SP_BLOCK) k_bgemm(BgArgs A, const double *__restrict__ x, const double *__restrict__ c,
                                                   double *y, long long *slots)
{
    extern __shared__ double bg_lds[];   // [ch x G: the chunk of fl(alpha * C)] [SP_WAVES x (S R) x (xc + 1): rows of X]
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int G = 1 << A.lg, S = 64 >> A.lg, g = lane & (G - 1), s = lane >> A.lg;
    const int RW = S * A.R, xc = 1 << A.lgxc, pitch = xc + 1;
    double *cs = bg_lds, *xs = bg_lds + A.ch * G + w * RW * pitch;
    if constexpr (!PLAIN) {
        for (int t = lane; t < NL; t += 64) acc[w][t] = 0;
        sp_wave_sync();
    }
    const int nchunks = (A.p + A.ch - 1) / A.ch;
    long long staged = -1;
    unsigned long long n_reg = 0, n_fb = 0;
    const long long it0 = (long long)blockIdx.x * A.per, it1 = min(A.nitems, it0 + A.per);
    for (long long it = it0; it < it1; ++it) {   // workgroup-uniform
        const long long tile = it / A.nrb, rb = it % A.nrb;
        const long long row0 = (rb * SP_WAVES + w) * RW;   // the wave's first row: beyond n the wave only keeps the barriers
        const long long j = tile * G + g;
        const bool colok = j < A.q;

        double f[BG_R][SP_N], ps[BG_R];
        unsigned flags[BG_R];
#pragma unroll
        for (int r = 0; r < BG_R; ++r) {
            ps[r] = 0.0;
            flags[r] = 0;
#pragma unroll
            for (int i = 0; i < SP_N; ++i) f[r][i] = 0.0;
        }

        if (!A.force) {   // forced: bg_resolve does all the work
            for (int c0 = 0; c0 < A.p; c0 += A.ch) {
                const int ncc = min(A.ch, A.p - c0);
                const long long id = tile * nchunks + c0 / A.ch;
                if (id != staged) {
                    __syncthreads();   // every wave has read the chunk that goes
                    for (int t = threadIdx.x; t < ncc * G; t += SP_BLOCK) {
                        const int i = t >> A.lg;
                        const long long jj = tile * G + (t & (G - 1));
                        cs[t] = jj < A.q ? A.alpha * c[(long long)(c0 + i) * A.ldc + jj] : 0.0;
                    }
                    __syncthreads();
                    staged = id;
                }
                for (int x0 = 0; x0 < ncc; x0 += xc) {
                    const int nc = min(xc, ncc - x0);
                    // the wave's RW rows, columns c0 + x0 .. of X; zero beyond n and beyond the chunk
                    for (int t = lane; t < RW * xc; t += 64) {
                        const int lr = t >> A.lgxc, cc = t & (xc - 1);
                        const long long row = row0 + lr;
                        double v = 0.0;
                        if (row < A.n && cc < nc) v = x[row * A.ldx + c0 + x0 + cc];
                        xs[lr * pitch + cc] = v;
                    }
                    sp_wave_sync();
                    for (int cc0 = 0; cc0 < nc; cc0 += BG_U) {
                        double cv[BG_U];
#pragma unroll
                        for (int u = 0; u < BG_U; ++u) cv[u] = cc0 + u < nc ? cs[(x0 + cc0 + u) * G + g] : 0.0;
#pragma unroll
                        for (int r = 0; r < BG_R; ++r) {
                            if (r < A.R) {   // wave-uniform
                                const double *xr = xs + (r * S + s) * pitch + cc0;   // (zero where cc0 + u >= nc)
                                if constexpr (PLAIN) {
#pragma unroll
                                    for (int u = 0; u < BG_U; ++u)
                                        if (cc0 + u < nc) ps[r] += xr[u] * cv[u];
                                } else {
                                    double pr[BG_U], er[BG_U];
#pragma unroll
                                    for (int u = 0; u < BG_U; ++u) pr[u] = two_prod(xr[u], cv[u], er[u]);
                                    SpLaneSink sink{flags[r]};
                                    fpe_absorb_prod<SP_N, true, BG_U>(f[r], pr, er, sink);
                                }
                            }
                        }
                    }
                    sp_wave_sync();   // the rows are read before the next step replaces them
                }
            }
        }

#pragma unroll
        for (int r = 0; r < BG_R; ++r) {
            if (r < A.R) {   // wave-uniform
                const long long row = row0 + r * S + s;
                const bool ok = colok && row < A.n;
                double *yp = ok ? y + row * A.ldy + j : y;
                if constexpr (PLAIN) {
                    if (ok) *yp = (A.beta == 0.0) ? ps[r] : ps[r] + A.beta * *yp;
                } else {
                    SpLaneSink sink{flags[r]};
                    if (!A.force) sp_absorb_beta(f[r], ok, A.beta, yp, 0, sink);
                    bool fb = false;
                    if (ok) {
                        double rr;
                        if (!A.force && flags[r] == 0 && spmv_round_fast<SP_N>(f[r], rr)) *yp = rr;
                        else fb = true;
                    }
                    unsigned long long fbm = __ballot(fb);
                    n_reg += __popcll(__ballot(ok && !fb));
                    n_fb += __popcll(fbm);
                    while (fbm) {   // wave-uniform
                        const int l = __builtin_ctzll(fbm);
                        fbm &= fbm - 1ull;
                        bg_resolve(A, x, c, y, row0 + r * S + (l >> A.lg), tile * G + (l & (G - 1)), acc[w]);
                    }
                }
            }
        }
    }
    blk_store_counters(cnt, n_reg, n_fb, slots, blockIdx.x);
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain product, >= 2 the expansions.  The caller checked the
// arguments.
hipError_t exbgemm_dispatch(Ctx &c, long long n, int p, int q, double alpha, const double *x, long long ldx,
                            const double *cm, long long ldc, double beta, double *y, long long ldy, int fpe, int early_exit,
                            int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.bgemm_slots = SlotInfo();
    if (n == 0 || q == 0) return hipSuccess;
    const int path = c.bgemm_path;
    BgArgs A;
    A.n = n, A.ldx = ldx, A.ldc = ldc, A.ldy = ldy, A.p = p, A.q = q, A.alpha = alpha, A.beta = beta;
    A.lg = 0;
    while ((1 << A.lg) < min(q, path == 3 ? BG_SMALL : BG_TILE)) ++A.lg;
    const int G = 1 << A.lg, S = 64 >> A.lg;
    const long long tiles = ((long long)q + G - 1) >> A.lg;
    A.R = path == 2 ? 1 : BG_R;
    const int RW = S * A.R, chmax = path == 3 ? BG_SMALL : BG_CH;
    // xc: a power of two in [4, chmax], no more than BG_XS doubles a step and no wider than p needs
    int xc = BG_U;
    while (2 * xc <= chmax && 2 * xc * RW <= BG_XS && xc < p) xc *= 2;
    A.lgxc = 0;
    while ((1 << A.lgxc) < xc) ++A.lgxc;
    A.ch = min(chmax, max(1, (p + xc - 1) / xc) * xc);   // a multiple of xc
    const StRule rule = st_rule(fpe, path, round_mode);
    A.force = rule.force_fb, A.round_mode = rule.round_mode;
    A.nrb = (n + (long long)SP_WAVES * RW - 1) / ((long long)SP_WAVES * RW);
    A.nitems = A.nrb * tiles;
    const auto [grid, per] = blk_partition(c, A.nitems);
    A.per = per;
    hipError_t e = hipSuccess;
    long long *slots = blk_reserve_slots(c, c.bgemm_slots, grid, st, &e);
    if (!slots) return e;
    const size_t lds = ((size_t)A.ch * G + (size_t)SP_WAVES * RW * (xc + 1)) * sizeof(double);
    if (fpe == 1)
        hipLaunchKernelGGL((k_bgemm<true>), dim3(grid), dim3(SP_BLOCK), lds, st, A, x, cm, y, slots);
    else
        hipLaunchKernelGGL((k_bgemm<false>), dim3(grid), dim3(SP_BLOCK), lds, st, A, x, cm, y, slots);
    return hipGetLastError();
}

}  // namespace exb
