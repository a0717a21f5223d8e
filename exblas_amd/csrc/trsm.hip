// trsm.hip -- ExTRSM for gfx950: exact, reproducible dense triangular solve with the column-major triangle of ExTRSV
// (uplo, transa, diag, lda) and a dense row-major block X of k right-hand sides (leading dimension ldx), solved in place.
//
// Contract: column j of X is, bit for bit, what ExTRSV (trsv.hip) gives for (uplo, transa, diag, A, B[:, j]):
//   x_ij = fl( Round( b_ij - sum_{c before i} op(A)(i,c) * x_cj ) / op(A)(i,i) )
// in substitution order, the sum exact over the already fixed doubles (every entry of the strict triangle counts: a zero
// times an infinite x_cj is NaN) and rounded once; the other triangle, the lda padding and the diagonal under 'U' are
// never read.  Every path sums ExTRSV's multiset of TwoProd pairs exactly, so the bits depend on the data and (uplo,
// transa, diag, rounding mode) only.
//
// Structure: per column panel (kp <= panel columns, one after the other in stream order) the preset kernel of the sparse
// solves (ticket zero, mailbox empty; the first one also clears the counters and the watchdog flag) and ONE solve kernel.
//   * LANES OWN COLUMNS.  A work item is TR_R consecutive rows in substitution order (4; 1 on path 2) times one tile of
//     G <= 64 columns; persistent waves take items from one atomic ticket that enumerates row groups major, column tiles
//     minor.  Lane g keeps one 4-term expansion per row of the item -- the register block: a solved row x_c fetched from
//     the mailbox (mailbox[c * kp + tile * G + g], one contiguous read across the lanes) is multiplied into all rows of
//     the item before the next one is fetched.  For kp < 64, G is kp rounded up to a power of two and the 64 / G lane
//     groups ("slices") share the columns of op(A) round-robin; the slices of a column of X are merged exactly by the
//     shuffle cascade of the sparse routines.
//   * op(A) is read in tiles of TR_R rows x 64 columns through the wave's LDS, along whichever stride is 1.  transa 'T'
//     (a row of op(A) is contiguous): one load per row, 64 consecutive doubles.  transa 'N' (a column of op(A) is
//     contiguous): the item's TR_R rows of a column are one run of 32 bytes, a load takes 16 columns, every fetched
//     sector is used whole and no lane walks a stride of its own.  The tile is read back as a broadcast: the lanes of a
//     slice read the same word.
//   * The chain.  Row group t cannot finish before row group t - 1 has: what lies between the two is kept short.  The
//     columns of op(A) before the last TR_R ones are taken by the slices and merged first; the last TR_R columns -- the
//     rows of the previous item, posted last -- go to the leader lanes alone in one fetch, and b is absorbed before
//     them.  The rows of the item then follow one after the other: certify, divide, post, and the
//     products with the item's later rows from its TR_R x TR_R diagonal block in LDS.
//   * The mailbox is n x kp doubles, indexed by substitution position, with the conventions of sptrs_common.hip.h as
//     they are: the reserved NaN pattern, st_post, st_fetch with its 2 s watchdog, st_take_ticket, st_preset, the header.
//   * Rounding.  Lane g certifies its own output with spmv_round_fast.  What it cannot certify (ties, near-ties inside
//     the margin, spills, non-finite flags, results out of its range, the reference rounding mode, fpe = 0, path 1) cannot
//     wait for a later kernel, because later rows wait for the value: the wave resolves every such column on the spot, in
//     a wave-uniform loop over the failing columns -- all 64 lanes stride the row of op(A) for that column through the
//     same staged tiles, every value they need is posted (or in LDS) by then, the products go into the wave's ONE
//     integer accumulator in LDS, finish_wave rounds, then the division and the post follow.
//
// Progress.  A wave only ever WAITS (polls the mailbox) for a value owned by a lower ticket: (row i, tile c) depends on
// (earlier rows, tile c), which lie in earlier row groups -- lower tickets, since row groups are major -- or in i's own
// item, where they are found in LDS, written before row i started.  Lower tickets are held by waves that have taken them,
// i.e. that are resident and run (or have finished), so the wave with the lowest unfinished ticket never waits for
// anything that is not posted, and by induction every wave finishes: no workgroup barrier across items, no need for the
// grid to be co-resident, no input can deadlock.  The fallback loop asks for nothing the first pass did not.
//
// Watchdog: that of the sparse solves (2 s on one poll, the header flag, everything behind it drains as NaN).
// fpe == 1 runs the same structure with plain fp64 sums in a fixed order (deterministic, not exact).
// sptrs_common.hip.h holds what is shared with sptrsm.hip (the tile widths, the host loop st_block_solve).  The
// lane geometry, the publication of a solved value and the certify / fall-back block are the same text in both files:
// a fix to one goes into the other (sptrs_common.hip.h says why they are not one helper).
#include "../../include/exblas_hip.h"
#include "sptrs_common.hip.h"

namespace exb {
namespace {

constexpr int TR_R = 4;            // rows per item: four 4-term expansions per lane
constexpr int TR_U = 4;            // columns of op(A) per slice and step (mailbox loads in flight per lane)
constexpr int TR_CH = 64;          // columns of op(A) in a staged tile
constexpr int TR_PITCH = 72;       // doubles per staged row: the 'N' fill (4 rows x 16 columns per store) meets no bank twice
static_assert(TR_R == 4, "tr_stage's 'N' fill is written for 4 rows x 16 columns per load");
static_assert(TR_U >= TR_R, "one step takes the previous item's rows");

struct TrArgs {
    int n, kp, lg, tiles, rev, unit, force_fb, round_mode, R;
    long long rs, cs, ldx, limit;   // op(A)(i, c) = a[phys(i) * rs + phys(c) * cs]: one of rs, cs is 1, the other lda
};

// the wave's LDS
struct TrLds {
    long long *acc;   // NL limbs: the one integer accumulator
    double *xs;       // TR_R x 64: b of the item's rows, then their solved values
    double *sa;       // TR_R x TR_PITCH: a tile of op(A)
    double *dg;       // TR_R x TR_R: the item's diagonal block (strict triangle, and the diagonal under 'N')
};

__device__ __forceinline__ long long tr_phys(const TrArgs &A, long long k) { return A.rev ? (long long)A.n - 1 - k : k; }

// sa[r * TR_PITCH + cc] := op(A)(pos0 + r, c0 + cc) for r < nrows, cc < nc, zero elsewhere; c0 + nc <= pos0, so only the
// strict triangle is touched.  Ends with the wave's LDS hand-over.
__device__ __forceinline__ void tr_stage(const TrArgs &A, const double *__restrict__ a, long long pos0, int nrows,
                                         long long c0, int nc, double *sa)
{
    const int lane = threadIdx.x & 63;
    if (A.cs == 1) {   // a row of op(A) is contiguous: 64 consecutive columns of one row per load
        const long long pc = tr_phys(A, c0 + lane);
#pragma unroll
        for (int r = 0; r < TR_R; ++r) {
            double v = 0.0;
            if (r < nrows && lane < nc) v = a[tr_phys(A, pos0 + r) * A.rs + pc];
            sa[r * TR_PITCH + lane] = v;
        }
    } else {           // a column of op(A) is contiguous (rs == 1): the item's TR_R rows of 16 columns per load
        const int r = lane & (TR_R - 1), q = lane >> 2;
        const long long pr = tr_phys(A, pos0 + r);
#pragma unroll
        for (int h = 0; h < TR_CH / 16; ++h) {
            const int cc = h * 16 + q;
            double v = 0.0;
            if (r < nrows && cc < nc) v = a[pr + tr_phys(A, c0 + cc) * A.cs];
            sa[r * TR_PITCH + cc] = v;
        }
    }
    sp_wave_sync();
}

// What no lane could certify: output (row r of the item, column jj of the panel; l its place in the tile) through the
// wave's integer accumulator.  Every x it needs is posted (the first pass waited for it) or in LDS.  Wave-uniform.
__device__ void tr_resolve(const TrArgs &A, const double *__restrict__ a, long long pos0, int nrows, int r, long long jj,
                           int l, double d, double *x, long long *hdr, double *xq, const TrLds &L)
{
    const int lane = threadIdx.x & 63;
    unsigned fl = 0;
    RowSink asink{L.acc, fl};
    for (long long c0 = 0; c0 < pos0; c0 += TR_CH) {
        const int nc = (int)min((long long)TR_CH, pos0 - c0);
        tr_stage(A, a, pos0, nrows, c0, nc, L.sa);
        double xv[1];
        const bool want[1] = {lane < nc};
        const long long at[1] = {want[0] ? (c0 + lane) * (long long)A.kp + jj : 0};
        st_fetch<1>(xq, at, want, xv, hdr, A.limit);
        if (want[0]) {
            double e;
            const double p = two_prod(L.sa[r * TR_PITCH + lane], -xv[0], e);
            sink_product(asink, p, e);
        }
        sp_wave_sync();   // the tile is read before the next one replaces it
    }
    if (lane < r) {       // the item's earlier rows
        double e;
        const double p = two_prod(L.dg[r * TR_R + lane], -L.xs[lane * 64 + l], e);
        sink_product(asink, p, e);
    }
    if (lane == 0) lds_add<1>(L.acc, L.xs[r * 64 + l], fl);   // b: the row's slot holds it until the row is solved
    sp_wave_sync();
    double v = sp_acc_round(L.acc, NonFiniteLanes(fl).of(~0ull), A.round_mode);
    if (!A.unit) v = v / d;
    if (lane == 0) {
        st_post(xq + (pos0 + r) * (long long)A.kp + jj, v);
        x[tr_phys(A, pos0 + r) * A.ldx + jj] = v;
        L.xs[r * 64 + l] = v;
    }
    sp_wave_sync();
}

// the item of rows pos0 .. (substitution positions) and columns tile * G .. of the panel
template <bool PLAIN>
__device__ __forceinline__ void tr_item(const TrArgs &A, long long pos0, int tile, const double *__restrict__ a, double *x,
                                        long long *hdr, double *xq, const TrLds &L, StCounters &cn)
{
    const int lane = threadIdx.x & 63;
    const int G = 1 << A.lg, S = 64 >> A.lg;
    const int g = lane & (G - 1), s = lane >> A.lg;
    const long long j = (long long)tile * G + g;
    const bool active = j < A.kp, leader = active && s == 0;
    const int nrows = (int)min((long long)A.R, (long long)A.n - pos0);

    // b of the item's rows into the slots that take the solved rows later, and the diagonal block
    if (leader) {
#pragma unroll
        for (int r = 0; r < TR_R; ++r)
            if (r < nrows) L.xs[r * 64 + g] = x[tr_phys(A, pos0 + r) * A.ldx + j];
    }
    if (lane < TR_R * TR_R) {
        const int r = lane / TR_R, c = lane % TR_R;
        double v = 0.0;
        if (r < nrows && (c < r || (c == r && !A.unit))) v = a[tr_phys(A, pos0 + r) * A.rs + tr_phys(A, pos0 + c) * A.cs];
        L.dg[lane] = v;
    }
    sp_wave_sync();

    double f[TR_R][SP_N], ps[TR_R];
    unsigned flags[TR_R];
#pragma unroll
    for (int r = 0; r < TR_R; ++r) {
        ps[r] = 0.0;
        flags[r] = 0;
#pragma unroll
        for (int i = 0; i < SP_N; ++i) f[r][i] = 0.0;
    }

    // one step: the columns cc0, cc0 + stride, ... (TR_U of them) of the staged tile, for the lanes where `mine` holds,
    // against every row of the item
    auto step = [&](long long c0, int nc, int cc0, int stride, bool mine) {
        double xv[TR_U];
        long long at[TR_U];
        bool want[TR_U];
        int cc[TR_U];
#pragma unroll
        for (int u = 0; u < TR_U; ++u) {
            cc[u] = cc0 + u * stride;
            want[u] = mine && cc[u] < nc;
            at[u] = want[u] ? (c0 + cc[u]) * (long long)A.kp + j : 0;
        }
        st_fetch<TR_U>(xq, at, want, xv, hdr, A.limit);
#pragma unroll
        for (int r = 0; r < TR_R; ++r) {
            if (r < nrows) {   // wave-uniform
                double p[TR_U], er[TR_U];
#pragma unroll
                for (int u = 0; u < TR_U; ++u) {
                    const double av = want[u] ? L.sa[r * TR_PITCH + cc[u]] : 0.0;
                    if constexpr (PLAIN) {
                        if (want[u]) ps[r] -= av * xv[u];
                    } else {
                        p[u] = two_prod(av, -xv[u], er[u]);
                    }
                }
                if constexpr (!PLAIN) {
                    SpLaneSink sink{flags[r]};
                    fpe_absorb_prod<SP_N, true, TR_U>(f[r], p, er, sink);
                }
            }
        }
    };

    // ---- the columns before the previous item's rows: the slices share them ----
    const long long tail = min(pos0, (long long)TR_R), head = pos0 - tail;
    for (long long c0 = 0; c0 < head; c0 += TR_CH) {   // wave-uniform
        const int nc = (int)min((long long)TR_CH, head - c0);
        tr_stage(A, a, pos0, nrows, c0, nc, L.sa);
        for (int cc0 = 0; cc0 < nc; cc0 += S * TR_U) step(c0, nc, cc0 + s, S, active);
        sp_wave_sync();   // the tile is read before the next one replaces it
    }

    // ---- b_ij, then the slices of a column become one: all of it before the chain arrives ----
#pragma unroll
    for (int r = 0; r < TR_R; ++r) {
        if (r < nrows) {   // wave-uniform
            if constexpr (PLAIN) {
                if (leader) ps[r] += L.xs[r * 64 + g];
                for (int st = G; st < 64; st <<= 1) ps[r] += __shfl_down(ps[r], st, 64);
            } else {
                SpLaneSink sink{flags[r]};
                double bv[1] = {leader ? L.xs[r * 64 + g] : 0.0};
                sp_absorb_beta(f[r], leader, 1.0, bv, 0, sink);
                for (int st = G; st < 64; st <<= 1) sp_cascade_step(f[r], flags[r], st, (lane & (2 * st - 1)) < G, sink);
            }
        }
    }

    // ---- the previous item's rows, posted last: the leaders alone ----
    if (tail > 0) {
        tr_stage(A, a, pos0, nrows, head, (int)tail, L.sa);
        step(head, (int)tail, 0, 1, leader);
        sp_wave_sync();
    }

    // ---- the rows of the item, one after the other ----
#pragma unroll
    for (int r = 0; r < TR_R; ++r) {
        if (r < nrows) {   // wave-uniform
            const double d = A.unit ? 1.0 : L.dg[r * TR_R + r];
            const long long pos = pos0 + r;
            double *xp = x + tr_phys(A, pos) * A.ldx + j, *qp = xq + pos * (long long)A.kp + j;
            if constexpr (PLAIN) {
                if (leader) {
                    const double v = A.unit ? ps[r] : ps[r] / d;
                    st_post(qp, v);
                    *xp = v;
                    L.xs[r * 64 + g] = v;
                }
            } else {
                bool fb = false;
                if (leader) {
                    double rr;
                    if (!A.force_fb && flags[r] == 0 && spmv_round_fast<SP_N>(f[r], rr)) {
                        const double v = A.unit ? rr : rr / d;
                        st_post(qp, v);
                        *xp = v;
                        L.xs[r * 64 + g] = v;
                    } else {
                        fb = true;
                    }
                }
                unsigned long long fbm = __ballot(fb);
                const unsigned long long regm = __ballot(leader && !fb);
                if (lane == 0) {
                    cn.reg += __popcll(regm);
                    cn.fb += __popcll(fbm);
                }
                while (fbm) {   // wave-uniform
                    const int l = __builtin_ctzll(fbm);   // a leader lane: l < G is the column's place in the tile
                    fbm &= fbm - 1ull;
                    tr_resolve(A, a, pos0, nrows, r, (long long)tile * G + l, l, d, x, hdr, xq, L);
                }
            }
            // the row is in LDS before anything reads it
            sp_wave_sync();
            // ---- the later rows of the item take their product with it ----
#pragma unroll
            for (int r2 = r + 1; r2 < TR_R; ++r2) {
                if (r2 < nrows) {   // wave-uniform
                    const double av = leader ? L.dg[r2 * TR_R + r] : 0.0, v = leader ? L.xs[r * 64 + g] : 0.0;
                    if constexpr (PLAIN) {
                        if (leader) ps[r2] -= av * v;
                    } else {
                        double p[1], er[1];
                        p[0] = two_prod(av, -v, er[0]);
                        SpLaneSink sink{flags[r2]};
                        fpe_absorb_prod<SP_N, true, 1>(f[r2], p, er, sink);
                    }
                }
            }
        }
    }
    // the item's LDS is read before the next item replaces it
    sp_wave_sync();
}

template <bool PLAIN>
__global__ void __launch_bounds__(SP_BLOCK) k_trsm(TrArgs A, const double *__restrict__ a, double *x, long long *hdr,
                                                  double *xq)
{
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ double xs[SP_WAVES][TR_R * 64];
    __shared__ double sa[SP_WAVES][TR_R * TR_PITCH];
    __shared__ double dg[SP_WAVES][TR_R * TR_R];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if constexpr (!PLAIN) {
        for (int t = lane; t < NL; t += 64) acc[w][t] = 0;
        sp_wave_sync();
    }
    const TrLds L{acc[w], xs[w], sa[w], dg[w]};
    const long long nitems = (((long long)A.n + A.R - 1) / A.R) * A.tiles;
    StCounters cn;
    for (;;) {
        const long long t = st_take_ticket(hdr);
        if (t >= nitems) break;
        tr_item<PLAIN>(A, (t / A.tiles) * A.R, (int)(t % A.tiles), a, x, hdr, xq, L, cn);
    }
    st_flush_counters(cn, hdr);
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain solve, 2..8 the expansions (the caller refused the rest)
hipError_t extrsm_dispatch(Ctx &c, char uplo, char transa, char diag, int n, int k, const double *a, int lda, double *x,
                           long long ldx, int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    const bool lower = (uplo == 'L' || uplo == 'l'), trans = (transa == 'T' || transa == 't');
    // A**T of a lower matrix is upper: backward substitution
    const StOrient o{(lower != trans) ? 0 : 1, st_orient(uplo, diag).unit};
    auto launch = [&](const StPanel &P, int grid, long long *hdr, double *xq) {
        const TrArgs A{n, P.kp, P.lg, P.tiles, P.o.rev, P.o.unit, P.rule.force_fb, P.rule.round_mode, P.R,
                       trans ? (long long)lda : 1ll, trans ? 1ll : (long long)lda, ldx, P.limit};
        if (fpe == 1)
            hipLaunchKernelGGL((k_trsm<true>), dim3(grid), dim3(SP_BLOCK), 0, st, A, a, x + P.j0, hdr, xq);
        else
            hipLaunchKernelGGL((k_trsm<false>), dim3(grid), dim3(SP_BLOCK), 0, st, A, a, x + P.j0, hdr, xq);
        return hipGetLastError();
    };
    return st_block_solve(c, c.trsm_info_dev, n, k, TR_R, o, st_rule(fpe, c.trsm_path, round_mode),
                          EXBLAS_TRSM_MAILBOX_BYTES, st, launch);
}

}  // namespace exb
