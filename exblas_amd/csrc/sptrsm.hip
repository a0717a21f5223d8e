// sptrsm.hip -- ExSpTRSM for gfx950: exact, reproducible sparse triangular solve with A in CSR (int32 or int64 indices)
// and a dense row-major block X of k right-hand sides (leading dimension ldx), solved in place.
//
// Contract: column j of X is, bit for bit, what ExSpTRSV (sptrsv.hip) gives for (uplo, diag, A, B[:, j]):
//   x_ij = fl( Round( b_ij - sum_p val[p] * x[col[p], j] ) / d_i )     p: the stored entries of row i before the diagonal
// in substitution order, the sum exact over the already fixed doubles and rounded once, d_i the first stored diagonal
// entry; the other triangle, later diagonal entries and the diagonal under 'U' are skipped unread; a column outside
// [0, m) makes the whole row NaN.  Every path sums ExSpTRSV's multiset of doubles exactly, so the bits depend on the data
// and (uplo, diag, rounding mode) only.
//
// Structure: per column panel (kp <= panel columns, one after the other in stream order) a preset kernel (ticket zero,
// mailbox empty; the first one also clears the counters and the watchdog flag) and ONE solve kernel.
//   * LANES OWN COLUMNS.  A work item is R consecutive rows in substitution order (R = 8; 1 on path 2) times one tile of
//     G <= 64 columns; persistent waves take items from one atomic ticket that enumerates row groups major, column tiles
//     minor.  The wave walks the rows of its item one after the other.  For a stored dependency the column index and the
//     value are the same for every lane; lane g fetches mailbox[col * kp + tile * G + g] -- one contiguous read across the
//     lanes -- and keeps its own 4-term expansion, so for k >= 64 no cross-lane merge exists.  For kp < 64, G is kp
//     rounded up to a power of two and the 64 / G lane groups ("slices") share the row's entries round-robin; the slices
//     of a column are merged exactly by the shuffle cascade of sptrsv.hip.
//   * The mailbox is m x kp doubles, preset to the reserved NaN pattern (the value is its own ready flag): agent-scope
//     relaxed atomic stores and loads, a wave-uniform poll loop that sleeps lightly (sptrs_common.hip.h).  Rows solved
//     inside the item are also kept in the wave's LDS (R x 64 doubles): a dependency on a row of the own item is read
//     from there, not polled for.
//   * The rows of an item run one after the other, so what a row loads must not form a chain: the item's row_ptr
//     entries are loaded side by side, its indices and values (up to 256 entries) in one coalesced pass into LDS, b_ij
//     before anything else of its row.  What a row then waits for is the mailbox alone.
//   * Rounding.  Lane g certifies its own output with spmv_round_fast.  What it cannot certify (ties, near-ties inside the
//     margin, spills, non-finite flags, results out of its range, the reference rounding mode, fpe = 0, path 1) cannot
//     wait for a later kernel, because later rows wait for the value: the wave resolves every such column on the spot, in
//     a wave-uniform loop over the failing columns -- all 64 lanes stride the row's entries for that column, every value
//     they need is posted (or in LDS) by then, the products go into the wave's ONE integer accumulator in LDS,
//     finish_wave rounds, then the division and the post follow.
//
// Progress.  A wave only ever WAITS (polls the mailbox) for a value owned by a lower ticket: a dependency of (row i,
// tile c) is (an earlier row, tile c), which lies in an earlier row group -- a lower ticket, since row groups are major
// -- or in i's own item, where it is found in LDS, written before row i started.  Lower tickets are held by waves that
// have taken them, i.e. that are resident and run (or have finished), so the wave with the lowest unfinished ticket
// never waits for anything that is not posted, and by induction every wave finishes: no workgroup barrier, no need for
// the grid to be co-resident, no input can deadlock.  The fallback loop asks for nothing the first pass did not.
//
// Watchdog: that of sptrsv.hip (2 s on one poll, the header flag, everything behind it drains as NaN).
// fpe == 1 runs the same structure with plain fp64 sums in a fixed order (deterministic, not exact).
// sptrs_common.hip.h holds what is shared with trsm.hip (the tile widths, the host loop st_block_solve).  The
// lane geometry, the publication of a solved value and the certify / fall-back block are the same text in both files:
// a fix to one goes into the other (sptrs_common.hip.h says why they are not one helper).
#include "../../include/exblas_hip.h"
#include "sptrs_common.hip.h"

namespace exb {
namespace {

constexpr int TM_R = 8;            // rows per item
constexpr int TM_U = 4;            // stored entries per slice and step (mailbox loads in flight per lane)
constexpr int TM_STAGE = 256;      // entries of an item that are staged in LDS (a wave's: 4 KiB)

struct TmArgs {
    int m, kp, lg, tiles, rev, unit, force_fb, round_mode, count;   // count: this panel counts the structure
    long long ldx, limit;
};

// The stored entries of an item.  A row of a solve is a chain of dependent loads (row_ptr, then the indices, then the
// values and the solved values, then the divisor), and the rows of an item run one after the other: so the wave loads the
// item's row_ptr entries once, side by side, and, when the item's rows hold at most TM_STAGE entries between them, its
// indices and values in one coalesced pass into LDS.  What a row then waits for is the mailbox alone.
template <class I>
struct TmEntries {
    const I *__restrict__ ci;
    const double *__restrict__ val;
    const long long *sci;   // LDS: the item's column indices and values from entry `base` on, when staged
    const double *sval;
    long long base;
    bool staged;            // wave-uniform
    __device__ __forceinline__ long long col(long long k) const { return staged ? sci[k - base] : (long long)ld_nt(ci + k); }
    __device__ __forceinline__ double value(long long k) const { return staged ? sval[k - base] : ld_nt(val + k); }
};

// the row at substitution position pos0 + r of the item (rows pos0 ..), entries [p0, p1), x the columns tile * G .. of
// the panel
template <bool WIDE, bool PLAIN, class I>
__device__ __forceinline__ void tm_row(const TmArgs &A, bool count, long long pos0, int r, int tile, long long p0,
                                       long long p1, const TmEntries<I> &E, double *x, long long *hdr, double *xq,
                                       long long *acc, double *xs, StCounters &cn)
{
    const int lane = threadIdx.x & 63, m = A.m;
    const int G = WIDE ? 64 : 1 << A.lg, S = WIDE ? 1 : 64 >> A.lg;
    const int g = WIDE ? lane : lane & (G - 1), s = WIDE ? 0 : lane >> A.lg;
    const long long j = (long long)tile * G + g;
    const bool active = j < A.kp, leader = active && s == 0;
    const long long pos = pos0 + r, row = A.rev ? (long long)m - 1 - pos : pos;
    double *xp = x + row * A.ldx + j, *qp = xq + row * (long long)A.kp + j;
    double bv[1] = {0.0};
    if (leader) bv[0] = xs[r * 64 + g];   // b_ij: loaded with the item's other rows' when the item was taken
    // the slices that hold entries: slice t takes the entries t * TM_U .. of every ns * TM_U (a short row has one slice,
    // and nothing to merge)
    int ns = 1;
    while (ns < S && (long long)ns * TM_U < p1 - p0) ns <<= 1;
    unsigned flags = 0;
    long long kdiag = ST_NO_DIAG;
    SpLaneSink sink{flags};
    StCounters seen;   // the structure of the row as this lane met it
    double f[SP_N];
#pragma unroll
    for (int i = 0; i < SP_N; ++i) f[i] = 0.0;
    double ps = 0.0;   // PLAIN: the lane's running sum

    // ---- the row's entries ----
    for (long long q0 = p0; q0 < p1; q0 += (long long)ns * TM_U) {   // wave-uniform
        double a[TM_U], xv[TM_U];
        long long at[TM_U];
        bool want[TM_U];
        int loc[TM_U];
#pragma unroll
        for (int u = 0; u < TM_U; ++u) {
            const long long k = q0 + (long long)s * TM_U + u;
            a[u] = 0.0;
            at[u] = 0;
            want[u] = false;
            loc[u] = -1;
            if (s < ns && k < p1) {
                const long long c = E.col(k);
                int ds = 0;
                const int kind = st_classify(c, k, m, A.rev, row, pos, pos0, ds, kdiag, flags, seen);
                if (kind && active) {   // the value is looked at for dependencies only
                    a[u] = E.value(k);
                    if (kind == 1) {
                        want[u] = true;
                        at[u] = c * (long long)A.kp + j;
                    } else {
                        loc[u] = ds;
                    }
                }
            }
        }
        st_fetch<TM_U>(xq, at, want, xv, hdr, A.limit);
#pragma unroll
        for (int u = 0; u < TM_U; ++u)
            if (loc[u] >= 0) xv[u] = xs[loc[u] * 64 + g];   // a row of this item: solved before this one started
        if constexpr (PLAIN) {
#pragma unroll
            for (int u = 0; u < TM_U; ++u)
                if (want[u] || loc[u] >= 0) ps -= a[u] * xv[u];
        } else {
            double p[TM_U], er[TM_U];
#pragma unroll
            for (int u = 0; u < TM_U; ++u) p[u] = two_prod(a[u], -xv[u], er[u]);
            fpe_absorb_prod<SP_N, true, TM_U>(f, p, er, sink);
        }
    }

    // ---- b_ij, then the slices of a column become one ----
    if constexpr (PLAIN) {
        if (leader) ps += bv[0];
        if (flags & FLAG_NAN) ps = __builtin_nan("");
    } else {
        sp_absorb_beta(f, leader, 1.0, bv, 0, sink);
    }
    if constexpr (!WIDE) {
        for (int st = G; st < G * ns; st <<= 1) {   // wave-uniform
            const bool take = (lane & (2 * st - 1)) < G;
            kdiag = min(kdiag, (long long)__shfl_xor(kdiag, st, 64));
            if constexpr (PLAIN) {
                ps += __shfl_down(ps, st, 64);
            } else {
                sp_cascade_step(f, flags, st, take, sink);
            }
        }
        kdiag = lane_bcast(kdiag, 0);
    }

    // ---- the divisor: the first stored diagonal entry, in storage order; the structure counts once per call ----
    const bool has = kdiag != ST_NO_DIAG;
    double d = 1.0;
    if (!A.unit) d = has ? E.value(kdiag) : 0.0;
    if (count) {
        if (g == 0) cn.skipped += seen.skipped;
        if (lane == 0 && !A.unit) {
            cn.skipped -= has ? 1 : 0;   // (the divisor is not a skipped entry)
            cn.nodiag += has ? 0 : 1;
        }
    }

    if constexpr (PLAIN) {
        if (leader) {
            const double v = A.unit ? ps : ps / d;
            st_post(qp, v);
            *xp = v;
            xs[r * 64 + g] = v;
        }
    } else {
        bool fb = false;
        if (leader) {
            double rr;
            if (!A.force_fb && flags == 0 && spmv_round_fast<SP_N>(f, rr)) {
                const double v = A.unit ? rr : rr / d;
                st_post(qp, v);
                *xp = v;
                xs[r * 64 + g] = v;
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
        // ---- what no lane could certify: one column at a time through the wave's integer accumulator ----
        while (fbm) {   // wave-uniform
            const int l = __builtin_ctzll(fbm);   // a leader lane: l < G is the column's place in the tile
            fbm &= fbm - 1ull;
            const long long jj = (long long)tile * G + l;
            unsigned fl = 0;
            long long kd = ST_NO_DIAG;
            StCounters again;
            RowSink asink{acc, fl};
            for (long long k0 = p0; k0 < p1; k0 += 64) {
                const long long k = k0 + lane;
                double a[1] = {0.0}, xv[1];
                long long at[1] = {0};
                bool want[1] = {false};
                int loc = -1;
                if (k < p1) {
                    const long long c = E.col(k);
                    int ds = 0;
                    const int kind = st_classify(c, k, m, A.rev, row, pos, pos0, ds, kd, fl, again);
                    if (kind) a[0] = E.value(k);
                    if (kind == 1) {
                        want[0] = true;
                        at[0] = c * (long long)A.kp + jj;
                    } else if (kind == 2) {
                        loc = ds;
                    }
                }
                st_fetch<1>(xq, at, want, xv, hdr, A.limit);   // (posted: the first pass waited for it)
                if (loc >= 0) xv[0] = xs[loc * 64 + l];
                if (want[0] || loc >= 0) {
                    double e;
                    const double p = two_prod(a[0], -xv[0], e);
                    sink_product(asink, p, e);
                }
            }
            double *xj = x + row * A.ldx + jj;
            if (lane == 0) lds_add<1>(acc, xs[r * 64 + l], fl);   // b: the row's slot holds it until the row is solved
            sp_wave_sync();
            double v = sp_acc_round(acc, NonFiniteLanes(fl).of(~0ull), A.round_mode);
            if (!A.unit) v = v / d;
            if (lane == 0) {
                st_post(xq + row * (long long)A.kp + jj, v);
                *xj = v;
                xs[r * 64 + l] = v;
            }
            sp_wave_sync();
        }
    }
    // the row is in LDS before the next row of the item reads it
    sp_wave_sync();
}

template <bool WIDE, bool PLAIN, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_sptrsm(TmArgs A, int R, const I *__restrict__ rp, const I *__restrict__ ci,
                                                    const double *__restrict__ val, double *x, long long *hdr, double *xq)
{
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ double xs[SP_WAVES][TM_R * 64];
    __shared__ long long sci[SP_WAVES][TM_STAGE];
    __shared__ double sval[SP_WAVES][TM_STAGE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if constexpr (!PLAIN) {
        for (int t = lane; t < NL; t += 64) acc[w][t] = 0;
        sp_wave_sync();
    }
    const long long nitems = (((long long)A.m + R - 1) / R) * A.tiles;
    StCounters cn;
    for (;;) {
        const long long t = st_take_ticket(hdr);
        if (t >= nitems) break;
        const long long pos0 = (t / A.tiles) * R;
        const int tile = (int)(t % A.tiles);
        const int nrows = (int)min((long long)R, (long long)A.m - pos0);
        const bool count = A.count && tile == 0;   // the structure is counted by the first tile of the first panel
        // the item's rows are the physical rows low .. low + nrows - 1: lane i holds row_ptr[low + i], i <= nrows
        const long long low = A.rev ? (long long)A.m - pos0 - nrows : pos0;
        const long long bnd = lane <= nrows ? (long long)rp[low + lane] : 0;
        const long long P0 = lane_bcast(bnd, 0), P1 = lane_bcast(bnd, nrows);
        const long long nxt = __shfl_down(bnd, 1, 64);
        const bool fits = lane >= nrows || (bnd >= P0 && bnd <= nxt && nxt <= P1);   // (a row_ptr that is not monotone)
        TmEntries<I> E{ci, val, sci[w], sval[w], P0, P1 - P0 <= TM_STAGE && !__any(!fits)};
        if (E.staged) {
            for (long long e = lane; e < P1 - P0; e += 64) {
                sci[w][e] = (long long)ld_nt(ci + P0 + e);
                sval[w][e] = ld_nt(val + P0 + e);
            }
            sp_wave_sync();
        }
        // b of the item's rows, side by side, into the slots that take the solved rows later
        {
            const int G = WIDE ? 64 : 1 << A.lg;
            const long long j = (long long)tile * G + (lane & (G - 1));
            if (lane < G && j < A.kp) {
#pragma unroll
                for (int r = 0; r < TM_R; ++r) {
                    const long long row = A.rev ? (long long)A.m - 1 - (pos0 + r) : pos0 + r;
                    if (r < nrows) xs[w][r * 64 + (lane & (G - 1))] = x[row * A.ldx + j];
                }
            }
            sp_wave_sync();
        }
        for (int r = 0; r < nrows; ++r) {
            const int at = A.rev ? nrows - 1 - r : r;
            const long long p0 = lane_bcast(bnd, at);
            tm_row<WIDE, PLAIN>(A, count, pos0, r, tile, p0, max(p0, lane_bcast(bnd, at + 1)), E, x, hdr, xq, acc[w], xs[w], cn);
        }
    }
    st_flush_counters(cn, hdr);
}

}  // namespace

hipError_t exsptrsm_dispatch(Ctx &c, char uplo, char diag, int m, int k, int index_bits, const void *row_ptr,
                             const void *col_idx, const double *val, double *x, long long ldx, int fpe, int early_exit,
                             int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    auto launch = [&](const StPanel &P, int grid, long long *hdr, double *xq) {
        const TmArgs A{m, P.kp, P.lg, P.tiles, P.o.rev, P.o.unit, P.rule.force_fb, P.rule.round_mode, P.first, ldx, P.limit};
        return sp_dispatch(index_bits, fpe, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
            constexpr bool PLAIN = decltype(plain)::value;
            using I = std::remove_cv_t<std::remove_pointer_t<decltype(rp)>>;
            if (A.lg == 6)
                hipLaunchKernelGGL((k_sptrsm<true, PLAIN, I>), dim3(grid), dim3(SP_BLOCK), 0, st, A, P.R, rp, ci, val, x + P.j0,
                                   hdr, xq);
            else
                hipLaunchKernelGGL((k_sptrsm<false, PLAIN, I>), dim3(grid), dim3(SP_BLOCK), 0, st, A, P.R, rp, ci, val, x + P.j0,
                                   hdr, xq);
            return hipGetLastError();
        });
    };
    return st_block_solve(c, c.sptrsm_info_dev, m, k, TM_R, st_orient(uplo, diag), st_rule(fpe, c.sptrsm_path, round_mode),
                          EXBLAS_SPTRSM_MAILBOX_BYTES, st, launch);
}

}  // namespace exb
