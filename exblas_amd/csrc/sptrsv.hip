// sptrsv.hip -- ExSpTRSV for gfx950: exact, reproducible sparse triangular solve with A in CSR (int32 or int64 indices).
//
// Contract: ExTRSV's, on the stored entries of a row.  In substitution order (rows 0 .. m-1 for 'L', m-1 .. 0 for 'U')
//   x_i = fl( Round( b_i - sum_p val[p] * x[col[p]] ) / d_i )          p: the stored entries of row i before the diagonal
// with the sum exact over the already fixed doubles x_j (TwoProd of every stored product, duplicates of a column each
// count) and rounded once; d_i is the first stored entry with col == i (+0.0 when there is none, not read under 'U').
// Entries of the other triangle, later diagonal duplicates and the diagonal under 'U' are skipped without their values
// being looked at; a column outside [0, m) makes x_i NaN.  Every path sums the same multiset of doubles exactly, so the
// bits depend on the data and (uplo, diag, rounding mode) only.
//
// Structure: the preset kernel (sptrs_common.hip.h: header zero, mailbox empty) and ONE solve kernel, no host
// synchronisation, no analysis phase.
//   * Work items are groups of R consecutive rows in substitution order (R = 8; R = 1 on path 2), handed out by an
//     atomic ticket that a wave takes when it is ready to work on the item (persistent waves, no workgroup barrier).
//   * Solved values travel through a mailbox of m doubles preset to a reserved NaN pattern (the value is its own ready
//     flag, as in trsv.hip): agent-scope relaxed atomic stores and loads, a wave-uniform poll loop that sleeps lightly.
//     The plain store to x is separate; x is only ever read (b_i) and written by the wave that owns the row.
//   * An item whose rows all hold at most 64 entries runs as a batch: 8 lanes per row, the k_spmv_rows<8> layout.  An
//     item with a longer row (and every item on path 2) runs its rows one after the other, 64 lanes striding the row.
//
// Progress.  A wave only ever WAITS (polls the mailbox) for a value owned by a lower ticket: a dependency of row i is a
// row before i in substitution order, which lies in an earlier item or in i's own item.  Lower tickets are held by
// waves that have already taken them, i.e. that are resident and run (or have finished), so the wave with the lowest
// unfinished ticket never waits on anything that is not posted, and by induction every wave finishes: no input can
// deadlock, whatever the grid.  Dependencies inside an item are never polled for in the batch form: the first pass
// consumes every entry whose column lies outside the item (polling), the entries inside it are kept in registers, and
// the wave then walks its rows in order -- merge row s, round, divide, post, let the later rows of the batch take their
// products with x_s -- so each row of a wave is finished before a later row of the same wave needs it.  The walk is
// skipped when a ballot shows no such entry.  In the row-by-row form a row is posted before the next one starts, so a
// dependency inside the item is found in the mailbox like any other.
//
// Per row (spmv.hip's row step): b_i and the negated TwoProd pairs enter 4-term lane expansions, the lanes of the row
// are merged exactly, the leader certifies the rounding with spmv_round_fast; ties, near-ties inside its margin, spills,
// non-finite flags, results outside its range, the reference rounding mode, fpe = 0 and path 1 go through the row's LDS
// accumulator and finish_wave.  Then one IEEE division, the post, the store.
//
// Watchdog.  A wave that has polled for one value for more than 2 s of wall_clock64() (or sees the flag raised by
// another wave) raises the header flag, takes the canonical NaN for what it waited for and goes on, so everything
// behind it drains as NaN and the host reports the call as failed.  No valid input reaches it.
// fpe == 1 runs the same structure with plain fp64 sums in a fixed order (deterministic, not exact).
// The workspace, the fpe / path / rounding-mode rule and the grid (st_workspace, st_rule, st_grid) are sptrs_common.hip.h's.
#include "sptrs_common.hip.h"

namespace exb {
namespace {

constexpr int ST_R = 8;                    // rows per item (batch form: 8 lanes each)

// the rows at substitution positions pos0 .. pos0 + nrows - 1 (nrows <= 64 / G), G lanes per row.  G == 8: every row
// holds at most 64 entries (8 per lane); G == 64: one row of any length.  acc: the wave's 8 row accumulators in LDS.
template <int G, bool PLAIN, class I>
__device__ __forceinline__ void st_rows(long long pos0, int nrows, int m, const I *__restrict__ rp, const I *__restrict__ ci,
                                        const double *__restrict__ val, double *x, int rev, int unit, int force_fb,
                                        int round_mode, long long limit, long long *hdr, double *xq, long long (*acc)[NL],
                                        StCounters &cn)
{
    constexpr int U = 2, PER = G == 8 ? 8 : 1;   // PER: entries a lane can hold back for the walk
    const int lane = threadIdx.x & 63, slot = lane / G, sub = lane % G;
    const bool valid = slot < nrows;
    const long long pos = pos0 + slot;
    const long long row = valid ? (rev ? (long long)m - 1 - pos : pos) : 0;
    long long p0 = 0, p1 = 0;
    if (valid) {
        p0 = (long long)rp[row];
        p1 = max(p0, (long long)rp[row + 1]);
    }
    unsigned flags = 0;
    long long kdiag = ST_NO_DIAG;
    RowSink sink{acc[slot], flags};
    double f[SP_N];
#pragma unroll
    for (int i = 0; i < SP_N; ++i) f[i] = 0.0;
    double ps = 0.0;             // PLAIN: the lane's running sum
    double da[PER];              // entries against rows of this batch, by position in the lane's list
    unsigned dsl = 0xffffffffu;  // ... and their slots, 4 bits each (15: none)
#pragma unroll
    for (int j = 0; j < PER; ++j) da[j] = 0.0;

    // ---- pass 1: every entry whose column lies outside the item ----
    auto step = [&](const long long (&k)[U], const int e0) __attribute__((always_inline)) {
        double a[U], xv[U];
        long long at[U];
        bool want[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            a[j] = 0.0;
            at[j] = 0;
            want[j] = false;
            if (k[j] < p1) {
                int ds = 0;
                at[j] = (long long)ld_nt(ci + k[j]);
                const int kind = st_classify(at[j], k[j], m, rev, row, pos, pos0, ds, kdiag, flags, cn);
                if (kind) a[j] = ld_nt(val + k[j]);   // the value is looked at for dependencies only
                want[j] = kind == 1;
                if constexpr (G == 8) {
                    if (kind == 2) {
                        da[e0 + j] = a[j];
                        dsl &= ~(15u << (4 * (e0 + j)));
                        dsl |= (unsigned)ds << (4 * (e0 + j));
                    }
                }
                if (kind != 1) a[j] = 0.0;
            }
        }
        st_fetch<U>(xq, at, want, xv, hdr, limit);
        if constexpr (PLAIN) {
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (want[j]) ps -= a[j] * xv[j];
        } else {
            double p[U], er[U];
#pragma unroll
            for (int j = 0; j < U; ++j) p[j] = two_prod(a[j], -xv[j], er[j]);
            fpe_absorb_prod<SP_N, true, U>(f, p, er, sink);
        }
    };
    if constexpr (G == 8) {
#pragma unroll
        for (int it = 0; it < PER / U; ++it) {
            long long k[U];
#pragma unroll
            for (int j = 0; j < U; ++j) k[j] = p0 + (long long)(it * U + j) * G + sub;
            if (__any(k[0] < p1)) step(k, it * U);   // wave-uniform
        }
    } else {
        for (long long k0 = p0; k0 < p1; k0 += (long long)G * U) {   // one row: p0, p1 are wave-uniform
            long long k[U];
#pragma unroll
            for (int j = 0; j < U; ++j) k[j] = k0 + sub + (long long)j * G;
            step(k, 0);
        }
    }

    // ---- the divisor: the first stored diagonal entry, in storage order ----
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) kdiag = min(kdiag, (long long)__shfl_xor(kdiag, o, 64));
    const bool leader = valid && sub == 0;
    double d = 1.0;
    if (leader && !unit) {
        const bool has = kdiag != ST_NO_DIAG;
        d = has ? val[kdiag] : 0.0;
        cn.skipped -= has ? 1 : 0;   // (two plain updates: a select between the counters' addresses would put them in scratch)
        cn.nodiag += has ? 0 : 1;
    }
    // ---- b_i ----
    if constexpr (PLAIN) {
        if (leader) ps += x[row];
        if (flags & FLAG_NAN) ps = __builtin_nan("");
    } else {
        sp_absorb_beta(f, leader, 1.0, x, row, sink);
    }

    bool walk = false;
    if constexpr (G == 8) walk = __any(dsl != 0xffffffffu);
    if (!walk) {
        // ---- no dependency inside the item: all rows at once (spmv.hip: k_spmv_rows) ----
        if constexpr (PLAIN) {
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) ps += __shfl_down(ps, o, G);
            if (leader) {
                const double v = unit ? ps : ps / d;
                st_post(xq + row, v);
                x[row] = v;
            }
        } else {
#pragma unroll
            for (int s = 1; s < G; s <<= 1) sp_cascade_step(f, flags, s, (sub & (2 * s - 1)) == 0, sink);
            bool fb = false;
            if (leader) {
                double r;
                fb = !sp_certify_or_spill(f, flags, force_fb, acc[slot], r);
                if (!fb) {
                    const double v = unit ? r : r / d;
                    st_post(xq + row, v);
                    x[row] = v;
                }
            }
            const unsigned long long regm = __ballot(leader && !fb);
            if (lane == 0) cn.reg += __popcll(regm);
            unsigned long long fbm = __ballot(fb);
            if (lane == 0) cn.fb += __popcll(fbm);
            if (fbm) {
                sp_wave_sync();
                while (fbm) {   // wave-uniform: every lane runs the finish of each falling-back row
                    const int l = __builtin_ctzll(fbm), sl = l / G;
                    fbm &= fbm - 1ull;
                    const unsigned fl = (unsigned)__shfl((int)flags, l, 64) & FLAG_NONFINITE;
                    const long long r_row = __shfl(row, l, 64);
                    const double r_d = __shfl(d, l, 64);
                    double v = sp_acc_round(acc[sl], fl, round_mode);
                    if (lane == 0) {
                        if (!unit) v = v / r_d;
                        st_post(xq + r_row, v);
                        x[r_row] = v;
                    }
                    sp_wave_sync();
                }
            }
        }
        return;
    }

    // ---- the walk: rows of the batch in order; row s is finished and posted before a later row takes x_s ----
    if constexpr (G == 8) {
        for (int s = 0; s < nrows; ++s) {   // wave-uniform
            const int L = s * G;            // the leader lane of row s
            const bool mine = slot == s;
            double v;
            if constexpr (PLAIN) {
#pragma unroll
                for (int o = G / 2; o > 0; o >>= 1) {
                    const double t = __shfl_down(ps, o, G);
                    if (mine) ps += t;
                }
                v = __shfl(ps, L, 64);
            } else {
#pragma unroll
                for (int st = 1; st < G; st <<= 1)
                    sp_cascade_step<true>(f, flags, st, mine && (sub & (2 * st - 1)) == 0, sink);
                bool fb = false;
                double r = 0.0;
                if (lane == L) fb = !sp_certify_or_spill(f, flags, force_fb, acc[slot], r);
                if (__ballot(fb)) {
                    if (lane == 0) ++cn.fb;
                    sp_wave_sync();
                    const unsigned fl = (unsigned)__shfl((int)flags, L, 64) & FLAG_NONFINITE;
                    v = sp_acc_round(acc[s], fl, round_mode);
                    sp_wave_sync();
                } else {
                    if (lane == 0) ++cn.reg;
                    v = __shfl(r, L, 64);
                }
                // a finished row's lanes hold nothing any more (a stale head must never reach the range guard)
                if (mine) {
#pragma unroll
                    for (int i = 0; i < SP_N; ++i) f[i] = 0.0;
                }
            }
            if (!unit) v = v / __shfl(d, L, 64);
            if (lane == L) {
                st_post(xq + row, v);
                x[row] = v;
            }
            // the later rows of the batch take their products with x_s
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const bool match = slot > s && (int)((dsl >> (4 * j)) & 15u) == s;
                if (__any(match)) {
                    if constexpr (PLAIN) {
                        if (match) ps -= da[j] * v;
                    } else {
                        double p[1], er[1];
                        p[0] = two_prod(match ? da[j] : 0.0, match ? -v : 0.0, er[0]);
                        fpe_absorb_prod<SP_N, true, 1>(f, p, er, sink);
                    }
                }
            }
        }
    }
}

template <bool PLAIN, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_sptrsv(int m, const I *__restrict__ rp, const I *__restrict__ ci,
                                                    const double *__restrict__ val, double *x, int rev, int unit, int R,
                                                    int force_fb, int round_mode, long long limit, long long *hdr, double *xq)
{
    __shared__ long long acc[SP_WAVES][ST_R][NL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if constexpr (!PLAIN) {
        for (int t = lane; t < ST_R * NL; t += 64) (&acc[w][0][0])[t] = 0;
    }
    const long long nitems = ((long long)m + R - 1) / R;
    StCounters cn;
    for (;;) {
        const long long t = st_take_ticket(hdr);
        if (t >= nitems) break;
        const long long pos0 = t * R;
        const int nrows = (int)min((long long)R, (long long)m - pos0);
        bool wide = R == 1;
        if (!wide) {
            long long len = 0;
            if (lane < nrows) {
                const long long r = rev ? (long long)m - 1 - (pos0 + lane) : pos0 + lane;
                len = (long long)rp[r + 1] - (long long)rp[r];
            }
            wide = __any(len > SP_SHORT_MAX);
        }
        if (wide) {
            for (int r = 0; r < nrows; ++r)
                st_rows<64, PLAIN>(pos0 + r, 1, m, rp, ci, val, x, rev, unit, force_fb, round_mode, limit, hdr, xq, acc[w], cn);
        } else {
            st_rows<8, PLAIN>(pos0, nrows, m, rp, ci, val, x, rev, unit, force_fb, round_mode, limit, hdr, xq, acc[w], cn);
        }
    }
    st_flush_counters(cn, hdr);
}

}  // namespace

hipError_t exsptrsv_dispatch(Ctx &c, char uplo, char diag, int m, int index_bits, const void *row_ptr, const void *col_idx,
                             const double *val, double *x, int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.sptrsv_info_dev = nullptr;
    if (m == 0) return hipSuccess;
    const StOrient o = st_orient(uplo, diag);
    StSpace w;   // the mailbox holds m doubles
    if (hipError_t e = st_workspace(c, (size_t)m, st, w); e != hipSuccess) return e;
    if (hipError_t e = st_preset(c, m, 1, w.hdr, w.xq, st); e != hipSuccess) return e;
    c.sptrsv_info_dev = w.hdr;
    const int R = c.sptrsv_path == 2 ? 1 : ST_R;
    const StRule rule = st_rule(fpe, c.sptrsv_path, round_mode);
    const long long nitems = ((long long)m + R - 1) / R, limit = watchdog_ticks(c.device);
    const int grid = st_grid(c, nitems, SP_WAVES);
    return sp_dispatch(index_bits, fpe, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
        using I = std::remove_cv_t<std::remove_pointer_t<decltype(rp)>>;
        hipLaunchKernelGGL((k_sptrsv<decltype(plain)::value, I>), dim3(grid), dim3(SP_BLOCK), 0, st, m, rp, ci, val, x, o.rev,
                           o.unit, R, rule.force_fb, rule.round_mode, limit, w.hdr, w.xq);
        return hipGetLastError();
    });
}

}  // namespace exb
