// spilu0.hip -- ExSpILU0 for gfx950: the exact-sum ILU(0) factor of a square CSR matrix (int32 or int64 indices), on the
// device, on A's own pattern.
//
// Contract (include/exblas_hip.h).  Every row has strictly ascending columns and a stored diagonal; S is the set of stored
// positions.  For every stored (i, j), rows in ascending order,
//   c_ij = Round( a_ij - sum_k l_ik u_kj )        k < min(i, j), (i, k) in S, (k, j) in S
//   j <  i:  l_ij = fl( c_ij / u_jj )             ONE IEEE division
//   j >= i:  u_ij = c_ij
// the sum exact over the already fixed doubles (TwoProd of every product) and rounded once: getrf_batched.hip's step
// without the pivot search, on the pattern.  L has a unit diagonal and lies strictly below it, U on and above it, both in
// ONE value array on A's row_ptr / col_idx: ExSpTRSV ('L', 'U') and then ('U', 'N') apply it as it is.  Non-finite operands
// and zero pivots follow IEEE arithmetic, the factorisation does not stop.  Every path sums the same multiset exactly, so
// the bits depend on the data and the rounding mode only.
// info[0]: 0, or r + 1 for the smallest row r with a structural defect (row_ptr decreasing or outside the entries the call
// may touch, a column outside [0, m), columns not strictly ascending, no stored diagonal, more than
// EXBLAS_SPILU0_MAX_ROW entries); lu is then not written at all.  info[1]: 0, or r + 1 for the smallest row whose pivot
// u_rr is zero or NaN.  Both are minima, so they do not depend on the order in which the waves meet them.
//
// Structure: three kernels in stream order, no host synchronisation between them (the preset and the check live in
// spfactor_common.hip.h, shared with ExSpIC0).
//   * k_spilu0_preset: info := 0, the header := 0, the mailbox := "not posted".  It is a launch of its own because a grid
//     has no order between one workgroup's zero and another's atomic minimum.
//   * k_spilu0_check: one thread per row over the indices alone.  A defect lowers info[0] (compare-and-swap minimum);
//     a sound row records the position of its diagonal in the workspace.
//   * k_spilu0: ONE persistent kernel on the frame of sptrsv.hip.  It reads info[0] first and returns if it is set.  Rows
//     are handed out in ascending order by st_take_ticket; ONE WAVE OWNS ONE ROW and its lanes own the row's stored
//     entries: one per lane up to 64 entries (the design range), up to EXBLAS_SPILU0_MAX_ROW / 64 per lane beyond.  The
//     row's columns and values are staged in the wave's LDS once (a_ij is read there and nowhere else, so lu may be val).
//     Each lane keeps one SP_N-term expansion per entry, seeded with a_ij.  The wave walks the L part of its row in
//     ascending k: the lane that owns (i, k) certifies its rounding (before the wave waits for row k: c_ik needs nothing of
//     it), the columns of row k right of its diagonal are staged in LDS, every lane with j > k finds (k, j) there by
//     binary search (row k is sorted), ONE fetch brings u_kk and the u_kj from the mailbox, the wave divides and keeps
//     l_ik, the lanes absorb TwoProd(l_ik, -u_kj).  After the last step the U lanes
//     certify, store and post.
//   * What cannot be certified in registers (ties, near-ties inside spmv_round_fast's margin, spills, non-finite flags,
//     fpe = 0, path 1, the reference rounding mode) is settled on the spot through the wave's ONE integer accumulator in
//     LDS: the lanes stride the L entries of the row, look (k, j) up again, add the exact products and a_ij, sp_acc_round
//     rounds (il_resolve).  Nothing is rounded twice and no tie is decided in registers.
//
// Hand-off: the project's mailbox.  One double per stored entry, indexed by CSR position, preset to ST_EMPTY; the value is
// its own ready flag (st_post / st_fetch: agent-scope relaxed atomics), so there is no flag word guarding plain stores and
// no release per row.  Only the U parts are ever posted and fetched.  The plain store to lu is separate; lu is written by
// the wave that owns the row and read by nobody.
//
// Progress: sptrsv.hip's argument.  A wave only ever WAITS (polls the mailbox) for u_kj of a row k < i, a lower ticket.
// Lower tickets are held by waves that have already taken them, i.e. that are resident and run (or have finished), so the
// wave with the lowest unfinished ticket never waits for anything that is not posted, and by induction every wave
// finishes: no workgroup barrier, no need for the grid to be co-resident, no input can deadlock.  il_resolve asks for
// nothing the first pass did not.  Watchdog: st_fetch's 2 s, the header flag, EXBLAS_SPTRSV_STALLED.
// fpe == 1 runs the same structure with plain fp64 sums: s = a_ij, then s -= l_ik * u_kj for k ascending.
#include "../../include/exblas_hip.h"
#include "spfactor_common.hip.h"

namespace exb {
namespace {

struct IlArgs {
    int m, force_fb, round_mode, wide_all;   // wide_all: path 2
    long long cap, limit;                    // cap: the entries the call may touch (the mailbox slots)
};

// What no lane could certify: Round(a - sum l_ik u_kj) of entry `et` of the staged row (scol: its columns, sv: the l_ik
// fixed so far and, from the entry's own place on, the a_ij) through the wave's accumulator.  n: the L entries before it.
// Wave-uniform; every lane gets the value, and the accumulator is zero again.
template <class I>
__device__ double il_resolve(const IlArgs &A, int et, int n, const int *scol, const double *sv, const I *__restrict__ rp,
                             const I *__restrict__ ci, const long long *__restrict__ dpos, const double *xq, long long *hdr,
                             long long *acc)
{
    const int lane = threadIdx.x & 63;
    unsigned fl = 0;
    RowSink sink{acc, fl};
    sp_wave_sync();   // the l_ik of the steps so far are in sv
    const long long j = scol[et];
    for (int k0 = 0; k0 < n; k0 += 64) {   // wave-uniform
        const int kk = k0 + lane;
        long long at[1] = {0};
        bool want[1] = {false};
        double uv[1], l = 0.0;
        if (kk < n) {
            const long long k = scol[kk];
            l = sv[kk];
            long long lo = dpos[k] + 1, hi = (long long)rp[k + 1];
            const long long end = hi;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if ((long long)ci[mid] < j) lo = mid + 1;
                else hi = mid;
            }
            if (lo < end && (long long)ci[lo] == j) {
                want[0] = true;
                at[0] = lo;
            }
        }
        st_fetch<1>(xq, at, want, uv, hdr, A.limit);   // (posted: the first pass waited for it)
        if (want[0]) {
            double e;
            const double p = two_prod(l, -uv[0], e);
            sink_product(sink, p, e);
        }
    }
    if (lane == 0) sink.add(sv[et]);
    sp_wave_sync();
    const double v = sp_acc_round(acc, NonFiniteLanes(fl).of(~0ull), A.round_mode);
    sp_wave_sync();
    return v;
}

// One row.  S entries per lane: entry e of the row belongs to lane e % W, slot e / W (W = 64; 8 on path 2 for a row of at
// most 64 entries, so that the several-entries form is walked by small rows as well).
template <int S, bool PLAIN, class I>
__device__ __forceinline__ void il_row(const IlArgs &A, long long row, const I *__restrict__ rp, const I *__restrict__ ci,
                                       const double *val, double *lu, long long *info, long long *hdr, double *xq,
                                       const long long *__restrict__ dpos, long long *acc, int *scol, double *sv, int *kc,
                                       StCounters &cn)
{
    const int lane = threadIdx.x & 63;
    const long long p0 = (long long)rp[row];
    const int len = (int)((long long)rp[row + 1] - p0), nl = (int)(dpos[row] - p0);
    const int lgw = (S > 1 && len <= 64) ? 3 : 6, W = 1 << lgw;
    // ---- the row into LDS: a_ij is read here and nowhere else ----
    for (int t = lane; t < len; t += 64) {
        scol[t] = (int)ld_nt(ci + p0 + t);   // (checked: a column lies in [0, m), m an int)
        sv[t] = ld_nt(val + p0 + t);
    }
    sp_wave_sync();
    int e[S];
    bool own[S];
    int c[S];
    unsigned fl[S];
    double f[S][SP_N], ps[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        e[s] = s * W + lane;
        own[s] = lane < W && e[s] < len;
        c[s] = own[s] ? scol[e[s]] : -1;
        fl[s] = 0;
        ps[s] = own[s] ? sv[e[s]] : 0.0;
#pragma unroll
        for (int i = 0; i < SP_N; ++i) f[s][i] = 0.0;
        if constexpr (!PLAIN) {
            if (S == 1 || s * W < len) {   // wave-uniform
                double pr[1] = {ps[s]}, er[1] = {0.0};
                SpLaneSink sink{fl[s]};
                fpe_absorb_prod<SP_N, true, 1>(f[s], pr, er, sink);
            }
        }
    }

    // ---- the L part, k ascending ----
    for (int kk = 0; kk < nl; ++kk) {   // wave-uniform
        const long long k = scol[kk];
        const int ol = kk & (W - 1), os = kk >> lgw;   // the lane and the slot that own (i, k)
        const long long q0 = dpos[k] + 1;
        const int nu = (int)((long long)rp[k + 1] - q0);   // entries of row k right of its diagonal
        for (int t = lane; t < nu; t += 64) kc[t] = (int)ld_nt(ci + q0 + t);
        // c_ik needs nothing of row k: it is rounded before the wave waits for that row
        double v = 0.0;
        bool fb = false;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (s == os && lane == ol) {
                if constexpr (PLAIN) {
                    v = ps[s];
                } else {
                    double r = 0.0;
                    if (!A.force_fb && fl[s] == 0 && spmv_round_fast<SP_N>(f[s], r)) v = r;
                    else fb = true;
                }
            }
        }
        if constexpr (!PLAIN) {
            if (__any(fb)) {
                if (lane == 0) ++cn.fb;
                v = il_resolve(A, kk, kk, scol, sv, rp, ci, dpos, xq, hdr, acc);
            } else {
                if (lane == 0) ++cn.reg;
                v = lane_bcast(v, ol);
            }
        } else {
            v = lane_bcast(v, ol);
        }
        sp_wave_sync();   // row k's columns are in kc
        // u_kk and, for every entry right of (i, k), u_kj where row k stores column j: ONE wait for row k
        long long at[S + 1];
        bool want[S + 1];
        double uv[S + 1];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            at[s] = 0;
            want[s] = false;
            if (own[s] && e[s] > kk) {
                const int ix = il_find(kc, nu, c[s]);
                if (ix >= 0) {
                    want[s] = true;
                    at[s] = q0 + ix;
                    ++cn.nodiag;   // (the product terms: every lane counts its own)
                }
            }
        }
        at[S] = q0 - 1;
        want[S] = true;
        st_fetch<S + 1>(xq, at, want, uv, hdr, A.limit);
        const double l = v / uv[S];
        if (lane == 0) {
            sv[kk] = l;   // (il_resolve reads it behind a sp_wave_sync of its own)
            lu[p0 + kk] = l;
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if constexpr (PLAIN) {
                if (want[s]) ps[s] -= l * uv[s];
            } else {
                if (__any(want[s])) {
                    double pr[1], er[1];
                    pr[0] = two_prod(want[s] ? l : 0.0, want[s] ? -uv[s] : 0.0, er[0]);
                    SpLaneSink sink{fl[s]};
                    fpe_absorb_prod<SP_N, true, 1>(f[s], pr, er, sink);
                }
            }
        }
        sp_wave_sync();   // kc is read before the next step stages its row
    }

    // ---- the U part: certify, store, post ----
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (S > 1 && s * W >= len) break;   // wave-uniform
        const bool isu = own[s] && e[s] >= nl;
        double v = 0.0;
        bool fb = false;
        if (isu) {
            if constexpr (PLAIN) {
                v = ps[s];
            } else {
                double r = 0.0;
                if (!A.force_fb && fl[s] == 0 && spmv_round_fast<SP_N>(f[s], r)) v = r;
                else fb = true;
            }
            if (!fb) {
                lu[p0 + e[s]] = v;
                st_post(xq + p0 + e[s], v);
                if (e[s] == nl && (v == 0.0 || v != v)) il_info_min(&info[1], row + 1);
            }
        }
        if constexpr (!PLAIN) {
            unsigned long long fbm = __ballot(fb);
            const unsigned long long regm = __ballot(isu && !fb);
            if (lane == 0) {
                cn.reg += __popcll(regm);
                cn.fb += __popcll(fbm);
            }
            while (fbm) {   // wave-uniform
                const int l = __builtin_ctzll(fbm);
                fbm &= fbm - 1ull;
                const int et = s * W + l;
                const double t = il_resolve(A, et, nl, scol, sv, rp, ci, dpos, xq, hdr, acc);
                if (lane == 0) {
                    lu[p0 + et] = t;
                    st_post(xq + p0 + et, t);
                    if (et == nl && (t == 0.0 || t != t)) il_info_min(&info[1], row + 1);
                }
            }
        }
    }
    sp_wave_sync();   // the staged row is done with before the next one comes in
}

template <bool PLAIN, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spilu0(IlArgs A, const I *__restrict__ rp, const I *__restrict__ ci,
                                                    const double *val, double *lu, long long *info, long long *hdr, double *xq,
                                                    const long long *__restrict__ dpos)
{
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ int scol[SP_WAVES][IL_MAX], kc[SP_WAVES][IL_MAX];
    __shared__ double sv[SP_WAVES][IL_MAX];
    if (info[0] != 0) return;   // a structural defect: lu is not written at all
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if constexpr (!PLAIN) {
        for (int t = lane; t < NL; t += 64) acc[w][t] = 0;
        sp_wave_sync();
    }
    StCounters cn;
    for (;;) {
        const long long row = st_take_ticket(hdr);
        if (row >= A.m) break;
        const long long len = (long long)rp[row + 1] - (long long)rp[row];
        if (A.wide_all || len > 64) {
            if (lane == 0) ++cn.skipped;   // (the rows in the several-entries-per-lane form)
            il_row<IL_S, PLAIN>(A, row, rp, ci, val, lu, info, hdr, xq, dpos, acc[w], scol[w], sv[w], kc[w], cn);
        } else {
            il_row<1, PLAIN>(A, row, rp, ci, val, lu, info, hdr, xq, dpos, acc[w], scol[w], sv[w], kc[w], cn);
        }
    }
    st_flush_counters(cn, hdr);
}

}  // namespace

// Workspace: spf_space (spfactor_common.hip.h).
hipError_t exspilu0_dispatch(Ctx &c, int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                             double *lu, long long *info, int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.spilu0_info_dev = nullptr;
    if (m == 0) {
        hipLaunchKernelGGL(k_spilu0_preset, dim3(1), dim3(SP_BLOCK), 0, st, 0ll, (long long *)nullptr, (long long *)nullptr, info);
        return hipGetLastError();
    }
    SpfSpace w;
    if (hipError_t e = spf_space(c, m, index_bits, row_ptr, c.spilu0_m, c.spilu0_nnz, st, w); e != hipSuccess) return e;
    const long long nnz = w.nnz;
    long long *hdr = w.hdr, *dpos = w.dpos;
    double *xq = w.xq;
    hipError_t e = hipSuccess;
    hipLaunchKernelGGL(k_spilu0_preset, dim3(max(1, st_grid(c, nnz, SP_BLOCK))), dim3(SP_BLOCK), 0, st, nnz, hdr, (long long *)xq,
                       info);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    c.spilu0_info_dev = hdr;
    const StRule rule = st_rule(fpe, c.spilu0_path, round_mode);
    const IlArgs A{m, rule.force_fb, rule.round_mode, c.spilu0_path == 2 ? 1 : 0, nnz, watchdog_ticks(c.device)};
    const int cgrid = st_grid(c, m, SP_BLOCK), grid = st_grid(c, m, SP_WAVES);
    return sp_dispatch(index_bits, fpe, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
        using I = std::remove_cv_t<std::remove_pointer_t<decltype(rp)>>;
        hipLaunchKernelGGL((k_spilu0_check<I>), dim3(cgrid), dim3(SP_BLOCK), 0, st, m, rp, ci, A.cap, info, dpos);
        if (hipError_t e2 = hipGetLastError(); e2 != hipSuccess) return e2;
        hipLaunchKernelGGL((k_spilu0<decltype(plain)::value, I>), dim3(grid), dim3(SP_BLOCK), 0, st, A, rp, ci, val, lu, info, hdr,
                           xq, dpos);
        return hipGetLastError();
    });
}

}  // namespace exb
