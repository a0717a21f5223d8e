// spic0.hip -- ExSpIC0 for gfx950: the exact-sum IC(0) factor of a symmetric square CSR matrix (int32 or int64 indices),
// on the device, on A's own pattern.
//
// Contract (include/exblas_hip.h).  Every row has strictly ascending columns and a stored diagonal, and the pattern S is
// structurally symmetric; only the entries on and below the diagonal are read.  For every stored (i, j) with j <= i, rows
// in ascending order,
//   c_ij = Round( a_ij - sum_k l_ik l_jk )        k < j, (i, k) in S, (j, k) in S   (j = i: the l_ik^2)
//   j <  i:  l_ij = fl( c_ij / l_jj )             ONE IEEE division
//   j == i:  l_ii = fl( sqrt(c_ii) )              ONE correctly rounded square root, as in potrf.hip
// the sum exact over the already fixed doubles (TwoProd of every product) and rounded once.  The factor goes to ONE value
// array on A's row_ptr / col_idx: L on and below the diagonal, and every stored (j, i) above it holds the same double
// l_ij (L^T as a mirror), so ExSpTRSV ('L', 'N') and then ('U', 'N') apply (L L^T)^-1 as it is.  A radicand that is not
// > 0 gives sqrt(c_ii) by IEEE arithmetic and the factorisation goes on (ExSpILU0's rule, not ExPOTRF's stop).
// info[0]: 0, or r + 1 for the smallest row r with a structural defect, in two phases: ExSpILU0's defects first; only
// when there is none, the smallest row r that stores some (r, j) without a stored (j, r).  ll is then not written at
// all.  info[1]: 0, or r + 1 for the smallest row whose radicand c_rr is not > 0 (zero, negative or NaN).
//
// Structure: four kernels in stream order, no host synchronisation between them.
//   * k_spilu0_preset (spfactor_common.hip.h): info := 0, the header := 0, the mailbox := "not posted".
//   * k_spilu0_check (spfactor_common.hip.h): phase 1, one thread per row over the indices alone; a sound row records
//     the position of its diagonal.
//   * k_spic0_mirror: phase 2, returns at once if info[0] is set.  One thread per row; every off-diagonal (r, j) looks
//     (j, r) up by binary search in row j (sorted: phase 1 has shown it).  A missing mirror lowers hdr[IC_MIRROR], not
//     info[0]: a workgroup that starts late must not take another's phase-2 finding for phase 1's.
//   * k_spic0: ONE persistent kernel on the frame of spilu0.hip.  It returns if info[0] or hdr[IC_MIRROR] is set (its
//     first workgroup moves the latter into info[0]).  Rows are handed out in ascending order by st_take_ticket; ONE WAVE
//     OWNS ONE ROW and its lanes own the row's entries ON AND BELOW the diagonal (the owned part: one per lane up to 64,
//     up to IL_MAX / 64 per lane beyond; path 2: 8 lanes share an owned part of at most 64).  The owned part is staged in
//     LDS once (a_ij is read there and nowhere else, so ll may be val; nothing above the diagonal is read).  Each lane
//     keeps one SP_N-term expansion per entry, seeded with a_ij.  The wave walks the L part in ascending k:
//       1. the lane that owns (i, k) certifies c_ik (it needs nothing of row k: before any wait);
//       2. the columns of row k right of its diagonal are staged in LDS;
//       3. ONE st_fetch brings l_kk (at dpos[k]) and, for every owned j in (k, i) that row k stores, l_jk from the
//          mailbox slot of the mirror position (k, j) (posted there by row j at its step k);
//       4. l_ik = c_ik / l_kk;
//       5. (k, i) is found among the staged columns; l_ik goes to ll at (i, k) and (k, i) and is posted to the mailbox
//          at (k, i) at once, not at the end of the row;
//       6. lane j absorbs TwoProd(l_ik, -l_jk), the diagonal lane TwoProd(l_ik, -l_ik).
//     After the last step the diagonal lane certifies the radicand; the root is stored at dpos[i] and posted there.
//   * What cannot be certified in registers (ties, near-ties inside spmv_round_fast's margin, spills, non-finite flags,
//     fpe = 0, path 1, the reference rounding mode) is settled on the spot through the wave's ONE integer accumulator in
//     LDS (ic_resolve: the lanes stride the L entries before it, look (k, j) up again, add the exact products and a_ij).
//
// Hand-off: the project's mailbox, one double per stored entry, indexed by CSR position, preset to ST_EMPTY, the value its
// own ready flag (st_post / st_fetch).  Only positions on and above the diagonal are ever posted: l_jk at (k, j), l_kk at
// (k, k).  Each such position is posted once, by the row that owns its mirror.
//
// Progress: sptrsv.hip's argument.  Row i only ever WAITS for l_kk (posted by row k < i at its end) and l_jk for k < j < i
// (posted by row j < i at its step k, which needs rows below j alone): posts by lower tickets.  Lower tickets are held by
// waves that have already taken them, i.e. that are resident and run (or have finished), so the wave with the lowest
// unfinished ticket never waits for anything that is not posted, and by induction every wave finishes: no workgroup
// barrier, no need for the grid to be co-resident, no input can deadlock.  ic_resolve asks for nothing the first pass did
// not.  Watchdog: st_fetch's 2 s, the header flag, EXBLAS_SPTRSV_STALLED.
// fpe == 1 runs the same structure with plain fp64 sums: s = a_ij, then s -= l_ik * l_jk for k ascending, then the
// division or the square root.
#include "../../include/exblas_hip.h"
#include "spfactor_common.hip.h"

namespace exb {
namespace {

constexpr int IC_MIRROR = 2;   // header word: phase 2's finding (r + 1 of the smallest row with a missing mirror)

struct IcArgs {
    int m, force_fb, round_mode, wide_all;   // wide_all: path 2
    long long limit;
};

// phase 2 of the check: the smallest row r that stores an (r, j) without a stored (j, r), into hdr[IC_MIRROR]
template <class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spic0_mirror(int m, const I *__restrict__ rp, const I *__restrict__ ci,
                                                           const long long *info, long long *hdr)
{
    if (info[0] != 0) return;   // phase 1 found a defect: the rows may not even be sorted
    for (long long r = (long long)blockIdx.x * SP_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * SP_BLOCK) {
        const long long p1 = (long long)rp[r + 1];
        for (long long p = (long long)rp[r]; p < p1; ++p) {
            const long long j = (long long)ci[p];
            if (j == r) continue;
            long long lo = (long long)rp[j], hi = (long long)rp[j + 1];
            const long long end = hi;
            while (lo < hi) {
                const long long mid = (lo + hi) >> 1;
                if ((long long)ci[mid] < r) lo = mid + 1;
                else hi = mid;
            }
            if (lo == end || (long long)ci[lo] != r) {
                il_info_min(&hdr[IC_MIRROR], r + 1);
                break;
            }
        }
    }
}

// What no lane could certify: Round(a_ij - sum l_ik l_jk) of owned entry `et` of the staged row (scol: its columns, sv:
// the l_ik fixed so far and, from the entry's own place on, the a_ij) through the wave's accumulator.  n: the L entries
// before it.  The diagonal (column `row`) takes the squares of the staged l_ik; another entry looks (k, j) up in row k and
// fetches l_jk there.  Wave-uniform; every lane gets the value, and the accumulator is zero again.
template <class I>
__device__ double ic_resolve(const IcArgs &A, int et, int n, long long row, const int *scol, const double *sv,
                             const I *__restrict__ rp, const I *__restrict__ ci, const long long *__restrict__ dpos,
                             const double *xq, long long *hdr, long long *acc)
{
    const int lane = threadIdx.x & 63;
    unsigned fl = 0;
    RowSink sink{acc, fl};
    sp_wave_sync();   // the l_ik of the steps so far are in sv
    const long long j = scol[et];
    const bool dg = j == row;
    for (int k0 = 0; k0 < n; k0 += 64) {   // wave-uniform
        const int kk = k0 + lane;
        long long at[1] = {0};
        bool want[1] = {false}, take = false;
        double uv[1], l = 0.0;
        if (kk < n) {
            const long long k = scol[kk];
            l = sv[kk];
            if (dg) {
                take = true;
            } else {
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
        }
        st_fetch<1>(xq, at, want, uv, hdr, A.limit);   // (posted: the first pass waited for it)
        if (want[0] || take) {
            double e;
            const double p = two_prod(l, -(take ? l : uv[0]), e);
            sink_product(sink, p, e);
        }
    }
    if (lane == 0) sink.add(sv[et]);
    sp_wave_sync();
    const double v = sp_acc_round(acc, NonFiniteLanes(fl).of(~0ull), A.round_mode);
    sp_wave_sync();
    return v;
}

// The rounded total of owned entry `et`, owned by slot os of lane ol: certified in registers by its lane, else through
// the accumulator.  Wave-uniform; every lane gets the value.
template <int S, bool PLAIN, class I>
__device__ __forceinline__ double ic_total(const IcArgs &A, int et, int ol, int os, int n, long long row, double (&f)[S][SP_N],
                                           const unsigned (&fl)[S], const double (&ps)[S], const int *scol, const double *sv,
                                           const I *__restrict__ rp, const I *__restrict__ ci,
                                           const long long *__restrict__ dpos, const double *xq, long long *hdr,
                                           long long *acc, StCounters &cn)
{
    const int lane = threadIdx.x & 63;
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
            return ic_resolve(A, et, n, row, scol, sv, rp, ci, dpos, xq, hdr, acc);
        }
        if (lane == 0) ++cn.reg;
    }
    return lane_bcast(v, ol);
}

// One row.  S entries per lane: owned entry e belongs to lane e % W, slot e / W (W = 64; 8 on path 2 for an owned part of
// at most 64 entries, so that the several-entries form is walked by small rows as well).
template <int S, bool PLAIN, class I>
__device__ __forceinline__ void ic_row(const IcArgs &A, long long row, const I *__restrict__ rp, const I *__restrict__ ci,
                                       const double *val, double *ll, long long *info, long long *hdr, double *xq,
                                       const long long *__restrict__ dpos, long long *acc, int *scol, double *sv, int *kc,
                                       StCounters &cn)
{
    const int lane = threadIdx.x & 63;
    const long long p0 = (long long)rp[row];
    const int nl = (int)(dpos[row] - p0), len = nl + 1;   // the L entries, the owned part (the diagonal last)
    const int lgw = (S > 1 && len <= 64) ? 3 : 6, W = 1 << lgw;
    // ---- the owned part into LDS: a_ij is read here and nowhere else ----
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
        const long long q0 = dpos[k] + 1;
        const int nu = (int)((long long)rp[k + 1] - q0);   // entries of row k right of its diagonal
        for (int t = lane; t < nu; t += 64) kc[t] = (int)ld_nt(ci + q0 + t);
        // c_ik needs nothing of row k: it is rounded before the wave waits for that row
        const double v = ic_total<S, PLAIN>(A, kk, kk & (W - 1), kk >> lgw, kk, row, f, fl, ps, scol, sv, rp, ci, dpos, xq,
                                            hdr, acc, cn);
        sp_wave_sync();   // row k's columns are in kc
        // l_kk and, for every owned j in (k, i) that row k stores, l_jk at the mirror (k, j): ONE wait for row k
        long long at[S + 1];
        bool want[S + 1], sq[S];
        double uv[S + 1];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            at[s] = 0;
            want[s] = false;
            sq[s] = own[s] && e[s] == nl;   // the diagonal: l_ik^2
            if (own[s] && e[s] > kk && e[s] < nl) {
                const int ix = il_find(kc, nu, c[s]);
                if (ix >= 0) {
                    want[s] = true;
                    at[s] = q0 + ix;
                }
            }
            if (want[s] || sq[s]) ++cn.nodiag;   // (the product terms: every lane counts its own)
        }
        at[S] = q0 - 1;
        want[S] = true;
        st_fetch<S + 1>(xq, at, want, uv, hdr, A.limit);
        const double l = v / uv[S];
        const int mi = il_find(kc, nu, (int)row);   // (k, i): stored, as phase 2 of the check has shown
        if (lane == 0) {
            sv[kk] = l;   // (ic_resolve reads it behind a sp_wave_sync of its own)
            ll[p0 + kk] = l;
            if (mi >= 0) {
                ll[q0 + mi] = l;
                st_post(xq + q0 + mi, l);
            }
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const bool use = want[s] || sq[s];
            const double o = sq[s] ? l : uv[s];
            if constexpr (PLAIN) {
                if (use) ps[s] -= l * o;
            } else {
                if (__any(use)) {
                    double pr[1], er[1];
                    pr[0] = two_prod(use ? l : 0.0, use ? -o : 0.0, er[0]);
                    SpLaneSink sink{fl[s]};
                    fpe_absorb_prod<SP_N, true, 1>(f[s], pr, er, sink);
                }
            }
        }
        sp_wave_sync();   // kc is read before the next step stages its row
    }

    // ---- the diagonal: certify the radicand, root, store, post ----
    const double rad = ic_total<S, PLAIN>(A, nl, nl & (W - 1), nl >> lgw, nl, row, f, fl, ps, scol, sv, rp, ci, dpos, xq, hdr,
                                          acc, cn);
    const double d = __builtin_sqrt(rad);
    if (lane == 0) {
        ll[p0 + nl] = d;
        st_post(xq + p0 + nl, d);
        if (!(rad > 0.0)) il_info_min(&info[1], row + 1);
    }
    sp_wave_sync();   // the staged row is done with before the next one comes in
}

template <bool PLAIN, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spic0(IcArgs A, const I *__restrict__ rp, const I *__restrict__ ci,
                                                   const double *val, double *ll, long long *info, long long *hdr, double *xq,
                                                   const long long *__restrict__ dpos)
{
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ int scol[SP_WAVES][IL_MAX], kc[SP_WAVES][IL_MAX];
    __shared__ double sv[SP_WAVES][IL_MAX];
    // a structural defect: ll is not written at all.  Phase 2's finding is moved into info[0] by one thread; every
    // workgroup reads the header word itself, which no kernel of this launch writes.
    const long long mirror = hdr[IC_MIRROR];
    if (info[0] != 0) return;
    if (mirror != 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) info[0] = mirror;
        return;
    }
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if constexpr (!PLAIN) {
        for (int t = lane; t < NL; t += 64) acc[w][t] = 0;
        sp_wave_sync();
    }
    StCounters cn;
    for (;;) {
        const long long row = st_take_ticket(hdr);
        if (row >= A.m) break;
        const long long len = dpos[row] + 1 - (long long)rp[row];
        if (A.wide_all || len > 64) {
            if (lane == 0) ++cn.skipped;   // (the rows in the several-entries-per-lane form)
            ic_row<IL_S, PLAIN>(A, row, rp, ci, val, ll, info, hdr, xq, dpos, acc[w], scol[w], sv[w], kc[w], cn);
        } else {
            ic_row<1, PLAIN>(A, row, rp, ci, val, ll, info, hdr, xq, dpos, acc[w], scol[w], sv[w], kc[w], cn);
        }
    }
    st_flush_counters(cn, hdr);
}

}  // namespace

// Workspace: spf_space (spfactor_common.hip.h), the same as ExSpILU0's.
hipError_t exspic0_dispatch(Ctx &c, int m, int index_bits, const void *row_ptr, const void *col_idx, const double *val,
                            double *ll, long long *info, int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.spic0_info_dev = nullptr;
    if (m == 0) {
        hipLaunchKernelGGL(k_spilu0_preset, dim3(1), dim3(SP_BLOCK), 0, st, 0ll, (long long *)nullptr, (long long *)nullptr, info);
        return hipGetLastError();
    }
    SpfSpace w;
    if (hipError_t e = spf_space(c, m, index_bits, row_ptr, c.spic0_m, c.spic0_nnz, st, w); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_spilu0_preset, dim3(max(1, st_grid(c, w.nnz, SP_BLOCK))), dim3(SP_BLOCK), 0, st, w.nnz, w.hdr,
                       (long long *)w.xq, info);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    c.spic0_info_dev = w.hdr;
    const StRule rule = st_rule(fpe, c.spic0_path, round_mode);
    const IcArgs A{m, rule.force_fb, rule.round_mode, c.spic0_path == 2 ? 1 : 0, watchdog_ticks(c.device)};
    const int cgrid = st_grid(c, m, SP_BLOCK), grid = st_grid(c, m, SP_WAVES);
    return sp_dispatch(index_bits, fpe, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
        using I = std::remove_cv_t<std::remove_pointer_t<decltype(rp)>>;
        hipLaunchKernelGGL((k_spilu0_check<I>), dim3(cgrid), dim3(SP_BLOCK), 0, st, m, rp, ci, w.nnz, info, w.dpos);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL((k_spic0_mirror<I>), dim3(cgrid), dim3(SP_BLOCK), 0, st, m, rp, ci, (const long long *)info, w.hdr);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
        hipLaunchKernelGGL((k_spic0<decltype(plain)::value, I>), dim3(grid), dim3(SP_BLOCK), 0, st, A, rp, ci, val, ll, info,
                           w.hdr, w.xq, w.dpos);
        return hipGetLastError();
    });
}

}  // namespace exb
