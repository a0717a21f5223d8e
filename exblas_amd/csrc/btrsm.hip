// btrsm.hip -- ExBTRSM for gfx950: exact, reproducible triangular solve FROM THE RIGHT on a tall row-major block:
// X op(T) = alpha B with T the p x p column-major triangle of ExTRSV (uplo, transt, diag, ldt) and X n x p (ldx), B on
// entry, solved in place.  The design range is p <= 64; p up to EXBLAS_BTRSM_MAX_P is served.
//
// Contract: per row r, in substitution order over the columns (forward when op(T) is upper),
//   x_rj = fl( Round( alpha * b_rj - sum_{i before j} x_ri * op(T)(i, j) ) / op(T)(j, j) )
// the sum exact over the already fixed doubles (every entry of the strict triangle counts: a zero times an infinite x_ri is
// NaN) and rounded once, then one IEEE division (none under diag 'U').  With alpha = 1 row r is, bit for bit, what ExTRSV
// (trsv.hip) writes for (uplo, the other trans, diag, T, B[r, :]).  The alpha term follows ExBGEMM's beta term: 1 adds b
// exactly, 0 does not read B, anything else adds the error-free product, both parts.  Every path sums that multiset of
// TwoProd pairs exactly, so the bits depend on the data, (uplo, transt, diag, alpha) and the rounding mode only.
//
// Structure: the frame of block_common.hip.h (one kernel, certify in registers or settle through the wave's accumulator,
// a counter slot per workgroup, the plain kernel of fpe == 1).  No mailbox and no ticket: rows are independent, the chain
// runs along a row.  What is this routine's own:
//   * LANES OWN ROWS.  A wave's item is RW consecutive rows (a power of two, 64 when the LDS allows, 4 on path 3); lane
//     lr + s * RW is slice s of row lr.  The S = 64 / RW slices of a row share the earlier columns i round-robin in groups
//     of four and are merged exactly by the shuffle cascade of the sparse routines before the certificate.
//   * The item's rows go through the wave's LDS: loaded along the unit stride of X, pitch p | 1 doubles (odd: the lanes'
//     reads of one column of RW rows meet no bank twice), solved in place there, stored back along the unit stride, one
//     store per output.
//   * op(T) is staged by the workgroup in substitution order, row i of the chunk holding op(T)(i, j..) contiguously:
//     the strict triangle, the diagonal under 'N', zero elsewhere.  p <= 64: the whole triangle once per workgroup.
//     Beyond (and on path 3): chunks of 64 (4) rows times 4 columns, staged again per item and column block.
//   * Register block: a lane keeps BT_NB (4; 1 on path 2) 4-term expansions, for the columns j0 .. j0 + 3.  Per group of
//     four earlier columns it reads its own four x_ri from LDS and the 16 entries of op(T) (broadcast).  Then the alpha
//     term (sp_absorb_beta), the merge, and the 4 x 4 diagonal block one column after the other: certify, divide, write
//     x to the LDS row, multiply into the later columns of the block.
//   * Rounding.  The fall-back (bt_resolve) settles an output before the lane's chain goes on: the lanes stride the
//     earlier columns of that one output (x_ri from the wave's LDS row, op(T)(i, j) from memory), lane 0 adds the alpha
//     term, then the division.
#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int BT_NB = 4;                 // columns per register block: four 4-term expansions
constexpr int BT_U = 4;                  // earlier columns per step of the inner loop
constexpr int BT_CH = 64;                // rows of op(T) in a staged chunk ...
constexpr int BT_SMALL = 4;              // ... on path 3, and the rows of its wave item
constexpr size_t BT_LDS = 78 * 1024;     // dynamic LDS of a workgroup: with the 2.2 KiB of the accumulators, two
                                         // workgroups (and more at small p) stay resident on the 160 KiB of a CU

struct BtArgs {
    long long n, ldx, rs, cs, nitems, per;   // op(T)(i, j) = t[phys(i) * rs + phys(j) * cs]: one of rs, cs is 1, the other ldt
    int p, lgr, nb, lgch, lgcw, tsz, rev, unit, force, round_mode, dq, dr;   // dq, dr: 64 / p, 64 % p
    double alpha;
};

// substitution position -> physical column of X, row / column of T
__device__ __forceinline__ int bt_phys(const BtArgs &A, int k) { return A.rev ? A.p - 1 - k : k; }

// ts[il * CW + jl] := op(T)(c0 + il, J0 + jl) for the rows of the chunk below p: the strict triangle (i < j < p) and,
// under 'N', the diagonal; zero elsewhere.  Between two workgroup barriers.
__device__ __forceinline__ void bt_stage(const BtArgs &A, const double *__restrict__ t, int c0, int J0, double *ts)
{
    const int CH = 1 << A.lgch, CW = 1 << A.lgcw, nr = min(CH, A.p - c0);
    for (int k = threadIdx.x; k < (nr << A.lgcw); k += SP_BLOCK) {
        int il, jl;
        if (A.cs == 1 || nr != CH) {   // a row of op(T) is contiguous (or a partial chunk): columns fastest
            il = k >> A.lgcw, jl = k & (CW - 1);
        } else {                       // a column of op(T) is contiguous: rows fastest
            il = k & (CH - 1), jl = k >> A.lgch;
        }
        const int i = c0 + il, j = J0 + jl;
        double v = 0.0;
        if (j < A.p && (i < j || (i == j && !A.unit))) v = t[bt_phys(A, i) * A.rs + bt_phys(A, j) * A.cs];
        ts[(il << A.lgcw) + jl] = v;
    }
}

// What no lane could certify: substitution column j of the wave's LDS row xrow through the wave's integer accumulator,
// op(T) from memory.  The row holds x at the earlier columns and b at j.  Wave-uniform.
__device__ void bt_resolve(const BtArgs &A, const double *__restrict__ t, double *xrow, int j, long long *acc)
{
    const int pj = bt_phys(A, j);
    const double *tj = t + pj * A.cs;
    double v = blk_resolve(
        acc, j, A.round_mode,
        [&](int i, double &a, double &b) {
            const int pi = bt_phys(A, i);
            a = tj[pi * A.rs], b = -xrow[pi];
        },
        [&](RowSink &sink) {
            if (A.alpha != 0.0) blk_sink_term(sink, A.alpha, xrow[pj]);
        });
    if (!A.unit) v = v / tj[pj * A.rs];
    if ((threadIdx.x & 63) == 0) xrow[pj] = v;
    sp_wave_sync();
}

template <bool PLAIN>
__global__ void __launch_bounds__(SP_BLOCK) k_btrsm(BtArgs A, const double *__restrict__ t, double *x, long long *slots)
{
    extern __shared__ double bt_lds[];   // [the chunk of op(T): tsz] [SP_WAVES x RW x pitch: the waves' rows of X]
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int RW = 1 << A.lgr, S = 64 >> A.lgr, lr = lane & (RW - 1), s = lane >> A.lgr;
    const int CH = 1 << A.lgch, CW = 1 << A.lgcw, pitch = A.p | 1;
    const bool leader = s == 0;
    double *ts = bt_lds, *xs = bt_lds + A.tsz + w * RW * pitch, *xrow = xs + lr * pitch;
    if constexpr (!PLAIN) {
        for (int k = lane; k < NL; k += 64) acc[w][k] = 0;
        sp_wave_sync();
    }
    const int lr0 = lane / A.p, cc0 = lane - lr0 * A.p;   // where the lane starts in the wave's rows, 64 entries a step
    const int nch = (A.p + CH - 1) >> A.lgch;
    long long staged = -1;
    unsigned long long n_reg = 0, n_fb = 0;
    const long long it0 = (long long)blockIdx.x * A.per, it1 = min(A.nitems, it0 + A.per);
    for (long long it = it0; it < it1; ++it) {   // workgroup-uniform
        const long long row0 = (it * SP_WAVES + w) * RW;   // the wave's first row: beyond n the wave only keeps the barriers
        const bool rowok = row0 + lr < A.n;

        // the wave's rows of B, along the unit stride; zero beyond n, and for alpha == 0 (B is not read)
        for (int r = lr0, cc = cc0; r < RW;) {
            double v = 0.0;
            if (A.alpha != 0.0 && row0 + r < A.n) v = x[(row0 + r) * A.ldx + cc];
            xs[r * pitch + cc] = v;
            cc += A.dr, r += A.dq;
            if (cc >= A.p) cc -= A.p, ++r;
        }
        sp_wave_sync();

        for (int j0 = 0; j0 < A.p; j0 += A.nb) {   // workgroup-uniform
            double f[BT_NB][SP_N], ps[BT_NB];
            unsigned flags[BT_NB];
#pragma unroll
            for (int c = 0; c < BT_NB; ++c) {
                ps[c] = 0.0;
                flags[c] = 0;
#pragma unroll
                for (int i = 0; i < SP_N; ++i) f[c][i] = 0.0;
            }
            const int J0 = j0 & ~(CW - 1), cd = j0 & ~(CH - 1);   // the chunk (cd, J0) holds the diagonal block

            if (!A.force) {   // forced: bt_resolve does all the work
                // ---- the earlier columns, chunk by chunk: the slices share them ----
                for (int c0 = 0; c0 <= cd; c0 += CH) {
                    const long long id = (long long)(J0 >> A.lgcw) * nch + (c0 >> A.lgch);
                    if (id != staged) {
                        __syncthreads();   // every wave has read the chunk that goes
                        bt_stage(A, t, c0, J0, ts);
                        __syncthreads();
                        staged = id;
                    }
                    const int iend = min(c0 + CH, j0);
                    for (int ib = c0; ib < iend; ib += S * BT_U) {   // wave-uniform: the absorb votes across the wave
                        const int i0 = ib + s * BT_U;
                        double xv[BT_U];
                        int ti[BT_U];
                        bool ok[BT_U];
#pragma unroll
                        for (int u = 0; u < BT_U; ++u) {
                            ok[u] = i0 + u < iend;
                            xv[u] = ok[u] ? xrow[bt_phys(A, i0 + u)] : 0.0;
                            ti[u] = ok[u] ? ((i0 + u - c0) << A.lgcw) + (j0 - J0) : 0;
                        }
#pragma unroll
                        for (int c = 0; c < BT_NB; ++c) {
                            if (c < A.nb) {   // wave-uniform
                                double pr[BT_U], er[BT_U];
#pragma unroll
                                for (int u = 0; u < BT_U; ++u) {
                                    const double tv = ok[u] ? ts[ti[u] + c] : 0.0;
                                    if constexpr (PLAIN) {
                                        if (ok[u]) ps[c] -= tv * xv[u];
                                    } else {
                                        pr[u] = two_prod(tv, -xv[u], er[u]);
                                    }
                                }
                                if constexpr (!PLAIN) {
                                    SpLaneSink sink{flags[c]};
                                    fpe_absorb_prod<SP_N, true, BT_U>(f[c], pr, er, sink);
                                }
                            }
                        }
                    }
                }

                // ---- alpha * b_rj, then the slices of a row become one ----
#pragma unroll
                for (int c = 0; c < BT_NB; ++c) {
                    if (c < A.nb && j0 + c < A.p) {   // wave-uniform
                        const int pj = bt_phys(A, j0 + c);
                        if constexpr (PLAIN) {
                            if (leader && A.alpha != 0.0) ps[c] += A.alpha == 1.0 ? xrow[pj] : A.alpha * xrow[pj];
                            for (int st = RW; st < 64; st <<= 1) ps[c] += __shfl_down(ps[c], st, 64);
                        } else {
                            SpLaneSink sink{flags[c]};
                            sp_absorb_beta(f[c], leader, A.alpha, xrow, pj, sink);
                            for (int st = RW; st < 64; st <<= 1)
                                sp_cascade_step(f[c], flags[c], st, (lane & (2 * st - 1)) < RW, sink);
                        }
                    }
                }
            }

            // ---- the columns of the block, one after the other ----
#pragma unroll
            for (int c = 0; c < BT_NB; ++c) {
                if (c < A.nb && j0 + c < A.p) {   // wave-uniform
                    const int j = j0 + c, pj = bt_phys(A, j);
                    const double *trow = ts + ((j - cd) << A.lgcw) + (j0 - J0);   // op(T)(j, j0 ..) of the staged chunk
                    if constexpr (PLAIN) {
                        if (leader) xrow[pj] = A.unit ? ps[c] : ps[c] / trow[c];
                    } else {
                        bool fb = false;
                        const bool mine = leader && rowok;
                        if (mine) {
                            double rr;
                            if (!A.force && flags[c] == 0 && spmv_round_fast<SP_N>(f[c], rr))
                                xrow[pj] = A.unit ? rr : rr / trow[c];
                            else
                                fb = true;
                        }
                        unsigned long long fbm = __ballot(fb);
                        n_reg += __popcll(__ballot(mine && !fb));
                        n_fb += __popcll(fbm);
                        while (fbm) {   // wave-uniform
                            const int l = __builtin_ctzll(fbm);   // a leader lane: l is its row of the item
                            fbm &= fbm - 1ull;
                            bt_resolve(A, t, xs + l * pitch, j, acc[w]);
                        }
                    }
                    // the column is in LDS before anything reads it
                    sp_wave_sync();
                    if (!A.force) {
                        // ---- the later columns of the block take their product with it ----
#pragma unroll
                        for (int c2 = c + 1; c2 < BT_NB; ++c2) {
                            if (c2 < A.nb && j0 + c2 < A.p) {   // wave-uniform
                                const double tv = leader ? trow[c2] : 0.0, v = leader ? xrow[pj] : 0.0;
                                if constexpr (PLAIN) {
                                    if (leader) ps[c2] -= tv * v;
                                } else {
                                    double pr[1], er[1];
                                    pr[0] = two_prod(tv, -v, er[0]);
                                    SpLaneSink sink{flags[c2]};
                                    fpe_absorb_prod<SP_N, true, 1>(f[c2], pr, er, sink);
                                }
                            }
                        }
                    }
                }
            }
        }

        // the solved rows, along the unit stride: one store per output
        for (int r = lr0, cc = cc0; r < RW;) {
            if (row0 + r < A.n) x[(row0 + r) * A.ldx + cc] = xs[r * pitch + cc];
            cc += A.dr, r += A.dq;
            if (cc >= A.p) cc -= A.p, ++r;
        }
        sp_wave_sync();   // the rows are stored before the next item replaces them
    }
    blk_store_counters(cnt, n_reg, n_fb, slots, blockIdx.x);
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain solve, 2..8 the expansions (the caller refused the rest
// and p > EXBLAS_BTRSM_MAX_P)
hipError_t exbtrsm_dispatch(Ctx &c, char uplo, char transt, char diag, long long n, int p, double alpha, const double *t,
                            int ldt, double *x, long long ldx, int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.btrsm_slots = SlotInfo();
    if (n == 0 || p == 0) return hipSuccess;
    const int path = c.btrsm_path;
    const bool lower = (uplo == 'L' || uplo == 'l'), trans = (transt == 'T' || transt == 't');
    BtArgs A;
    A.n = n, A.ldx = ldx, A.p = p, A.alpha = alpha;
    A.rs = trans ? (long long)ldt : 1ll, A.cs = trans ? 1ll : (long long)ldt;
    A.rev = (lower == trans) ? 0 : 1;   // op(T) upper ('U','N' or 'L','T'): forward over the columns
    A.unit = (diag == 'U' || diag == 'u') ? 1 : 0;
    A.nb = path == 2 ? 1 : BT_NB;
    // the staged chunk: the whole triangle for p <= 64 (its row pitch p rounded up to a power of two, at least 4),
    // else BT_CH (path 3: BT_SMALL) rows times 4 columns
    const bool whole = path != 3 && p <= BT_CH;
    int cw = 4;
    while (whole && cw < p) cw *= 2;
    const int ch = path == 3 ? BT_SMALL : BT_CH;
    A.lgch = 0, A.lgcw = 0;
    while ((1 << A.lgch) < ch) ++A.lgch;
    while ((1 << A.lgcw) < cw) ++A.lgcw;
    A.tsz = min(ch, (p + 3) & ~3) * cw;
    // rows per wave: the most the LDS budget holds
    const size_t pitch = (size_t)(p | 1);
    int rw = path == 3 ? BT_SMALL : 64;
    while (rw > 1 && ((size_t)A.tsz + (size_t)SP_WAVES * rw * pitch) * sizeof(double) > BT_LDS) rw >>= 1;
    A.lgr = 0;
    while ((1 << A.lgr) < rw) ++A.lgr;
    A.dq = 64 / p, A.dr = 64 % p;
    const StRule rule = st_rule(fpe, path, round_mode);
    A.force = rule.force_fb, A.round_mode = rule.round_mode;
    A.nitems = (n + (long long)SP_WAVES * rw - 1) / ((long long)SP_WAVES * rw);
    const auto [grid, per] = blk_partition(c, A.nitems);
    A.per = per;
    static std::atomic<unsigned long long> optin{0};
    hipError_t e = blk_lds_optin(optin, c.device, BT_LDS, {(const void *)k_btrsm<true>, (const void *)k_btrsm<false>});
    if (e != hipSuccess) return e;
    long long *slots = blk_reserve_slots(c, c.btrsm_slots, grid, st, &e);
    if (!slots) return e;
    const size_t lds = ((size_t)A.tsz + (size_t)SP_WAVES * rw * pitch) * sizeof(double);
    if (fpe == 1)
        hipLaunchKernelGGL((k_btrsm<true>), dim3(grid), dim3(SP_BLOCK), lds, st, A, t, x, slots);
    else
        hipLaunchKernelGGL((k_btrsm<false>), dim3(grid), dim3(SP_BLOCK), lds, st, A, t, x, slots);
    return hipGetLastError();
}

}  // namespace exb
