// potrf.hip -- ExPOTRF for gfx950: exact-sum Cholesky factorisation of a small symmetric positive definite matrix (the
// Gram matrix X^T X of CholQR, the P^T A P of a block CG), in place on the p x p column-major triangle of ExTRSV, so that
// its output is what ExTRSM / ExBTRSM take.  The design range is p <= 64; p up to EXBLAS_BTRSM_MAX_P is served.
//
// Contract (logical upper orientation, G = R^T R; uplo 'L' is L = R^T, the same numbers in the other triangle), row by
// row, j = 0 .. p-1:
//   r_jj = sqrt( Round( g_jj - sum_{k<j} r_kj^2 ) )
//   r_ji = fl( Round( g_ji - sum_{k<j} r_kj * r_ki ) / r_jj )      for i > j
// every sum exact over the already fixed doubles (both parts of every TwoProd, every entry, zeros included: a zero times an
// infinite entry is NaN) and rounded once under the rounding mode, then ONE correctly rounded square root or ONE IEEE
// division.  Every path sums the same multiset exactly, so the bits depend on the data, uplo and the rounding mode only.
// Breakdown (LAPACK's rule): at the first j whose rounded radicand v is not > 0 the kernel stores v at (j, j), leaves the
// rest of row j and all later rows as they were, and reports j + 1 in the info word; otherwise 0.  The word is written
// by every launch with a plain store.  The other triangle and the padding of a column are neither read nor written.
//
// Structure: the frame of block_common.hip.h (one kernel, certify in registers or settle through the wave's accumulator,
// the counter slot, the plain kernel of fpe == 1) with ONE workgroup (no mailbox, no ticket; the chain of p pivots is the
// problem).  What is this routine's own:
//   * R(k, i) = g[k * rs + i * cs]: 'U' has rs = 1, 'L' has cs = 1; nothing else knows about uplo.
//   * p <= 64 (not on path 3): the triangle is loaded once into LDS along its unit stride (row pitch 65: odd), factored
//     there and stored back once, the fixed entries only.  Beyond: factored in place in global memory; the rows a wave
//     fixed are read by the others after a workgroup barrier.
//   * Left-looking over row blocks of PO_NB (4; 1 on path 2) rows j0 .. j0 + 3.  LANES OWN COLUMNS i, in column tiles of
//     tw (64; 4 on path 3) starting at j0; a lane keeps one 4-term expansion per row of the block.
//   * Tile 0 holds the diagonal block.  The earlier rows k < j0 are split over the four waves as slices, round-robin in
//     groups of four; the slices pass through LDS and are merged exactly (fpe_cascade) by wave 0, which then walks the
//     4 x 4 diagonal block row after row: certify, square root (every lane takes it of the broadcast radicand), divide,
//     multiply the fixed row into the later rows of the block.
//   * The tiles beyond (p > 64, path 3) follow after a barrier, a tile per wave, unsliced: they need only the diagonal
//     block and their own columns.
//   * Rounding.  The fall-back (po_resolve) hands the rounded value to every lane; the square root or the division
//     follows.  The radicand is an ordinary output (r_kj against itself); it is settled before the rest of its row is
//     counted.
//   * Waves: four, one per SIMD; while wave 0 walks the diagonal block the others wait at the barrier.  Measured (DESIGN
//     5m): 3.1 to 3.5 us per pivot at p = 16 .. 64.
#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int PO_NB = 4;        // rows per register block: four 4-term expansions
constexpr int PO_U = 4;         // earlier rows per step of the inner loop
constexpr int PO_TILE = 64;     // columns of a tile, and the largest p that is staged in LDS
constexpr int PO_SMALL = 4;     // ... on path 3
constexpr int PO_PITCH = 65;    // row pitch of the staged triangle (odd)

struct PoArgs {
    long long rs, cs;   // R(k, i) = g[k * rs + i * cs]: one of them is 1, the other ldg
    int p, ldg, nb, tw, force, round_mode;
};

// the factor while it is made: the LDS triangle (STAGED) or G itself
template <bool STAGED>
struct PoStore {
    double *tri, *g;
    long long rs, cs;
    __device__ __forceinline__ double &at(int k, int i) const
    {
        if constexpr (STAGED) return tri[k * PO_PITCH + i];
        else return g[k * rs + i * cs];
    }
};

// What no lane could certify: Round(g_ji - sum_{k<j} r_kj r_ki) through the wave's integer accumulator.  (j, i) still
// holds g_ji.  Wave-uniform; every lane gets the value.
template <bool STAGED>
__device__ double po_resolve(const PoArgs &A, const PoStore<STAGED> &R, int j, int i, long long *acc)
{
    const double v = blk_resolve(
        acc, j, A.round_mode, [&](int k, double &a, double &b) { a = R.at(k, j), b = -R.at(k, i); },
        [&](RowSink &sink) { sink.add(R.at(j, i)); });
    sp_wave_sync();
    return v;
}

// a lane's share of the rows [0, j0) for its column i and the rows j0 .. j0 + nb - 1 of the block: slice s of S takes the
// groups of PO_U rows round-robin.  act[c]: the lane owns (j0 + c, i).  Wave-uniform.
template <bool PLAIN, bool STAGED>
__device__ __forceinline__ void po_earlier(const PoArgs &A, const PoStore<STAGED> &R, int j0, int i, int s, int S,
                                           const bool (&act)[PO_NB], double (&f)[PO_NB][SP_N], double (&ps)[PO_NB],
                                           unsigned (&flags)[PO_NB])
{
    for (int ib = 0; ib < j0; ib += S * PO_U) {
        const int k0 = ib + s * PO_U;
        double xv[PO_U];
        bool ok[PO_U];
#pragma unroll
        for (int u = 0; u < PO_U; ++u) {
            ok[u] = k0 + u < j0;
            xv[u] = (ok[u] && act[0]) ? R.at(k0 + u, i) : 0.0;   // act[0] is the widest: i >= j0 and i < p
        }
#pragma unroll
        for (int c = 0; c < PO_NB; ++c) {
            if (c < A.nb && j0 + c < A.p) {   // wave-uniform
                double pr[PO_U], er[PO_U];
#pragma unroll
                for (int u = 0; u < PO_U; ++u) {
                    const double tv = (ok[u] && act[c]) ? R.at(k0 + u, j0 + c) : 0.0, x = act[c] ? xv[u] : 0.0;
                    if constexpr (PLAIN) {
                        ps[c] -= tv * x;
                        pr[u] = er[u] = 0.0;
                    } else {
                        pr[u] = two_prod(tv, -x, er[u]);
                    }
                }
                if constexpr (!PLAIN) {
                    SpLaneSink sink{flags[c]};
                    fpe_absorb_prod<SP_N, true, PO_U>(f[c], pr, er, sink);
                }
            }
        }
    }
}

// g_ji joins the lane's sums
template <bool PLAIN, bool STAGED>
__device__ __forceinline__ void po_add_g(const PoArgs &A, const PoStore<STAGED> &R, int j0, int i, const bool (&act)[PO_NB],
                                         double (&f)[PO_NB][SP_N], double (&ps)[PO_NB], unsigned (&flags)[PO_NB])
{
#pragma unroll
    for (int c = 0; c < PO_NB; ++c) {
        if (c < A.nb && j0 + c < A.p) {   // wave-uniform
            const double gv = act[c] ? R.at(j0 + c, i) : 0.0;
            if constexpr (PLAIN) {
                ps[c] += gv;
            } else {
                double pr[1] = {gv}, er[1] = {0.0};
                SpLaneSink sink{flags[c]};
                fpe_absorb_prod<SP_N, true, 1>(f[c], pr, er, sink);
            }
        }
    }
}

// The rows of the block, one after the other, for one tile of columns (first column i0, the lane's i).  LEAD: the tile
// holds the diagonal block (i0 == j0): the pivots are made here, and a radicand that is not > 0 ends the factorisation
// (returns the pivot + 1, else 0).  Otherwise the `rows` fixed rows of the block are applied with the pivots and the
// diagonal block read from the store.  Wave-uniform.
template <bool PLAIN, bool STAGED, bool LEAD>
__device__ __forceinline__ int po_rows(const PoArgs &A, const PoStore<STAGED> &R, int j0, int i0, int i, int rows,
                                       const bool (&act)[PO_NB], double (&f)[PO_NB][SP_N], double (&ps)[PO_NB],
                                       unsigned (&flags)[PO_NB], long long *acc, unsigned long long &n_reg,
                                       unsigned long long &n_fb)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int c = 0; c < PO_NB; ++c) {
        if (c < A.nb && c < rows) {   // wave-uniform
            const int j = j0 + c;
            double v = 0.0;
            unsigned long long fbm = 0, regm = 0;
            if constexpr (PLAIN) {
                v = ps[c];
            } else {
                bool fb = false;
                if (act[c]) {
                    double rr;
                    if (!A.force && flags[c] == 0 && spmv_round_fast<SP_N>(f[c], rr)) v = rr;
                    else fb = true;
                }
                fbm = __ballot(fb);
                regm = __ballot(act[c] && !fb);
            }
            double d;
            if constexpr (LEAD) {
                // the radicand first: lane c holds it
                const unsigned long long pm = 1ull << c;
                if constexpr (!PLAIN) {
                    if (fbm & pm) {
                        const double t = po_resolve(A, R, j, j, acc);
                        if (lane == c) v = t;
                    }
                    n_reg += (regm & pm) ? 1 : 0;
                    n_fb += (fbm & pm) ? 1 : 0;
                    fbm &= ~pm, regm &= ~pm;
                }
                d = __shfl(v, c, 64);
                if (!(d > 0.0)) {
                    if (lane == c) R.at(j, j) = d;
                    return j + 1;
                }
            } else {
                d = R.at(j, j);   // the pivot itself
            }
            if constexpr (!PLAIN) {
                n_reg += __popcll(regm);
                n_fb += __popcll(fbm);
                while (fbm) {   // wave-uniform
                    const int l = __builtin_ctzll(fbm);
                    fbm &= fbm - 1ull;
                    const double t = po_resolve(A, R, j, i0 + l, acc);
                    if (lane == l) v = t;
                }
            }
            double out;
            if constexpr (LEAD) {
                const double rjj = __builtin_sqrt(d);
                out = lane == c ? rjj : v / rjj;
            } else {
                out = v / d;
            }
            if (act[c]) R.at(j, i) = out;
            // ---- the later rows of the block take their product with the fixed row ----
#pragma unroll
            for (int c2 = c + 1; c2 < PO_NB; ++c2) {
                if (c2 < A.nb && c2 < rows) {   // wave-uniform
                    double tv;
                    if constexpr (LEAD) tv = __shfl(out, c2, 64);   // r_(j, j0 + c2): lane c2 made it (or owns nothing)
                    else tv = R.at(j, j0 + c2);
                    const double a = act[c2] ? tv : 0.0, b = act[c2] ? out : 0.0;
                    if constexpr (PLAIN) {
                        ps[c2] -= a * b;
                    } else {
                        double pr[1], er[1];
                        pr[0] = two_prod(a, -b, er[0]);
                        SpLaneSink sink{flags[c2]};
                        fpe_absorb_prod<SP_N, true, 1>(f[c2], pr, er, sink);
                    }
                }
            }
            sp_wave_sync();   // the row is in the store before po_resolve reads it
        }
    }
    return 0;
}

template <bool PLAIN, bool STAGED>
__global__ void __launch_bounds__(SP_BLOCK) k_potrf(PoArgs A, double *g, int *info, long long *slots)
{
    __shared__ double tri[STAGED ? PO_TILE * PO_PITCH : 1];
    __shared__ double scr[SP_WAVES - 1][PO_NB][SP_N][64];   // the slices of the waves 1 .. 3 on their way to wave 0
    __shared__ unsigned scf[SP_WAVES - 1][PO_NB][64];
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    __shared__ int stop;   // pivot + 1 of the breakdown, else 0
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = A.p;
    const PoStore<STAGED> R{tri, g, A.rs, A.cs};
    if constexpr (!PLAIN) {
        for (int k = lane; k < NL; k += 64) acc[w][k] = 0;
    }
    if (threadIdx.x == 0) stop = 0;
    if constexpr (STAGED) {
        // the triangle, along the unit stride of G
        for (int x = threadIdx.x; x < p * p; x += SP_BLOCK) {
            const int a = x / p, b = x - a * p;
            const int k = A.rs == 1 ? b : a, i = A.rs == 1 ? a : b;
            if (k <= i) tri[k * PO_PITCH + i] = g[(long long)a * A.ldg + b];
        }
    }
    __syncthreads();

    unsigned long long n_reg = 0, n_fb = 0;
    for (int j0 = 0; j0 < p; j0 += A.nb) {   // workgroup-uniform
        double f[PO_NB][SP_N], ps[PO_NB];
        unsigned flags[PO_NB];
        bool act[PO_NB];
        // ---- tile 0: the diagonal block and the columns beside it; the waves are the slices of the earlier rows ----
        {
            const int i = j0 + lane;
#pragma unroll
            for (int c = 0; c < PO_NB; ++c) {
                ps[c] = 0.0, flags[c] = 0;
                act[c] = lane < A.tw && i < p && i >= j0 + c && c < A.nb;
#pragma unroll
                for (int t = 0; t < SP_N; ++t) f[c][t] = 0.0;
            }
            po_earlier<PLAIN, STAGED>(A, R, j0, i, w, SP_WAVES, act, f, ps, flags);
            if (w > 0) {
#pragma unroll
                for (int c = 0; c < PO_NB; ++c) {
                    if constexpr (PLAIN) {
                        scr[w - 1][c][0][lane] = ps[c];
                    } else {
#pragma unroll
                        for (int t = 0; t < SP_N; ++t) scr[w - 1][c][t][lane] = f[c][t];
                        scf[w - 1][c][lane] = flags[c];
                    }
                }
            }
            __syncthreads();
            if (w == 0) {
                for (int s = 1; s < SP_WAVES; ++s) {
#pragma unroll
                    for (int c = 0; c < PO_NB; ++c) {
                        if (c < A.nb && j0 + c < p) {   // wave-uniform
                            if constexpr (PLAIN) {
                                ps[c] += scr[s - 1][c][0][lane];
                            } else {
                                double q[SP_N];
#pragma unroll
                                for (int t = 0; t < SP_N; ++t) q[t] = scr[s - 1][c][t][lane];
                                flags[c] |= scf[s - 1][c][lane];
                                SpLaneSink sink{flags[c]};
                                fpe_cascade<SP_N, true, SP_N>(f[c], q, 0, sink);
                            }
                        }
                    }
                }
                po_add_g<PLAIN, STAGED>(A, R, j0, i, act, f, ps, flags);
                const int st = po_rows<PLAIN, STAGED, true>(A, R, j0, j0, i, min(A.nb, p - j0), act, f, ps, flags, acc[0],
                                                            n_reg, n_fb);
                if (st && lane == 0) stop = st;
            }
            __syncthreads();   // the rows of the block, tile 0, are in the store (block-scope fence included)
        }
        const int st = stop, rows = st ? st - 1 - j0 : min(A.nb, p - j0);
        // ---- the tiles beyond: a tile per wave, unsliced ----
        for (int i0 = j0 + (1 + w) * A.tw; i0 < p && rows > 0; i0 += SP_WAVES * A.tw) {   // wave-uniform
            const int i = i0 + lane;
#pragma unroll
            for (int c = 0; c < PO_NB; ++c) {
                ps[c] = 0.0, flags[c] = 0;
                act[c] = lane < A.tw && i < p && c < rows;
#pragma unroll
                for (int t = 0; t < SP_N; ++t) f[c][t] = 0.0;
            }
            // (act[0] is the widest here too: rows > 0)
            po_earlier<PLAIN, STAGED>(A, R, j0, i, 0, 1, act, f, ps, flags);
            po_add_g<PLAIN, STAGED>(A, R, j0, i, act, f, ps, flags);
            po_rows<PLAIN, STAGED, false>(A, R, j0, i0, i, rows, act, f, ps, flags, acc[w], n_reg, n_fb);
        }
        __syncthreads();   // every row of the block is fixed before the next block reads it
        if (st) break;
    }

    const int st = stop;
    if constexpr (STAGED) {
        // what was fixed goes back along the unit stride: the rows before the breakdown, and its pivot
        const int nfix = st ? st - 1 : p;
        for (int x = threadIdx.x; x < p * p; x += SP_BLOCK) {
            const int a = x / p, b = x - a * p;
            const int k = A.rs == 1 ? b : a, i = A.rs == 1 ? a : b;
            if (k <= i && (k < nfix || (k == i && k == nfix))) g[(long long)a * A.ldg + b] = tri[k * PO_PITCH + i];
        }
    }
    // the counters and the info word: plain stores, nothing to clear beforehand
    blk_store_counters(cnt, n_reg, n_fb, slots, 0);
    if (threadIdx.x == 64) info[0] = st;
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain factorisation, 2..8 the expansions (the caller refused
// the rest and p > EXBLAS_BTRSM_MAX_P)
hipError_t expotrf_dispatch(Ctx &c, char uplo, int p, double *g, int ldg, int *info, int fpe, int early_exit, int round_mode,
                            hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.potrf_slots = SlotInfo();
    if (p == 0) return hipSuccess;
    const int path = c.potrf_path;
    const bool lower = (uplo == 'L' || uplo == 'l');
    PoArgs A;
    A.p = p, A.ldg = ldg;
    A.rs = lower ? (long long)ldg : 1ll, A.cs = lower ? 1ll : (long long)ldg;
    A.nb = path == 2 ? 1 : PO_NB;
    A.tw = path == 3 ? PO_SMALL : PO_TILE;
    const StRule rule = st_rule(fpe, path, round_mode);
    A.force = rule.force_fb, A.round_mode = rule.round_mode;
    const bool staged = path != 3 && p <= PO_TILE;
    hipError_t e = hipSuccess;
    long long *slots = blk_reserve_slots(c, c.potrf_slots, 1, st, &e);
    if (!slots) return e;
    if (fpe == 1) {
        if (staged) hipLaunchKernelGGL((k_potrf<true, true>), dim3(1), dim3(SP_BLOCK), 0, st, A, g, info, slots);
        else hipLaunchKernelGGL((k_potrf<true, false>), dim3(1), dim3(SP_BLOCK), 0, st, A, g, info, slots);
    } else {
        if (staged) hipLaunchKernelGGL((k_potrf<false, true>), dim3(1), dim3(SP_BLOCK), 0, st, A, g, info, slots);
        else hipLaunchKernelGGL((k_potrf<false, false>), dim3(1), dim3(SP_BLOCK), 0, st, A, g, info, slots);
    }
    return hipGetLastError();
}

}  // namespace exb
