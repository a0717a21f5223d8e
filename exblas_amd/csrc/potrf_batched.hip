// potrf_batched.hip -- batched ExPOTRF for gfx950: the exact-sum Cholesky factorisation of `batch` independent small symmetric
// positive definite matrices (the diagonal blocks of a block-Jacobi preconditioner), each in place on its p x p column-major
// triangle at g + b * stride, p <= EXBLAS_POTRF_BATCHED_MAX_P.
//
// Contract: matrix b is factored exactly as potrf.hip defines for one matrix (row by row, every sum exact over the already
// fixed doubles and rounded once, then ONE square root or ONE IEEE division; LAPACK's breakdown rule per matrix, its info
// word written by every launch).  Every path sums the same multiset exactly, so the bits of a matrix depend on its data, uplo
// and the rounding mode only: not on the batch, its place in it, its neighbours, ldg, stride or the path.
//
// Structure: the frame of block_common.hip.h (one kernel, certify in registers or settle through the wave's accumulator, the
// counter slots, the plain kernel of fpe == 1).  What is this routine's own:
//   * ONE WAVE WALKS A MATRIX: no workgroup barrier in the pivot chain, no slices.  The four waves of a workgroup carry four
//     independent chains; a workgroup item is four wave items (one on path 3), the items go to workgroups by blk_partition.
//   * Packing: with pw = p rounded up to a power of two, a wave carries G = 64 / pw matrices (1 on the paths 2 and 3); lane
//     = (matrix gi, column i).  The triangles are staged in the wave's own LDS along the unit stride of G (row pitch p | 1:
//     odd), factored there and stored back once, the fixed entries only.
//   * Left-looking, one row at a time: lane (gi, i) sums row j of its matrix over the earlier rows in a 4-term expansion,
//     certifies, the radicand is shuffled from the group's diagonal lane, every lane takes its square root, divides.
//   * A group whose radicand is not > 0 stores it, notes j + 1 and idles to the end of the wave's chain; so does a group past
//     the end of the batch.
//   * The fall-back is wave-uniform: one output at a time through the wave's one accumulator (blk_resolve), over the ballot
//     across all groups; the radicands are settled before the rest of their rows is counted.
//   * fpe == 1: s = g_ji, then s -= r_kj * r_ki for k ascending, in fp64.
// Host side: the argument struct and the plan are BjfArgs and bjf_plan of block_common.hip.h, shared with getrf_batched.hip.
#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int PB_U = 4;   // earlier rows per step of the inner loop

// What no lane could certify: Round(g_ji - sum_{k<j} r_kj r_ki) of the staged matrix M through the wave's accumulator.
// (j, i) still holds g_ji.  Wave-uniform; every lane gets the value.
__device__ double pb_resolve(const double *M, int pitch, int j, int i, int round_mode, long long *acc)
{
    const double v = blk_resolve(
        acc, j, round_mode, [&](int k, double &a, double &b) { a = M[k * pitch + j], b = -M[k * pitch + i]; },
        [&](RowSink &sink) { sink.add(M[j * pitch + i]); });
    sp_wave_sync();
    return v;
}

// the wave's G triangles between global memory and LDS, along the unit stride of G.  STORE: only what was fixed goes back
// (the rows before a breakdown and its pivot)
template <bool STORE>
__device__ __forceinline__ void pb_move(const BjfArgs &A, double *g, double *tri, long long m0, const int *stop)
{
    const int lane = threadIdx.x & 63, p = A.p, pp = p * p, pitch = p | 1, msz = p * pitch;
    for (int x = lane; x < A.G * pp; x += 64) {
        const int gg = x / pp, r = x - gg * pp, a = r / p, b = r - a * p;
        const int k = A.hirow ? a : b, c = A.hirow ? b : a;   // hirow: 'L'
        if (m0 + gg >= A.batch || k > c) continue;
        double *at = g + (m0 + gg) * A.stride + (long long)a * A.ld + b;
        if constexpr (STORE) {
            const int st = stop[gg], nfix = st ? st - 1 : p;
            if (k < nfix || (k == c && k == nfix)) *at = tri[gg * msz + k * pitch + c];
        } else {
            tri[gg * msz + k * pitch + c] = *at;
        }
    }
}

template <bool PLAIN>
__global__ void __launch_bounds__(SP_BLOCK) k_potrf_batched(BjfArgs A, double *g, int *info, long long *slots)
{
    extern __shared__ double pb_lds[];   // SP_WAVES x tsz: the waves' triangles
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    __shared__ int stop[SP_WAVES][64];   // per group: pivot + 1 of its breakdown, else 0
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = A.p, pitch = p | 1, msz = p * pitch;
    const int pw = 1 << A.lgpw, gi = lane >> A.lgpw, i = lane & (pw - 1), base = gi << A.lgpw;
    double *tri = pb_lds + (size_t)w * A.tsz, *mine = tri + gi * msz;
    if constexpr (!PLAIN) {
        for (int k = lane; k < NL; k += 64) acc[w][k] = 0;
    }
    unsigned long long n_reg = 0, n_fb = 0;
    const long long t1 = min(((long long)blockIdx.x + 1) * A.per, A.nitems);
    for (long long t = (long long)blockIdx.x * A.per; t < t1; ++t) {   // workgroup-uniform
        const long long m0 = (t * A.wpi + w) * A.G;   // the wave's first matrix
        if (w >= A.wpi || m0 >= A.batch) continue;    // wave-uniform
        const bool owns = gi < A.G && m0 + gi < A.batch;
        stop[w][lane] = 0;
        pb_move<false>(A, g, tri, m0, stop[w]);
        sp_wave_sync();
        bool alive = owns;
        int st = 0;
        for (int j = 0; j < p && __any(alive); ++j) {   // wave-uniform
            const bool act = alive && i >= j && i < p, dg = i == j;
            double f[SP_N], ps = act ? mine[j * pitch + i] : 0.0;
            unsigned flags = 0;
#pragma unroll
            for (int t4 = 0; t4 < SP_N; ++t4) f[t4] = 0.0;
            for (int k0 = 0; k0 < j; k0 += PB_U) {
                double pr[PB_U], er[PB_U];
#pragma unroll
                for (int u = 0; u < PB_U; ++u) {
                    const bool ok = act && k0 + u < j;
                    const double tv = ok ? mine[(k0 + u) * pitch + j] : 0.0, x = ok ? mine[(k0 + u) * pitch + i] : 0.0;
                    if constexpr (PLAIN) {
                        ps -= tv * x;
                        pr[u] = er[u] = 0.0;
                    } else {
                        pr[u] = two_prod(tv, -x, er[u]);
                    }
                }
                if constexpr (!PLAIN) {
                    SpLaneSink sink{flags};
                    fpe_absorb_prod<SP_N, true, PB_U>(f, pr, er, sink);
                }
            }
            double v = ps;
            bool fb = false;
            if constexpr (!PLAIN) {
                double pr[1] = {ps}, er[1] = {0.0};   // g_ji joins the lane's sum
                SpLaneSink sink{flags};
                fpe_absorb_prod<SP_N, true, 1>(f, pr, er, sink);
                v = 0.0;
                if (act) {
                    double rr;
                    if (!A.force && flags == 0 && spmv_round_fast<SP_N>(f, rr)) v = rr;
                    else fb = true;
                }
                // the radicands first: the diagonal lane of every group holds one
                const unsigned long long dm = __ballot(act && dg);
                unsigned long long dfb = __ballot(act && dg && fb);
                n_reg += __popcll(dm & ~dfb);
                n_fb += __popcll(dfb);
                while (dfb) {   // wave-uniform
                    const int l = __builtin_ctzll(dfb);
                    dfb &= dfb - 1ull;
                    const double tt = pb_resolve(tri + (l >> A.lgpw) * msz, pitch, j, j, A.round_mode, acc[w]);
                    if (lane == l) v = tt;
                }
            }
            const double d = __shfl(v, base + j, 64);   // the group's radicand
            if (alive && !(d > 0.0)) {
                if (act && dg) mine[j * pitch + j] = d;
                st = j + 1;
                alive = false;
            }
            const bool go = act && alive;
            if constexpr (!PLAIN) {
                const unsigned long long om = __ballot(go && !dg);
                unsigned long long ofb = __ballot(go && !dg && fb);
                n_reg += __popcll(om & ~ofb);
                n_fb += __popcll(ofb);
                while (ofb) {   // wave-uniform
                    const int l = __builtin_ctzll(ofb);
                    ofb &= ofb - 1ull;
                    const double tt = pb_resolve(tri + (l >> A.lgpw) * msz, pitch, j, l & (pw - 1), A.round_mode, acc[w]);
                    if (lane == l) v = tt;
                }
            }
            const double rjj = __builtin_sqrt(d);
            if (go) mine[j * pitch + i] = dg ? rjj : v / rjj;
            sp_wave_sync();   // the row is in the triangle before the next row, and pb_resolve, read it
        }
        if (owns && i == 0) {
            stop[w][gi] = st;
            info[m0 + gi] = st;
        }
        sp_wave_sync();
        pb_move<true>(A, g, tri, m0, stop[w]);
        sp_wave_sync();   // the triangles are out before the next item's come in
    }
    blk_store_counters(cnt, n_reg, n_fb, slots, blockIdx.x);
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain factorisation, 2..8 the expansions (the caller refused the
// rest and p > EXBLAS_POTRF_BATCHED_MAX_P)
hipError_t expotrf_batched_dispatch(Ctx &c, char uplo, int p, long long batch, double *g, int ldg, long long stride, int *info,
                                    int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.potrf_batched_slots = SlotInfo();
    if (p == 0 || batch == 0) return hipSuccess;
    BjfArgs A;
    const bool lower = uplo == 'L' || uplo == 'l';
    const BlkPartition P = bjf_plan(c, A, c.potrf_batched_path, p, batch, ldg, stride, lower, fpe, round_mode);
    static std::atomic<unsigned long long> optin{0};
    hipError_t e = blk_lds_optin(optin, c.device, BJF_LDS,
                                 {(const void *)k_potrf_batched<true>, (const void *)k_potrf_batched<false>});
    if (e != hipSuccess) return e;
    long long *slots = blk_reserve_slots(c, c.potrf_batched_slots, P.grid, st, &e);
    if (!slots) return e;
    const size_t lds = (size_t)SP_WAVES * A.tsz * sizeof(double);
    if (fpe == 1) hipLaunchKernelGGL((k_potrf_batched<true>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, g, info, slots);
    else hipLaunchKernelGGL((k_potrf_batched<false>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, g, info, slots);
    return hipGetLastError();
}

}  // namespace exb
