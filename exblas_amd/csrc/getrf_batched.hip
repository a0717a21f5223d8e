// getrf_batched.hip -- batched ExGETRF for gfx950: the exact-sum LU factorisation with partial pivoting of `batch` independent
// small general matrices (the diagonal blocks of a block-Jacobi preconditioner of a nonsymmetric or indefinite operator),
// each in place on its p x p matrix at a + b * stride, p <= EXBLAS_GETRF_BATCHED_MAX_P, column- or row-major (`order`).
//
// Contract (include/exblas_hip.h): the compact Doolittle LU, step j = 0 .. p - 1 on the working matrix W:
//   candidates  c_i = Round(w_ij - sum_{k<j} l_ik u_kj), i >= j      (exact sum over the already fixed doubles, rounded once)
//   pivot       the smallest i >= j with the largest |c_i| (a NaN ranks above +Inf), ipiv[j] = piv + 1
//   breakdown   c_piv zero or NaN: the candidates are stored, no swap, ipiv[i] = i + 1 for i >= j, info = j + 1, the rest of
//               the matrix stays as it is and the matrix idles
//   column of L rows j and piv swapped whole, u_jj = c_piv, l_ij = fl(c_i / u_jj): ONE IEEE division
//   row of U    u_ji = Round(w_ji - sum_{k<j} l_jk u_ki), i > j
// Every path sums the same multiset exactly, so the bits of a matrix depend on its data and the rounding mode only: not on the
// batch, its place in it, its neighbours, order, lda, stride or the path.
//
// Structure: the frame of block_common.hip.h, on the pattern of potrf_batched.hip.  What is this routine's own:
//   * ONE WAVE WALKS A MATRIX: no workgroup barrier in the pivot chain.  With pw = p rounded up to a power of two a wave
//     carries G = 64 / pw matrices (1 on the paths 2 and 3); lane = (matrix gi, index i).
//   * The whole matrix is staged ROW-wise in the wave's own LDS (row pitch p | 1: odd), whatever `order` is, factored there
//     and stored back once, with ipiv and info.
//   * A step has two certify / ballot / blk_resolve rounds: lane i is ROW i for the candidates (it walks its row of L against
//     column j of U) and COLUMN i for the row of U (row j of L against its column of U).
//   * The pivot is found by xor shuffles inside the lane group, carrying (rank of |c|, index), the first index winning.
//   * The rows are swapped in LDS, each lane its own column; the candidates are in the matrix by then and move with them.
//   * A group that breaks down stores its candidates, notes j + 1 and idles to the end of the wave's chain; so does a group
//     past the end of the batch.
//   * fpe == 1: s = w, then s -= l * u for k ascending, in fp64.
// Host side: the argument struct and the plan are BjfArgs and bjf_plan of block_common.hip.h, shared with potrf_batched.hip.
#include "../../include/exblas_hip.h"
#include "block_common.hip.h"

namespace exb {
namespace {

constexpr int GF_U = 4;   // earlier steps per pass of the inner loop

// What no lane could certify: Round(w_rc - sum_{k<j} l_rk u_kc) of the staged matrix M through the wave's accumulator.
// (r, c) still holds w_rc.  Wave-uniform; every lane gets the value.
__device__ double gf_resolve(const double *M, int pitch, int j, int r, int c, int round_mode, long long *acc)
{
    const double v = blk_resolve(
        acc, j, round_mode, [&](int k, double &a, double &b) { a = M[r * pitch + k], b = -M[k * pitch + c]; },
        [&](RowSink &sink) { sink.add(M[r * pitch + c]); });
    sp_wave_sync();
    return v;
}

// the wave's G matrices between global memory and LDS, along the unit stride of `order`
template <bool STORE>
__device__ __forceinline__ void gf_move(const BjfArgs &A, double *a, double *mat, long long m0)
{
    const int lane = threadIdx.x & 63, p = A.p, pp = p * p, pitch = p | 1, msz = p * pitch;
    for (int x = lane; x < A.G * pp; x += 64) {
        const int gg = x / pp, q = x - gg * pp, hi = q / p, lo = q - hi * p;
        const int r = A.hirow ? hi : lo, c = A.hirow ? lo : hi;   // hirow: row-major
        if (m0 + gg >= A.batch) continue;
        double *at = a + (m0 + gg) * A.stride + (long long)hi * A.ld + lo;
        if constexpr (STORE) *at = mat[gg * msz + r * pitch + c];
        else mat[gg * msz + r * pitch + c] = *at;
    }
}

// the rank of a candidate in the pivot search: 0 for a lane that holds none, else 1 + the bits of |c| (a NaN above +Inf)
__device__ __forceinline__ unsigned long long gf_rank(bool act, double c)
{
    if (!act) return 0ull;
    if (c != c) return 0x7ff8000000000001ull;
    return (unsigned long long)__double_as_longlong(__builtin_fabs(c)) + 1ull;
}

template <bool PLAIN>
__global__ void __launch_bounds__(SP_BLOCK) k_getrf_batched(BjfArgs A, double *a, int *ipiv, int *info, long long *slots)
{
    extern __shared__ double gf_lds[];   // SP_WAVES x tsz: the waves' matrices
    __shared__ long long acc[SP_WAVES][NL];
    __shared__ unsigned long long cnt[SP_WAVES][2];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, p = A.p, pitch = p | 1, msz = p * pitch;
    const int pw = 1 << A.lgpw, gi = lane >> A.lgpw, i = lane & (pw - 1), base = gi << A.lgpw;
    double *mat = gf_lds + (size_t)w * A.tsz, *mine = mat + gi * msz;
    if constexpr (!PLAIN) {
        for (int k = lane; k < NL; k += 64) acc[w][k] = 0;
    }
    unsigned long long n_reg = 0, n_fb = 0;
    const long long t1 = min(((long long)blockIdx.x + 1) * A.per, A.nitems);
    for (long long t = (long long)blockIdx.x * A.per; t < t1; ++t) {   // workgroup-uniform
        const long long m0 = (t * A.wpi + w) * A.G;   // the wave's first matrix
        if (w >= A.wpi || m0 >= A.batch) continue;    // wave-uniform
        const bool owns = gi < A.G && m0 + gi < A.batch && i < p;
        gf_move<false>(A, a, mat, m0);
        sp_wave_sync();
        bool alive = owns;
        int st = 0, piv_mine = i + 1;   // lane i keeps ipiv[i]
        for (int j = 0; j < p && __any(alive); ++j) {   // wave-uniform
            // two rounds over one body: rd 0 the candidates of column j (lane i is row i), then the pivot and the swap;
            // rd 1 the row of U (lane i is column i)
            double v = 0.0;
            int piv = j;
            for (int rd = 0; rd < 2; ++rd) {   // wave-uniform
                const bool act = alive && (rd ? i > j : i >= j);
                // the output is (rr, cc): k walks along row rr of L and down column cc of U
                const int rr = rd ? j : i, cc = rd ? i : j;
                double f[SP_N], ps = act ? mine[rr * pitch + cc] : 0.0;
                unsigned flags = 0;
#pragma unroll
                for (int t4 = 0; t4 < SP_N; ++t4) f[t4] = 0.0;
                for (int k0 = 0; k0 < j; k0 += GF_U) {
                    double pr[GF_U], er[GF_U];
#pragma unroll
                    for (int u = 0; u < GF_U; ++u) {
                        const bool ok = act && k0 + u < j;
                        const double lv = ok ? mine[rr * pitch + k0 + u] : 0.0, uv = ok ? mine[(k0 + u) * pitch + cc] : 0.0;
                        if constexpr (PLAIN) {
                            ps -= lv * uv;
                            pr[u] = er[u] = 0.0;
                        } else {
                            pr[u] = two_prod(lv, -uv, er[u]);
                        }
                    }
                    if constexpr (!PLAIN) {
                        SpLaneSink sink{flags};
                        fpe_absorb_prod<SP_N, true, GF_U>(f, pr, er, sink);
                    }
                }
                v = ps;
                if constexpr (!PLAIN) {
                    double pr[1] = {ps}, er[1] = {0.0};   // w joins the lane's sum
                    SpLaneSink sink{flags};
                    fpe_absorb_prod<SP_N, true, 1>(f, pr, er, sink);
                    bool fb = false;
                    v = 0.0;
                    if (act) {
                        double r1;
                        if (!A.force && flags == 0 && spmv_round_fast<SP_N>(f, r1)) v = r1;
                        else fb = true;
                    }
                    const unsigned long long om = __ballot(act);
                    unsigned long long fbm = __ballot(fb);
                    n_reg += __popcll(om & ~fbm);
                    n_fb += __popcll(fbm);
                    while (fbm) {   // wave-uniform
                        const int l = __builtin_ctzll(fbm);
                        fbm &= fbm - 1ull;
                        const int li = l & (pw - 1);
                        const double tt = gf_resolve(mat + (l >> A.lgpw) * msz, pitch, j, rd ? j : li, rd ? li : j,
                                                     A.round_mode, acc[w]);
                        if (lane == l) v = tt;
                    }
                }
                if (act) mine[rr * pitch + cc] = v;   // the candidate (the rows move with it), or u_ji
                if (rd) break;
                // ---- the pivot: (rank, index) through the lane group, the first index winning ----
                unsigned long long rk = gf_rank(act, v);
                int ix = i;
                for (int d = pw >> 1; d > 0; d >>= 1) {
                    const unsigned long long ork = __shfl_xor(rk, d, 64);
                    const int oix = __shfl_xor(ix, d, 64);
                    if (ork > rk || (ork == rk && oix < ix)) rk = ork, ix = oix;
                }
                const double cp = __shfl(v, base + (ix & (pw - 1)), 64);   // the group's pivot candidate
                if (alive) {
                    if (cp == 0.0 || cp != cp) {   // breakdown: no swap, the identity from here on
                        st = j + 1;
                        alive = false;
                        if (i >= j) piv_mine = i + 1;
                    } else {
                        piv = ix;
                        if (i == j) piv_mine = piv + 1;
                    }
                }
                sp_wave_sync();   // the candidates are in the matrix
                if (alive && piv != j) {   // rows j and piv, each lane its own column
                    const double tj = mine[j * pitch + i], tp = mine[piv * pitch + i];
                    mine[j * pitch + i] = tp, mine[piv * pitch + i] = tj;
                }
                sp_wave_sync();
            }
            // ---- the column of L: one division; nothing of this step reads it ----
            if (alive && i > j) mine[i * pitch + j] = mine[i * pitch + j] / mine[j * pitch + j];
            sp_wave_sync();   // the step is in the matrix before the next one, and gf_resolve, read it
        }
        if (owns) {
            ipiv[(m0 + gi) * p + i] = piv_mine;
            if (i == 0) info[m0 + gi] = st;
        }
        gf_move<true>(A, a, mat, m0);
        sp_wave_sync();   // the matrices are out before the next item's come in
    }
    blk_store_counters(cnt, n_reg, n_fb, slots, blockIdx.x);
}

}  // namespace

// fpe: 0 every output from the integer accumulator, 1 the plain factorisation, 2..8 the expansions (the caller refused the
// rest and p > EXBLAS_GETRF_BATCHED_MAX_P)
hipError_t exgetrf_batched_dispatch(Ctx &c, char order, int p, long long batch, double *a, int lda, long long stride, int *ipiv,
                                    int *info, int fpe, int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    c.getrf_batched_slots = SlotInfo();
    if (p == 0 || batch == 0) return hipSuccess;
    BjfArgs A;
    const bool rowmajor = order == 'R' || order == 'r';
    const BlkPartition P = bjf_plan(c, A, c.getrf_batched_path, p, batch, lda, stride, rowmajor, fpe, round_mode);
    static std::atomic<unsigned long long> optin{0};
    hipError_t e = blk_lds_optin(optin, c.device, BJF_LDS,
                                 {(const void *)k_getrf_batched<true>, (const void *)k_getrf_batched<false>});
    if (e != hipSuccess) return e;
    long long *slots = blk_reserve_slots(c, c.getrf_batched_slots, P.grid, st, &e);
    if (!slots) return e;
    const size_t lds = (size_t)SP_WAVES * A.tsz * sizeof(double);
    if (fpe == 1) hipLaunchKernelGGL((k_getrf_batched<true>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, a, ipiv, info, slots);
    else hipLaunchKernelGGL((k_getrf_batched<false>), dim3(P.grid), dim3(SP_BLOCK), lds, st, A, a, ipiv, info, slots);
    return hipGetLastError();
}

}  // namespace exb
