// spmv.hip -- ExSpMV for gfx950: exact, reproducible y = alpha A x + beta y with A in CSR (int32 or int64 indices).
//
// Contract: row i is what ExGEMV 'N' computes for the 1 x k_i matrix of its stored values against the gathered x,
//   y_i = Round( sum_p val[p] * fl(alpha * x[col[p]])  (+)  beta * y_i )
// with ExGEMV's alpha / beta / product-domain rules (blas2.hip: k_gemvN_fpe, k_gemv_finish).  Every path below sums
// the same multiset of doubles {p, e} (TwoProd of every stored product, the beta terms) exactly and rounds it once,
// so the bits depend on nothing but the data.
//
// Structure (all classification on the device, no host synchronisation, workspace from the context):
//   k_spmv_classify   one thread per row: short rows (<= SP_SHORT_MAX entries) stay where they are; medium rows are
//                     appended to a list (wave-aggregated atomics); long rows (> SP_LONG_MIN) get a global accumulator
//                     slot, which the classifier zeroes
//   k_spmv_rows<8>    short rows in natural order, 8 lanes per row: TwoProd + FPE cascade per lane, exact tree merge of
//                     the 8 expansions, then a certified in-register rounding test (spmv_round_fast); rows the test
//                     cannot decide fall back to the row's LDS accumulator and finish_wave
//   k_spmv_rows<64>   medium rows from the list, one wave per row, same finish
//   k_spmv_long_prep  one workgroup: chunk counts of the long rows -> exclusive scan (chunk bases)
//   k_spmv_long       one wave per chunk of SP_CHUNK entries: expansions + spills -> LDS -> integer atomics into the
//                     row's global accumulator (order-free)
//   k_spmv_long_finish one wave per long row: beta terms, finish_wave, store
// fpe == 1 runs the same structure with plain fp64 sums (the non-reproducible baseline).
//
// Narrow entries (exspmv_lp_dispatch): the kernels are templates on VT, the element type of the values, and XT, that of
// x and y (lowp_types.hip.h); <LpF64, LpF64> is the fp64 routine.  A narrow element is loaded at its own width and
// widened exactly, so the multiset {p, e} is the one of the fp64 entry on the widened operands (e = 0 when both factors
// are narrow).  A narrow y is rounded ONCE from that exact sum: in registers behind the interval certificate
// (sp_round_fast_to), or from the accumulator's digits (sp_pick_to) -- never from the rounded double.
#include "spmv_common.hip.h"

namespace exb {

// ---------------------------------------------------------------------------------------------
// classification
// ---------------------------------------------------------------------------------------------
template <class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmv_classify(int m, const I *__restrict__ rp, long long short_max,
                                                           long long long_min, int lcap, long long *__restrict__ hdr,
                                                           int *__restrict__ med, int *__restrict__ lrows,
                                                           long long *__restrict__ lacc)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    long long len = 0;
    if (i < m) len = max(0ll, (long long)rp[i + 1] - (long long)rp[i]);
    bool is_med = i < m && len > short_max && len <= long_min;
    if (i < m && len > short_max && len > long_min) {
        const long long slot = (long long)atomicAdd((unsigned long long *)&hdr[1], 1ull);
        if (slot < lcap) {
            lrows[slot] = i;
            long long *a = lacc + slot * SET_WORDS;
            for (int t = 0; t < SET_WORDS; ++t) a[t] = 0;
        } else {
            is_med = true;   // out of slots: the row runs whole (same bits)
        }
    }
    const unsigned long long mask = __ballot(is_med);
    if (mask) {
        const int leader = __builtin_ctzll(mask);
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd((unsigned long long *)&hdr[0], (unsigned long long)__popcll(mask));
        base = (unsigned long long)lane_bcast((long long)base, leader);
        if (is_med) med[base + __popcll(mask & ((1ull << lane) - 1ull))] = i;
    }
}

// ---------------------------------------------------------------------------------------------
// one row per group of G lanes (8 short, 64 medium); persistent waves over batches of 64 / G rows
// ---------------------------------------------------------------------------------------------
template <int G, bool LIST, bool PLAIN, class VT, class XT, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmv_rows(int m, int n, const I *__restrict__ rp, const I *__restrict__ ci,
                                                       const typename VT::elem *__restrict__ val, double alpha,
                                                       const typename XT::elem *__restrict__ x, double beta,
                                                       typename XT::elem *__restrict__ y, long long short_max, const int *__restrict__ list,
                                                       long long *__restrict__ hdr, int force_fb, int round_mode)
{
    constexpr int RPW = 64 / G;   // rows per wave and batch
    constexpr int U = G >= 64 ? 4 : 2;
    __shared__ long long acc[SP_WAVES][RPW][NL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, slot = lane / G, sub = lane % G;
    if constexpr (!PLAIN) {
        for (int t = lane; t < RPW * NL; t += 64) (&acc[w][0][0])[t] = 0;
    }
    const long long count = LIST ? hdr[0] : (long long)m;
    const long long nbatch = (count + RPW - 1) / RPW;
    const long long wave0 = (long long)blockIdx.x * SP_WAVES + w, nwaves = (long long)gridDim.x * SP_WAVES;
    unsigned long long n_reg = 0, n_fb = 0;
    for (long long b = wave0; b < nbatch; b += nwaves) {
        const long long e = b * RPW + slot;
        long long row = -1;
        if (e < count) row = LIST ? (long long)list[e] : e;
        long long p0 = 0, p1 = 0;
        if (row >= 0) {
            p0 = (long long)rp[row];
            p1 = max(p0, (long long)rp[row + 1]);
            if (!LIST && p1 - p0 > short_max) row = -1;   // medium / long rows: other kernels
        }
        const bool valid = row >= 0;
        if (!valid) p1 = p0;
        unsigned flags = 0;
        if constexpr (PLAIN) {
            double s = 0.0;
            for (long long k = p0 + sub; k < p1; k += G) {
                const I c = ld_nt(ci + k);
                const double v = ld_nt(val + k);
                s += v * gather_x<XT>(x, c, n, alpha, flags);
            }
            if (flags & FLAG_NAN) s = __builtin_nan("");
#pragma unroll
            for (int o = G / 2; o > 0; o >>= 1) s += __shfl_down(s, o, G);
            if (valid && sub == 0) y[row] = (beta == 0.0) ? s : s + beta * y[row];
        } else {
            RowSink sink{acc[w][slot], flags};
            double f[SP_N];
#pragma unroll
            for (int i = 0; i < SP_N; ++i) f[i] = 0.0;
            for (long long k0 = p0; k0 < p1; k0 += (long long)G * U) {
                double p[U], er[U];
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const long long k = k0 + sub + (long long)j * G;
                    double a = 0.0, xv = 0.0;
                    if (k < p1) {
                        const I c = ld_nt(ci + k);
                        a = VT::widen(ld_nt(val + k));
                        xv = gather_x<XT>(x, c, n, alpha, flags);
                    }
                    p[j] = two_prod(a, xv, er[j]);
                }
                fpe_absorb_prod<SP_N, true, U>(f, p, er, sink);
            }
            sp_absorb_beta<XT>(f, valid && sub == 0, beta, y, row, sink);
            // exact tree merge of the group's expansions into its first lane
#pragma unroll
            for (int s = 1; s < G; s <<= 1) sp_cascade_step(f, flags, s, (sub & (2 * s - 1)) == 0, sink);
            const bool leader = valid && sub == 0;
            bool fb = false;
            if (leader) {
                if constexpr (XT::DT == DT_F64) {   // (the fp64 kernel's own lines, here and below: its code stays what it was)
                    double r;
                    fb = !sp_certify_or_spill(f, flags, force_fb, acc[w][slot], r);
                    if (!fb) y[row] = r;
                } else {
                    unsigned long long r;
                    fb = !sp_certify_or_spill_to<XT>(f, flags, force_fb, acc[w][slot], r);
                    if (!fb) XT::store(y + row, r);
                }
            }
            n_reg += __popcll(__ballot(leader && !fb));
            unsigned long long fbm = __ballot(fb);
            n_fb += __popcll(fbm);
            if (fbm) {
                sp_wave_sync();
                while (fbm) {   // wave-uniform: every lane runs the finish of each falling-back row
                    const int l = __builtin_ctzll(fbm), sl = l / G;
                    fbm &= fbm - 1ull;
                    const unsigned fl = (unsigned)__shfl((int)flags, l, 64) & FLAG_NONFINITE;
                    const long long r_row = __shfl(row, l, 64);
                    if constexpr (XT::DT == DT_F64) {
                        const double v = sp_acc_round(acc[w][sl], fl, round_mode);
                        if (lane == 0) y[r_row] = v;
                    } else {
                        const unsigned long long v = sp_acc_round_to<XT>(acc[w][sl], fl, round_mode);
                        if (lane == 0) XT::store(y + r_row, v);
                    }
                    sp_wave_sync();
                }
            }
        }
    }
    if constexpr (!PLAIN) {
        if (lane == 0 && n_reg) atomicAdd((unsigned long long *)&hdr[4], n_reg);
        if (lane == 0 && n_fb) atomicAdd((unsigned long long *)&hdr[5], n_fb);
    }
}

// ---------------------------------------------------------------------------------------------
// long rows: chunks, finish (the chunk bases come from k_spmv_long_prep, spmv_common.hip.h)
// ---------------------------------------------------------------------------------------------
template <bool PLAIN, class VT, class XT, class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spmv_long(int n, const I *__restrict__ rp, const I *__restrict__ ci,
                                                       const typename VT::elem *__restrict__ val, double alpha,
                                                       const typename XT::elem *__restrict__ x,
                                                       const int *__restrict__ lrows,
                                                       const long long *__restrict__ lbase, int lcap, long long chunk,
                                                       long long *__restrict__ hdr, long long *__restrict__ lacc)
{
    constexpr int U = 4;
    __shared__ long long acc[SP_WAVES][NL];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long nl = min(hdr[1], (long long)lcap), total = hdr[2];
    if constexpr (!PLAIN) {
        for (int t = lane; t < NL; t += 64) acc[w][t] = 0;
    }
    const long long wave0 = (long long)blockIdx.x * SP_WAVES + w, nwaves = (long long)gridDim.x * SP_WAVES;
    unsigned long long n_chunks = 0;
    for (long long t = wave0; t < total; t += nwaves) {
        const long long lo = sp_chunk_owner(lbase, nl, t);
        const int row = lrows[lo];
        const long long r0 = (long long)rp[row], r1 = max(r0, (long long)rp[row + 1]);
        const long long p0 = r0 + (t - lbase[lo]) * chunk, p1 = min(r1, p0 + chunk);
        long long *g = lacc + lo * SET_WORDS;
        unsigned flags = 0;
        ++n_chunks;
        if constexpr (PLAIN) {
            double s = 0.0;
            for (long long k = p0 + lane; k < p1; k += 64) s += ld_nt(val + k) * gather_x<XT>(x, ld_nt(ci + k), n, alpha, flags);
            if (flags & FLAG_NAN) s = __builtin_nan("");
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
            if (lane == 0) atomicAdd((double *)g, s);
        } else {
            RowSink sink{acc[w], flags};
            double f[SP_N];
#pragma unroll
            for (int i = 0; i < SP_N; ++i) f[i] = 0.0;
            for (long long k0 = p0; k0 < p1; k0 += 64 * U) {
                double p[U], er[U];
#pragma unroll
                for (int j = 0; j < U; ++j) {
                    const long long k = k0 + lane + 64 * j;
                    double a = 0.0, xv = 0.0;
                    if (k < p1) {
                        a = VT::widen(ld_nt(val + k));
                        xv = gather_x<XT>(x, ld_nt(ci + k), n, alpha, flags);
                    }
                    p[j] = two_prod(a, xv, er[j]);
                }
                fpe_absorb_prod<SP_N, true, U>(f, p, er, sink);
            }
            fpe_flush_sink<SP_N>(f, sink);
            sp_wave_sync();
            const unsigned long long any = __ballot((flags & SP_SPILL) != 0);
            if (any) {
                const long long v0 = acc[w][lane], v1 = lane < NL - 64 ? acc[w][64 + lane] : 0;
                if (v0) atomicAdd((unsigned long long *)&g[lane], (unsigned long long)v0);
                if (v1) atomicAdd((unsigned long long *)&g[64 + lane], (unsigned long long)v1);
                sp_acc_clear(acc[w]);
                const unsigned nf = flags & FLAG_NONFINITE;
                if (nf) atomicOr((unsigned *)&g[SP_ACC_FLAGS], nf);
                sp_wave_sync();
            }
        }
    }
    if (lane == 0 && n_chunks) atomicAdd((unsigned long long *)&hdr[7], n_chunks);
}

template <bool PLAIN, class XT>
__global__ void __launch_bounds__(SP_BLOCK) k_spmv_long_finish(const int *__restrict__ lrows, int lcap, double beta,
                                                              typename XT::elem *__restrict__ y,
                                                              long long *__restrict__ hdr,
                                                              const long long *__restrict__ lacc, int round_mode)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long nl = min(hdr[1], (long long)lcap);
    const long long wave0 = (long long)blockIdx.x * SP_WAVES + w, nwaves = (long long)gridDim.x * SP_WAVES;
    unsigned long long n_rows = 0;
    for (long long i = wave0; i < nl; i += nwaves) {
        const int row = lrows[i];
        const long long *g = lacc + i * SET_WORDS;
        ++n_rows;
        if constexpr (PLAIN) {
            const double s = __longlong_as_double(g[0]);
            if (lane == 0) y[row] = (beta == 0.0) ? s : s + beta * y[row];
        } else {
            long long v0 = g[lane], v1 = lane < NL - 64 ? g[64 + lane] : 0;
            unsigned flags = (unsigned)g[SP_ACC_FLAGS] & FLAG_NONFINITE;
            sp_wave_add_beta<XT>(v0, v1, beta, y, row, flags);
            const WaveFinish r = finish_wave(v0, v1, flags);
            const unsigned long long v = sp_pick_to<XT>(r, flags, round_mode);
            if (lane == 0) XT::store(y + row, v);
        }
    }
    if (lane == 0 && n_rows) atomicAdd((unsigned long long *)&hdr[6], n_rows);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------

template <bool PLAIN, class VT, class XT, class I>
static hipError_t spmv_launch(Ctx &c, int m, int n, const I *rp, const I *ci, const typename VT::elem *val, double alpha,
                              const typename XT::elem *x, double beta, typename XT::elem *y, int force_fb, int round_mode,
                              hipStream_t st)
{
    const int path = c.spmv_path;
    const long long short_max = path == 3 ? -1 : SP_SHORT_MAX;
    const auto [long_min, chunk] = sp_split_rule(path, SP_LONG_MIN, SP_CHUNK);
    const int lcap = path == 3 ? m : (int)min((long long)m, SP_LCAP);
    const size_t b_hdr = 256, b_med = align256((size_t)m * 4), b_lrows = align256((size_t)lcap * 4),
                 b_lbase = align256((size_t)(lcap + 1) * 8), b_lacc = (size_t)lcap * SET_WORDS * 8;
    hipError_t e;
    char *base = (char *)workspace(c, b_hdr + b_med + b_lrows + b_lbase + b_lacc, st, &e);
    if (!base) return e;
    long long *hdr = (long long *)base;
    int *med = (int *)(base + b_hdr);
    int *lrows = (int *)(base + b_hdr + b_med);
    long long *lbase = (long long *)(base + b_hdr + b_med + b_lrows);
    long long *lacc = (long long *)(base + b_hdr + b_med + b_lrows + b_lbase);
    c.spmv_info_dev = hdr;
    hipLaunchKernelGGL(k_sp_zero_header, dim3(1), dim3(64), 0, st, hdr, SP_HDR);
    const int cap = c.num_cu * 8;
    hipLaunchKernelGGL((k_spmv_classify<I>), dim3((m + SP_BLOCK - 1) / SP_BLOCK), dim3(SP_BLOCK), 0, st, m, rp, short_max,
                       long_min, lcap, hdr, med, lrows, lacc);
    {
        const long long waves = ((long long)m + 64 / SP_G_SHORT - 1) / (64 / SP_G_SHORT);
        const int grid = (int)min((long long)cap, (waves + SP_WAVES - 1) / SP_WAVES);
        hipLaunchKernelGGL((k_spmv_rows<SP_G_SHORT, false, PLAIN, VT, XT, I>), dim3(grid), dim3(SP_BLOCK), 0, st, m, n, rp, ci, val,
                           alpha, x, beta, y, short_max, (const int *)nullptr, hdr, force_fb, round_mode);
    }
    {
        const int grid = (int)min((long long)cap, ((long long)m + SP_WAVES - 1) / SP_WAVES);
        hipLaunchKernelGGL((k_spmv_rows<64, true, PLAIN, VT, XT, I>), dim3(grid), dim3(SP_BLOCK), 0, st, m, n, rp, ci, val, alpha,
                           x, beta, y, short_max, (const int *)med, hdr, force_fb, round_mode);
    }
    hipLaunchKernelGGL((k_spmv_long_prep<I>), dim3(1), dim3(1024), 0, st, rp, (const int *)lrows, lcap, chunk, hdr, lbase);
    hipLaunchKernelGGL((k_spmv_long<PLAIN, VT, XT, I>), dim3(cap), dim3(SP_BLOCK), 0, st, n, rp, ci, val, alpha, x,
                       (const int *)lrows, (const long long *)lbase, lcap, chunk, hdr, lacc);
    {
        const int grid = (int)min((long long)c.num_cu * 2, ((long long)lcap + SP_WAVES - 1) / SP_WAVES);
        hipLaunchKernelGGL((k_spmv_long_finish<PLAIN, XT>), dim3(grid), dim3(SP_BLOCK), 0, st, (const int *)lrows, lcap, beta,
                           y, hdr, (const long long *)lacc, round_mode);
    }
    return hipGetLastError();
}

hipError_t exspmv_dispatch(Ctx &c, int m, int n, int index_bits, const void *row_ptr, const void *col_idx,
                           const double *val, double alpha, const double *x, double beta, double *y, int fpe,
                           int early_exit, int round_mode, hipStream_t st)
{
    (void)early_exit;   // every (fpe >= 2, early_exit) gives the same bits: one expansion size serves them all
    if (m == 0) return hipSuccess;
    // fpe == 0 (superaccumulator only, as in the other routines) and the accumulator test path round every row from
    // its integer accumulator; the reference rounding mode is only reproduced there
    const int force_fb = (fpe == 0 || c.spmv_path == 1 || round_mode) ? 1 : 0;
    return sp_dispatch(index_bits, fpe, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
        constexpr bool PLAIN = decltype(plain)::value;   // the plain kernels neither force the accumulator nor round
        return spmv_launch<PLAIN, LpF64, LpF64>(c, m, n, rp, ci, val, alpha, x, beta, y, PLAIN ? 0 : force_fb,
                                                PLAIN ? 0 : round_mode, st);
    });
}

// The narrow entry: values of the type val_dtype, x and y of vec_dtype (float64 or val_dtype; the caller has checked the
// pair and that fpe != 1).  The same kernels with another front end: the exact sum is the one of the fp64 entry on the
// widened operands.  A float64 y is rounded as there; a narrow y once, to nearest even whatever the mode (the reference
// mode still sends every row through its accumulator, which changes no bit).
template <class VT, class XT>
static hipError_t spmv_lp_typed(Ctx &c, int m, int n, int index_bits, const void *row_ptr, const void *col_idx,
                                const void *val, double alpha, const void *x, double beta, void *y, int force_fb,
                                int round_mode, hipStream_t st)
{
    return sp_dispatch(index_bits, 0, row_ptr, col_idx, [&](auto plain, auto *rp, auto *ci) {
        if constexpr (decltype(plain)::value) return hipErrorInvalidValue;   // (fpe = 0 was passed: never taken)
        else
            return spmv_launch<false, VT, XT>(c, m, n, rp, ci, (const typename VT::elem *)val, alpha,
                                              (const typename XT::elem *)x, beta, (typename XT::elem *)y, force_fb,
                                              round_mode, st);
    });
}

hipError_t exspmv_lp_dispatch(Ctx &c, int m, int n, int index_bits, const void *row_ptr, const void *col_idx,
                              int val_dtype, const void *val, double alpha, int vec_dtype, const void *x, double beta,
                              void *y, int fpe, int round_mode, hipStream_t st)
{
    if (m == 0) return hipSuccess;
    const int force_fb = (fpe == 0 || c.spmv_path == 1 || round_mode) ? 1 : 0;
    hipError_t e = hipErrorInvalidValue;
    auto run = [&](auto vt, auto xt) {
        e = spmv_lp_typed<decltype(vt), decltype(xt)>(c, m, n, index_bits, row_ptr, col_idx, val, alpha, x, beta, y,
                                                      force_fb, round_mode, st);
    };
    auto by_value = [&](auto vt) {
        if (vec_dtype == DT_F64) run(vt, LpF64());
        else run(vt, vt);
    };
    if (val_dtype == DT_F32) by_value(LpF32());
    else if (val_dtype == DT_F16) by_value(LpF16());
    else if (val_dtype == DT_BF16) by_value(LpBF16());
    return e;
}

}  // namespace exb
