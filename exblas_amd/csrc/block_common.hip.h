// block_common.hip.h -- the frame of the seven block routines: those of the CholQR / block-CG chain (bgemm.hip: ExBGEMM,
// btrsm.hip: ExBTRSM, potrf.hip: ExPOTRF) and the block-Jacobi family (potrf_batched.hip, getrf_batched.hip: the batched
// ExPOTRF and ExGETRF; bjacobi_apply.hip: the batched ExPOTRS and ExGETRS).  Each is ONE kernel and nothing else: no preset
// kernel and no memset node (a memset node replayed in a captured graph was seen to leave the counters undefined from the
// second replay on).
//   * A lane keeps 4-term expansions in registers with no accumulator behind them (SpLaneSink: whatever would spill only
//     raises SP_SPILL), spmv_round_fast certifies the rounding there and the lane stores.
//   * What it cannot certify (ties, near-ties inside the margin, spills, non-finite flags, values outside its range), and
//     every output under fpe == 0, path 1 or the reference rounding mode (st_rule's force_fb), is settled on the spot by the
//     whole wave: the lanes stride the products of that one output into the wave's ONE integer accumulator in LDS, lane 0
//     adds the one term that is no product of the sum, sp_acc_round rounds (blk_resolve).  No bitmap, no second kernel.
//   * The info counters (outputs rounded in registers, outputs rounded from the accumulator) are not shared words that
//     would have to be zeroed first: every workgroup stores its own pair into its slot of the workspace
//     (blk_store_counters), the context remembers the slots (SlotInfo, blk_reserve_slots) and exblas_last_*_info adds
//     them up on the host.
//   * fpe == 1 runs the same structure with plain fp64 sums (deterministic, not exact; both counters 0).
// Host side: the rule for fpe, path and rounding mode is st_rule (spmv_common.hip.h), the items of a call go to workgroups
// in contiguous ranges (blk_partition), more than 64 KiB of dynamic LDS is asked for by blk_lds_optin, and the two batched
// factorisations share their argument struct and their plan (BjfArgs, bjf_plan).
// Left per file on purpose: the certify / ballot / count / fall-back loop, the item loops, the staging of C / op(T) / the
// triangle / the matrix and the lane geometry.  Sharing such blocks of register-tight kernels kept registers and bits and
// cost 1 to 5 % (profiles/block_solve_refactor_ab.md); what is shared here and why is in profiles/block_frame_refactor.md
// and profiles/bjacobi_refactor.md.
#pragma once
#include <atomic>
#include <initializer_list>

#include "spmv_common.hip.h"

namespace exb {

// coef * v with coef != 0 into an output's accumulator: 1 adds v exactly, anything else the error-free product, both parts
__device__ __forceinline__ void blk_sink_term(RowSink &sink, double coef, double v)
{
    if (coef == 1.0) {
        sink.add(v);
    } else {
        double e;
        const double pr = two_prod(coef, v, e);
        sink_product(sink, pr, e);
    }
}

// What no lane could certify: one output through the wave's integer accumulator `acc`.  prod(i, a, b) yields the two
// factors of product i < n, the lanes stride them; term(sink) is lane 0's addition.  Wave-uniform; every lane gets the
// rounded value, and the accumulator is zero again.  The caller stores (and divides), then sp_wave_sync.
template <class Prod, class Term>
__device__ __forceinline__ double blk_resolve(long long *acc, int n, int round_mode, Prod &&prod, Term &&term)
{
    const int lane = threadIdx.x & 63;
    unsigned fl = 0;
    RowSink sink{acc, fl};
    for (int i = lane; i < n; i += 64) {
        double a, b, e;
        prod(i, a, b);
        const double pr = two_prod(a, b, e);
        sink_product(sink, pr, e);
    }
    if (lane == 0) term(sink);
    sp_wave_sync();
    return sp_acc_round(acc, NonFiniteLanes(fl).of(~0ull), round_mode);
}

// the workgroup's counters into slot `block`: plain stores, nothing to zero beforehand (both 0 for the plain kernels)
__device__ __forceinline__ void blk_store_counters(unsigned long long (&cnt)[SP_WAVES][2], unsigned long long n_reg,
                                                   unsigned long long n_fb, long long *slots, long long block)
{
    if ((threadIdx.x & 63) == 0) {
        cnt[threadIdx.x >> 6][0] = n_reg;
        cnt[threadIdx.x >> 6][1] = n_fb;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long t = 0;
        for (int v = 0; v < SP_WAVES; ++v) t += cnt[v][threadIdx.x];
        slots[2 * block + threadIdx.x] = (long long)t;
    }
}

// nitems work items over at most 8 workgroups per CU: `per` consecutive items to each of `grid` workgroups
struct BlkPartition {
    int grid;
    long long per;
};
static inline BlkPartition blk_partition(const Ctx &c, long long nitems)
{
    const long long most = min((long long)c.num_cu * 8, nitems), per = (nitems + most - 1) / most;
    return {(int)((nitems + per - 1) / per), per};
}

// Forgets the last call's counter slots, reserves a pair for each of `blocks` workgroups in the workspace and records
// them.  nullptr with *err set when the workspace refuses (`info` then stays empty).  A dispatch also empties `info` first
// thing, before it can return early, and reserves once its argument struct is filled.
static inline long long *blk_reserve_slots(Ctx &c, SlotInfo &info, int blocks, hipStream_t st, hipError_t *err)
{
    info = SlotInfo();
    long long *slots = (long long *)workspace(c, (size_t)blocks * 2 * sizeof(long long), st, err);
    if (slots) info = {slots, blocks};
    return slots;
}

// More than 64 KiB of dynamic LDS has to be asked for, once per device and kernel instance (no stream operation).  `done` is
// the caller's own word, a bit per device: a file asks for all its instances at once.
static inline hipError_t blk_lds_optin(std::atomic<unsigned long long> &done, int device, size_t bytes,
                                       std::initializer_list<const void *> kernels)
{
    const unsigned long long bit = 1ull << (device & 63);
    if (done.load() & bit) return hipSuccess;
    for (const void *k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess) return e;
    }
    done.fetch_or(bit);
    return hipSuccess;
}

// ---- the two batched factorisations (potrf_batched.hip, getrf_batched.hip): one argument struct, one host plan ----
constexpr size_t BJF_LDS = (size_t)SP_WAVES * 64 * 65 * sizeof(double);   // four staged matrices of p = 64

struct BjfArgs {
    long long stride, batch, nitems, per;   // nitems workgroup items, `per` of them to a workgroup
    // hirow: the slow index of a stored matrix is the row of its staged image ('L' of a triangle, 'R' of a matrix);
    // wpi wave items per workgroup item, tsz doubles per wave
    int p, ld, hirow, lgpw, G, wpi, tsz, force, round_mode;
};

// Fills A for `batch` matrices of order p and returns the grid.  With pw = p rounded up to a power of two a wave carries
// G = 64 / pw matrices (1 on the paths 2 and 3), fewer where its share of LDS does not hold them; a workgroup item is four
// wave items (one on path 3).
static inline BlkPartition bjf_plan(const Ctx &c, BjfArgs &A, int path, int p, long long batch, int ld, long long stride,
                                    bool hirow, int fpe, int round_mode)
{
    A.p = p, A.ld = ld, A.stride = stride, A.batch = batch, A.hirow = hirow ? 1 : 0;
    A.lgpw = 0;
    while ((1 << A.lgpw) < p) ++A.lgpw;
    A.G = (path == 2 || path == 3) ? 1 : 64 >> A.lgpw;
    const int msz = p * (p | 1);
    while (A.G > 1 && (size_t)SP_WAVES * A.G * msz * sizeof(double) > BJF_LDS) A.G >>= 1;   // the wave's share of LDS
    A.wpi = path == 3 ? 1 : SP_WAVES;
    A.tsz = A.G * msz;
    const StRule rule = st_rule(fpe, path, round_mode);
    A.force = rule.force_fb, A.round_mode = rule.round_mode;
    const long long per_item = (long long)A.G * A.wpi;
    A.nitems = (batch + per_item - 1) / per_item;
    BlkPartition P = blk_partition(c, A.nitems);
    if (path == 3) {   // a handful of workgroups: each walks several items already at a small batch
        const long long most = min(5ll, A.nitems);
        P.per = (A.nitems + most - 1) / most;
        P.grid = (int)((A.nitems + P.per - 1) / P.per);
    }
    A.per = P.per;
    return P;
}

}  // namespace exb
