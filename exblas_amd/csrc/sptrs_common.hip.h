// sptrs_common.hip.h -- what the three mailbox solves (sptrsv.hip: ExSpTRSV, sptrsm.hip: ExSpTRSM, trsm.hip: ExTRSM) share.
// All three: the workspace header and its carving (st_workspace), the mailbox conventions (a reserved "not posted"
// pattern, the canonical NaN, agent-scope relaxed atomic store and load, a wave-uniform poll loop with a light sleep and
// the 2 s watchdog), the preset kernel, the ticket take, the counters and their flush, the grid size (st_grid), the
// decoding of uplo / diag; the rule for fpe, path and rounding mode (st_rule) is spmv_common.hip.h's.  The two sparse ones:
// the classification of one stored entry.  The two block solves: the tile widths, the sink of a lane's expansion
// (spmv_common.hip.h's SpLaneSink) and the host loop over the column panels (StPanel, st_block_solve).  Their lane
// geometry, publication and certify / fall-back blocks stay one copy per file: the exact kernels sit at the SGPR limit,
// every shared spelling compiled changed the count of spilled SGPRs they read back, and all of them together ran 1 to 4 %
// slower (profiles/block_solve_refactor_ab.md).  A change to one copy has to be made in the other by hand.
#pragma once
#include "spmv_common.hip.h"

namespace exb {

constexpr int ST_HDR_BYTES = 256;          // header: int64 words
constexpr int ST_TICKET = 0, ST_WATCHDOG = 1, ST_INFO = 4;   // [4] register rows [5] accumulator rows [6] no diagonal [7] skipped
constexpr long long ST_EMPTY = -1ll;       // mailbox: "not posted yet", a NaN pattern no posted value carries
constexpr long long ST_NAN = 0x7ff8000000000000ll;
constexpr long long ST_NO_DIAG = 0x7fffffffffffffffll;

struct StCounters {
    long long reg = 0, fb = 0, nodiag = 0, skipped = 0;   // reg / fb: lane 0 counts; the others: every lane counts its own
};

__device__ __forceinline__ void st_post(double *xq, double v)
{
    long long b = __double_as_longlong(v);
    if (b == ST_EMPTY) b = ST_NAN;
    __hip_atomic_store((long long *)xq, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lanes with want[j] set fetch xq[at[j]], polling until every one of them has been posted (wave-uniform loop); the
// others get 0.0.  Only values owned by lower tickets are ever asked for here.
template <int U>
__device__ __forceinline__ void st_fetch(const double *xq, const long long (&at)[U], const bool (&want)[U], double (&out)[U],
                                         long long *hdr, long long limit)
{
    long long b[U];
#pragma unroll
    for (int j = 0; j < U; ++j) b[j] = 0;
    long long t0 = 0;
    for (;;) {
        bool missing = false;
#pragma unroll
        for (int j = 0; j < U; ++j) {
            if (want[j]) b[j] = __hip_atomic_load((const long long *)(xq + at[j]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            missing |= want[j] && b[j] == ST_EMPTY;
        }
        if (!__any(missing)) break;
        __builtin_amdgcn_s_sleep(1);
        // watchdog: a cap on a broken hand-off, never reached by a valid input
        const long long now = (long long)wall_clock64();
        const long long raised = __hip_atomic_load(&hdr[ST_WATCHDOG], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t0 == 0) t0 = now;
        if (now - t0 > limit || raised) {
            if ((threadIdx.x & 63) == 0) __hip_atomic_store(&hdr[ST_WATCHDOG], 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int j = 0; j < U; ++j)
                if (want[j] && b[j] == ST_EMPTY) b[j] = ST_NAN;
            break;
        }
    }
#pragma unroll
    for (int j = 0; j < U; ++j) out[j] = want[j] ? __longlong_as_double(b[j]) : 0.0;
}

// One stored entry k, of column index `col`, of the row at substitution position `pos` (physical row `row`).  Returns 0
// for an entry that adds nothing (skipped, diagonal, out of range), 1 for a dependency outside the item (to be fetched
// from the mailbox), 2 for a dependency inside the item (slot `ds` of the item, which starts at position pos0).
__device__ __forceinline__ int st_classify(long long col, long long k, int m, int rev, long long row, long long pos,
                                           long long pos0, int &ds, long long &kdiag, unsigned &flags, StCounters &cn)
{
    if ((unsigned long long)col >= (unsigned long long)m) {
        flags |= FLAG_NAN | SP_SPILL;
        return 0;
    }
    if (col == row) {
        kdiag = min(kdiag, k);
        ++cn.skipped;   // (the leader takes the divisor's one back)
        return 0;
    }
    const long long cpos = rev ? (long long)m - 1 - col : col;
    if (cpos > pos) {
        ++cn.skipped;
        return 0;
    }
    if (cpos >= pos0) {
        ds = (int)(cpos - pos0);
        return 2;
    }
    return 1;
}

// the next work item of a persistent wave (wave-uniform)
__device__ __forceinline__ long long st_take_ticket(long long *hdr)
{
    long long t = 0;
    if ((threadIdx.x & 63) == 0) t = (long long)atomicAdd((unsigned long long *)&hdr[ST_TICKET], 1ull);
    return lane_bcast(t, 0);
}

// a wave's counters, summed over its lanes, into hdr[ST_INFO ..]
__device__ __forceinline__ void st_flush_counters(const StCounters &cn, long long *hdr)
{
    long long tot[4] = {cn.reg, cn.fb, cn.nodiag, cn.skipped};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) tot[i] += __shfl_down(tot[i], o, 64);
        if ((threadIdx.x & 63) == 0 && tot[i]) atomicAdd((unsigned long long *)&hdr[ST_INFO + i], (unsigned long long)tot[i]);
    }
}

// ---- the block solves: lanes own columns ----

constexpr int ST_TILE = 64;        // columns per tile ...
constexpr int ST_TILE_SMALL = 4;   // ... and on path 3, where the panel is as narrow

// ticket := 0, mailbox of n values := "not posted" (a kernel, not memset nodes: one node kind in a captured graph); with
// `first` the whole header is cleared: the counters and the watchdog flag, which add up over the launches that follow
static __global__ void __launch_bounds__(SP_BLOCK) k_sptrs_preset(long long n, int first, long long *__restrict__ hdr,
                                                                  long long *__restrict__ xq)
{
    const long long i0 = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (first ? i0 < ST_HDR_BYTES / 8 : i0 == ST_TICKET) hdr[i0] = 0;
    for (long long i = i0; i < n; i += (long long)gridDim.x * SP_BLOCK) xq[i] = ST_EMPTY;
}

// blocks of a persistent kernel (or of the preset) over `nitems` items, `per` of them to a block
static inline int st_grid(const Ctx &c, long long nitems, int per)
{
    return (int)min((long long)c.num_cu * 8, (nitems + per - 1) / per);
}

static inline hipError_t st_preset(const Ctx &c, long long n, int first, long long *hdr, double *xq, hipStream_t st)
{
    hipLaunchKernelGGL(k_sptrs_preset, dim3(st_grid(c, n, SP_BLOCK)), dim3(SP_BLOCK), 0, st, n, first, hdr, (long long *)xq);
    return hipGetLastError();
}

// the workspace of a solve: the header, then the mailbox of `slots` doubles
struct StSpace {
    long long *hdr;
    double *xq;
};
static inline hipError_t st_workspace(Ctx &c, size_t slots, hipStream_t st, StSpace &w)
{
    hipError_t e = hipSuccess;
    char *base = (char *)workspace(c, ST_HDR_BYTES + slots * sizeof(double), st, &e);
    if (base) w = {(long long *)base, (double *)(base + ST_HDR_BYTES)};
    return base ? hipSuccess : e;
}

// 'U' solves in reverse row order; diag 'U' divides by nothing
struct StOrient {
    int rev, unit;
};
static inline StOrient st_orient(char uplo, char diag)
{
    return {(uplo == 'U' || uplo == 'u') ? 1 : 0, (diag == 'U' || diag == 'u') ? 1 : 0};
}

// ticks of wall_clock64() in the watchdog's 2 s
static inline long long watchdog_ticks(int device)
{
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) {
        (void)hipGetLastError();
        khz = 100000;   // the constant 100 MHz counter of gfx9
    }
    return 2000ll * khz;
}

// One column panel of a block solve, as its launch sees it: kp columns from j0 on in `tiles` tiles of 1 << lg, items of
// R rows, first: the first panel of the call
struct StPanel {
    int kp, lg, tiles, R, first;
    long long j0, limit;
    StOrient o;
    StRule rule;
};

// The host side of a block solve of n rows and k columns in items of R rows (1 on path 2).  Column panels, one after the
// other in stream order: the largest multiple of 64 columns whose n x panel mailbox fits `budget` bytes, at least 64 (4 on
// path 3).  Per panel the preset (the first one also clears the counters and the watchdog flag) and launch(P, grid, hdr,
// xq), which fills the routine's argument struct and starts its ONE solve kernel.  info_dev: the header, once a preset has
// run (nullptr: the call launched nothing).
template <class Launch>
static hipError_t st_block_solve(Ctx &c, const long long *&info_dev, int n, int k, int R, StOrient o, StRule rule,
                                 size_t budget, hipStream_t st, Launch &&launch)
{
    info_dev = nullptr;
    if (n == 0 || k == 0) return hipSuccess;
    const int path = rule.path, tile = path == 3 ? ST_TILE_SMALL : ST_TILE;
    const long long panel = path == 3 ? ST_TILE_SMALL : max(64ll, (long long)(budget / ((size_t)n * sizeof(double))) / 64 * 64);
    StSpace w;
    if (hipError_t e = st_workspace(c, (size_t)n * (size_t)min((long long)k, panel), st, w); e != hipSuccess) return e;
    StPanel P;
    P.R = path == 2 ? 1 : R;
    P.limit = watchdog_ticks(c.device);
    P.o = o;
    P.rule = rule;
    for (P.j0 = 0; P.j0 < k; P.j0 += panel) {
        P.kp = (int)min(panel, (long long)k - P.j0);
        P.lg = 0;
        while ((1 << P.lg) < min(P.kp, tile)) ++P.lg;
        P.tiles = (P.kp + (1 << P.lg) - 1) >> P.lg;
        P.first = P.j0 == 0;
        const long long nitems = (((long long)n + P.R - 1) / P.R) * P.tiles;
        if (hipError_t e = st_preset(c, (long long)n * P.kp, P.first, w.hdr, w.xq, st); e != hipSuccess) return e;
        info_dev = w.hdr;
        if (hipError_t e = launch(P, st_grid(c, nitems, SP_WAVES), w.hdr, w.xq); e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace exb
