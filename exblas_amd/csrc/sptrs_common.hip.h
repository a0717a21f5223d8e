// sptrs_common.hip.h -- what the two sparse triangular solves (sptrsv.hip: ExSpTRSV, sptrsm.hip: ExSpTRSM) share: the
// workspace header, the mailbox conventions (a reserved "not posted" pattern, the canonical NaN, agent-scope relaxed
// atomic store and load, a wave-uniform poll loop with a light sleep and the 2 s watchdog), the preset kernel, the ticket
// take, the classification of one stored entry, the counters and their flush, and the decoding of uplo / diag.
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

// ticket := 0, mailbox of n values := "not posted" (a kernel, not memset nodes: one node kind in a captured graph); with
// `first` the whole header is cleared: the counters and the watchdog flag, which add up over the launches that follow
static __global__ void __launch_bounds__(SP_BLOCK) k_sptrs_preset(long long n, int first, long long *__restrict__ hdr,
                                                                  long long *__restrict__ xq)
{
    const long long i0 = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (first ? i0 < ST_HDR_BYTES / 8 : i0 == ST_TICKET) hdr[i0] = 0;
    for (long long i = i0; i < n; i += (long long)gridDim.x * SP_BLOCK) xq[i] = ST_EMPTY;
}

static inline hipError_t st_preset(const Ctx &c, long long n, int first, long long *hdr, double *xq, hipStream_t st)
{
    hipLaunchKernelGGL(k_sptrs_preset, dim3((int)min((long long)c.num_cu * 8, (n + SP_BLOCK - 1) / SP_BLOCK)), dim3(SP_BLOCK),
                       0, st, n, first, hdr, (long long *)xq);
    return hipGetLastError();
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

}  // namespace exb
