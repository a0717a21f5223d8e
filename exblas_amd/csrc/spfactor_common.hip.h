// spfactor_common.hip.h -- what the two incomplete factors on a CSR pattern (spilu0.hip: ExSpILU0, spic0.hip: ExSpIC0)
// share: the order-independent minimum of an info word, the preset and the structure check (phase 1 of ExSpIC0's check),
// the binary search of a column among the staged ones, and the host side's workspace of header, diagonal positions and
// mailbox.  The row steps stay one per file.
#pragma once
#include "sptrs_common.hip.h"

namespace exb {
namespace {

constexpr int IL_MAX = EXBLAS_SPILU0_MAX_ROW;   // entries of the longest row that is served
constexpr int IL_S = IL_MAX / 64;               // entries per lane of such a row
static_assert(IL_MAX % 64 == 0, "a lane holds a whole number of entries");

// *w := v when *w is 0 or above v (v > 0): an order-independent minimum over a word that starts at 0
__device__ __forceinline__ void il_info_min(long long *w, long long v)
{
    unsigned long long *p = (unsigned long long *)w;
    unsigned long long old = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (old == 0ull || old > (unsigned long long)v) {
        const unsigned long long seen = atomicCAS(p, old, (unsigned long long)v);
        if (seen == old) break;
        old = seen;
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_spilu0_preset(long long n, long long *__restrict__ hdr,
                                                            long long *__restrict__ xq, long long *__restrict__ info)
{
    const long long i0 = (long long)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i0 < 2) info[i0] = 0;
    if (hdr && i0 < ST_HDR_BYTES / 8) hdr[i0] = 0;
    for (long long i = i0; i < n; i += (long long)gridDim.x * SP_BLOCK) xq[i] = ST_EMPTY;
}

// the structure of every row, from the indices alone; nothing outside [0, cap) of col_idx is read
template <class I>
__global__ void __launch_bounds__(SP_BLOCK) k_spilu0_check(int m, const I *__restrict__ rp, const I *__restrict__ ci,
                                                           long long cap, long long *info, long long *__restrict__ dpos)
{
    for (long long r = (long long)blockIdx.x * SP_BLOCK + threadIdx.x; r < m; r += (long long)gridDim.x * SP_BLOCK) {
        const long long p0 = (long long)rp[r], p1 = (long long)rp[r + 1];
        bool bad = p0 < 0 || p1 < p0 || p1 > cap || p1 - p0 > IL_MAX;
        long long d = -1;
        if (!bad) {
            long long prev = -1;
            for (long long p = p0; p < p1; ++p) {
                const long long c = (long long)ci[p];
                if ((unsigned long long)c >= (unsigned long long)m || c <= prev) {
                    bad = true;
                    break;
                }
                if (c == r) d = p;
                prev = c;
            }
        }
        if (bad || d < 0) il_info_min(&info[0], r + 1);
        else dpos[r] = d;
    }
}

// the index in the sorted kc[0 .. n) that holds column c, or -1
__device__ __forceinline__ int il_find(const int *kc, int n, int c)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (kc[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return (lo < n && kc[lo] == c) ? lo : -1;
}

}  // namespace

// The workspace of a factor call: the header, the diagonal position of every row (8 m bytes, rounded up to 256), the
// mailbox (8 nnz bytes).  The C ABI carries no nnz, so a call outside a stream capture reads row_ptr[m] (one stream-ordered
// copy of one word and a wait for it) before it sizes the mailbox; a call that is being captured takes what the workspace
// holds -- the nnz of the routine's last call of the same m (last_m, last_nnz), else all of it -- and the check kernel
// refuses a row that does not fit (info[0]).
struct SpfSpace {
    long long *hdr, *dpos;
    double *xq;
    long long nnz;
};
static inline hipError_t spf_space(Ctx &c, int m, int index_bits, const void *row_ptr, int &last_m, long long &last_nnz,
                                   hipStream_t st, SpfSpace &w)
{
    const size_t isz = (size_t)index_bits / 8, fixed = ST_HDR_BYTES + align256((size_t)m * sizeof(long long));
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = st && hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    long long nnz = 0;
    if (capturing) {
        if (c.ws_bytes < fixed + sizeof(double)) return hipErrorStreamCaptureUnsupported;   // reserve, or call once, first
        const long long room = (long long)((c.ws_bytes - fixed) / sizeof(double));
        nnz = (last_m == m && last_nnz <= room) ? last_nnz : room;
    } else {
        long long last = 0;   // (an int32 lands in the low half: little endian)
        hipError_t e = hipMemcpyAsync(&last, (const char *)row_ptr + (size_t)m * isz, isz, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return e;
        nnz = index_bits == 32 ? (long long)(int)last : last;
        if (nnz < 0) nnz = 0;
    }
    hipError_t e = hipSuccess;
    char *base = (char *)workspace(c, fixed + (size_t)nnz * sizeof(double), st, &e);
    if (!base) return e;
    last_m = m;
    last_nnz = nnz;
    w = {(long long *)base, (long long *)(base + ST_HDR_BYTES), (double *)(base + fixed), nnz};
    return hipSuccess;
}

}  // namespace exb
