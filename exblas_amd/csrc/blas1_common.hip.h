// blas1_common.hip.h -- what the streaming ExSUM / ExDOT kernels of blas1.hip (fp64) and blas1_lowp.hip (float32,
// float16, bfloat16) share: the workgroup shape, the LDS sink wrappers, the block epilogue into the context's group
// accumulators and the launch plumbing.  Both files add into the same accumulators, so their calls fold into one
// exact reduction.
#pragma once
#include "superacc.hip.h"
#include "fpe.hip.h"
#include "exblas_internal.h"
#include <hip/hip_ext.h>

namespace exb {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;

// blas1 sinks everything into the wave's LDS accumulator column
template <int N, bool EE, int COPIES, int CNT, int ZM = 0>
__device__ __forceinline__ void fpe_absorb(double (&a)[N > 0 ? N : 1], double (&x)[CNT], int from,
                                           long long *col, unsigned &flags)
{
    LdsSink<COPIES> sink{col, flags};
    fpe_absorb_sink<N, EE, CNT, LdsSink<COPIES>, ZM>(a, x, from, sink);
}

template <int N, int COPIES>
__device__ __forceinline__ void fpe_flush(double (&a)[N > 0 ? N : 1], long long *col, unsigned &flags)
{
    LdsSink<COPIES> sink{col, flags};
    fpe_flush_sink<N>(a, sink);
}

// block epilogue: columns -> one limb vector -> global group accumulator
template <int COPIES>
__device__ __forceinline__ void block_epilogue(long long *s_acc, unsigned flags, long long *gacc,
                                               unsigned *gflags, int ngroups)
{
    __shared__ unsigned s_flags;
    if (threadIdx.x == 0) s_flags = 0;
    __syncthreads();  // also orders every wave's LDS atomics before the merge
    if (flags) atomicOr(&s_flags, flags);
    long long *g = gacc + (size_t)(blockIdx.x % ngroups) * NL;
    for (int l = threadIdx.x; l < NL; l += BLOCK) {
        long long sum = 0;
#pragma unroll
        for (int w = 0; w < WAVES; ++w)
#pragma unroll
            for (int c = 0; c < COPIES; ++c) sum += s_acc[(w * NL + l) * COPIES + c];
        if (sum != 0) atomicAdd((unsigned long long *)&g[l], (unsigned long long)sum);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_flags) atomicOr(gflags, s_flags);
}

// streaming-kernel launch: plain, or -- when the context holds events for it -- with the events attached to the
// dispatch packet itself (exblas_internal.h: launch_stop_event)
#define EXB_LAUNCH_STREAMING(c, kernel, grid, st, ...)                                                                \
    do {                                                                                                               \
        if ((c).launch_stop_event || (c).launch_start_event) {                                                         \
            hipEvent_t ev0_ = (c).launch_start_event, ev1_ = (c).launch_stop_event;                                    \
            (c).launch_start_event = (c).launch_stop_event = nullptr;                                                  \
            hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, st, ev0_, ev1_, 0, __VA_ARGS__);                 \
        } else {                                                                                                       \
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(BLOCK), 0, st, __VA_ARGS__);                                   \
        }                                                                                                              \
    } while (0)

static inline int grid_for(const Ctx &c, long long work_items, long long per_block, int blocks_per_cu)
{
    long long want = (work_items + per_block - 1) / per_block;
    long long cap = (long long)c.num_cu * blocks_per_cu;
    if (want < 1) want = 1;
    if (want >= cap) return (int)max(1ll, cap + c.grid_adj);
    return (int)want;
}

}  // namespace exb
