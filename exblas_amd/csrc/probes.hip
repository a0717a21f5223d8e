// probes.hip -- the counter-based input generator and the two read-bandwidth probes: the kernels and their three
// device-pointer entry points (include/exblas_hip.h).  Of the context they use only the launch geometry.
#include "../../include/exblas_hip.h"
#include "exblas_internal.h"

#include <cmath>

namespace exb {

// ---------------------------------------------------------------------------------------------
// counter-based generators: the device twin of oracle/exblas_oracle.c:orc_gen_one (integer math,
// exact conversions and power-of-two scalings only, so the bits are identical on CPU and GPU)
// ---------------------------------------------------------------------------------------------
__host__ __device__ inline unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ inline unsigned long long rnd(unsigned long long seed, unsigned long long i, unsigned long long k)
{
    return mix64(seed * 0xD1342543DE82EF95ull + (2 * i + k + 1) * 0x9E3779B97F4A7C15ull);
}
__device__ inline double pow2i(int e) { return __longlong_as_double((long long)(e + 1023) << 52); }
__device__ inline double mant12(unsigned long long r)
{
    return __longlong_as_double((long long)(0x3FF0000000000000ull | (r >> 12)));
}
__device__ inline double mant_signed(unsigned long long r)
{
    long long k = (long long)(r >> 11);
    return (double)(2 * k - (1ll << 53)) * 0x1p-53;
}
__device__ inline unsigned uni(unsigned long long r, unsigned range)
{
    return (unsigned)(((r >> 32) * (unsigned long long)range) >> 32);
}

__global__ void __launch_bounds__(256) k_gen(int kind, unsigned long long seed, long long first, long long count,
                                             long long n, int i0, int i1, double dscale, double *out)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < count;
         t += (long long)gridDim.x * blockDim.x) {
        const long long i = first + t;
        const unsigned long long r0 = rnd(seed, (unsigned long long)i, 0), r1 = rnd(seed, (unsigned long long)i, 1);
        double v = 0.0;
        switch (kind) {
        case EXBLAS_GEN_NAIVE: v = 1.1; break;
        case EXBLAS_GEN_FPUNIFORM:
        case EXBLAS_GEN_FPUNIFORM_SIGNED: {
            int e = i1 - i0 + (i0 > 0 ? (int)uni(r1, (unsigned)i0) : 0);
            v = mant12(r0) * pow2i(e);
            if (kind == EXBLAS_GEN_FPUNIFORM_SIGNED && (r1 & 1)) v = -v;
            break;
        }
        case EXBLAS_GEN_LOGNORMAL: {
            long long z = (long long)(r1 & 0xffff) + (long long)((r1 >> 16) & 0xffff) +
                          (long long)((r1 >> 32) & 0xffff) + (long long)((r1 >> 48) & 0xffff) - 2 * 65535;
            int e = (int)rint((double)z * dscale) + i0;
            e = e > 1000 ? 1000 : (e < -1000 ? -1000 : e);
            v = mant12(r0) * pow2i(e);
            break;
        }
        case EXBLAS_GEN_ILLCOND: {
            const int bh = i0;
            const long long n2 = n / 2;
            int e;
            if (i < n2) e = (i == 0) ? bh + 1 : (int)uni(r1, (unsigned)(bh + 1));
            else e = (n - n2 > 0) ? (int)(((i - n2) * (long long)bh) / (n - n2)) : 0;
            v = mant_signed(r0) * pow2i(e);
            break;
        }
        case EXBLAS_GEN_CANCEL: {
            const long long h = n / 2;
            if (i >= 2 * h) v = 0.0;
            else if (i == h - 1) v = 1.0;
            else if (i == 2 * h - 1) v = 0x1p-60;
            else {
                const long long j = (i < h) ? i : i - h;
                const unsigned long long q0 = rnd(seed, (unsigned long long)j, 0),
                                         q1 = rnd(seed, (unsigned long long)j, 1);
                double w = mant_signed(q0) * pow2i(i0 > 0 ? (int)uni(q1, (unsigned)i0) : 0);
                v = (i < h) ? w : -w;
            }
            break;
        }
        default: break;
        }
        out[t] = v;
    }
}

// plain (inexact) streaming sum: read-bandwidth probe
typedef double d2_t __attribute__((ext_vector_type(2)));
__global__ void __launch_bounds__(256) k_stream_read(const double *a, long long n, double *sink)
{
    const d2_t *v = (const d2_t *)a;
    const long long nv = n >> 1;
    double s0 = 0, s1 = 0;
    constexpr int U = 4;
    const long long tile = 256ll * U, ntiles = nv / tile;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const d2_t *p = v + t * tile + threadIdx.x;
        d2_t r[U];
#pragma unroll
        for (int u = 0; u < U; ++u) r[u] = __builtin_nontemporal_load(p + u * 256);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s0 += r[u].x;
            s1 += r[u].y;
        }
    }
    if (s0 + s1 == 0x1.23456789abcdep-333) *sink = s0;  // keeps the loads alive, never true in practice
}

// plain (inexact) two-stream dot: read-bandwidth probe for the ExDOT access pattern
__global__ void __launch_bounds__(256) k_stream_read2(const double *a, const double *b, long long n, double *sink)
{
    const d2_t *va = (const d2_t *)a, *vb = (const d2_t *)b;
    const long long nv = n >> 1;
    double s0 = 0, s1 = 0;
    constexpr int U = 4;
    const long long tile = 256ll * U, ntiles = nv / tile;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long base = t * tile + threadIdx.x;
        d2_t r[U], q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            r[u] = __builtin_nontemporal_load(va + base + u * 256);
            q[u] = __builtin_nontemporal_load(vb + base + u * 256);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            s0 += r[u].x * q[u].x;
            s1 += r[u].y * q[u].y;
        }
    }
    if (s0 + s1 == 0x1.23456789abcdep-333) *sink = s0;
}

}  // namespace exb

using namespace exb;

extern "C" {

int exblas_gen_dev(int kind, uint64_t seed, int64_t first, int64_t count, int64_t n_total, double p0, double p1,
                   double *d_out, void *stream)
{
    Ctx &c = ctx(-1);
    if (count <= 0) return 0;
    int i0 = 0, i1 = 0;
    double dscale = 0.0;
    switch (kind) {
    case EXBLAS_GEN_FPUNIFORM:
    case EXBLAS_GEN_FPUNIFORM_SIGNED: i0 = (int)p0; i1 = (int)p1; break;
    case EXBLAS_GEN_LOGNORMAL:
        // same expressions as orc_gen_one, evaluated on the host in IEEE double
        dscale = p1 * (1.0 / (0.6931471805599453 * 37837.22690659431));
        i0 = (int)rint(p0 * (1.0 / 0.6931471805599453));
        break;
    case EXBLAS_GEN_ILLCOND: i0 = (int)rint(log2(p0) * 0.5); break;
    case EXBLAS_GEN_CANCEL: i0 = (int)p0; break;
    default: break;
    }
    long long blocks = (count + 255) / 256;
    long long cap = (long long)c.num_cu * 16;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(k_gen, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, kind,
                       (unsigned long long)seed, (long long)first, (long long)count, (long long)n_total, i0, i1,
                       dscale, d_out);
    return (int)hipGetLastError();
}

int exblas_stream_read_dev(const double *d_a, int64_t n, void *stream, double *d_sink)
{
    Ctx &c = ctx(-1);
    long long blocks = (long long)c.num_cu * c.blocks_per_cu;
    hipLaunchKernelGGL(k_stream_read, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_a, (long long)n,
                       d_sink);
    return (int)hipGetLastError();
}

int exblas_stream_read2_dev(const double *d_a, const double *d_b, int64_t n, int blocks_per_cu, void *stream,
                            double *d_sink)
{
    Ctx &c = ctx(-1);
    long long blocks = (long long)c.num_cu * (blocks_per_cu > 0 ? blocks_per_cu : c.bpc_dot);
    hipLaunchKernelGGL(k_stream_read2, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_a, d_b, (long long)n,
                       d_sink);
    return (int)hipGetLastError();
}

}  // extern "C"
