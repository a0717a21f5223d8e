// lowp_types.hip.h -- the element front ends of the narrow entries: how a float64 / float32 / float16 / bfloat16 element lies
// in memory, how it widens (exactly) to a double, and how a rounded bit pattern of its format is stored.  Shared by the
// narrow reductions (blas1_lowp.hip) and the narrow sparse products (spmv.hip, spmm.hip).
// Widening: v_cvt_f32_f16 / v_cvt_f64_f32 obey the wave's denormal mode, which the build leaves at "keep" (see the header
// of blas1_lowp.hip).  bfloat16 is bits << 16 read as a float32.
#pragma once
#include <hip/hip_runtime.h>
#include "round_lowp.hip.h"

namespace exb {

typedef unsigned u4_t __attribute__((ext_vector_type(4)));

// element types: `elem` as it lies in memory, DT its EXBLAS_DT_* code, widen() the exact double, store() the low bits of
// a pattern; for the streaming kernels `vec` the 16 loaded bytes, VEC elements in them, at() element j of a loaded vector
struct LpF64 {
    typedef double elem;
    static constexpr int DT = DT_F64;
    static __device__ __forceinline__ double widen(elem v) { return v; }
    static __device__ __forceinline__ void store(elem *p, unsigned long long bits)
    {
        *p = __longlong_as_double((long long)bits);
    }
};
struct LpF32 {
    typedef float elem;
    typedef u4_t vec;
    static constexpr int VEC = 4, DT = DT_F32;
    static __device__ __forceinline__ double widen(elem v) { return (double)v; }
    static __device__ __forceinline__ double at(const u4_t &r, int j) { return (double)__uint_as_float(r[j]); }
    static __device__ __forceinline__ void store(elem *p, unsigned long long bits) { *p = __uint_as_float((unsigned)bits); }
};
struct LpF16 {
    typedef _Float16 elem;
    typedef u4_t vec;
    static constexpr int VEC = 8, DT = DT_F16;
    static __device__ __forceinline__ double widen(elem v) { return (double)(float)v; }
    static __device__ __forceinline__ double at(const u4_t &r, int j)
    {
        const unsigned w = r[j >> 1];
        return widen(__builtin_bit_cast(_Float16, (unsigned short)((j & 1) ? (w >> 16) : (w & 0xffffu))));
    }
    static __device__ __forceinline__ void store(elem *p, unsigned long long bits)
    {
        *p = __builtin_bit_cast(_Float16, (unsigned short)bits);
    }
};
struct LpBF16 {
    typedef unsigned short elem;   // raw words
    typedef u4_t vec;
    static constexpr int VEC = 8, DT = DT_BF16;
    static __device__ __forceinline__ double widen(elem v) { return (double)__uint_as_float((unsigned)v << 16); }
    static __device__ __forceinline__ double at(const u4_t &r, int j)
    {
        const unsigned w = r[j >> 1];
        return (double)__uint_as_float((j & 1) ? (w & 0xffff0000u) : (w << 16));
    }
    static __device__ __forceinline__ void store(elem *p, unsigned long long bits) { *p = (unsigned short)bits; }
};

}  // namespace exb
