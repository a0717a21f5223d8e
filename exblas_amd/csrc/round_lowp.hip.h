// round_lowp.hip.h -- one rounding of the exact digit set straight into float64 / float32 / float16 / bfloat16.
//
// A reduction of narrow inputs that rounds its exact total to a double first and casts that double afterwards rounds
// TWICE, and the second rounding goes the wrong way on near-ties: 1 + 2^-24 + 2^-60 is 1 + 2^-24 as a double (a tie of
// float32, which the cast resolves to even: 1.0), while the total itself lies above the tie and rounds to 1 + 2^-23.
// round_digits_to rounds once, from all 68 digits with a full sticky.  Host and device: the host entry
// (exblas_round_digits_host) is what the CPU tests drive, k_round_records (blas1_lowp.hip) is the device form.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace exb {

// element / target formats of the narrow entries (EXBLAS_DT_* of include/exblas_hip.h)
constexpr int DT_F64 = 0, DT_F32 = 1, DT_F16 = 2, DT_BF16 = 3;

__host__ __device__ inline bool dtype_known(int dtype) { return dtype >= DT_F64 && dtype <= DT_BF16; }
__host__ __device__ inline int dtype_bytes(int dtype) { return dtype == DT_F64 ? 8 : (dtype == DT_F32 ? 4 : 2); }

// A binary format as (precision incl. the hidden bit, emin, emax); its width is 1 + exponent bits + precision - 1
struct NarrowFormat {
    int prec, emin, emax, bits;
};
__host__ __device__ inline NarrowFormat format_of(int dtype)
{
    switch (dtype) {
    case DT_F32: return {24, -126, 127, 32};
    case DT_F16: return {11, -14, 15, 16};
    case DT_BF16: return {8, -126, 127, 16};
    default: return {53, -1022, 1023, 64};
    }
}

// Round-to-nearest-even of value = 2^-1074 * sum_i v[i] 2^(32 i) (the 68 normalised digits of a record, words
// [48, 116): digits 0..66 in [0, 2^32), the top one signed) into the format `dtype`; returns the bit pattern in the low
// bits.  One rounding: the round bit and a sticky over EVERY digit below it.  Subnormal results, the carry into the next
// binade (and from the largest subnormal into the smallest normal) and the overflow to +-Inf all come out of adding the
// rounded significand to the exponent field.  An exact zero is +0; a negative total that rounds to zero is -0 (IEEE).
// For DT_F64 this is round_exact_bits (superacc.hip.h) bit for bit.
__host__ __device__ inline unsigned long long round_digits_to(const long long *v, int dtype)
{
    constexpr int ND = 68, UNIT = 1074;
    const NarrowFormat f = format_of(dtype);
    const bool neg = v[ND - 1] < 0;
    unsigned mag[ND];
    if (!neg) {
        for (int i = 0; i < ND; ++i) mag[i] = (unsigned)v[i];
    } else {
        unsigned long long c = 1;
        for (int i = 0; i < ND; ++i) {
            const unsigned long long t = (unsigned long long)(~(unsigned)v[i]) + c;
            mag[i] = (unsigned)t;
            c = t >> 32;
        }
    }
    int t = ND - 1;
    while (t >= 0 && mag[t] == 0) --t;
    if (t < 0) return 0ull;
    const unsigned long long sign = neg ? 1ull << (f.bits - 1) : 0ull;
    int lz = 0;
    for (unsigned m = mag[t]; !(m & 0x80000000u); m <<= 1) ++lz;
    const int msb = 32 * t + 31 - lz;              // the value lies in [2^(msb - UNIT), 2^(msb - UNIT + 1))
    const int low = f.emin + UNIT;                 // bit position of 2^emin: below it the results are subnormal
    const int ebase = msb > low ? msb : low;       // exponent the quantum is taken from
    const int qb = ebase - (f.prec - 1);           // bit position of the quantum (one unit in the last place)
    const unsigned long long inf = (unsigned long long)(2 * f.emax + 1) << (f.prec - 1);
    if (ebase - low > 2 * f.emax) return sign | inf;
    auto digit = [&](int i) -> unsigned long long { return (i >= 0 && i < ND) ? mag[i] : 0u; };
    unsigned long long m;                          // the significand: the bits from qb up (fewer than 2^prec)
    bool half = false, sticky = false;
    if (qb <= 0) {                                 // (float64 only: totals below 2^53 units are exact)
        m = (digit(0) | (digit(1) << 32)) << -qb;
    } else {
        const int d = qb >> 5, r = qb & 31;
        const unsigned long long lo = digit(d) | (digit(d + 1) << 32);
        m = r ? ((lo >> r) | (digit(d + 2) << (64 - r))) : lo;
        const int hb = qb - 1, hd = hb >> 5, hr = hb & 31;
        half = (mag[hd] >> hr) & 1u;
        sticky = (mag[hd] & ((1u << hr) - 1u)) != 0;
        for (int i = hd - 1; i >= 0 && !sticky; --i) sticky = mag[i] != 0;
    }
    if (half && (sticky || (m & 1ull))) m += 1;
    // exponent field - 1 (normal) or 0 (subnormal) plus the significand with its hidden bit: a carry out of the
    // significand, or the hidden bit of a result that became normal, steps the field
    unsigned long long bits = ((unsigned long long)(ebase - low) << (f.prec - 1)) + m;
    if ((bits >> (f.prec - 1)) >= (unsigned long long)(2 * f.emax + 1)) bits = inf;
    return sign | bits;
}

}  // namespace exb
