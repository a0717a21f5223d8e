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

// The same rounding from what a wave holds of the magnitude after finish_wave (superacc.hip.h): `msb` the position of the
// leading bit (the value lies in [2^(msb - 1074), 2^(msb - 1073))), `w` the 64 bits from the leading bit down (bit 63 is
// the leading bit, zeros below position 0) and `below` whether any bit under those 64 is set.  64 bits hold the
// significand and the round bit of every format here; the sticky is (rest of w) | below.  Bit for bit round_digits_to.
__host__ __device__ inline unsigned long long round_window_to(bool neg, int msb, unsigned long long w, bool below, int dtype)
{
    constexpr int UNIT = 1074;
    const NarrowFormat f = format_of(dtype);
    const unsigned long long sign = neg ? 1ull << (f.bits - 1) : 0ull;
    const unsigned long long inf = (unsigned long long)(2 * f.emax + 1) << (f.prec - 1);
    const int low = f.emin + UNIT;
    const int ebase = msb > low ? msb : low;
    if (ebase - low > 2 * f.emax) return sign | inf;
    const int nbits = msb - ebase + f.prec;   // bits of the significand that the value reaches: prec, fewer when subnormal
    unsigned long long m = 0;
    bool half = false, sticky = true;
    if (nbits >= 1) {
        m = w >> (64 - nbits);
        half = (w >> (63 - nbits)) & 1ull;
        sticky = (w & ((1ull << (63 - nbits)) - 1ull)) != 0 || below;
    } else if (nbits == 0) {   // the leading bit is the round bit
        half = true;
        sticky = (w << 1) != 0 || below;
    }
    if (half && (sticky || (m & 1ull))) m += 1;
    unsigned long long bits = ((unsigned long long)(ebase - low) << (f.prec - 1)) + m;
    if ((bits >> (f.prec - 1)) >= (unsigned long long)(2 * f.emax + 1)) bits = inf;
    return sign | bits;
}

// +-Inf and NaN in the format `dtype` from the non-finite verdict of an exact sum (the bits of the double it gives)
__host__ __device__ inline unsigned long long nonfinite_to(unsigned long long double_bits, int dtype)
{
    const NarrowFormat f = format_of(dtype);
    const unsigned long long inf = (unsigned long long)(2 * f.emax + 1) << (f.prec - 1);
    if (double_bits & 0x000fffffffffffffull) return inf | (1ull << (f.prec - 2));   // the quiet NaN
    return inf | ((double_bits >> 63) << (f.bits - 1));
}

// ---------------------------------------------------------------------------------------------
// Certified rounding of an interval [res - bound, res + bound] into a narrow format
// ---------------------------------------------------------------------------------------------
// the magnitude pattern (no sign bit) of |a| rounded once, to nearest even, into a narrow format (prec <= 24); a finite
__host__ __device__ inline unsigned long long round_double_mag_to(unsigned long long a_bits, const NarrowFormat &f)
{
    const int ef = (int)((a_bits >> 52) & 0x7ffull);
    if (ef == 0) return 0ull;   // below 2^-1022: far under half the smallest subnormal of every narrow format
    const unsigned long long mant = (a_bits & 0x000fffffffffffffull) | 0x0010000000000000ull;
    const int E = ef - 1023;
    const unsigned long long inf = (unsigned long long)(2 * f.emax + 1) << (f.prec - 1);
    if (E > f.emax) return inf;
    const int ebase = E > f.emin ? E : f.emin;
    const int shift = 53 - f.prec + (ebase - E);   // bits of the 53 that fall below the quantum (>= 29)
    if (shift > 54) return 0ull;                   // the whole value lies below half a quantum
    unsigned long long m = shift >= 64 ? 0ull : mant >> shift;   // (shift <= 54 here)
    const bool half = (mant >> (shift - 1)) & 1ull;
    const bool sticky = (mant & ((1ull << (shift - 1)) - 1ull)) != 0;
    if (half && (sticky || (m & 1ull))) m += 1;
    unsigned long long bits = ((unsigned long long)(ebase - f.emin) << (f.prec - 1)) + m;
    if (bits > inf) bits = inf;
    return bits;
}

// the value of a magnitude pattern of a narrow format as a double (exact); the pattern of Inf gives 2^(emax + 1), the
// value its place on the grid would have, so that the midpoint below it is the overflow threshold
__host__ __device__ inline double narrow_mag_value(unsigned long long pat, const NarrowFormat &f)
{
    const int e = (int)(pat >> (f.prec - 1));
    const unsigned long long m = pat & ((1ull << (f.prec - 1)) - 1ull);
    const unsigned long long sig = e ? (m | (1ull << (f.prec - 1))) : m;
    const int ex = (e ? e - 1 : 0) + f.emin - (f.prec - 1);   // >= -149: 2^ex is a normal double
    union {
        unsigned long long u;
        double d;
    } p2;
    p2.u = (unsigned long long)(ex + 1023) << 52;
    return (double)(long long)sig * p2.d;
}

// Soundness: returns 1 with the pattern of the ONE `dtype` value that every real number of [res - bound, res + bound]
// rounds to (to nearest, ties to even), and 0 when the interval reaches a rounding boundary of the format (or the caller's
// numbers are not finite, or bound < 0).  Rounding is monotone, so the two ends rounding alike is the whole condition; it
// is tested here without rounding the ends: p = RN(res) is formed by integer arithmetic on the bits of res (one rounding,
// float16 does not pass through float32), the two boundaries of p's cell -- the midpoints to its neighbours, exact doubles
// since the formats have at most 24 bits -- are subtracted from res EXACTLY (both are multiples of ulp(res) and the
// difference is no larger than |res|), and bound must lie strictly below both distances.  Towards zero the cell of the
// zero pattern ends AT zero: a sum of the other sign rounds to the other zero.  bound == 0 says that res is the exact
// value: then ties are decided here (to even), and res == 0 gives +0.  For float64 the boundaries are not doubles; the
// test is then the one of spmv_round_fast: bound below a quarter of ulp(res) (a half when res is no power of two) less a
// margin of 2^-30 of it, with |res| in [2^-960, 2^1020).
__host__ __device__ inline int round_interval_to(double res, double bound, int dtype, unsigned long long *bits)
{
    union {
        double d;
        unsigned long long u;
    } r;
    r.d = res;
    const unsigned long long abits = r.u & 0x7fffffffffffffffull;
    if (abits >= 0x7ff0000000000000ull || !(bound >= 0.0) || !(bound < 1.797e308)) return 0;
    if (abits == 0) {
        *bits = 0ull;
        return bound == 0.0;
    }
    const NarrowFormat f = format_of(dtype);
    const unsigned long long sign = (r.u >> 63) << (f.bits - 1);
    if (dtype == DT_F64) {
        *bits = r.u;
        if (bound == 0.0) return 1;
        const unsigned ef = (unsigned)(abits >> 52);
        if (ef < 1023u - 960u || ef >= 1023u + 1020u) return 0;
        const bool pow2 = (abits & 0x000fffffffffffffull) == 0;
        r.u = (unsigned long long)(ef - (pow2 ? 54u : 53u)) << 52;
        return bound < r.d - r.d * 0x1p-30;
    }
    const unsigned long long inf = (unsigned long long)(2 * f.emax + 1) << (f.prec - 1);
    const unsigned long long p = round_double_mag_to(abits, f);
    *bits = sign | p;
    if (bound == 0.0) return 1;
    r.u = abits;
    const double a = r.d;
    const double lo = p ? 0.5 * (narrow_mag_value(p - 1, f) + narrow_mag_value(p, f)) : 0.0;
    // (in the cell of Inf, res may lie far above the threshold `lo`, where a - lo would round: a / 2 <= a - lo is exact)
    if (!(bound < (a >= 2.0 * lo ? 0.5 * a : a - lo))) return 0;
    if (p < inf) {
        const double hi = 0.5 * (narrow_mag_value(p, f) + narrow_mag_value(p + 1, f));
        if (!(bound < hi - a)) return 0;
    }
    return 1;
}

}  // namespace exb
