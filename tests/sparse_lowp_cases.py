"""Constructed rows for the narrow ExSpMV / ExSpMM (values in float32, float16 or bfloat16; vectors in float64 or in the
values' type) -- the counterpart of tests/lowp_cases.py for rows of products.

Nothing here touches the GPU or the library.  Only Python integers decide: a row is a list of (value pattern, column)
against a vector of patterns, its exact total an int, its expected output a bit pattern from lowp_cases.round_to.

Units.  Planted totals T are in units of 2^-1074, as in lowp_cases.  A product of two narrow values can be finer than
that (float32: down to 2^-298, in range; but a product of a narrow value and a double can go below 2^-1074), so
row_total() sums in the FINE unit 2^-2148 = (2^-1074)^2, in which the product of any two finite values of the four
formats is an integer; round_fine() rounds such a total into a narrow format (what lies below 2^-1074 can only be sticky
there: the smallest half quantum of the three formats is 2^-150).  alpha enters as the one rounded fp64 multiply
fl64(alpha * W(x)) of the contract, done by numpy in float64; beta is not modelled here (beta = 0).

  table(dtype)            the vector every planted row is read against: 2^b for every exponent b the dtype holds
                          (subnormal powers included), by column b - lo
  split_products(T, dt)   T as a list of (value pattern, b): chunks of at most `prec` bits, each the exact product of one
                          value of the dtype and 2^b from the table
  planted_rows(dt)        rows on every edge of the OUTPUT format dt (values and vector of that type), both signs:
                          exact; tie to even / to odd; the tie +- the smallest reachable unit (the square of the smallest
                          subnormal); the all-ones carry; one unit below and at the overflow threshold; the largest
                          subnormal plus half a quantum; half the smallest subnormal and its two neighbours; cancellation
                          to zero.  The builder asserts that every row's exact total IS its T.
  trap_rows(dt)           rows on which "round to double, then cast" is wrong (asserted): a tie of dt with a perturbation
                          56 to 100 bits below the leading bit (float16: leading bit at 2^14 / 2^15, the perturbation the
                          smallest subnormal squared, 2^-48)
  cell(res, dt)           the rounding cell of a double in the format dt, its two boundaries as exact fractions; and
  endpoint_patterns()     the exact roundings of res - bound and res + bound: the model of the interval certificate
"""
from fractions import Fraction

import numpy as np

import lowp_cases as L
from lowp_cases import FORMATS, U, encode, realise, round_to

UF = 2 * U
NARROW = L.NARROW
PAIRS = [(v, x) for v in NARROW for x in ("float64", v)]


def lo_exp(dtype):
    prec, emin, emax, _ = FORMATS[dtype]
    return emin - (prec - 1)


def pow2_pattern(dtype, b):
    prec, emin, emax, _ = FORMATS[dtype]
    assert lo_exp(dtype) <= b <= emax
    if b >= emin:
        return encode(dtype, False, b + U, 1 << (prec - 1))
    return encode(dtype, False, emin + U, 1 << (b - lo_exp(dtype)))


def table(dtype):
    """patterns of 2^b, b = lo .. emax; column of 2^b: b - lo"""
    return [pow2_pattern(dtype, b) for b in range(lo_exp(dtype), FORMATS[dtype][2] + 1)]


def unit_bit(dtype):
    """bit (in units of 2^-1074) of the smallest product the dtype reaches: its smallest subnormal squared"""
    return 2 * lo_exp(dtype) + U


def split_products(T, dtype):
    """[(value pattern, b)]: T = sum of W(value) * 2^b exactly (asserted by the callers through row_total)"""
    prec, emin, emax, _ = FORMATS[dtype]
    lo = lo_exp(dtype)
    out, neg, M = [], T < 0, abs(T)
    while M:
        top = M.bit_length() - 1
        q = max(top - (prec - 1), (M & -M).bit_length() - 1)
        m = M >> q
        M -= m << q
        s = q - U                                         # the chunk is m * 2^s
        b_lo, b_hi = max(lo, top - U - emax), min(emax, s - lo)
        assert b_lo <= b_hi, "out of the reach of products of the dtype"
        b = min(max(0, b_lo), b_hi)
        pats = realise((-1 if neg else 1) * (m << (s - b + U)), dtype)
        assert pats is not None and len(pats) == 1
        out.append((pats[0], b))
    return out


def fine_units(pattern, dtype):
    """a finite pattern's value in units of 2^-1074 (an int)"""
    return L.value_units(pattern, dtype)


def row_total(val_pats, vt, x_pats, xt, alpha=1.0):
    """the exact total of sum W(val) * fl64(alpha * W(x)) in the FINE unit 2^-2148"""
    tot = 0
    for vp, xp in zip(val_pats, x_pats):
        xu = fine_units(xp, xt)
        if alpha != 1.0:
            xd = np.float64(alpha) * np.float64(Fraction(xu, 1 << U))      # W(x) is a double: the Fraction converts exactly
            xu = fine_units(int(np.array([xd]).view(np.uint64)[0]), "float64")
        tot += fine_units(vp, vt) * xu
    return tot


def round_fine(Tf, dtype):
    """round-to-nearest-even of a total in the fine unit into a NARROW format (the bits below 2^-1074 are sticky)"""
    assert dtype in NARROW
    M = abs(Tf)
    hi = (M >> U) | (1 if M & ((1 << U) - 1) else 0)
    return round_to(-hi if Tf < 0 else hi, dtype) if hi else 0


def parts(dtype, *ts):
    """the entries of a row whose total is sum(ts), every part split on its own (head and perturbation stay apart)"""
    return [e for t in ts for e in split_products(t, dtype)]


class Row:
    __slots__ = ("dtype", "kind", "T", "want", "entries", "must_acc")

    def __init__(self, dtype, kind, T, want, entries=None):
        self.dtype, self.kind, self.T, self.want = dtype, kind, int(T), int(want)
        self.entries = split_products(self.T, dtype) if entries is None else entries
        tot = row_total([p for p, _ in self.entries], dtype, [pow2_pattern(dtype, b) for _, b in self.entries], dtype)
        assert tot == self.T << U, (dtype, kind)           # the row's exact total is its intended T
        assert round_to(self.T, dtype) == self.want, (dtype, kind)
        M = abs(self.T)
        span = (M >> ((M & -M).bit_length() - 1)).bit_length() if M else 0
        # a near-tie that no double holds: the register expansion has a non-zero tail next to a tie, so the row must be
        # rounded from its accumulator
        self.must_acc = span > 53 and kind.split(":")[0] in ("tie+u", "tie-u", "trap")

    def __repr__(self):
        return f"<{self.dtype} {self.kind} {'-' if self.T < 0 else '+'}{abs(self.T).bit_length()}b {len(self.entries)} entries>"


def _around(dtype, ebase, m, unit, tag):
    prec = FORMATS[dtype][0]
    q = ebase - (prec - 1)
    out = []
    if q < 1:
        return out
    base, half = m << q, 1 << (q - 1)
    even = m if m % 2 == 0 else m + 1
    for neg in (False, True):
        s = -1 if neg else 1
        e = lambda mm: encode(dtype, neg, ebase, mm)     # noqa: E731
        out += [Row(dtype, f"exact:{tag}", s * base, e(m)),
                Row(dtype, ("tie_even:" if m % 2 == 0 else "tie_odd:") + tag, s * (base + half), e(even))]
        if unit < half:
            out += [Row(dtype, f"tie+u:{tag}", s * (base + half + unit), e(m + 1), parts(dtype, s * (base + half), s * unit)),
                    Row(dtype, f"tie-u:{tag}", s * (base + half - unit), e(m), parts(dtype, s * (base + half), -s * unit))]
    return out


def planted_rows(dtype):
    prec, emin, emax, width = FORMATS[dtype]
    low, top = emin + U, emax + U
    unit = 1 << unit_bit(dtype)
    ones, mid_even, mid_odd = (1 << prec) - 1, (1 << (prec - 1)) | 2, (1 << (prec - 1)) | 5
    out = [Row(dtype, "cancel", 0, 0, split_products(ones << (U - 3), dtype) + split_products(-(ones << (U - 3)), dtype)),
           Row(dtype, "empty", 0, 0, [])]
    for ebase in sorted({low + 3, U - 7, U, U + 5, top - 1, top}):
        for m in (1 << (prec - 1), mid_even, mid_odd, ones - 1, ones):
            if ebase == top and m == ones:
                continue
            out += _around(dtype, ebase, m, unit, f"e{ebase - U}")
    q = top - (prec - 1)
    thr = (ones << q) + (1 << (q - 1))
    for neg in (False, True):
        s = -1 if neg else 1
        out += [Row(dtype, "below_overflow", s * (thr - unit), encode(dtype, neg, top, ones), parts(dtype, s * thr, -s * unit)),
                Row(dtype, "at_overflow", s * thr, encode(dtype, neg, top, ones + 1)),
                Row(dtype, "above_overflow", s * (thr + unit), encode(dtype, neg, top, ones + 1), parts(dtype, s * thr, s * unit)),
                Row(dtype, "max", s * (ones << q), encode(dtype, neg, top, ones))]
    q = low - (prec - 1)
    for m in (1, 2, 5, (1 << (prec - 2)) | 2, (1 << (prec - 1)) - 2):
        out += _around(dtype, low, m, unit, "sub")
    big = (1 << (prec - 1)) - 1
    for neg in (False, True):
        s, sign = (-1 if neg else 1), ((1 << (width - 1)) if neg else 0)
        out += [Row(dtype, "sub_max+half", s * ((big << q) + (1 << (q - 1))), encode(dtype, neg, low, big + 1)),
                Row(dtype, "half_min", s * (1 << (q - 1)), sign),
                Row(dtype, "half_min+u", s * ((1 << (q - 1)) + unit), sign | 1),
                Row(dtype, "half_min-u", s * ((1 << (q - 1)) - unit), sign, parts(dtype, s * (1 << (q - 1)), -s * unit))]
    return out


def trap_rows(dtype):
    """near-ties of the OUTPUT format that a double cannot tell from the tie; .kind "trap:<bits below the leading bit>" """
    prec, emin, emax, width = FORMATS[dtype]
    out = []
    tiny_bit = unit_bit(dtype) if dtype == "float16" else U - 60       # float16: 2^-48; the others: 2^-60 = 2^-30 * 2^-30
    for lead in ((14, 15) if dtype == "float16" else (0, 3, 20)):
        ebase = lead + U
        depth = ebase - tiny_bit
        assert 56 <= depth <= 100
        q = ebase - (prec - 1)
        for m, d in (((1 << (prec - 1)) | 2, 1), ((1 << (prec - 1)) | 5, -1)):
            for s in (1, -1):
                T = s * ((m << q) + (1 << (q - 1)) + d * (1 << tiny_bit))
                one, two = round_to(T, dtype), L.double_then_cast(T, dtype)
                assert one != two and one == encode(dtype, s < 0, ebase, m + (1 if d > 0 else 0))
                head = s * ((m << q) + (1 << (q - 1)))
                out.append(Row(dtype, f"trap:{depth}", T, one, parts(dtype, head, T - head)))
    return out


def all_rows(dtype):
    return planted_rows(dtype) + trap_rows(dtype)


# ---------------------------------------------------------------------------------------------
# the certificate's model: rounding boundaries as exact numbers
# ---------------------------------------------------------------------------------------------
def pattern_value(bits, dtype):
    """the magnitude pattern `bits` (no sign) as a Fraction; the Inf pattern counts as 2^(emax + 1)"""
    prec, emin, emax, width = FORMATS[dtype]
    e, m = bits >> (prec - 1), bits & ((1 << (prec - 1)) - 1)
    sig, ex = ((m | (1 << (prec - 1))), e - 1) if e else (m, 0)
    return Fraction(sig) * Fraction(2) ** (ex + emin - (prec - 1))


def cell(res, dtype):
    """(pattern, lower boundary, upper boundary) of the rounding cell that the double res != 0 (as a Fraction) lies in, magnitudes: the
    boundaries are the midpoints to the neighbouring values (towards zero the cell of 0 ends AT 0: the other side rounds
    to the other zero); upper is None in the cell of Inf"""
    prec, emin, emax, width = FORMATS[dtype]
    Tf = abs(res) * (1 << UF)
    assert Tf.denominator == 1                         # every double is an integer in the fine unit
    p = round_fine(int(Tf), dtype)
    inf = (2 * emax + 1) << (prec - 1)
    lower = (pattern_value(p - 1, dtype) + pattern_value(p, dtype)) / 2 if p else Fraction(0)
    upper = (pattern_value(p, dtype) + pattern_value(p + 1, dtype)) / 2 if p < inf else None
    return p, lower, upper


def sign_bit(dtype):
    return 1 << (FORMATS[dtype][3] - 1)


def endpoint_patterns(res, bound, dtype):
    """the patterns that the two ends of [res - bound, res + bound] (doubles, so integers in the fine unit) round to"""
    r, b = Fraction(res), Fraction(bound)
    ends = []
    for v in (r - b, r + b):
        Tf = v * (1 << UF)
        assert Tf.denominator == 1
        pat = round_fine(int(Tf), dtype)
        ends.append(pat)
    return ends


def double_of(T):
    """(RN64(T) as a float, a double >= |T - RN64(T)| that is 0 exactly when T is a double)"""
    d = round_to(T, "float64")
    res = float(np.array([d], dtype=np.uint64).view(np.float64)[0])
    err = abs(Fraction(T, 1 << U) - Fraction(res))
    b = float(err)
    if Fraction(b) < err:
        b = float(np.nextafter(b, np.inf))
    return res, b
