"""Constructed ExSUM / ExDOT inputs, and raw limb sets for the finalize kernel, whose exact totals are known as Python
integers -- the blas1 counterpart of tests/exact_cases.py.

Nothing here touches the GPU, the library or the oracle.  Every exact total T is a Python int in units of 2^-1074, the
least significant bit of the accumulator (and of the doubles).  The expected values of a case are
  the double          exact_cases.round_nearest_even(Fraction(T, 2**1074))
  the digits          helpers.digits_from_int(T)        68 digits, 32 bits apart, the top one signed
  the canonical limbs canon_from_int(T)                 41 fields of 52 bits of T << 18, the top one signed
Every term is built as m * 2^s units with |m| < 2^53 and converted to a double by `term`, which asserts that the
double converts back to exactly that integer (`units`); every constructor asserts that the exact sum of its own
terms -- sum(Fraction(x)), taken in integer units -- is T.

Families (the rounding code they aim at: finish_wave in exblas_amd/csrc/superacc.hip.h, k_finalize in blas1.hip):
  A  position sweep: a 53-bit mantissa M (even, odd, all ones) with its leading bit at every position p = 53 .. 2097,
     alone (``exact``), plus half a unit in the last place (``tie``), plus that and one unit more / less (``tie+1`` /
     ``tie-1``: the latter leaves a run of all-ones digits below the half bit), plus a quarter unit (``below``), plus /
     minus one unit (``+1`` / ``-1``: a sticky bit up to 65 limbs below the rounding window).  With h = p - 53 == 0 the
     half unit is the unit itself: only ``exact`` and ``tie`` exist there.  Both signs.  Every leading-zero count of the
     top digit (0 .. 31) in every limb 1 .. 65; the all-ones ties at p = 2097 round to +-Inf.
  B  small totals, at most 53 bits (nothing to round) and just above, and totals that straddle limb 0 / limb 1.
  C  carry and borrow chains: +-(2^a - 2^b) given as its two terms, -2^a + 1, and 2^a - 1 - 2^a = -1 (every digit
     0xffffffff).  `ones_run` is the number of consecutive 0xffffffff digits among the 67 unsigned ones, asserted
     against a closed form.
  D  beyond the double range and back: k copies of a huge value followed by k - 1 copies of its negative and a tail.
     The running total passes 2^1024 (k = 16384 fills limb 65, k = 16385 reaches limb 66) and the positives come first, so that an
     expansion without the 2^1000 guard overflows; magnitudes DBL_MAX, 2^1000 and 2^1000 (1 - 2^-53) (either side of
     the guard's threshold).  And DBL_MAX + 2^970 (a tie that rounds to Inf), DBL_MAX + 2^970 - 2^-1074 (DBL_MAX).
  E  raw limb sets for exblas_finalize_dev: [nsets, 72] int64, un-normalised words below 2^63 in magnitude -- what the
     kernel reads from the group accumulators.  Limbs of +-(2^62 + small) whose naive int64 sum over the sets overflows
     (asserted), a carry and a borrow ripple through all 67 lanes, totals with the top in limb 66 / 67, the top limb
     alone negative.  A total of 2^2125 units or more does not fit the canonical limbs (`canon` is None there).
  F  ExDOT: a main part H (totals of A and B, as products x * 1.0) plus a part f below one unit made of products below
     2^-1074 -- exactly 1/2, 1/2 +- 2^-1200, 2^-1200, 1 - 2^-1200 units-and-below, and parts that add up to exactly 0 or
     exactly one unit -- in all four sign combinations; and products beyond 2^1024 that cancel onto a tie of A or add up
     to +-2^2175, +-(2^2175 - 2^2100), +-2^2176 units, either side of what the 68 digits hold.  `exact` is the Fraction
     sum of the products, `flags` the record's flag word.
"""
import functools
import math
from fractions import Fraction

import numpy as np

import exact_cases as X
from helpers import digits_from_int

U = 1074                                  # T counts units of 2^-U
ONE = 1 << U
NDIG = 68
DIGIT = 0xffffffff
P_MIN, P_MAX = 53, 2097                   # leading-bit positions of Family A (2097: the binade of DBL_MAX)
DBL_MAX_UNITS = ((1 << 53) - 1) << (P_MAX - 52)
CANON_LIMIT = 1 << (52 * 40 - 18 + 63)    # |T| below this fits the signed top canonical limb
DIGITS_LIMIT = 1 << (32 * NDIG - 1)       # -DIGITS_LIMIT <= T < DIGITS_LIMIT fits 68 digits of 32 bits, the top one signed
FLAG_PINF, FLAG_NINF, FLAG_PUNDER, FLAG_POVER, FLAG_PLOW_EXACT, FLAG_PHIGH_EXACT = 1, 2, 8, 16, 32, 64
A_KINDS = ("exact", "tie", "tie+1", "tie-1", "below", "+1", "-1")
A_MANTISSAS = ("even", "odd", "ones")


class Case:
    """one constructed input: family, kind (how it was built), cls (exact_cases.classify of T), terms (float64 tuple),
    T, want; p and mant for Family A; a, b, exact, flags for ExDOT; sets, ones_run, canon for E / C"""
    __slots__ = ("family", "kind", "cls", "p", "mant", "terms", "T", "want", "a", "b", "exact", "flags", "sets", "ones_run")

    def __init__(self, family, kind, T, terms=(), **kw):
        for s in self.__slots__:
            setattr(self, s, None)
        self.family, self.kind, self.T, self.terms = family, kind, int(T), tuple(terms)
        self.cls = X.classify(T)[0]
        self.want = X.round_nearest_even(Fraction(self.T, ONE))
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        if self.T is None:
            return f"<{self.family} {self.kind} p={self.p} {self.mant} want={self.want!r} flags={self.flags}>"
        return f"<{self.family} {self.kind} p={self.p} {self.mant} T={'-' if self.T < 0 else '+'}{abs(self.T).bit_length()}b>"


# ---------------------------------------------------------------------------------------------
# integers <-> doubles, digits, canonical limbs
# ---------------------------------------------------------------------------------------------
def units(x):
    """a finite double as an exact integer count of 2^-1074"""
    n, d = float(x).as_integer_ratio()
    assert ONE % d == 0
    return n * (ONE // d)


@functools.lru_cache(maxsize=None)
def term(m, s):
    """m * 2^s units as a double, asserting that it converts back to exactly that"""
    assert abs(m) < 1 << 53 and s >= 0
    x = math.ldexp(float(m), s - U)
    assert units(x) == m << s, "a term is not representable as a double"
    return x


def total_of(terms):
    """sum(Fraction(x)) over the terms, in units (an int)"""
    return sum(units(x) for x in terms)


def canon_from_int(T):
    """the 41 canonical limbs (52 bits each, limb j weighs 2^(52 (j - 21))) of T units: fields of T << 18, all in
    [0, 2^52) but the signed top one"""
    assert -CANON_LIMIT <= T < CANON_LIMIT, "the total does not fit the canonical limbs"
    v = int(T) << 18
    out = [(v >> (52 * j)) & ((1 << 52) - 1) for j in range(40)]
    out.append(v >> (52 * 40))
    return np.array(out, dtype=np.int64)


def canon_fits(T):
    return -CANON_LIMIT <= T < CANON_LIMIT


def digits_matrix(Ts):
    """[n, 68] int64: helpers.digits_from_int of every T, vectorised (the GPU tests compare whole records at once)"""
    nd = NDIG + 2
    raw = b"".join(int(T).to_bytes(4 * nd, "little", signed=True) for T in Ts)
    d = np.frombuffer(raw, dtype="<u4").reshape(len(Ts), nd).astype(np.int64)
    out = d[:, :NDIG].copy()
    out[:, NDIG - 1] |= d[:, NDIG] << 32                 # (int64 wraps: the signed top digit)
    return out


def canon_matrix(Ts):
    """[n, 41] int64: canon_from_int of every T, vectorised; every T must fit"""
    assert all(canon_fits(T) for T in Ts)
    nd = NDIG + 2
    raw = b"".join((int(T) << 18).to_bytes(4 * nd, "little", signed=True) for T in Ts)
    d = np.frombuffer(raw, dtype="<u4").reshape(len(Ts), nd).astype(np.uint64)
    out = np.zeros((len(Ts), 41), dtype=np.int64)
    for j in range(41):
        q, r = (52 * j) >> 5, np.uint64((52 * j) & 31)
        lo, hi = d[:, q] | (d[:, q + 1] << np.uint64(32)), d[:, q + 2] | (d[:, q + 3] << np.uint64(32))
        win = (lo >> r) | (hi << (np.uint64(64) - r)) if r else lo
        out[:, j] = (win if j == 40 else win & np.uint64((1 << 52) - 1)).view(np.int64)
    return out


def ones_run(T):
    """the longest run of consecutive 0xffffffff digits among the 67 unsigned digits of T"""
    best = run = 0
    for d in digits_from_int(T)[:NDIG - 1].tolist():
        run = run + 1 if d == DIGIT else 0
        best = max(best, run)
    return best


def _mantissa(name, p):
    if name == "ones":
        return (1 << 53) - 1
    m = (1 << 52) | ((0x9E3779B97F4A7C15 * (p + 1)) & ((1 << 52) - 2))    # 53 bits that change with p, even
    return m | 1 if name == "odd" else m


def _signed(family, kind, sign, spec, **kw):
    """one case from (m, s) pairs, negated as a whole for sign = -1"""
    terms = [term(sign * m, s) for m, s in spec]
    T = sign * sum(m << s for m, s in spec)
    assert total_of(terms) == T
    return Case(family, kind, T, terms, **kw)


# ---------------------------------------------------------------------------------------------
# Family A
# ---------------------------------------------------------------------------------------------
def a_specs(p, M):
    """kind -> (m, s) pairs for the mantissa M with its leading bit at position p"""
    s, h = p - 52, p - 53
    base = (M, s)
    out = {"exact": [base], "tie": [base, (1, h)]}
    if h >= 1:     # (with h == 0 the half unit is bit 0: the other kinds need bits below it, or are the tie again)
        out.update({"tie+1": [base, (1, h), (1, 0)], "tie-1": [base, (1, h), (-1, 0)], "below": [base, (1, h - 1)],
                    "+1": [base, (1, 0)], "-1": [base, (-1, 0)]})
    return out


def family_a(positions=None, kinds=A_KINDS, signs=(1, -1)):
    full = positions is None and kinds == A_KINDS and signs == (1, -1)
    out = []
    for p in (range(P_MIN, P_MAX + 1) if positions is None else positions):
        for name in A_MANTISSAS:
            M = _mantissa(name, p)
            assert M.bit_length() == 53 and (M & 1) == (name != "even")
            for kind, spec in a_specs(p, M).items():
                if kind in kinds:
                    for sign in signs:
                        c = _signed("A", kind, sign, spec, p=p, mant=name)
                        assert abs(c.T).bit_length() - 1 == p
                        out.append(c)
    if full:
        assert len(out) == 85860 and sum(len(c.terms) for c in out) == 183978
        ties_away = sum(1 for c in out if c.kind == "tie" and (math.isinf(c.want) or abs(units(c.want)) > abs(c.T)))
        assert ties_away == 8180 == sum(1 for c in out if c.kind == "tie" and c.mant != "even")
        assert sum(1 for c in out if math.isinf(c.want)) == 4
    return out


def a_positions_for_limbs(limbs):
    """the positions p whose top digit lies in one of `limbs`: every leading-zero count 0 .. 31 in each"""
    return [32 * t + 31 - lz for t in limbs for lz in range(32) if P_MIN <= 32 * t + 31 - lz <= P_MAX]


# ---------------------------------------------------------------------------------------------
# Family B
# ---------------------------------------------------------------------------------------------
def family_b():
    out = [Case("B", "zero by cancellation", 0, (term(12345, 700), term(-12345, 700))),
           Case("B", "zero by cancellation, three terms", 0, (term(3, 0), term(-1, 1), term(-1, 0)))]
    two53 = [(1, 53)]
    specs = [("1", [(1, 0)]), ("2^52-1", [((1 << 52) - 1, 0)]), ("2^53-1", [((1 << 53) - 1, 0)]), ("2^53", two53),
             ("2^53+1 tie to even", two53 + [(1, 0)]), ("2^53+3 tie away", [((1 << 52) + 1, 1), (1, 0)]),
             ("2^53+2^32+1", [((1 << 21) + 1, 32), (1, 0)]), ("2^53+2^32-1", [((1 << 21) + 1, 32), (-1, 0)]),
             # limb 0 / limb 1
             ("2^32-1", [(DIGIT, 0)]), ("2^32", [(1, 32)]), ("2^32+1", [(1, 32), (1, 0)]),
             ("2^32-1 by borrow", [(1, 32), (-1, 0)]), ("2^32 by carry", [(DIGIT, 0), (1, 0)]),
             ("2^31+2^31", [(1, 31), (1, 31)]), ("2^33-1", [((1 << 33) - 1, 0)]),
             ("(2^53-1) 2^11: limbs 0..1 full above bit 11", [((1 << 53) - 1, 11)]),
             ("2^64-1 by borrow", [(1, 64), (-1, 0)]), ("2^52+2^31 across the boundary", [((1 << 21) + 1, 31)])]
    for kind, spec in specs:
        for sign in (1, -1):
            out.append(_signed("B", kind, sign, spec))
    assert {c.T for c in out} >= {0, 1, -1, (1 << 52) - 1, -(1 << 53) + 1, 1 << 53, -(1 << 53), (1 << 53) + 3}
    assert [c.want for c in out if c.kind.startswith("2^53+1")] == [math.ldexp(1.0, 53 - U), -math.ldexp(1.0, 53 - U)]
    return out


# ---------------------------------------------------------------------------------------------
# Family C
# ---------------------------------------------------------------------------------------------
C_A = (64, 1024, 2047, 2048, 2049, 2080, 2097)


def _c_run(a, b, sign):
    """closed form of ones_run for sign (2^a - 2^b), b < a: bits b .. a-1 are ones for the positive value; the negative
    one is ... 1 1 1 [bit a] 0 .. 0 1 [bit b] 0 .. 0 in two's complement (all ones from bit b up when b == a - 1)"""
    if sign > 0:
        return max(0, a // 32 - (b + 31) // 32)
    low = b if b == a - 1 else a
    return (NDIG - 1) - (low + 31) // 32


def family_c():
    out = []
    for a in C_A:
        for b in sorted({0, 31, 32, 33, a - 54, a - 53, a - 1}):
            if 0 <= b < a:
                for sign in (1, -1):
                    c = _signed("C", f"2^{a}-2^{b}", sign, [(1, a), (-1, b)])
                    c.ones_run = ones_run(c.T)
                    assert c.ones_run == _c_run(a, b, sign), (a, b, sign, c.ones_run)
                    out.append(c)
        c = _signed("C", f"-2^{a}+1", 1, [(-1, a), (1, 0)])
        c.ones_run = ones_run(c.T)
        assert c.ones_run == _c_run(a, 0, -1)
        out.append(c)
        # 2^a - 1 - 2^a = -1: every unsigned digit 0xffffffff, the highest non-zero raw limb is limb 0
        c = Case("C", f"2^{a}-1-2^{a}", -1, (term(1, a), term(-1, 0), term(-1, a)))
        assert total_of(c.terms) == -1
        c.ones_run = ones_run(c.T)
        assert c.ones_run == NDIG - 1
        out.append(c)
    assert max(c.ones_run for c in out if c.T > 0) >= 65 and max(c.ones_run for c in out) == 67
    return out


# ---------------------------------------------------------------------------------------------
# Family D
# ---------------------------------------------------------------------------------------------
D_K = (2, 16384)


def family_d():
    big = {"DBL_MAX": ((1 << 53) - 1, P_MAX - 52), "2^1000": (1, 1000 + U), "2^1000(1-2^-53)": ((1 << 53) - 1, 1000 + U - 53)}
    p_tail = 1100
    tie_tail = a_specs(p_tail, _mantissa("odd", p_tail))["tie"]             # a Family A tie, far below the huge value
    out = []
    for name, (m, s) in big.items():
        half_ulp = [(1, (m << s).bit_length() - 54)]                        # makes what is left of the huge value a tie
        for k in D_K + ((16385,) if name == "DBL_MAX" else ()):
            for tname, tail in (("A tie", tie_tail), ("half ulp", half_ulp)):
                for sign in (1, -1):
                    terms = [term(sign * m, s)] * k + [term(-sign * m, s)] * (k - 1) + [term(sign * tm, ts) for tm, ts in tail]
                    T = sign * ((m << s) + sum(tm << ts for tm, ts in tail))
                    assert total_of(terms) == T
                    assert sum(units(x) for x in terms[:k]) == sign * k * (m << s)
                    out.append(Case("D", f"{k} x {name}, {k - 1} back, {tname}", T, terms))
    # 16384 DBL_MAX = 2^2112 - 2^2059 fills limb 65 to its last bit; one copy more and the running total is in limb 66
    assert (16384 * DBL_MAX_UNITS).bit_length() == 32 * 66 and (16385 * DBL_MAX_UNITS).bit_length() - 1 == 32 * 66
    for sign in (1, -1):
        out.append(_signed("D", "DBL_MAX+2^970", sign, [big["DBL_MAX"], (1, 970 + U)]))
        out.append(_signed("D", "DBL_MAX+2^970-1", sign, [big["DBL_MAX"], (1, 970 + U), (-1, 0)]))
    inf = [c.want for c in out if c.kind == "DBL_MAX+2^970"]
    assert inf == [math.inf, -math.inf]
    assert [c.want for c in out if c.kind == "DBL_MAX+2^970-1"] == [1.7976931348623157e308, -1.7976931348623157e308]
    return out


# ---------------------------------------------------------------------------------------------
# Family E
# ---------------------------------------------------------------------------------------------
E_NSETS = (1, 2, 15, 16, 17, 33)
SET_WORDS = 72


def _e_case(kind, sets):
    sets = np.asarray(sets, dtype=object)
    assert sets.shape[1] == SET_WORDS and all(int(v) == 0 for v in sets[:, NDIG:].ravel())
    assert all(abs(int(v)) < 1 << 63 for v in sets.ravel()), "a raw limb reaches 2^63"
    T = sum(int(v) << (32 * l) for row in sets for l, v in enumerate(row[:NDIG]))
    assert -DIGITS_LIMIT <= T < DIGITS_LIMIT
    top = sum(int(row[NDIG - 1]) for row in sets)
    assert abs(top) < 1 << 62                                              # (the top limb is added unsplit)
    return Case("E", kind, T, sets=np.array(sets.tolist(), dtype=np.int64))


def _spread(limbs, nsets):
    """one limb vector dealt over nsets sets: limb l goes to set l % nsets (the total is unchanged)"""
    sets = [[0] * SET_WORDS for _ in range(nsets)]
    for l, v in enumerate(limbs):
        sets[l % nsets][l] = v
    return sets


def naive_sum_overflows(sets):
    """does a plain int64 sum of the sets overflow in some limb?"""
    tot = np.asarray(sets, dtype=object).sum(axis=0)
    return any(not -(1 << 63) <= int(v) < (1 << 63) for v in tot)


def family_e():
    out = []
    rng = np.random.default_rng(20261018)
    # limbs of +-(2^62 + small) in limbs 0 .. top: top = 40 stays a finite double, top = 64 rounds to +-Inf
    for nsets in E_NSETS:
        for top, pattern in ((40, "+"), (40, "-"), (40, "+-"), (64, "+"), (64, "-"), (11, "-+")):
            sets = [[0] * SET_WORDS for _ in range(nsets)]
            for g in range(nsets):
                for l in range(top + 1):
                    sg = {"+": 1, "-": -1, "+-": 1 if l % 2 == 0 else -1, "-+": -1 if l % 3 == 0 else 1}[pattern]
                    sets[g][l] = sg * ((1 << 62) + int(rng.integers(0, 1 << 40)))
            c = _e_case(f"2^62 limbs {pattern} to limb {top}, {nsets} sets", sets)
            assert naive_sum_overflows(sets) == (nsets >= 2), "the low / high split is not under test"
            out.append(c)
    ripple = [DIGIT] * (NDIG - 1) + [0]
    neg_top = [0x7fffffff] * (NDIG - 1) + [-1]
    for i, nsets in enumerate(E_NSETS):
        up = list(ripple)
        up[0] += 1                                                         # 2^2144: the carry runs through 67 lanes
        out.append(_e_case(f"carry ripple, {nsets} sets", _spread(up, nsets)))
        out.append(_e_case(f"carry ripple negated, {nsets} sets", _spread([-v for v in up], nsets)))
        out.append(_e_case(f"ripple one short of the carry, {nsets} sets", _spread(ripple, nsets)))
        out.append(_e_case(f"borrow ripple 2^2144-1, {nsets} sets", _spread([-1] + [0] * (NDIG - 2) + [1], nsets)))
        if nsets >= 2:                                                     # the one that carries comes from another set
            two = _spread(ripple, nsets - 1) + [[1] + [0] * (SET_WORDS - 1)]
            out.append(_e_case(f"carry ripple, the unit in its own set, {nsets} sets", two))
        # the top in limb 66 / 67, both signs; alone they round to +-Inf (no flag), a second set cancels them back
        for l in (66, 67):
            for sign in (1, -1):
                v = [0] * NDIG
                v[l], v[5], v[0] = sign * (5 + i), 0x12345678, 7
                out.append(_e_case(f"top in limb {l} sign {sign}, {nsets} sets", _spread(v, nsets)))
                back = [0] * SET_WORDS
                back[l], back[5], back[0] = -v[l], -v[5], -v[0]
                back[40], back[39] = -sign * ((1 << 52) + 1), -sign * (1 << 31)              # what is left: a tie, odd mantissa
                out.append(_e_case(f"top in limb {l} sign {sign} cancelled, {nsets + 1} sets", _spread(v, nsets) + [back]))
        out.append(_e_case(f"top limb alone negative, {nsets} sets", _spread(neg_top, nsets)))
        small_neg = [0] * NDIG
        small_neg[NDIG - 1], small_neg[NDIG - 2], small_neg[3] = -1, DIGIT, 1 << 40          # -2^2112 + ...
        out.append(_e_case(f"top limb -1 over a full limb 66, {nsets} sets", _spread(small_neg, nsets)))
    assert any(c.T == 1 << (32 * 67) for c in out) and any(c.T == -(1 << (32 * 67)) for c in out)
    assert any(math.isinf(c.want) for c in out) and any(math.isfinite(c.want) and c.want != 0 for c in out)
    assert any(c.cls == "tie" for c in out)
    return out


# ---------------------------------------------------------------------------------------------
# Family F
# ---------------------------------------------------------------------------------------------
def _p2(e):
    return math.ldexp(1.0, e)


# parts below one unit as products (a, b), all below 2^-968: name -> (pairs, exact value in units as a Fraction)
F_PARTS = {
    "1/2": [(_p2(-537), _p2(-538))],
    "1/2+2^-1200": [(_p2(-537), _p2(-538)), (_p2(-600), _p2(-600))],
    "1/2-2^-1200": [(_p2(-537), _p2(-538)), (-_p2(-600), _p2(-600))],
    "2^-1200": [(_p2(-600), _p2(-600))],
    "1-2^-1200": [(_p2(-537), _p2(-537)), (-_p2(-600), _p2(-600))],
    "sum 0": [(_p2(-600), _p2(-600)), (-_p2(-600), _p2(-600))],
    "sum 1 unit": [(_p2(-537), _p2(-538)), (_p2(-537), _p2(-538))],
}
F_LIMBS = (3, 40)          # limb 3: H itself consists of products below 2^-968 (it is summed in the low accumulator)


def dot_flags(pairs, exact):
    """the record's flag word by the rules of include/exblas_hip.h, from the exact products: bit 3 + bit 5 when a product
    of two non-zero operands is below 2^-968, bit 4 + bit 6 when a product of finite operands is 2^1024 or more, and
    then bit 0 / bit 1 when the exact sum is beyond what the 68 digits (32 bits each, the top one signed) hold"""
    prods = [abs(Fraction(float(x)) * Fraction(float(y))) for x, y in pairs]
    fl = 0
    if any(0 < q < Fraction(1, 1 << 968) for q in prods):
        fl |= FLAG_PUNDER | FLAG_PLOW_EXACT
    if any(q >= 1 << 1024 for q in prods):
        fl |= FLAG_POVER | FLAG_PHIGH_EXACT
        S = exact * ONE
        fl |= FLAG_PINF if S >= DIGITS_LIMIT else (FLAG_NINF if S < -DIGITS_LIMIT else 0)
    return fl


def _dot_case(kind, pairs, **kw):
    a = np.array([p[0] for p in pairs], dtype=np.float64)
    b = np.array([p[1] for p in pairs], dtype=np.float64)
    exact = sum((Fraction(float(x)) * Fraction(float(y)) for x, y in pairs), Fraction(0))
    flags = dot_flags(pairs, exact)
    c = Case("F", kind, 0, a=a, b=b, exact=exact, flags=flags, **kw)
    c.T, c.cls = None, None
    c.want = X.round_nearest_even(exact)
    return c


def family_f_low(positions=None):
    """H + f: (case list).  H from Family A (kinds exact, tie, tie-1; the three mantissas; 64 positions: every
    leading-zero count in limbs 3 and 40 -- or the given positions, for a small batch) and from the positive totals of
    Family B"""
    hs = [c for c in family_a(a_positions_for_limbs(F_LIMBS) if positions is None else positions,
                              kinds=("exact", "tie", "tie-1"), signs=(1,))]
    hs += [c for c in family_b() if c.T >= 0]
    assert positions is not None or len(a_positions_for_limbs(F_LIMBS)) == 64
    assert any(c.T == (1 << 53) - 1 for c in hs)
    out = []
    for h in hs:
        for fname, pairs in F_PARTS.items():
            for sh in (1, -1):
                for sf in (1, -1):
                    prods = [(sh * x, 1.0) for x in h.terms] + [(sf * x, y) for x, y in pairs]
                    c = _dot_case(f"{h.family}:{h.kind} {'+' if sh > 0 else '-'}H {'+' if sf > 0 else '-'}f {fname}", prods,
                                  p=h.p, mant=h.mant)
                    assert c.flags == FLAG_PUNDER | FLAG_PLOW_EXACT
                    f_exact = sf * sum(Fraction(x) * Fraction(y) for x, y in pairs)
                    assert c.exact == Fraction(sh * h.T, ONE) + f_exact and abs(f_exact) * ONE <= 1
                    out.append(c)
    return out


def family_f_high():
    out = []
    EX = FLAG_POVER | FLAG_PHIGH_EXACT
    cancel = [(_p2(600), _p2(500)), (-_p2(600), _p2(500))]                  # +-2^1100
    # 2^1024 - (2^1024 - 2^971) = 2^971: two overflowing products that leave one unit in the last place of DBL_MAX's binade
    near = [(_p2(512), _p2(512)), (-_p2(512), _p2(512) * (1 - 2.0 ** -53))]
    for p in (2040, 2096, 2097):
        for h in family_a([p], kinds=("tie", "tie+1", "tie-1")):
            hp = [(x, 1.0) for x in h.terms]
            c = _dot_case(f"cancel onto A:{h.kind} p={p}", cancel[:1] + hp + cancel[1:], p=p, mant=h.mant)
            # (the deciding unit of tie+1 / tie-1 is itself a product below 2^-968: all four product flags)
            assert c.exact == Fraction(h.T, ONE) and c.flags == EX | (0 if h.kind == "tie" else FLAG_PUNDER | FLAG_PLOW_EXACT)
            out.append(c)
        for h in family_a([p], kinds=("exact",), signs=(1,)):
            if p < P_MAX:      # H + 2^971 stays finite
                out.append(_dot_case(f"near-cancel 2^971 onto A:exact p={p}", near[:1] + [(x, 1.0) for x in h.terms] + near[1:],
                                     p=p, mant=h.mant))
                assert out[-1].flags == EX
    sums = {"2^2175": [(_p2(600), _p2(501))], "2^2176": [(_p2(600), _p2(502))],
            "2^2175-2^2100": [(_p2(600), _p2(501)), (-_p2(600), _p2(426))]}
    for name, pairs in sums.items():
        for sign in (1, -1):
            prods = [(3.0, 5.0)] + [(sign * x, y) for x, y in pairs]
            S = sum(Fraction(x) * Fraction(y) for x, y in prods) * ONE
            assert S.denominator == 1 and abs(S.numerator - 15 * ONE) == {"2^2175": 1 << 2175, "2^2176": 1 << 2176,
                                                                         "2^2175-2^2100": (1 << 2175) - (1 << 2100)}[name]
            # what the 68 digits cannot hold is reported like an infinity in the input (include/exblas_hip.h, flags bit 0 / 1)
            S = S.numerator
            fl = EX | (FLAG_PINF if S >= DIGITS_LIMIT else (FLAG_NINF if S < -DIGITS_LIMIT else 0))
            c = _dot_case(f"{'+' if sign > 0 else '-'}({name}) units", prods)
            assert math.isinf(c.want) and (c.want > 0) == (sign > 0) and c.flags == fl
            out.append(c)
    assert {c.flags for c in out} == {EX, EX | FLAG_PINF, EX | FLAG_NINF, EX | FLAG_PUNDER | FLAG_PLOW_EXACT}
    return out


def family_f():
    return family_f_low() + family_f_high()


# ---------------------------------------------------------------------------------------------
# shared views
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sum_cases():
    """all of A, B, C, D, in that order (built once)"""
    return tuple(family_a() + family_b() + family_c() + family_d())


def kind_counts(cases):
    """{(family, kind, sign): count} -- sign by the expected double ('0' for a zero)"""
    out = {}
    for c in cases:
        v = c.want
        key = (c.family, c.kind, "+" if v > 0 else ("-" if v < 0 else "0"))
        out[key] = out.get(key, 0) + 1
    return out


def stride_sample(cases, count):
    """at least `count` cases (all of them if there are fewer), evenly strided within every kind so that none is left out"""
    by_kind = {}
    for c in cases:
        by_kind.setdefault((c.family, c.kind), []).append(c)
    per = -(-count // len(by_kind))
    while True:
        out = []
        for group in by_kind.values():
            out += group[::max(1, len(group) // per)]
        if len(out) >= min(count, len(cases)):
            return out
        per *= 2
