"""Constructed inputs and totals for the narrow-input ExSUM / ExDOT (float32, float16, bfloat16) and for the rounding of
a digit set into a narrow format -- the counterpart of tests/blas1_cases.py.

Nothing here touches the GPU or the library.  Every total T is a Python int in units of 2^-1074; every expected value
is a bit pattern (a Python int) computed from Python integers.  A format is (precision, emin, emax, width):
  float64 53 -1022 1023 64   float32 24 -126 127 32   float16 11 -14 15 16   bfloat16 8 -126 127 16

  units(x[, y])        the exact total of an array of any of the four dtypes (numpy, or a torch tensor: bfloat16), or
                       of the element-wise products of two such arrays, as an int
  round_to(T, dtype)   round-to-nearest-even of T into the format; `mutant` selects one of the four wrong roundings
                       the planted totals must be seen to tell apart (MUTANTS)
  planted(dtype)       totals aimed at the rounding code, for the TARGET format `dtype`: a significand m placed with its
                       quantum at bit q, both signs, in normal binades and (narrow targets) in the subnormal range --
                       exact; tie to even; tie to odd; tie +- one unit of 2^-1074 (the sticky bit in the lowest digit,
                       up to 65 digits below the rounding position); all-ones significands (the carry into the next
                       binade); one below and at the overflow threshold; the largest subnormal plus half a quantum;
                       half the smallest subnormal (a tie to zero) and one unit above it; and 0.  `want` of every case is
                       written down from its construction (encode), not from round_to.
  traps(dtype)         totals whose "round to double, then cast" answer differs from the single rounding (asserted)
  realise(T, dtype)    bit patterns of a short array of the INPUT dtype whose exact sum is T (None when T has bits the
                       dtype cannot reach); input_cases(dtype) are the planted-style totals scaled into that reach, the
                       dtype's subnormals and largest finite values among the terms
  dot_range_pairs      ExDOT operands whose products reach 2^-298 (float32: the smallest subnormal squared) and nearly
                       2^256 (the largest finite value squared)
  NONFINITE            tables with +Inf, -Inf, both, NaN and Inf x 0
"""
import numpy as np

U = 1074
FORMATS = {"float64": (53, -1022, 1023, 64), "float32": (24, -126, 127, 32), "float16": (11, -14, 15, 16),
           "bfloat16": (8, -126, 127, 16)}
NARROW = ("float32", "float16", "bfloat16")
ALL = ("float64",) + NARROW
DT_CODE = {"float64": 0, "float32": 1, "float16": 2, "bfloat16": 3}
NDIG = 68
MUTANTS = ("sticky_next_digit", "ties_away", "flush_subnormal", "overflow_late")


def name_of(dtype):
    return str(dtype).rsplit(".", 1)[-1] if not isinstance(dtype, (np.dtype, type)) else np.dtype(dtype).name


# ---------------------------------------------------------------------------------------------
# bit patterns <-> integers
# ---------------------------------------------------------------------------------------------
class Raw:
    """bfloat16 patterns (uint16 words) where no torch tensor is at hand"""
    def __init__(self, p):
        self.p = np.asarray(p, dtype=np.uint16)


def patterns(x):
    """(unsigned bit patterns as a numpy array, format name) of a numpy array, a torch tensor of one of the four dtypes,
    or Raw bfloat16 words"""
    if isinstance(x, Raw):
        return x.p.reshape(-1), "bfloat16"
    if hasattr(x, "data_ptr"):                       # torch
        import torch
        name = name_of(x.dtype)
        width = FORMATS[name][3]
        it = {64: torch.int64, 32: torch.int32, 16: torch.int16}[width]
        x = x.detach().cpu().contiguous().view(it).numpy()
    else:
        x = np.ascontiguousarray(x)
        name = x.dtype.name
        width = FORMATS[name][3]
    return x.reshape(-1).view({64: np.uint64, 32: np.uint32, 16: np.uint16}[width]), name


def _split(pat, name):
    """signed significands (int64) and unit shifts (value = m * 2^shift units) of finite patterns"""
    prec, emin, emax, width = FORMATS[name]
    p = pat.astype(np.uint64)
    frac = (p & np.uint64((1 << (prec - 1)) - 1)).astype(np.int64)
    e = ((p >> np.uint64(prec - 1)) & np.uint64((1 << (width - prec)) - 1)).astype(np.int64)
    assert (e != 2 * emax + 1).all(), "units() takes finite values"
    m = np.where(e > 0, frac | (1 << (prec - 1)), frac)
    m = np.where((p >> np.uint64(width - 1)) != 0, -m, m)
    shift = np.maximum(e, 1) - 1 + (emin - (prec - 1)) + U
    return m, shift


def _sum_groups(m, shift):
    tot = 0
    for s in np.unique(shift):
        sel = m[shift == s]
        for k in range(0, sel.size, 4096):           # |m| < 2^49 (products): 4096 of them stay below 2^62
            tot += int(sel[k:k + 4096].sum()) << int(s)
    return tot


def units(x, y=None):
    """the exact total of x (or of x * y, element-wise) in units of 2^-1074"""
    px, nx = patterns(x)
    mx, sx = _split(px, nx)
    if y is None:
        assert (sx >= 0).all()
        return _sum_groups(mx, sx)
    py, ny = patterns(y)
    assert nx == ny and nx != "float64" and px.size == py.size, "products of two arrays of one narrow dtype"
    my, sy = _split(py, ny)
    m, s = mx * my, sx + sy - U                       # at most 48 bits; 2^-298 = 2^776 units at the least
    assert (s[m != 0] >= 0).all()
    return _sum_groups(m, np.where(m != 0, s, 0))


def value_units(bits, dtype):
    """one finite bit pattern as units"""
    m, sh = _split(np.array([bits], dtype=np.uint64), dtype)
    return int(m[0]) << int(sh[0])


def digits_of(T):
    """the 68 normalised digits of T (the top one signed), as int64"""
    out = [(T >> (32 * i)) & 0xffffffff for i in range(NDIG - 1)]
    out.append(T >> (32 * (NDIG - 1)))
    return np.array(out, dtype=np.int64)


# ---------------------------------------------------------------------------------------------
# the rounding model
# ---------------------------------------------------------------------------------------------
def encode(dtype, negative, ebase, m):
    """the pattern of +-m * 2^q with the quantum q = ebase - (prec - 1): ebase is max(leading bit, bit of 2^emin) BEFORE
    m was rounded, so m may be 2^prec (the next binade) or, with ebase at 2^emin, anything below 2^prec"""
    prec, emin, emax, width = FORMATS[dtype]
    inf = (2 * emax + 1) << (prec - 1)
    bits = ((ebase - (emin + U)) << (prec - 1)) + m
    return ((1 << (width - 1)) if negative else 0) | min(bits, inf)


def round_to(T, dtype, mutant=None):
    prec, emin, emax, width = FORMATS[dtype]
    assert mutant is None or mutant in MUTANTS
    if T == 0:
        return 0
    M = abs(T)
    ebase = max(M.bit_length() - 1, emin + U)
    q = ebase - (prec - 1)
    if q <= 0:
        m = M << -q
    else:
        m, rem, half = M >> q, M & ((1 << q) - 1), 1 << (q - 1)
        if mutant == "sticky_next_digit" and rem > half:
            # looks for the sticky bit in the rest of the half bit's digit and in the next digit down only
            lo = max(((q - 1) >> 5) - 1, 0) * 32
            rem = half + (((rem - half) >> lo) << lo)
        up = rem > half or (rem == half and (m & 1 or mutant == "ties_away"))
        m += 1 if up else 0
    if mutant == "flush_subnormal" and M.bit_length() - 1 < emin + U and m < (1 << (prec - 1)):
        m = 0
    if mutant == "overflow_late" and ebase == emax + U and m == 1 << prec:
        m -= 1                                         # the tie at the threshold stays finite
    return encode(dtype, T < 0, ebase, m)


def _finite(bits, dtype):
    prec, emin, emax, width = FORMATS[dtype]
    return (bits >> (prec - 1)) & ((1 << (width - prec)) - 1) != 2 * emax + 1


def double_then_cast(T, dtype):
    """what rounding T to a double first and that double to `dtype` gives"""
    prec, emin, emax, width = FORMATS[dtype]
    d = round_to(T, "float64")
    if _finite(d, "float64"):
        return round_to(value_units(d, "float64"), dtype)
    return ((d >> 63) << (width - 1)) | ((2 * emax + 1) << (prec - 1))      # +-Inf stays +-Inf


# ---------------------------------------------------------------------------------------------
# planted totals
# ---------------------------------------------------------------------------------------------
class Planted:
    __slots__ = ("dtype", "kind", "T", "want", "subnormal")

    def __init__(self, dtype, kind, T, want, subnormal=False):
        self.dtype, self.kind, self.T, self.want, self.subnormal = dtype, kind, int(T), int(want), subnormal

    def __repr__(self):
        return f"<{self.dtype} {self.kind}{' sub' if self.subnormal else ''} {'-' if self.T < 0 else '+'}{abs(self.T).bit_length()}b>"


def _around(dtype, ebase, m, subnormal, unit=1):
    """the kinds around the significand m (quantum at ebase - prec + 1 >= 2), both signs; `unit`: what "one unit" is"""
    prec = FORMATS[dtype][0]
    q = ebase - (prec - 1)
    assert q >= 2 and unit < (1 << (q - 1))
    base, half = m << q, 1 << (q - 1)
    even = m if m % 2 == 0 else m + 1                   # where a tie lands
    out = []
    for neg in (False, True):
        s = -1 if neg else 1
        e = lambda mm: encode(dtype, neg, ebase, mm)     # noqa: E731
        out += [Planted(dtype, "exact", s * base, e(m), subnormal),
                Planted(dtype, "tie_even" if m % 2 == 0 else "tie_odd", s * (base + half), e(even), subnormal),
                Planted(dtype, "tie+1", s * (base + half + unit), e(m + 1), subnormal),
                Planted(dtype, "tie-1", s * (base + half - unit), e(m), subnormal)]
    return out


def planted(dtype):
    prec, emin, emax, width = FORMATS[dtype]
    low, top = emin + U, emax + U
    ones, mid_even, mid_odd = (1 << prec) - 1, (1 << (prec - 1)) | 2, (1 << (prec - 1)) | 5
    out = [Planted(dtype, "zero", 0, 0)]
    # normal binades: the lowest where a tie exists, one in every 32-bit phase near the middle, the highest
    ebases = sorted({max(low + 1, prec + 1), low + 3, (low + top) // 2, (low + top) // 2 + 13, top - 1, top})
    for ebase in ebases:
        if ebase - (prec - 1) < 2:
            continue
        for m in (1 << (prec - 1), mid_even, mid_odd, ones - 1, ones):
            if ebase == top and m == ones:
                continue                                # the ties of the last binade's all-ones: below
            out += _around(dtype, ebase, m, False)
    q = top - (prec - 1)
    thr = (ones << q) + (1 << (q - 1))                  # 2^(emax+1) - half a quantum: the first total that is +-Inf
    for neg in (False, True):
        s = -1 if neg else 1
        out += [Planted(dtype, "below_overflow", s * (thr - 1), encode(dtype, neg, top, ones)),
                Planted(dtype, "at_overflow", s * thr, encode(dtype, neg, top, ones + 1)),
                Planted(dtype, "max", s * (ones << q), encode(dtype, neg, top, ones))]
    q = low - (prec - 1)                                # the quantum of the subnormals (bit 0 for float64: all exact)
    if q >= 2:
        for m in (1, 2, 5, (1 << (prec - 2)) | 2, (1 << (prec - 1)) - 2):
            out += _around(dtype, low, m, True)
        big = (1 << (prec - 1)) - 1
        for neg in (False, True):
            s, sign = (-1 if neg else 1), ((1 << (width - 1)) if neg else 0)
            out += [Planted(dtype, "sub_max+half", s * ((big << q) + (1 << (q - 1))), encode(dtype, neg, low, big + 1), True),
                    Planted(dtype, "half_min", s * (1 << (q - 1)), sign, True),           # a tie between 0 and the odd 1
                    Planted(dtype, "half_min+1", s * ((1 << (q - 1)) + 1), sign | 1, True),
                    Planted(dtype, "half_min-1", s * ((1 << (q - 1)) - 1), sign, True)]
    else:
        for m in (1, 2, (1 << 52) - 1):
            out += [Planted(dtype, "exact", s * m, encode(dtype, s < 0, low, m), True) for s in (1, -1)]
    return out


def traps(dtype):
    """near-ties of the narrow format that a double cannot tell from the tie: (T, single rounding, double-then-cast)"""
    prec, emin, emax, width = FORMATS[dtype]
    assert dtype in NARROW
    out = []
    for ebase in (emin + U + 5, U, U + 3, emax + U - 1):
        q = ebase - (prec - 1)
        tiny = 1 << (ebase - 60)                          # 7 bits below the double's last place
        for m, d in (((1 << (prec - 1)) | 2, 1), ((1 << (prec - 1)) | 5, -1)):   # even + above the tie, odd + below it
            for s in (1, -1):
                T = s * ((m << q) + (1 << (q - 1)) + d * tiny)
                one, two = round_to(T, dtype), double_then_cast(T, dtype)
                assert one != two and one == encode(dtype, s < 0, ebase, m + (1 if d > 0 else 0)), (dtype, ebase, m, d)
                out.append((T, one, two))
    return out


def random_totals(seed, per_position=2):
    """totals with the leading bit at every position the 68 digits hold below the sign, both signs"""
    rng = np.random.default_rng(seed)
    out = []
    for p in range(32 * NDIG - 1):
        for _ in range(per_position):
            body = int.from_bytes(rng.bytes((p + 7) // 8 + 1), "little") & ((1 << p) - 1)
            if rng.integers(4) == 0 and p > 70:           # a long run of zeros: the sticky far below
                body &= ~((1 << (p - 60)) - 1) | 1
            out.append(((1 << p) | body) * (1 if rng.integers(2) else -1))
    return out


# ---------------------------------------------------------------------------------------------
# inputs of a narrow dtype
# ---------------------------------------------------------------------------------------------
def reach(dtype):
    """(lowest bit, highest leading bit) of the units a finite value of the dtype can occupy"""
    prec, emin, emax, width = FORMATS[dtype]
    return emin - (prec - 1) + U, emax + U


def realise(T, dtype):
    """patterns of at most a few values of `dtype` that add up to T exactly, largest first; None when out of reach"""
    prec, emin, emax, width = FORMATS[dtype]
    lo, hi = reach(dtype)
    out, neg, M = [], T < 0, abs(T)
    if M & ((1 << lo) - 1) or M.bit_length() - 1 > hi:
        return None
    while M:
        top = M.bit_length() - 1
        q = max(top - (prec - 1), lo)
        m = M >> q
        M -= m << q
        out.append(encode(dtype, neg, max(top, emin + U), m) if top >= emin + U else encode(dtype, neg, emin + U, m))
    return out


def as_numpy(pats, dtype):
    """patterns -> the numpy array that holds them (float64 / float32 / float16; bfloat16: uint16 words)"""
    width = FORMATS[dtype][3]
    a = np.array(pats, dtype={64: np.uint64, 32: np.uint32, 16: np.uint16}[width])
    return a if dtype == "bfloat16" else a.view({"float64": np.float64, "float32": np.float32, "float16": np.float16}[dtype])


def as_torch(pats, dtype, device="cpu"):
    import torch
    width = FORMATS[dtype][3]
    a = np.array(pats, dtype={64: np.uint64, 32: np.uint32, 16: np.uint16}[width]).view({64: np.int64, 32: np.int32, 16: np.int16}[width])
    return torch.from_numpy(a.copy()).view(getattr(torch, dtype)).to(device)


def input_cases(dtype):
    """(kind, T, patterns) for the INPUT dtype: the kinds of _around with "one unit" = the dtype's smallest subnormal,
    for results in the dtype's own normal and subnormal range, the largest finite value against itself, a cancellation to
    0 -- every one realised by realise() (asserted), so subnormal inputs and the largest finite values occur"""
    prec, emin, emax, width = FORMATS[dtype]
    lo, hi = reach(dtype)
    out = []
    for ebase in (lo + prec + 3, U, hi - 1):
        for m in ((1 << (prec - 1)) | 2, (1 << (prec - 1)) | 5, (1 << prec) - 1):
            for c in _around(dtype, ebase, m, False, unit=1 << lo):
                out.append((c.kind, c.T))
    big = ((1 << prec) - 1) << (hi - (prec - 1))
    out += [("max", big), ("-max", -big), ("2max", 2 * big), ("max+min", big + (1 << lo)), ("min", 1 << lo), ("-min", -(1 << lo))]
    cases = []
    for kind, T in out:
        parts = [T] if abs(T) <= big else [big, T - big]
        pats = [p for part in parts for p in realise(part, dtype)]
        assert units(Raw(pats) if dtype == "bfloat16" else as_numpy(pats, dtype)) == T
        cases.append((kind, T, pats))
    cases.append(("cancel", 0, realise(big, dtype) + realise(1 << lo, dtype) + realise(-big, dtype) + realise(-(1 << lo), dtype)))
    return cases


def dot_range_pairs(dtype):
    """(a patterns, b patterns): products at both ends of the product range -- smallest subnormal squared (2^-298 for
    float32), largest finite squared (nearly 2^256), and their mixes; a tie-like pattern in between"""
    prec, emin, emax, width = FORMATS[dtype]
    tiny, big = 1, encode(dtype, False, emax + U, (1 << prec) - 1)
    one = encode(dtype, False, U, 1 << (prec - 1))
    neg = 1 << (width - 1)
    a = [tiny, big, big, tiny | neg, one, big | neg, tiny, one | 3]
    b = [tiny, big, tiny, tiny, one | 1, big, big | neg, one | 5]
    return a, b


INF, NAN = float("inf"), float("nan")
# name -> (values of an ExSUM, (a, b) of an ExDOT, flags word expected: bit 0 +Inf, 1 -Inf, 2 NaN)
NONFINITE = {
    "+inf": ([1.0, INF, -2.0, 0.5], ([1.0, INF, 2.0], [3.0, 2.0, -1.0]), 1),
    "-inf": ([1.0, -INF, -2.0, 0.5], ([1.0, INF, 2.0], [3.0, -2.0, -1.0]), 2),
    "both": ([INF, 1.0, -INF], ([INF, 1.0, -INF], [1.0, 1.0, 2.0]), 3),
    "nan": ([1.0, NAN, 2.0], ([1.0, NAN, 2.0], [1.0, 1.0, 1.0]), 4),
    "inf*0": (None, ([1.0, INF, 2.0], [1.0, 0.0, 1.0]), 4),
}
