"""Constructed ExGEMV / ExGEMM / ExSpMV / ExSpMM / ExTRSV inputs whose exact results are known as Python integers (for
ExTRSV: from a Fraction substitution), and the integer reference.

Nothing here touches the GPU, the library or the oracle: operands are built as Python integers (``dtype=object``
matrices) times powers of two, the exact result is ``ndarray.dot`` on those object arrays, and the expected double is
``float(Fraction)`` (correctly rounded to nearest, ties to even, subnormals included).  Every constructor converts its
operands to float64 and asserts that each one converts back to the integer it was built from.

Output classes (``classify``), in units of the result's least significant integer bit:
  ``zero``   the exact result is 0
  ``exact``  the result is representable (at most 53 significant bits): nothing to round
  ``tie``    exactly half a unit in the last place above a double (``tie_up``: round-to-even goes away from zero)
  ``carry``  a tie whose 53 kept bits are all ones: it rounds up into the next binade
  ``tie+1`` / ``tie-1``   one integer unit above / below a tie (in magnitude)
  ``max``    the largest magnitude the case can produce (worst-case families only)
  ``other``  anything else (never present in a planted case)
"""
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np


# ---------------------------------------------------------------------------------------------
# integer reference
# ---------------------------------------------------------------------------------------------
def round_nearest_even(v):
    """exact integer or Fraction -> the nearest double (ties to even); beyond the double range -> +-inf"""
    v = Fraction(v)
    try:
        return float(v)
    except OverflowError:
        return math.inf if v > 0 else -math.inf


def obj(a):
    """any integer array -> dtype=object array of Python ints (same shape)"""
    a = np.asarray(a)
    out = np.empty(a.shape, dtype=object)
    out.ravel()[:] = [int(v) for v in a.ravel().tolist()]
    return out


def to_f64(ints, exp=0):
    """integers (object array) times 2^exp (an int, or an int array that broadcasts) as float64 -- asserting that every
    entry converts back to the integer it was built from (2^66 + 1 would silently round)"""
    ints = np.asarray(ints, dtype=object)
    flat = ints.ravel().tolist()
    f = np.array([float(v) for v in flat], dtype=np.float64)
    assert [int(x) for x in f.tolist()] == flat, "an operand is not representable as a double"
    f = f.reshape(ints.shape)
    e = np.broadcast_to(np.asarray(exp, dtype=np.int64), ints.shape)
    out = np.ldexp(f, e)
    assert np.isfinite(out).all() and (np.ldexp(out, -e) == f).all(), "an operand leaves the double range when scaled"
    return out


def gemm_exact(a_int, b_int):
    """exact integer product of two object matrices"""
    return np.asarray(a_int, dtype=object).dot(np.asarray(b_int, dtype=object))


def gemv_exact(g_int, x_int, beta=0, y0_int=None):
    """exact G x + beta y0 (G: outputs x inner, object ints; beta a Fraction or int) as an object vector of integers"""
    y = np.asarray(g_int, dtype=object).dot(np.asarray(x_int, dtype=object))
    if y0_int is not None and beta != 0:
        t = [Fraction(beta) * int(v) + int(s) for v, s in zip(y0_int, y)]
        assert all(v.denominator == 1 for v in t), "beta * y0 is not an integer in the result's units"
        y = obj([int(v) for v in t])
    return y


def rounded(c_int, exp=0):
    """float64 array of round_nearest_even(c_int * 2^exp), exp an int or a broadcasting int array"""
    c_int = np.asarray(c_int, dtype=object)
    e = np.broadcast_to(np.asarray(exp, dtype=np.int64), c_int.shape).ravel().tolist()
    out = np.array([round_nearest_even(Fraction(int(v)) * Fraction(2) ** int(s)) for v, s in zip(c_int.ravel().tolist(), e)],
                   dtype=np.float64)
    return out.reshape(c_int.shape)


def span_bits(ints, axis):
    """the largest number of bits a vector of the matrix spans, from its highest set bit down to its lowest (rows of the
    matrix for axis = 1, columns for axis = 0): what ExGEMM's operand scan reports for A and for B"""
    ints = np.asarray(ints, dtype=object)
    best = 0
    for vec in (ints if axis == 1 else ints.T):
        mags = [abs(int(v)) for v in vec if int(v)]
        if mags:
            best = max(best, max(v.bit_length() for v in mags) - min((v & -v).bit_length() - 1 for v in mags))
    return best


def classify(v):
    """class of one exact integer result (module docstring) and whether round-to-even moves its magnitude up"""
    v = int(v)
    if v == 0:
        return "zero", False
    a = abs(v)
    sh = a.bit_length() - 53
    if sh <= 0 or a & ((1 << sh) - 1) == 0:
        return "exact", False
    r, half, mant = a & ((1 << sh) - 1), 1 << (sh - 1), a >> sh
    if r == half:
        return ("carry" if mant == (1 << 53) - 1 else "tie"), bool(mant & 1)
    if r == half + 1:
        return "tie+1", True
    if r == half - 1:
        return "tie-1", False
    return "other", r > half


def classify_all(c_int):
    c_int = np.asarray(c_int, dtype=object)
    pairs = [classify(v) for v in c_int.ravel().tolist()]
    cls = np.array([p[0] for p in pairs], dtype=object).reshape(c_int.shape)
    up = np.array([p[1] for p in pairs], dtype=bool).reshape(c_int.shape)
    return cls, up


def planted_mix(case):
    """The condition every planted case meets by construction: at least 40 % exact ties and at least 40 % one unit off a
    tie, ties that round up and ties that round down, near-ties above and below, a tie that carries into the next
    binade, both signs, and no output outside the planted classes.  Returns the class counts."""
    cls, up, c = case.classes.ravel(), case.tie_up.ravel(), case.c_int.ravel()
    total = cls.size
    count = {name: int((cls == name).sum()) for name in ("tie", "carry", "tie+1", "tie-1", "exact", "zero", "other")}
    ties = (cls == "tie") | (cls == "carry")
    near = (cls == "tie+1") | (cls == "tie-1")
    neg = np.array([int(v) < 0 for v in c.tolist()])
    assert count["other"] == 0, count
    assert 10 * int(ties.sum()) >= 4 * total and 10 * int(near.sum()) >= 4 * total, count
    assert (ties & up).any() and (ties & ~up).any(), "ties in both directions"
    assert count["tie+1"] and count["tie-1"] and count["carry"], count
    for sel in (ties, near):
        assert (sel & neg).any() and (sel & ~neg).any(), "both signs"
    return count


# ---------------------------------------------------------------------------------------------
# the residue path's moduli: 256, 255, 253, 251, 247, ... (greedy, pairwise coprime, counting down from 256)
# ---------------------------------------------------------------------------------------------
CRT_LMAX = 39


def crt_moduli(count=CRT_LMAX):
    ps, c = [], 256
    while len(ps) < count:
        if all(math.gcd(c, q) == 1 for q in ps):
            ps.append(c)
        c -= 1
    return ps


def crt_bits(count=CRT_LMAX):
    """bits[L] = floor(log2(p_0 ... p_{L-1})) for L = 0 .. count"""
    bits, prod = [0], 1
    for p in crt_moduli(count):
        prod *= p
        bits.append(prod.bit_length() - 1)
    return bits


def crt_need(bits_a, bits_b, k):
    return bits_a + bits_b + max(0, (k - 1).bit_length()) + 2


def crt_moduli_needed(bits_a, bits_b, k):
    """the smallest L with bits[L] >= bits_a + bits_b + ceil(log2 k) + 2"""
    need = crt_need(bits_a, bits_b, k)
    ps, prod, c = [], 1, 256
    while prod.bit_length() - 1 < need:
        if all(math.gcd(c, q) == 1 for q in ps):
            ps.append(c)
            prod *= c
        c -= 1
    return len(ps)


# ---------------------------------------------------------------------------------------------
# planted ties
# ---------------------------------------------------------------------------------------------
LAYOUTS = ("tail", "split", "head")
D_PATTERN = (0, 1, 0, -1)


def _k_order(k, layout):
    """positions along k, as a list of canonical indices (0 lead, 1 its duplicate, 2 .. k-3 random, k-2 H, k-1 d)"""
    lead, dup, h, d = 0, 1, k - 2, k - 1
    rnd = list(range(2, k - 2))
    half = len(rnd) // 2
    if layout == "tail":
        return [lead, dup] + rnd + [h, d]
    if layout == "split":          # H first, the leading products in the middle, the deciding unit last
        return [h] + rnd[:half] + [lead, dup] + rnd[half:] + [d]
    if layout == "head":           # the deciding unit first, H last
        return [d] + rnd[:half] + [lead, dup] + rnd[half:] + [h]
    raise ValueError(layout)


def planted_gemm(m, n, k, S, seed=0, layout="tail", ea=0, eb=0):
    """A (m x k) and B (k x n) with

        A = s_i * [ 2^S * (1, 0, u_i2 .. u_i,k-3) , 1 , 1 ]            u, v small random integers in [-8, 8]
        B = t_j * [ 3 * 2^18 ; 3 * 2^18 ; v_2j .. v_k-3,j ; h_j H ; d_j ]     H = 2^(S - 34), h_j in {1, 3}, d_j in {0, +1, 0, -1}

    so that C_ij = s_i t_j (2^S P_ij + h_j H + d_j) with P_ij of exactly 20 bits: H is half a unit in the last place,
    h_j = 3 makes the kept mantissa odd (the tie rounds away from zero), d_j = +-1 moves the sum one integer unit off the
    tie, S - 34 bits below the rounding position.  Carry columns (j % 16 in 12, 13, 15) hold 2^20 - 1 in the leading
    rows, zeros for v and 2^S - H in the H row: all 53 kept bits are ones and the tie carries into the next binade.
    With m >= 16, row 3 is +-2^S * 5 against the two equal leading rows of B (large products that cancel to exactly
    zero) and row m - 2 has no 2^S part (results of a few bits: nothing to round).  `layout` moves the leading, H and d
    positions along k; `ea`, `eb` scale A and B by powers of two."""
    assert k >= 5 and n >= 16 and S >= 54
    rng = np.random.default_rng([seed, m, n, k, S])
    U, V = obj(rng.integers(-8, 9, (m, k))), obj(rng.integers(-8, 9, (k, n)))
    H = 1 << (S - 34)
    A, B = np.empty((m, k), dtype=object), np.empty((k, n), dtype=object)
    s = [-1 if i % 3 == 1 else 1 for i in range(m)]
    t = [-1 if j % 7 in (2, 5) else 1 for j in range(n)]
    zero_row, exact_row = (3, m - 2) if m >= 16 else (-1, -1)
    for i in range(m):
        if i == zero_row:
            A[i, :] = 0
            A[i, 0], A[i, 1] = 5 << S, -(5 << S)
        elif i == exact_row:
            A[i, :] = U[i, :] * s[i]
            A[i, 0] = A[i, 1] = A[i, k - 2] = 0
            A[i, k - 1] = s[i]
        else:
            A[i, :] = U[i, :] * (s[i] << S)
            A[i, 0], A[i, 1], A[i, k - 2], A[i, k - 1] = s[i] << S, 0, s[i], s[i]
    for j in range(n):
        d = D_PATTERN[j % 4]
        if j % 16 in (12, 13, 15):
            B[:, j] = 0
            B[0, j] = B[1, j] = t[j] * ((1 << 20) - 1)
            B[k - 2, j] = t[j] * ((1 << S) - H)
        else:
            B[:, j] = V[:, j] * t[j]
            B[0, j] = B[1, j] = t[j] * (3 << 18)
            B[k - 2, j] = t[j] * H * (3 if (j // 4) % 2 else 1)
        B[k - 1, j] = t[j] * d
    order = _k_order(k, layout)
    A, B = A[:, order], B[order, :]
    c_int = gemm_exact(A, B)
    cls, up = classify_all(c_int)
    pos = {name: order.index(idx) for name, idx in (("lead", 0), ("dup", 1), ("H", k - 2), ("d", k - 1))}
    return SimpleNamespace(m=m, n=n, k=k, S=S, layout=layout, a_int=A, b_int=B, ea=ea, eb=eb, a=to_f64(A, ea), b=to_f64(B, eb),
                           c_int=c_int, c_exp=ea + eb, classes=cls, tie_up=up, want=rounded(c_int, ea + eb), pos=pos,
                           bits_a=span_bits(A, 1), bits_b=span_bits(B, 0))


def gemm_operand(mat, trans, pad, fill=3.0):
    """row-major storage of op(X) = mat for ExGEMM: 'N' stores mat, 'T' stores its transpose; `pad` extra columns of
    `fill` per stored row.  Returns (flat array, leading dimension)."""
    st = np.ascontiguousarray(mat.T if trans == "T" else mat, dtype=np.float64)
    ld = st.shape[1] + pad
    out = np.full((st.shape[0], ld), fill, dtype=np.float64)
    out[:, :st.shape[1]] = st
    return out.reshape(-1), ld


def planted_gemv(outputs, inner, S, seed=0, layout="tail", plant=None, beta=0):
    """The columns of planted_gemm's B as the rows of a matrix G (outputs x inner) and one ordinary row of its A as x:
    y_j = t_j (2^S P_j + h_j H + d_j), the same classes per output.  `plant` = 'H' or 'd' takes that term out of the
    inner product and plants it in y: beta = 1 with y0_j = the term; beta = -3/4 with y0_j = -4 term (beta y0 = 3 term)
    and -2 term left in the inner product.  With beta = 0, y0 holds finite values that must be ignored."""
    g = planted_gemm(1, outputs, inner, S, seed=seed, layout=layout)
    G, x = g.b_int.T.copy(), g.a_int[0].copy()
    beta = Fraction(beta)
    y0 = obj(np.zeros(outputs, dtype=np.int64))
    if plant is not None:
        assert beta in (1, Fraction(-3, 4))
        p = g.pos[plant]
        term = G[:, p] * x[p]
        if beta == 1:
            y0, x[p] = term, 0
        else:
            y0, x[p] = term * -4, x[p] * -2
    else:
        assert beta == 0
    y_int = gemv_exact(G, x, beta, y0)
    assert (y_int == g.c_int[0]).all()
    y0f = to_f64(y0) if beta != 0 else np.full(outputs, 12345.678)
    return SimpleNamespace(outputs=outputs, inner=inner, S=S, layout=layout, plant=plant, beta=float(beta), g_int=G, x_int=x,
                           y0_int=y0, g=to_f64(G), x=to_f64(x), y0=y0f, c_int=y_int, c_exp=0, classes=g.classes[0],
                           tie_up=g.tie_up[0], want=g.want[0], pos=g.pos)


def gemv_operands(g, x, y0, trans, pad=0, offa=0, incx=1, offx=0, incy=1, offy=0, fill=3.0):
    """ExGEMV's arguments for y = G x: column-major A with A = G ('N': m outputs, n inner) or A = G^T ('T': m inner, n
    outputs), lda = m + pad, strided / offset x and y.  Returns (m, n, a, lda, x, y)."""
    G = np.asarray(g, dtype=np.float64)
    outputs, inner = G.shape
    m, n = (inner, outputs) if trans == "T" else (outputs, inner)
    cols = G if trans == "T" else G.T                    # cols[c] = column c of A
    lda = m + pad
    a = np.full(offa + n * lda, fill, dtype=np.float64)
    av = a[offa:].reshape(n, lda)
    av[:, :m] = cols
    xs = np.full(offx + (inner - 1) * incx + 1, fill, dtype=np.float64)
    xs[offx::incx] = x
    ys = np.full(offy + (outputs - 1) * incy + 1, fill, dtype=np.float64)
    ys[offy::incy] = y0
    return m, n, a, lda, xs, ys


# ---------------------------------------------------------------------------------------------
# worst-case magnitudes for the residue path
# ---------------------------------------------------------------------------------------------
_WORST_K = (1, 2, 3, 16, 17, 256, 257, 8192, 8193, 5, 1024, 1025, 64, 65)
# the L whose M_L is barely above 2^bits[L] (M_L / 2^bits[L] = 1.03 .. 1.08) get a k that is exactly a power of two, so that
# k 2^na 2^nb is exactly 2^(bits[L] - 2) and the largest sum comes as close to M_L / 4 as doubles allow
_WORST_K_TIGHT = {11: 1024, 22: 8192, 27: 256, 28: 64, 29: 1024, 33: 4096}
_WORST_K_TIGHT[13] = 1      # the largest L a single product reaches: 50 + 50 + 2 bits


def _clog2(k):
    return max(0, (k - 1).bit_length())


def crt_worst_params(L):
    """(na, nb, k) with na + nb + ceil(log2 k) + 2 == bits[L], na, nb <= 126: k from a list of powers of two and powers
    of two plus one where the bits allow it.  k = 1 only serves na, nb <= 53 (a vector of one double spans 53 bits)."""
    need = crt_bits()[L]
    k = _WORST_K_TIGHT.get(L, _WORST_K[L % len(_WORST_K)])
    while need - 2 - _clog2(k) < 2:
        k = max(1, k // 4)
    if k == 1 and need - 2 > 106:
        k = 2
    while need - 2 - _clog2(k) > 252:
        k = 1 << (_clog2(k) + 1)
    rest = need - 2 - _clog2(k)
    na = min(126, (rest + 1) // 2)
    nb = rest - na
    assert 1 <= nb <= 126 and crt_need(na, nb, k) == need
    return na, nb, k


def _full_vector(nbits, k):
    """k magnitudes that span exactly `nbits` bits and are as large as doubles allow: 2^nbits - 1 everywhere when that
    is a double (nbits <= 53); else the top 53 bits set, (2^53 - 1) 2^(nbits - 53), except for the last entry (the last
    two from k = 4 on, so that alternating signs still cancel in pairs), which holds 2^53 - 1 and pins the unit"""
    if nbits <= 53:
        return [(1 << nbits) - 1] * k
    assert k >= 2
    lows = 2 if k >= 4 else 1
    return [((1 << 53) - 1) << (nbits - 53)] * (k - lows) + [(1 << 53) - 1] * lows


def crt_worst_case(L, m=12, n=12):
    """Operands at the largest magnitude (na, nb, k) = crt_worst_params(L) admits: every entry of a row of A is
    +-(2^na - 1) 2^ra_i -- for na > 53, which no double holds, +-(2^53 - 1) 2^(na - 53) 2^ra_i with 2^53 - 1 in the last
    position(s), _full_vector -- and likewise for the columns of B with nb, rb_j; ra, rb are per-row / per-column powers
    of two.  Rows and columns by index mod 6: all plus, all minus, alternating from plus, alternating from minus, a
    unit vector (a single +-1), all plus.  C then holds the largest sum (class ``max``), its negative, cancellation in
    pairs (to 0 when k is even), single products and +-1."""
    na, nb, k = crt_worst_params(L)
    X, Y = _full_vector(na, k), _full_vector(nb, k)

    def vec(kind, mags, unit):
        if kind in (0, 5):
            return list(mags)
        if kind == 1:
            return [-v for v in mags]
        if kind in (2, 3):
            return [v if (l + kind) % 2 == 0 else -v for l, v in enumerate(mags)]
        return [unit] + [0] * (k - 1)

    A, B = np.empty((m, k), dtype=object), np.empty((k, n), dtype=object)
    for i in range(m):
        A[i, :] = vec(i % 6, X, 1 if i % 12 < 6 else -1)
    for j in range(n):
        B[:, j] = vec(j % 6, Y, -1 if j % 12 < 6 else 1)
    ra = np.array([(7 * i) % 23 - 11 for i in range(m)], dtype=np.int64)
    rb = np.array([(5 * j) % 19 - 9 for j in range(n)], dtype=np.int64)
    a = to_f64(A, ra[:, None])
    b = to_f64(B, rb[None, :])
    c_int = gemm_exact(A, B)
    c_exp = ra[:, None] + rb[None, :]
    cls, up = classify_all(c_int)
    top = sum(x * y for x, y in zip(X, Y))
    cls[np.array([[abs(int(v)) == top for v in row] for row in c_int])] = "max"
    return SimpleNamespace(L=L, m=m, n=n, k=k, na=na, nb=nb, a_int=A, b_int=B, a=a, b=b, c_int=c_int, c_exp=c_exp,
                           classes=cls, tie_up=up, want=rounded(c_int, c_exp), bits_a=span_bits(A, 1), bits_b=span_bits(B, 0), top=top)


def crt_wrap_case(k, m=10, n=9, nbits=12, seed=0):
    """Every entry = 128 (mod 256) in the integer units the residue path works in: the symmetric residue of p = 256 is
    +128, which wraps to -128 as an int8, and with k = 8192 the int32 contraction of that modulus reaches exactly 2^27.
    Row 0 of A and column 0 of B carry one odd entry each, which pins the unit of every vector to 2^0."""
    rng = np.random.default_rng([seed, k])
    top = 1 << (nbits - 1)
    A = obj(top + 128 + 256 * rng.integers(0, top // 256, (m, k)))
    B = obj(top + 128 + 256 * rng.integers(0, top // 256, (k, n)))
    A *= obj(np.where(rng.random((m, 1)) < 0.4, -1, 1))
    A[0, 0], B[0, 0] = top + 1, -(top + 1)
    c_int = gemm_exact(A, B)
    cls, up = classify_all(c_int)
    return SimpleNamespace(m=m, n=n, k=k, na=nbits, nb=nbits, a_int=A, b_int=B, a=to_f64(A), b=to_f64(B), c_int=c_int,
                           c_exp=0, classes=cls, tie_up=up, want=rounded(c_int), bits_a=span_bits(A, 1), bits_b=span_bits(B, 0))


# ---------------------------------------------------------------------------------------------
# ExGEMV result-range rows
# ---------------------------------------------------------------------------------------------
def range_rows_gemv(inner=12):
    """Rows whose exact sums sit at the ends of the double range while every product is exact for TwoProd (a multiple
    of 2^-1074 below 2^1024).  Six positions of x are in use, spread over [0, inner): three hold small integers times
    2^-537 (G there: integers times 2^-537, products: multiples of 2^-1074), three hold 2^511 (G there: values times
    2^512, products up to 2^1023).  y0 (for beta = 1) adds the last term of two of the rows.
    Returns G, x, y0 (float64), the exact sums without and with y0 (Fractions), and row names."""
    assert inner >= 6
    lo = [0, inner // 2, inner - 1]                     # x = (1, 3, -2) * 2^-537
    hi = [1, inner // 2 - 1, inner - 2]                 # x = 2^511
    xl = (1, 3, -2)
    T52 = 1 << 52
    big = (1 << 53) - 1                                 # (2^53 - 1) * 2^(512 - 53) * 2^511 = 2^1023 - 2^970
    rows = [   # name, G at lo (integers, times 2^-537), G at hi (integers, times 2^(512 - 53)), y0
        ("subnormal 15 units", (5, 2, -2), (0, 0, 0), 0.0),
        ("subnormal -2 units", (-4, 0, -1), (0, 0, 0), 0.0),
        ("largest subnormal", (T52 - 7, 2, 0), (0, 0, 0), 0.0),
        ("smallest normal", (T52 - 6, 2, 0), (0, 0, 0), 0.0),
        ("4 x smallest normal", (T52, T52, 0), (0, 0, 0), 0.0),
        ("one unit after cancellation", (T52, 1, T52 // 2 + 1), (0, 0, 0), 0.0),
        ("partial sums overflow", (0, 0, 0), (T52 * 2, T52 * 2, -T52 * 2), 0.0),
        ("DBL_MAX", (0, 0, 0), (T52 * 2, big - 1, 0), 0.0),
        ("tie at the overflow threshold", (0, 0, 0), (T52 * 2, big - 1, 1), 0.0),
        ("just below the overflow tie", (0, 0, 0), (T52 * 2, big - 1, 0), 2.0 ** 970 - 2.0 ** 918),
        ("-DBL_MAX", (0, 0, 0), (-T52 * 2, -(big - 1), 0), 0.0),
        ("negative tie at the overflow threshold", (0, 0, 0), (-T52 * 2, -(big - 1), 0), -(2.0 ** 970)),
        ("huge products cancel, 3 units remain", (1, 0, -1), (T52 * 2, -T52 * 2, 0), 0.0),
        ("huge products cancel to zero", (0, 0, 0), (big, -T52, -(big - T52)), 0.0),
    ]
    nr = len(rows)
    Gi = np.zeros((nr, inner), dtype=object)
    ge = np.zeros(inner, dtype=np.int64)
    xi = np.zeros(inner, dtype=object)
    xe = np.zeros(inner, dtype=np.int64)
    for p, v in zip(lo, xl):
        xi[p], xe[p], ge[p] = v, -537, -537
    for p in hi:
        xi[p], xe[p], ge[p] = 1, 511, 512 - 53
    y0 = np.zeros(nr)
    for r, (_, gl, gh, yv) in enumerate(rows):
        for p, v in zip(lo, gl):
            Gi[r, p] = v
        for p, v in zip(hi, gh):
            Gi[r, p] = v
        y0[r] = yv
    G, x = to_f64(Gi, ge[None, :]), to_f64(xi, xe)
    sums = [sum(Fraction(int(Gi[r, t]) * int(xi[t])) * Fraction(2) ** int(ge[t] + xe[t]) for t in range(inner) if Gi[r, t])
            for r in range(nr)]
    with_y = [s + Fraction(float(v)) for s, v in zip(sums, y0)]
    for r in range(nr):                                 # every product is exact for TwoProd
        for t in range(inner):
            p = Fraction(int(Gi[r, t]) * int(xi[t])) * Fraction(2) ** int(ge[t] + xe[t])
            assert abs(p) < Fraction(2) ** 1024 and (p * Fraction(2) ** 1074).denominator == 1
    return SimpleNamespace(inner=inner, names=[r[0] for r in rows], g=G, x=x, y0=y0, exact=sums, exact_with_y=with_y,
                           want=np.array([round_nearest_even(s) for s in sums]),
                           want_with_y=np.array([round_nearest_even(s) for s in with_y]))


# ---------------------------------------------------------------------------------------------
# sparse views: the constructed rows as CSR (ExSpMV / ExSpMM)
# ---------------------------------------------------------------------------------------------
def csr_from_rows(g, x, itype=np.int64, n_cols=None, spread=False, zeros="keep", dup=None, shuffle=False, seed=0):
    """The dense constructed G (outputs x inner, float64) and x (inner, or inner x k for ExSpMM) as CSR: returns
    (crow, col, val, xs, n_cols).

    The columns are an injective random map of the positions along a row into [0, n_cols), n_cols >= inner (the default
    leaves about a sixth of the columns unused), so the indices are unsorted within a row.  The entries are stored in
    the order of the positions -- a layout's leading, H and d entries stay where the layout puts them, in whichever
    lane and chunk that is -- or in a random order with shuffle = True.  With spread = True every row has its own map
    and x is scattered once per row (n_cols >= outputs * inner), otherwise all rows share one.  Every entry (row) of xs
    that no stored entry refers to holds NaN.  zeros = "keep" stores the explicit zeros of G (every row has exactly
    `inner` entries), "drop" leaves them out (the lengths then mix).  dup = a position along the row: the entry there
    is stored as two entries of the same column whose values add up to it exactly (duplicate columns each count); the
    second one goes to the end of the row, which is one entry longer."""
    g, x = np.asarray(g, dtype=np.float64), np.asarray(x, dtype=np.float64)
    outputs, inner = g.shape
    assert x.shape[0] == inner and x.ndim in (1, 2) and zeros in ("keep", "drop")
    rng = np.random.default_rng([seed, outputs, inner, int(spread)])
    used = inner * (outputs if spread else 1)
    n_cols = max(int(n_cols or 0), used + used // 5 + 3)
    perm = rng.permutation(n_cols)
    xs = np.full((n_cols,) + x.shape[1:], np.nan)
    cols, vals, crow = [], [], [0]
    for i in range(outputs):
        cmap = perm[i * inner:(i + 1) * inner] if spread else perm[:inner]
        pos = np.arange(inner) if zeros == "keep" else np.nonzero(g[i])[0]
        c, v = cmap[pos], g[i, pos]
        xs[c] = x[pos]
        if dup is not None and (pos == dup).any():
            at = int(np.nonzero(pos == dup)[0][0])
            first = np.trunc(v[at] / 2)
            rest = v[at] - first
            assert first + rest == v[at] and Fraction(float(first)) + Fraction(float(rest)) == Fraction(float(v[at]))
            v = np.concatenate([v, [rest]])
            v[at] = first
            c = np.concatenate([c, [c[at]]])
        order = rng.permutation(len(v)) if shuffle else np.arange(len(v))
        cols.append(c[order])
        vals.append(v[order])
        crow.append(crow[-1] + len(v))
    col = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    val = np.concatenate(vals) if vals else np.zeros(0)
    assert n_cols < np.iinfo(itype).max and crow[-1] < np.iinfo(itype).max
    return np.array(crow, dtype=itype), col.astype(itype), val, xs, n_cols


def csr_dense_int(crow, col, val, xs):
    """The exact products of a CSR matrix with integer-valued entries against xs, row by row, as Python integers (the
    converter's round trip: every stored entry counts, duplicates included; an unreferenced NaN must not be read)."""
    out = []
    for i in range(len(crow) - 1):
        a, b = int(crow[i]), int(crow[i + 1])
        xv = xs[col[a:b]]
        assert not np.isnan(xv).any()
        out.append(sum(int(v) * int(w) for v, w in zip(val[a:b].tolist(), xv.tolist())))
    return obj(out) if out else np.zeros(0, dtype=object)


def planted_spmm(rows, kcols, inner, S, seed=0, layout="tail", plant=None, beta=0):
    """planted_gemm(kcols, rows, inner, S) as an ExSpMM: the sparse matrix is B^T (rows x inner, dense here: g_int / g,
    to be stored by csr_from_rows), X = A^T (inner x kcols, row-major) and Y = (A B)^T, so that every output is a planted
    class.  From kcols >= 16 on column 3 cancels to exactly zero and column kcols - 2 is a short exact value.  `plant` =
    'H' or 'd' moves that term of every output into Y0 (planted_gemv's options: beta = 1 with Y0 = the term, or
    beta = -3/4 with Y0 = -4 term and -2 term left in the product); with beta = 0, Y0 holds NaN."""
    c = planted_gemm(kcols, rows, inner, S, seed=seed, layout=layout)
    G, Xi = c.b_int.T.copy(), c.a_int.T.copy()
    beta = Fraction(beta)
    y0 = np.zeros((rows, kcols), dtype=object)
    if plant is not None:
        assert beta in (1, Fraction(-3, 4))
        p = c.pos[plant]
        term = np.outer(G[:, p], Xi[p, :])
        if beta == 1:
            y0, Xi[p, :] = term, 0
        else:
            y0, Xi[p, :] = term * -4, Xi[p, :] * -2
    else:
        assert beta == 0
    y_int = gemm_exact(G, Xi)
    if beta != 0:
        t = [[Fraction(beta) * int(v) + int(s) for v, s in zip(r0, r1)] for r0, r1 in zip(y0, y_int)]
        assert all(v.denominator == 1 for r in t for v in r)
        y_int = obj([[int(v) for v in r] for r in t])
    assert (y_int == c.c_int.T).all()
    y0f = to_f64(y0) if beta != 0 else np.full((rows, kcols), np.nan)
    return SimpleNamespace(rows=rows, kcols=kcols, inner=inner, S=S, layout=layout, plant=plant, beta=float(beta), g_int=G,
                           x_int=Xi, y0_int=y0, g=to_f64(G), x=to_f64(Xi), y0=y0f, c_int=y_int, c_exp=0,
                           classes=c.classes.T.copy(), tie_up=c.tie_up.T.copy(), want=np.ascontiguousarray(c.want.T), pos=c.pos)


COMPLETE_CLASSES = ("tie", "tie_odd", "carry", "tie+1", "tie-1")


def split53(v):
    """an integer as a list of integers of at most 53 significant bits each that add up to it"""
    sign, c, out = (-1 if v < 0 else 1), abs(int(v)), []
    while c:
        sh = max(0, c.bit_length() - 53)
        piece = (c >> sh) << sh
        out.append(sign * piece)
        c -= piece
    return out


def complete_to(T, cls, gap):
    """Terms that move the integer partial sum T to a chosen class: an exact tie whose kept mantissa is even (``tie``)
    or odd (``tie_odd``: round-to-even goes away from zero), a tie under 53 ones (``carry``), or one deciding unit above
    / below a tie in magnitude (``tie+1`` / ``tie-1``) with that unit `gap` >= 1 bits below the half unit.  The leading
    53 bits of T are kept (but for their last bit, or all ones for ``carry``); what T holds below them is cancelled.

    Returns a namespace: `terms` (integers of at most 53 significant bits, ceil(low / 53) + 1 of them at most, low the
    number of bits of the scaled T below the half unit; ``carry`` may take one more), `scale` (T counts in units of
    2^-scale of the terms: a short T is shifted up so that the deciding unit is an integer), `unit` (the deciding unit
    is 2^unit) and `total` = (T << scale) + sum(terms), whose class in units of 2^unit is asserted."""
    assert cls in COMPLETE_CLASSES and gap >= 1
    T = int(T)
    sign, a = (-1 if T < 0 else 1), abs(T)
    scale = max(0, gap + 54 - a.bit_length()) if a else 0
    a <<= scale
    if a == 0:
        a = 1 << (gap + 53)
    sh = a.bit_length() - 53
    mant = a >> sh
    if cls == "tie":
        mant &= ~1
    elif cls == "tie_odd":
        mant = (mant | 1) - (2 if mant | 1 == (1 << 53) - 1 else 0)      # (53 ones would be the carry class)
    elif cls == "carry":
        mant = (1 << 53) - 1
    d = {"tie+1": 1, "tie-1": -1}.get(cls, 0)
    unit = sh - 1 - gap
    assert unit >= 0
    total = sign * ((mant << sh) + (1 << (sh - 1)) + d * (1 << unit))
    terms = split53(total - (T << scale))
    assert len(terms) <= -(-(sh - 1) // 53) + (2 if cls == "carry" else 1), (len(terms), sh)
    assert (T << scale) + sum(terms) == total and total % (1 << unit) == 0
    got, up = classify(total >> unit)
    assert got == ("tie" if cls == "tie_odd" else cls) and (cls not in ("tie", "tie_odd") or up == (cls == "tie_odd"))
    return SimpleNamespace(terms=terms, scale=scale, unit=unit, total=total)


INEXACT_CLOSE = 4                      # positions along the row that complete_to's terms take (x = 1 there)
_INEXACT_CLASSES = ("tie", "tie+1", "tie_odd", "tie-1", "carry")


def planted_inexact(outputs, inner, S, seed=0, layout="tail", beta=0):
    """Rows G (outputs x inner) against one x whose two leading products are a * b with a, b odd integers of 40 to 53
    random bits -- up to 106 bits wide, so fl(a b) is inexact and the TwoProd error term carries bits of the result --
    then small exact products u v 2^f, and INEXACT_CLOSE positions with x = 1 that hold complete_to's terms: output j
    is of class (tie, tie+1, tie to odd, tie-1, carry)[j % 5], negative where j % 3 == 1, with the deciding unit
    gap = S - 34 bits below the half unit (as in planted_gemm).  `layout` moves the leading products and the closing
    terms along the row as in planted_gemm.  Every operand is an integer; `unit[j]` is the deciding unit of output j
    as a power of two.  beta = -3/4 adds beta y0 with y0_j = +-4 W_j 2^50, W_j odd of exactly 53 bits: 3 W_j has 54 or 55
    bits, so TwoProd(beta, y0_j) has a non-zero error term too, about as large as the half unit of the result; with
    beta = 0, y0 holds NaN."""
    assert inner >= 2 + INEXACT_CLOSE and S >= 35 and outputs >= 15
    beta = Fraction(beta)
    assert beta in (0, Fraction(-3, 4))
    rng = np.random.default_rng([seed, outputs, inner, S, 77])
    gap, nf = S - 34, inner - 2 - INEXACT_CLOSE

    def wide():
        bits = int(rng.integers(40, 54))
        return (int(rng.integers(0, 1 << 62)) % (1 << (bits - 1))) | (1 << (bits - 1)) | 1

    x = np.zeros(inner, dtype=object)
    x[0], x[1] = wide(), -wide()
    x[2:2 + nf] = obj(rng.integers(-8, 9, nf))
    x[2 + nf:] = 1
    G = np.zeros((outputs, inner), dtype=object)
    y0 = np.zeros(outputs, dtype=object)
    units = []
    for j in range(outputs):
        row = np.zeros(inner, dtype=object)
        row[0], row[1] = wide(), wide() * (1 if j % 2 else -1)
        f = rng.integers(0, 51, nf)
        row[2:2 + nf] = obj(rng.integers(-8, 9, nf)) * obj([1 << int(s) for s in f])
        yj = 0
        if beta != 0:
            yj = (4 * ((int(rng.integers(0, 1 << 52)) | (1 << 52) | 1)) << 50) * (1 if j % 4 < 2 else -1)
        T = int(row.dot(x)) - 3 * (yj // 4)
        if (T < 0) != (j % 3 == 1):
            row, yj, T = -row, -yj, -T
        fix = complete_to(T, _INEXACT_CLASSES[j % 5], gap)
        row = row * (1 << fix.scale)
        row[2 + nf:2 + nf + len(fix.terms)] = fix.terms
        G[j], y0[j] = row, yj << fix.scale
        units.append(fix.unit)
        assert int(row.dot(x)) - 3 * (int(y0[j]) // 4) == fix.total
    lead = [0, 1]
    rnd, close = list(range(2, 2 + nf)), list(range(2 + nf, inner))
    half = len(rnd) // 2
    order = {"tail": lead + rnd + close,
             "split": close[:1] + rnd[:half] + lead + rnd[half:] + close[1:],
             "head": close[:1:-1] + rnd[:half] + lead + rnd[half:] + close[1::-1]}[layout]
    assert sorted(order) == list(range(inner))
    G, x = G[:, order], x[order]
    c_int = gemv_exact(G, x, beta, y0)
    for row in G:                                        # ExGEMV's product domain: multiples of 2^-1074 below 2^1024
        assert all(abs(int(v) * int(w)) < 1 << 1024 for v, w in zip(row, x))
    reduced = obj([int(v) >> u for v, u in zip(c_int, units)])
    assert all(int(v) % (1 << u) == 0 for v, u in zip(c_int, units))
    cls, up = classify_all(reduced)
    gf, xf = to_f64(G), to_f64(x)
    with np.errstate(over="ignore"):                     # the error terms are there: fl(a b) != a b in the leading products
        p = gf[:, order.index(0)] * xf[order.index(0)]
    assert all(int(v) != int(G[j, order.index(0)]) * int(x[order.index(0)]) for j, v in enumerate(p.tolist()))
    pos = {"lead": order.index(0), "dup": order.index(1), "close": [order.index(q) for q in close]}
    y0f = to_f64(y0) if beta != 0 else np.full(outputs, np.nan)
    if beta != 0:                                        # ... and fl(beta y0) != beta y0
        assert all(Fraction(float(beta) * v) != beta * int(w) for v, w in zip(y0f.tolist(), y0))
    return SimpleNamespace(outputs=outputs, inner=inner, S=S, layout=layout, beta=float(beta), y0_int=y0, y0=y0f,
                           g_int=G, x_int=x, g=gf, x=xf, c_int=reduced,
                           c_exact=c_int, unit=units, classes=cls, tie_up=up, want=rounded(c_int), pos=pos)


ADVERSARIAL_WINDOWS = (60, 120, 200, 400)


def adversarial_rows(count, seed=0):
    """`count` CSR rows of 1 to 200 entries with private columns: integers of 1 to 53 random bits times powers of two
    spread over a window of 60, 120, 200 or 400 bits, against x = +-2^t (every product is exact).  A random subset of
    the entries of some rows is stored a second time, negated, elsewhere in the row (exact cancellation), and every
    second row that is long enough is closed by complete_to (class and gap in 1 .. 70 at random; its terms against
    x = 1).  Two rows in five have 56 to 72 entries before that, so the lengths straddle 64.  Every operand and product
    is a multiple of 2^-1074 below 2^1000 (and at least 2^-930, so that halving x is exact on the result).  Returns crow, col (int64), val, xs, n_cols, want (Fraction-rounded),
    classes, lens and the exact sums as (integer, exponent) pairs."""
    rng = np.random.default_rng([seed, count, 4242])
    vals, xvals, crow, want, classes, exact = [], [], [0], [], [], []
    for r in range(count):
        n = int(rng.integers(56, 73)) if r % 5 < 2 else int(rng.integers(1, 191))
        W = ADVERSARIAL_WINDOWS[int(rng.integers(0, 4))]
        close = r % 2 == 1 and n >= 4
        base = int(rng.integers(-900, 480 - W))
        bits = rng.integers(1, 54, n)
        mant = [(int(rng.integers(0, 1 << 62)) % (1 << (int(b) - 1))) | (1 << (int(b) - 1)) for b in bits]
        sgn = rng.choice((-1, 1), n)
        ve = base + rng.integers(0, W, n)
        t = rng.integers(-30, 31, n)
        xs_sgn = rng.choice((-1, 1), n)
        ent = [(int(s) * m, int(e), int(xs_), int(tt)) for s, m, e, xs_, tt in zip(sgn, mant, ve, xs_sgn, t)]
        if r % 3 == 0 and n >= 2:                       # exact cancellation: the entry again, negated
            twice = [q for q in ent if rng.random() < 0.35][:(200 - 10 - n)]
            ent += [(-m, e, xs_, tt) for m, e, xs_, tt in twice]
        lo = min(e + tt for _, e, _, tt in ent)
        T = sum((m * xs_) << (e + tt - lo) for m, e, xs_, tt in ent)
        cls_name = None
        if close:
            cls_name = COMPLETE_CLASSES[int(rng.integers(0, 5))]
            fix = complete_to(T, cls_name, int(rng.integers(1, 71)))
            assert lo - fix.scale >= -1074
            for term in fix.terms:
                tz = (term & -term).bit_length() - 1
                ent.append((term >> tz, lo - fix.scale + tz, 1, 0))
            T, lo = fix.total >> fix.unit, lo - fix.scale + fix.unit
        order = rng.permutation(len(ent))
        ent = [ent[int(q)] for q in order]
        assert 1 <= len(ent) <= 200
        for m, e, xs_, tt in ent:                       # operands and products: multiples of 2^-1074 below 2^1000
            assert e >= -1074 and e + tt - 1 >= -1074      # (ExSpMM also runs x / 2)
            assert abs(m).bit_length() + e < 1000 and abs(m).bit_length() + e + tt + 1 < 1000 and abs(m).bit_length() <= 53
            vals.append(math.ldexp(float(m), e))
            xvals.append(math.ldexp(float(xs_), tt))
        crow.append(crow[-1] + len(ent))
        cname = classify(T)[0]
        assert cls_name is None or cname == ("tie" if cls_name == "tie_odd" else cls_name)
        classes.append(cname)
        exact.append((T, lo))
        want.append(round_nearest_even(Fraction(T) * Fraction(2) ** lo))
    nnz = crow[-1]
    n_cols = nnz + nnz // 7 + 5
    col = rng.permutation(n_cols)[:nnz].astype(np.int64)
    xs = np.full(n_cols, np.nan)
    xs[col] = xvals
    lens = np.diff(crow)
    assert count < 500 or ((lens < 64).any() and (lens == 64).any() and (lens == 65).any() and (lens > 72).any())
    return SimpleNamespace(count=count, crow=np.array(crow, dtype=np.int64), col=col, val=np.array(vals), xs=xs, n_cols=n_cols,
                           want=np.array(want), classes=np.array(classes, dtype=object), lens=lens, exact=exact)


# ---------------------------------------------------------------------------------------------
# ExTRSV: planted totals along a substitution chain
# ---------------------------------------------------------------------------------------------
TRSV_BLOCK = 64                        # rows per block-row of the kernel: the anchors open every block of this size
TRSV_GAPS = (1, 30, 110, 250)          # bits between the half unit and the deciding unit: inside one double, inside the
#                                        three register levels, below them, far below them
TRSV_RAND = 5                          # random entries per planted row (against earlier planted rows' x)
# (n, W, mantissa bits, filler): the systems the CPU and the GPU tests share -- a partial block, exactly one block, one
# row more (that row closes against the first block's anchors only), a few blocks with the dense filler, more than
# ten blocks in both windows
TRSV_CASES = ((40, 40, 20, False), (64, 400, 53, False), (65, 40, 53, False), (200, 400, 53, True), (130, 40, 30, True),
              (700, 400, 53, False), (714, 40, 53, False))
# every (fpe, early_exit) variant of ExTRSV
TRSV_VARIANTS = [(0, False), (2, False), (3, False), (4, False), (5, False), (6, False), (7, False), (8, False),
                 (4, True), (6, True), (8, True)]


@functools.lru_cache(maxsize=None)
def planted_trsv_case(n, W, mbits, filler, unit):
    """planted_trsv on a row of TRSV_CASES, built once per session for every test file that solves it"""
    return planted_trsv(n, seed=21, W=W, mbits=mbits, filler=filler, unit=unit)


def _p2(e):
    return Fraction(2) ** int(e)


def _exact_double(v):
    """a dyadic Fraction -> the double that holds it exactly"""
    f = float(v)
    assert Fraction(f) == v, "an operand is not representable as a double"
    return f


def trsv_exact(L, b, unit=False):
    """Plain Fraction substitution on the logical lower-triangular system L x = b (dense float64, substitution order
    = row order):  T_i = b_i - sum_{j < i} L_ij x_j exactly over the already-fixed doubles x_j, then
    x_i = round_nearest_even(T_i) / L_ii as the IEEE quotient of two doubles (unit: x_i = round_nearest_even(T_i)).
    Zero entries are skipped, so a non-finite x_j may only sit where nothing consumes it.  Returns (x, totals)."""
    L, b = np.asarray(L, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = len(b)
    x, totals, xf = np.zeros(n), [], [None] * n
    for i in range(n):
        T = Fraction(float(b[i]))
        for j in np.nonzero(L[i, :i])[0].tolist():
            if xf[j] is None:
                xf[j] = Fraction(float(x[j]))
            T -= Fraction(float(L[i, j])) * xf[j]
        r = round_nearest_even(T)
        x[i] = r if unit else r / float(L[i, i])
        totals.append(T)
    return x, totals


def _odd(rng, bits):
    """an odd integer of exactly `bits` bits"""
    return (int(rng.integers(0, 1 << 62)) % (1 << (bits - 1))) | (1 << (bits - 1)) | 1


def _take(preferred, other):
    """the next column of the preferred pool, of the other one when that is empty"""
    return preferred.pop() if preferred else other.pop()


def planted_trsv(n, seed=0, W=40, mbits=53, filler=False, unit=False, anchors=None):
    """A logical lower-triangular system (dense L, b) whose row totals T_i = b_i - sum_j L_ij x_j are planted ties and
    near-ties over a solution of full 53-bit doubles, with the expected solution from Fraction arithmetic alone.

    The first `anchors` rows of every block of TRSV_BLOCK rows are anchor rows: x_i = 1 exactly (a random b_i, with the
    filler its products too, and L_ii := round_nearest_even(T_i); unit: b_i = 1 and nothing else).  A tail block that
    is no longer than `anchors` rows has none: its rows close against earlier blocks only.  Every other row is planted:
      * TRSV_RAND random entries against earlier planted columns, odd integers of `mbits` bits scaled so that the
        products a x_j step down from about 1 over a window of W bits (mbits = 53: every such product has fl(a x) != a x,
        asserted); with `filler`, +-2^f in every other earlier planted column (exact products below 2^-8), so that the
        strict triangle is dense but for the anchor columns;
      * the row is negated if need be so that planted row k is negative where k % 3 == 1, and closed by
        complete_to(T, COMPLETE_CLASSES[k % 5], TRSV_GAPS[(k // 5) % 4]).  Of the closing amount, the 52 bits around a
        quarter unit of the result go into b_i (so that b_i +- a quarter unit is a double again: `b_control`, which
        moves every planted total a quarter unit away from its tie); the rest, cut by split53, goes negated into
        anchor columns: the row's own block (consumed in the diagonal phase), earlier blocks (the tile phase), or
        alternating, by k % 3;
      * planted rows with k % 7 == 3 also get a pair +-G against two anchor columns (an earlier block's and the row's
        own where there is one), G of 53 random bits and 2^120 or 2^150 times the total (`cancel`): it cancels exactly,
        but while it sits in an expansion most bits of the total can only be kept in the remainder;
      * L_ii = +-d 2^e with d odd, 3 <= d < 4096, and e such that 1/2 < |x_i| < 2; unit: x_i = round_nearest_even(T_i),
        which is of the order of 1 because the entries are scaled against the x_j they meet.
    The first (planted rows) % 5 of them are turned into anchors, so the classes come in equal numbers.

    Returns L, b, want (x), totals (Fractions), per row: classes ('anchor' for anchors), tie_up, gap, c_int (the total
    in units of its deciding unit), own (per planted row: for each closing term in the matrix whether it sits in the
    row's own block, leading term first, the deciding one last), cancel, planted (mask), b_control, counts (planted_mix)."""
    A = anchors or (16 if W > 100 else 12)
    assert n > A and 1 <= mbits <= 53 and W >= 16
    rng = np.random.default_rng([seed, n, W, mbits, int(filler), int(unit), 4711])
    blocks = -(-n // TRSV_BLOCK)
    anchor = np.zeros(n, dtype=bool)
    for B in range(blocks):
        lo_, hi_ = B * TRSV_BLOCK, min(n, (B + 1) * TRSV_BLOCK)
        if B == 0 or hi_ - lo_ > A:
            anchor[lo_:lo_ + A] = True
    spare = np.nonzero(~anchor)[0]
    anchor[spare[:len(spare) % 5]] = True
    L, b, x, bc = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
    xf, totals = [None] * n, [None] * n
    classes = np.full(n, "anchor", dtype=object)
    tie_up, gap_of, c_int = np.zeros(n, dtype=bool), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=object)
    own, cancel = [None] * n, np.zeros(n, dtype=np.int64)
    done = []                                              # planted rows so far
    k = inexact = 0
    for i in range(n):
        blk = i // TRSV_BLOCK
        ent = {}                                           # column -> Fraction
        if anchor[i] and unit:
            b[i], x[i], xf[i], totals[i] = 1.0, 1.0, Fraction(1), Fraction(1)
            L[i, i] = 1.0
            continue
        cols = []
        if not anchor[i] and done:
            near = [j for j in done if j // TRSV_BLOCK == blk]
            cols = list(rng.choice(near, min(len(near), TRSV_RAND // 2), replace=False)) if near else []
            rest = [j for j in done if j not in cols]
            cols += list(rng.choice(rest, min(len(rest), TRSV_RAND - len(cols)), replace=False)) if rest else []
            for t, j in enumerate(int(c) for c in cols):
                o = 0 if t == 0 else int(rng.integers(1, W))
                xe = math.frexp(x[j])[1]
                a = Fraction(_odd(rng, mbits) * (1 if rng.random() < 0.5 else -1)) * _p2(-o - mbits + 1 - xe)
                ent[j] = a
                if mbits == 53 and abs(math.frexp(x[j])[0]) != 0.5:   # the TwoProd error term carries bits of the total
                    assert Fraction(float(a) * x[j]) != a * xf[j]      # (a carry row's x is a power of two if unit)
                    inexact += 1
        if filler and done:
            fs = rng.integers(8, min(W, 60), len(done))
            sg = rng.choice((-1, 1), len(done))
            for j, f, s in zip(done, fs.tolist(), sg.tolist()):
                if j not in ent:
                    ent[j] = s * _p2(-f - math.frexp(x[j])[1])
                    assert Fraction(float(ent[j]) * x[j]) == ent[j] * xf[j]
        T = -sum((a * xf[j] for j, a in ent.items()), Fraction(0))
        if anchor[i]:
            bi = Fraction(_odd(rng, 53) * (1 if rng.random() < 0.5 else -1)) * _p2(-52)
            T += bi
            r = round_nearest_even(T)
            assert r != 0.0
            b[i], L[i, i], x[i], xf[i], totals[i] = _exact_double(bi), r, 1.0, Fraction(1), T
            for j, a in ent.items():
                L[i, j] = _exact_double(a)
            continue
        cls, gap = COMPLETE_CLASSES[k % 5], TRSV_GAPS[(k // 5) % len(TRSV_GAPS)]
        if (T < 0) != (k % 3 == 1):
            ent, T = {j: -a for j, a in ent.items()}, -T
        lo = -(T.denominator.bit_length() - 1) if T else -(gap + 53)
        Ti = T.numerator
        assert Fraction(Ti) * _p2(lo) == T
        fix = complete_to(Ti, cls, gap)
        u = lo - fix.scale                                 # the closing terms count in units of 2^u
        diff = fix.total - (Ti << fix.scale)
        # The closing amount `diff` is cut in two.  b_i takes the 52 bits of |diff| from bit `low` up, a window that
        # holds the quarter-unit position sh - 2 with k0 = 2, 25 or 49 bits below it: |bpart| < 2^52 and q = 2^k0 in
        # units of 2^low, so bpart +- q has at most 53 bits and b_control is a double again.  What is left of diff
        # above and below the window goes to the anchor columns in pieces of 53 bits.
        sh = abs(fix.total).bit_length() - 53              # the unit in the last place of the rounded total is 2^sh
        k0 = min((2, 25, 49)[k % 3], sh - 2)
        low, q = sh - 2 - k0, 1 << (sh - 2)                # q: a quarter of that unit
        bpart = (-1 if diff < 0 else 1) * (((abs(diff) >> low) & ((1 << 52) - 1)) << low)
        terms = split53(diff - bpart)
        away = (-1 if fix.total < 0 else 1) * (-1 if cls == "tie-1" else 1)      # the side that leads away from the tie
        b[i], bc[i] = _exact_double(Fraction(bpart) * _p2(u)), _exact_double(Fraction(bpart + away * q) * _p2(u))
        mine = [j for j in np.nonzero(anchor[:i])[0].tolist() if j // TRSV_BLOCK == blk]
        early = [j for j in np.nonzero(anchor[:i])[0].tolist() if j // TRSV_BLOCK != blk]
        assert len(terms) <= len(mine) + len(early), "the closing terms do not fit the anchors available"
        mine = [mine[int(p)] for p in rng.permutation(len(mine))]
        early = [early[int(p)] for p in rng.permutation(len(early))]
        flags = []
        for t, term in enumerate(terms):                   # k % 3: own block first, earlier blocks first, alternating
            own_first = (True, False, t % 2 == 0)[k % 3]
            j = _take(mine, early) if own_first else _take(early, mine)
            flags.append(j // TRSV_BLOCK == blk)
            ent[j] = -Fraction(term) * _p2(u)
        if k % 7 == 3 and mine and len(mine) + len(early) >= 2:
            # a pair that cancels exactly, 2^120 or 2^150 times the total: while it is in the expansion the bits of the
            # total below 2^-39 (2^-9) of it can only be kept in the LDS remainder, under the bound B
            c = (120, 150)[(k // 7) % 2]
            big = Fraction(_odd(rng, 53)) * _p2(abs(fix.total).bit_length() + u + c - 53)
            ent[_take(early, mine)] = -big                 # consumed in the tile phase where there is an earlier block
            ent[_take(mine, early)] = big
            cancel[i] = c
        for j, a in ent.items():
            L[i, j] = _exact_double(a)
        tot = Fraction(fix.total) * _p2(u)
        assert tot == Fraction(float(b[i])) - sum((Fraction(float(L[i, j])) * xf[j] for j in ent), Fraction(0))
        r = round_nearest_even(tot)
        if unit:
            L[i, i], x[i] = 1.0, r
        else:
            d = _odd(rng, int(rng.integers(2, 13)))
            L[i, i] = math.ldexp(float(d), math.frexp(r)[1] - d.bit_length()) * (1 if rng.random() < 0.5 else -1)
            x[i] = r / float(L[i, i])
        xf[i], totals[i] = Fraction(float(x[i])), tot
        c_int[i] = fix.total >> fix.unit
        name, up = classify(c_int[i])
        classes[i], tie_up[i], gap_of[i], own[i] = name, up, gap, tuple(flags)
        done.append(i)
        k += 1
    planted = ~anchor
    assert np.isfinite(x).all() and (np.abs(x) > 2.0 ** -6).all() and (np.abs(x) < 2.0 ** 6).all()
    assert (x[anchor] == 1.0).all() and k % 5 == 0 and (mbits < 53 or inexact >= 3 * k)
    chk, chk_tot = trsv_exact(L, b, unit)                  # the whole system again, from the doubles alone
    assert (chk.view(np.int64) == x.view(np.int64)).all() and chk_tot == totals
    counts = planted_mix(SimpleNamespace(classes=classes[planted], tie_up=tie_up[planted], c_int=c_int[planted]))
    for g in TRSV_GAPS:
        assert ((gap_of == g) & planted).any()
    if any(anchor[B * TRSV_BLOCK] for B in range(1, blocks)):   # both placements of the deciding (last) closing term
        deep = [own[i][-1] for i in np.nonzero(planted & (gap_of >= 30))[0] if own[i]]
        assert any(deep) and not all(deep)
    assert (cancel == 120).any() and (cancel == 150).any()
    bc[anchor] = b[anchor]
    return SimpleNamespace(n=n, W=W, mbits=mbits, filler=filler, unit=unit, anchors=A, L=L, b=b, want=x, totals=totals,
                           classes=classes, tie_up=tie_up, gap=gap_of, c_int=c_int, own=own, cancel=cancel, planted=planted,
                           b_control=bc, counts=counts)


def trsv_must_round_as_integers(case):
    """rows the register certificate cannot decide: exact ties and carries, and near-ties whose deciding unit is 30 or
    more bits below the half unit (the kernel inflates its error bound by 1.0000001, about 1 + 2^-23.25, so a total
    within 2^-24 of the half unit, relative to it, cannot be certified: 30 leaves margin over that figure)"""
    ties = (case.classes == "tie") | (case.classes == "carry")
    near = (case.classes == "tie+1") | (case.classes == "tie-1")
    return int((ties | (near & (case.gap >= 30))).sum())


def trsv_operands(L, b, uplo, trans, diag="N", lda_pad=0, offa=0, incx=1, offx=0):
    """ExTRSV's arguments for the logical system (L, b): column-major A with op(A) lower ('L','N' stores L; 'U','T' its
    transpose) or upper ('U','N' and 'L','T': the system reversed, so that backward substitution meets the rows in the
    logical order).  The triangle that must not be read, the lda padding, the offset prefixes and the incx gaps hold
    NaN, and so does the stored diagonal for diag = 'U'.  Returns (a, lda, xs, idx): logical row i is xs[idx[i]]."""
    L = np.asarray(L, dtype=np.float64)
    n = L.shape[0]
    M = np.where(np.tri(n, dtype=bool), L, np.nan)         # logical, NaN above the diagonal
    if diag == "U":
        np.fill_diagonal(M, np.nan)
    forward = (uplo == "L") != (trans == "T")
    if not forward:
        M = M[::-1, ::-1]
    if trans == "T":
        M = M.T                                            # M[r, c] is now element (r, c) of the stored A
    lda = n + lda_pad
    a = np.full(offa + n * lda, np.nan)
    a[offa:].reshape(n, lda)[:, :n] = M.T                  # column c of A is contiguous
    idx = offx + (np.arange(n) if forward else np.arange(n - 1, -1, -1)) * incx
    xs = np.full(offx + (n - 1) * incx + 1, np.nan)
    xs[idx] = b
    return a, lda, xs, idx


def range_rows_trsv(lead=0):
    """Rows of a triangular system whose totals sit at the ends of the double range, after `lead` rows of x = 1 and
    six support rows that fix x = 2^511, 2^-537, v, w (v, w in [1, 2) with 53-bit odd mantissas), 1 and 2^-600.  With
    lead + 6 a multiple of 64 (lead = 58) the support rows close one block of the kernel and the range rows open the
    next: every huge or tiny product is then formed in the tile phase and handed over; otherwise (lead = 0, 70) support
    and range rows share a block and the products are formed in the diagonal phase.  The range rows come last in the
    substitution order and no row consumes them; the one that overflows is the very last (0 * inf is NaN).  Returns
    L, b, want, totals, names and `rows` (name -> index)."""
    v, w = math.ldexp(float((1 << 52) | 0x5a5a5a5a5a5a5 | 1), -52), math.ldexp(float((1 << 52) | 0x3c3c3c3c3c3c3 | 1), -52)
    dmax = float((1 << 1024) - (1 << 971))
    big = math.ldexp(float((1 << 53) - 1), 947)             # the largest double below 2^1000
    sup = [2.0 ** 511, 2.0 ** -537, v, w, 1.0, 2.0 ** -600]
    H, Lo, V, Wc, One, Sm = (lead + t for t in range(6))
    rows = [   # name, b, diagonal, {column: entry}
        ("just below the overflow tie", dmax, 1.0, {H: -2.0 ** 459, Lo: 2.0 ** -537}),
        ("b = 2^1000, tie to even", 2.0 ** 1000, 3.0, {H: -2.0 ** 436}),
        ("b below 2^1000, carry", big, -5.0, {H: -2.0 ** 435}),
        ("product = 2^1000, tie to odd", 3 * 2.0 ** 947, 7.0, {H: -2.0 ** 489}),
        ("product below 2^1000, carry", 2.0 ** 946, 3.0, {H: -math.ldexp(float((1 << 53) - 1), 947 - 511)}),
        ("subnormal total, quotient a tie", 2.0 ** -1022, 2.0, {Lo: math.ldexp(float((1 << 52) - 3), -537)}),
        ("subnormal total, negative", -2.0 ** -1022, 1.0, {Lo: -math.ldexp(float((1 << 52) - 5), -537)}),
        ("subnormal quotient", math.ldexp(1.0 + 2.0 ** -52, -1000), 3 * 2.0 ** 40, {Lo: -2.0 ** -516}),
        ("subnormal quotient of a near-tie", math.ldexp(1.0 + 2.0 ** -52, -1000), -3 * 2.0 ** 33,
         {Lo: -2.0 ** -516, Sm: 2.0 ** -474}),
        ("zero by cancellation, positive diagonal", 2.0 ** -30, 3.0, {V: w, Wc: -v, One: 2.0 ** -30}),
        ("zero by cancellation, negative diagonal", -2.0 ** -30, -3.0, {V: -w, Wc: v, One: -2.0 ** -30}),
        ("tie at the overflow threshold", dmax, 1.0, {H: -2.0 ** 459}),
    ]
    n = lead + len(sup) + len(rows)
    L, b = np.zeros((n, n)), np.ones(n)
    np.fill_diagonal(L, 1.0)
    b[lead:lead + len(sup)] = sup
    index = {}
    for t, (name, bi, dia, ent) in enumerate(rows):
        i = lead + len(sup) + t
        b[i], L[i, i], index[name] = bi, dia, i
        for j, a in ent.items():
            L[i, j] = a
    want, totals = trsv_exact(L, b)
    tiny = 5e-324
    assert (want[:lead + len(sup)] == b[:lead + len(sup)]).all() and np.isfinite(want[:-1]).all()
    assert want[index["just below the overflow tie"]] == dmax and want[index["tie at the overflow threshold"]] == math.inf
    assert totals[index["tie at the overflow threshold"]] == (1 << 1024) - (1 << 970)
    assert totals[index["just below the overflow tie"]] == (1 << 1024) - (1 << 970) - Fraction(1, 1 << 1074)
    assert want[index["b = 2^1000, tie to even"]] == 2.0 ** 1000 / 3.0
    assert want[index["b below 2^1000, carry"]] == 2.0 ** 1000 / -5.0
    assert want[index["product = 2^1000, tie to odd"]] == (2.0 ** 1000 + 2.0 ** 949) / 7.0
    assert want[index["product below 2^1000, carry"]] == 2.0 ** 1000 / 3.0
    assert totals[index["subnormal total, quotient a tie"]] == Fraction(3, 1 << 1074)
    assert want[index["subnormal total, quotient a tie"]] == 2 * tiny
    assert want[index["subnormal total, negative"]] == -5 * tiny
    for name in ("subnormal quotient", "subnormal quotient of a near-tie"):
        assert 0.0 < abs(want[index[name]]) < 2.0 ** -1030 and totals[index[name]] > Fraction(1, 1 << 1001)
    zp, zn = want[index["zero by cancellation, positive diagonal"]], want[index["zero by cancellation, negative diagonal"]]
    assert zp == 0.0 and zn == 0.0 and math.copysign(1.0, zp) == 1.0 and math.copysign(1.0, zn) == -1.0
    assert totals[index["zero by cancellation, positive diagonal"]] == 0 and Fraction(v * w) != Fraction(v) * Fraction(w)
    return SimpleNamespace(n=n, lead=lead, L=L, b=b, want=want, totals=totals, names=[r[0] for r in rows], rows=index)
