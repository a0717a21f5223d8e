"""Inputs that sit on the edges of ExGEMM's path decision and on the seams of its operand scan, with derived results.

ExGEMM scans its operands (k_scan_* in csrc/blas3.hip) before it picks a contraction path: per vector (row of A' = fl(alpha A),
column of B) the top exponent and the lowest set bit, globally one flag for anything that is not a finite normal
number or a zero.  k_i8_decide / k_crt_decide (device) and exgemm_try_mfma (host) turn that into "digit slices",
"residues", "fp64 slices" or "leave it to the scalar kernel".  Every case here is a base pair of operands well inside
every path's domain plus ONE planted element or ONE planted vector that alone decides; nothing touches the GPU, the
library or the oracle.

Base.  P (257 x k) is the probed operand's vectors, Q (3 x k) the partner's: integers in +-[1, 127], i.e. mantissas of
7 bits (the reference below is legal up to 20) at exponent 0.  Probing A: A = P[:V], B = Q^T (m = V, n = 3); probing B:
A = Q, B = P[:V]^T (m = 3, n = V).  V = 1 uses vector 0 of the same storage.  At every probed position l the partner
holds Q[:, l] = (4, 0, -2): a power of two >= 1 (the only kind of finite partner a subnormal meets, so the product is an
exact double), a zero (0 x Inf = NaN) and a negative power of two (the other infinity).  Q[:, 3] = Q[:, 2], so a vector
(.., c, -c, ..) at positions 2, 3 cancels exactly against every partner vector; P[:, 1] is odd, so every vector's
lowest set bit is bit 0.

Reference.  Every base sum is below 127^2 * 2049 < 2^52, so the base result is one exact int64 matmul; only the outputs
a planted vector reaches (its row of C, or its column) are recomputed, as Python integers at a common scale
(`exact_dot`), and rounded by exact_cases.round_nearest_even.  Non-finite outputs are derived (`derive`): NaN if any
product is NaN (a NaN operand, Inf x 0) or products of both infinite signs occur, else the infinity of that sign.

Geometry, from the launch code in csrc/blas3_i8.hip / blas3_crt.hip / blas3_mfma.hip (the three are identical):
  * k_scan_contig (A for 'N', B for 'T'): one workgroup of 256 threads per vector; thread t reads t + 256 u + 1024 j,
    u = 0..3 in flight, j the trip of its loop.  Seams: the first and last thread of a sweep (0, 255), the first element
    of the second load (256), the last of the fourth (1023), the first of the second trip (1024) and the ragged end
    k - 1; k from {1, 255, 1025, 2049} gives one element, one sweep with an idle last thread, one trip plus one element,
    two trips plus one.
  * k_scan_strided (A for 'T', B for 'N'): one thread per vector, gridDim.y = ysplit = 1 / 8 / 32 for k < 256 / < 2048 /
    >= 2048 slices of per = ceil(k / ysplit) elements, walked four at a time.  k from {255, 257, 2049} gives per = 255, 33
    and 65 (33 and 65 are no multiples of four: the last step of a slice is ragged).  Seams: 0, per - 1 | per between
    the first two slices, the first element of the last non-empty slice ((k - 1) // per * per) and k - 1.
  * vectors: k_scan_strided, k_scan_init and k_scan_finish put vector v in workgroup v / 256: with 257 vectors the
    seam is 255 | 256 = the last one; one vector alone is the other extreme.
"""
import functools
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

import exact_cases as X

NVEC = 257                                        # vectors of the probed operand (and 1: vector 0 of the same storage)
NPARTNER = 3
VECTORS = ((1, 0), (NVEC, 0), (NVEC, 255), (NVEC, 256))   # (vectors in use, probed vector)
LAYOUTS = (("A", "N"), ("A", "T"), ("B", "N"), ("B", "T"))
CONTIG_K = (1, 255, 1025, 2049)
STRIDED_K = (255, 257, 2049)
PARTNER_AT_PROBE = (4, 0, -2)
TWINS = (2, 3)                                    # Q[:, 3] == Q[:, 2]
I8_ERANGE, MFMA_ERANGE = 300, 400                 # |top exponent| the int8 paths / the fp64 slices accept
I8_SPAN, MFMA_SPAN = 126, 84                      # bits of one vector they accept (16 digits - 2; 4 slices of 21)
FLAG_KINDS = ("nan", "+inf", "-inf", "subnormal")
SUBNORMAL = 3 * 2.0 ** -1074


def contiguous(operand, trans):
    """whether the vectors of that operand are contiguous along k in row-major storage (k_scan_contig)"""
    return (operand == "A") == (trans == "N")


def partner_trans(operand, trans):
    """transpose of the other operand: the four layouts then also cover ('N','N'), ('T','T'), ('T','N'), ('N','T')"""
    return trans if operand == "A" else ("T" if trans == "N" else "N")


def ysplit(k):
    return 32 if k >= 2048 else (8 if k >= 256 else 1)


def slice_len(k):
    return -(-k // ysplit(k))


def contig_positions(k):
    return sorted({p for p in (0, 255, 256, 1023, 1024, k - 1) if 0 <= p < k})


def strided_positions(k):
    per = slice_len(k)
    return sorted({p for p in (0, per - 1, per, (k - 1) // per * per, k - 1) if 0 <= p < k})


def positions(operand, trans, k):
    return contig_positions(k) if contiguous(operand, trans) else strided_positions(k)


def layout_ks(operand, trans):
    return CONTIG_K if contiguous(operand, trans) else STRIDED_K


SEAM_IDS = [(op, tr, k) for op, tr in LAYOUTS for k in layout_ks(op, tr)]


# ---------------------------------------------------------------------------------------------
# base operands
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base(k):
    """P, Q as int64 and float64, the exact base result P Q^T (int64 and rounded), spans and top exponents"""
    rng = np.random.default_rng([20240, k])

    def draw(rows):
        return rng.integers(1, 128, (rows, k)) * rng.choice([-1, 1], (rows, k))

    P, Q = draw(NVEC), draw(NPARTNER)
    if k > 1:
        P[:, 1] |= 1                                            # (two's complement: keeps the sign, sets bit 0)
    probed = sorted(set(contig_positions(k)) | set(strided_positions(k)))
    for l in probed:
        Q[:, l] = PARTNER_AT_PROBE
    if k > TWINS[1]:
        assert not set(TWINS) & set(probed)
        Q[:, TWINS[1]] = Q[:, TWINS[0]]
    c = P @ Q.T                                                 # exact: |sum| < 2^52 (test_gemm_decision_cases.py)
    Pf = P.astype(np.float64)
    return SimpleNamespace(k=k, P=P, Q=Q, Pf=Pf, Qf=Q.astype(np.float64), c=c, want=X.rounded(X.obj(c)), probed=probed,
                           bits_q=X.span_bits(X.obj(Q), 1), bits_p={V: X.span_bits(X.obj(P[:V]), 1) for V in (1, NVEC)},
                           spans=[vector_facts(row)[0] for row in Pf])


# ---------------------------------------------------------------------------------------------
# integer reference of the outputs a planted vector reaches
# ---------------------------------------------------------------------------------------------
def _int_exp(x):
    """finite doubles -> (integers, exponents) with x = i * 2^e exactly (subnormals included)"""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    return (m * 2.0 ** 53).astype(np.int64).tolist(), (e.astype(np.int64) - 53).tolist()


def exact_dot(x, y):
    """sum x_l y_l of finite doubles as (Python integer, exponent)"""
    ix, ex = _int_exp(x)
    iy, ey = _int_exp(y)
    terms = [(a * b, p + q) for a, p, b, q in zip(ix, ex, iy, ey) if a and b]
    if not terms:
        return 0, 0
    e0 = min(e for _, e in terms)
    return sum(v << (e - e0) for v, e in terms), e0


def derive(x, y):
    """the correctly rounded double of sum x_l y_l, x a vector of A' and y one of B; non-finite by the rule above"""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(all="ignore"):
        p = x * y                                               # finite x finite never leaves the range here (|e| < 900)
    if np.isnan(p).any() or ((p == np.inf).any() and (p == -np.inf).any()):
        return math.nan
    if np.isinf(p).any():
        return math.inf if (p == np.inf).any() else -math.inf
    v, e = exact_dot(x, y)
    return X.round_nearest_even(Fraction(v) * Fraction(2) ** e)


def with_vector(b, V, v, vec, operand, alpha=1.0):
    """The expected A' B (before beta) when vector v of the probed operand holds `vec`: m x n doubles.  alpha must make
    fl(alpha a) exact on the base (a power of two, 3, 0) or be NaN; the planted vector's outputs go through derive()."""
    assert v < V
    if math.isnan(alpha):
        rows = np.full((V, NPARTNER), math.nan)
    else:
        num, den = Fraction(alpha).numerator, Fraction(alpha).denominator
        assert den & (den - 1) == 0 and ((b.Pf[:V] * alpha) * den == b.Pf[:V] * num).all()
        rows = b.want[:V].copy() if alpha == 1.0 else X.rounded(X.obj(b.c[:V]) * num, -(den.bit_length() - 1))
    with np.errstate(all="ignore"):
        scaled = np.asarray(vec, dtype=np.float64) * (alpha if operand == "A" else 1.0)
        part = b.Qf * (alpha if operand == "B" else 1.0)
    rows[v] = [derive(scaled, part[j]) if operand == "A" else derive(part[j], scaled) for j in range(NPARTNER)]
    return rows if operand == "A" else np.ascontiguousarray(rows.T)


def vector_facts(vec):
    """(span in bits, top exponent, flagged) of one vector as the scan sees it; zeros are skipped"""
    vec = np.asarray(vec, dtype=np.float64)
    flagged = bool((~np.isfinite(vec)).any() or ((vec != 0) & (np.abs(vec) < 2.0 ** -1022)).any())
    if flagged:
        return None, None, True
    ints, exps = _int_exp(vec)
    hi = [e + abs(i).bit_length() for i, e in zip(ints, exps) if i]
    lo = [e + (abs(i) & -abs(i)).bit_length() - 1 for i, e in zip(ints, exps) if i]
    return (max(hi) - min(lo), max(hi) - 1, False) if hi else (0, None, False)


# ---------------------------------------------------------------------------------------------
# what the decision must be
# ---------------------------------------------------------------------------------------------
def i8_digits(bits_a, bits_b):
    """k_i8_decide: span + 2 bits in 8-bit digits; counts within one of each other (from 4 up) are padded to a common
    count that splits into equal blocks (even beyond 9).  None: more than 16 digits."""
    sa, sb = max(1, (bits_a + 9) // 8), max(1, (bits_b + 9) // 8)
    if max(sa, sb) > 16:
        return None
    hi, lo = max(sa, sb), min(sa, sb)
    if lo >= hi - 1 and hi >= 4:
        sa = sb = hi if hi <= 9 else 2 * ((hi + 1) // 2)
    return sa, sb


def expected_info(path, bits_a, bits_b, k):
    """the leading words of exblas_last_gemm_info for an ACCEPTED product on a forced path"""
    if path == 2:
        return [2, *i8_digits(bits_a, bits_b)]
    if path == 3:
        s = max(2, -(-max(bits_a, bits_b) // 21))
        return [1, s, s]
    na, nb = max(bits_a, 1), max(bits_b, 1)
    return [4, na, nb, X.crt_moduli_needed(na, nb, k)]


def seen_bits(b, V, v, vec, operand, alpha=1.0):
    """(bits of A', bits of B) as the scan reports them with `vec` planted as vector v of the probed operand"""
    sp, sq = (alpha, 1.0) if operand == "A" else (1.0, alpha)
    others = [r for r in range(V) if r != v]
    if alpha == 1.0:
        rest, bq = max((b.spans[r] for r in others), default=0), b.bits_q
    else:
        rest, bq = max((vector_facts(b.Pf[r] * sp)[0] for r in others), default=0), bits_of(b.Qf * sq)
    bp = max(rest, vector_facts(np.asarray(vec, dtype=np.float64) * sp)[0])
    return (bp, bq) if operand == "A" else (bq, bp)


# ---------------------------------------------------------------------------------------------
# planted vectors
# ---------------------------------------------------------------------------------------------
def lone_special(b, v, pos, kind):
    """The base vector with one NaN / Inf at pos; for the subnormal the rest of the vector is (c, -c) on the twin
    positions (it cancels exactly, the subnormal's product is the result) -- with k = 1 the subnormal stands alone."""
    vec = b.Pf[v].copy()
    if kind == "subnormal":
        vec[:] = 0.0
        if b.k > TWINS[1]:
            vec[TWINS[0]], vec[TWINS[1]] = 5.0, -5.0
        vec[pos] = -SUBNORMAL if (v + pos) % 2 else SUBNORMAL
    else:
        vec[pos] = {"nan": math.nan, "+inf": math.inf, "-inf": -math.inf}[kind]
    return vec


def lone_setter(b, v, pos, kind, e=60):
    """"top": +-2^e, the single largest element; "low": +-3 * 2^-e, the single element with the lowest set bit"""
    vec = b.Pf[v].copy()
    vec[pos] = math.ldexp(1.0 if kind == "top" else 3.0, e if kind == "top" else -e) * (-1 if (v + pos) % 2 else 1)
    return vec


def scaled_vector(b, v, top):
    """the base vector times the power of two that puts its top exponent exactly at `top`"""
    _, t0, _ = vector_facts(b.Pf[v])
    return np.ldexp(b.Pf[v], top - t0)


def span_vector(b, v, pos, bits):
    """a vector of exactly `bits` bits: +-2^(bits - 1) at pos over the base, whose lowest set bit is bit 0"""
    return lone_setter(b, v, pos, "top", e=bits - 1)


def carry_vector(b, v, pos, mant):
    """top exponent 299 with the leading element mant * 2^292 (mant = 160 = 1.25 * 2^7 or 192 = 1.5 * 2^7; everything
    else stays below 128 * 2^292, and three times it below 2^301)"""
    vec = b.Pf[v].copy()
    vec[pos] = mant
    return np.ldexp(vec, 299 - 7)


def bits_of(mat):
    """the widest span of a row of finite doubles (what the scan reports for an operand with these vectors)"""
    return max(vector_facts(row)[0] for row in np.asarray(mat, dtype=np.float64))


def alpha_cases(b, v, pos):
    """(name, alpha, vector v of A, accepted) -- the scan looks at fl(alpha A): the exponent rule met through alpha by a
    power of two and by a carry into the next binade, overflow to Inf and underflow to a subnormal of finite normal
    entries, alpha = 0 (an all-zero operand: accepted; with an Inf in A: NaN) and alpha = NaN"""
    small = lone_special(b, v, pos, "subnormal")
    small[pos] = 3 * 2.0 ** -1000
    big = b.Pf[v].copy()
    big[pos] = -2.0 ** 1000
    return [("299 x 2", 2.0, scaled_vector(b, v, 299), True), ("299 x 4", 4.0, scaled_vector(b, v, 299), False),
            ("1.25 x 3", 3.0, carry_vector(b, v, pos, 160.0), True), ("1.5 x 3", 3.0, carry_vector(b, v, pos, 192.0), False),
            ("-299 / 2", 0.5, scaled_vector(b, v, -299), True), ("-299 / 4", 0.25, scaled_vector(b, v, -299), False),
            ("overflow", 2.0 ** 100, big, False), ("underflow", 2.0 ** -73, small, False),
            ("zero", 0.0, b.Pf[v].copy(), True), ("zero x inf", 0.0, lone_special(b, v, pos, "+inf"), False),
            ("nan", math.nan, b.Pf[v].copy(), False)]


def seam_probes(operand, trans, k):
    """The probes of one (layout, k): for every position and every (V, v) one flag probe, one top-exponent probe and one
    lowest-bit probe.  The flag kind rotates over the four vectors of a position, the forced path alternates, the
    (fpe, early_exit) variant rotates by index."""
    out = []
    for pi, pos in enumerate(positions(operand, trans, k)):
        for vi, (V, v) in enumerate(VECTORS):
            r = pi + vi
            out.append(SimpleNamespace(kind=FLAG_KINDS[r % 4], V=V, v=v, pos=pos, path=(2, 4)[r % 2], variant=r % 7, beta=0.0))
            out.append(SimpleNamespace(kind="top", V=V, v=v, pos=pos, path=(4, 2)[r % 2], variant=(r + 2) % 7, beta=float(r % 2)))
            out.append(SimpleNamespace(kind="low", V=V, v=v, pos=pos, path=(2, 4)[r % 2], variant=(r + 4) % 7,
                                       beta=float((r + 1) % 2)))
    return out


def c_template(m, n, beta, pad=2):
    """C (m x (n + pad)) before the call: NaN in the body when beta = 0 (it must be ignored), small integers otherwise,
    the sentinel -7 in the padding"""
    c = np.full((m, n + pad), -7.0)
    if beta == 0.0:
        c[:, :n] = math.nan
    else:
        i, j = np.indices((m, n))
        c[:, :n] = ((7 * i + 3 * j) % 11 - 5).astype(np.float64)
    return c


def with_beta(s, beta, c0):
    """what C must hold afterwards: s where beta = 0 (the old body is ignored), else fl(fl(beta c) + s)"""
    s = np.asarray(s, dtype=np.float64)
    if beta == 0.0:
        return s
    with np.errstate(all="ignore"):
        return beta * c0[:, :s.shape[1]] + s
