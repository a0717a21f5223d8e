"""Cases for the ExPOTRF tests: the exact-sum Cholesky factorisation in Fraction arithmetic, and matrices whose exact
totals sit on ties, carries and near-ties.  Nothing here calls the code under test.

The definition (logical upper orientation, G = R^T R; uplo 'L' is L = R^T), row by row:
    r_jj = sqrt(Round(g_jj - sum_{k<j} r_kj^2)),   r_ji = Round(g_ji - sum_{k<j} r_kj r_ki) / r_jj   (i > j)
every sum exact and rounded once; at the first radicand that is not > 0 the rounded radicand is stored at (j, j), the
rest stays as it was and info = j + 1 (LAPACK's rule).

Planted systems (`planted`).  G is block diagonal; a block is [[I_4, B], [B^T, D]] with B 4 x m.  The four identity rows
make r_kj = g_kj free doubles, so row 4 of the block (the PLANTED ROW) has totals over input doubles alone:
    t_0 = d_00 - sum_k b_k0^2,      t_i = d_0i - sum_k b_k0 b_ki.
Column 0 of B is few-bit (n0 odd, beta a power of two, n2, and a fourth entry that only the diagonal uses), so that b_k0 b_ki are exact and short, and the one free
double d_0i closes the total onto its class: b_0i = s (q + 1/2) makes n0 b_0i an odd multiple of the half unit, so
tie + Sigma is a double again; beta b_1i cancels the deciding unit of a near-tie however far below it lies.  The
diagonal radicand takes the squares n0^2 + beta^2 + n2^2 instead: squares only ADD, so a near-tie on the diagonal lies
below its tie (g = T + 2^-gap needs the fourth entry 2^-(gap/2): the gap is made even), and a quarter-unit control there uses a unit
of 8.  The other rows of D are a large random diagonal: what follows the planted row is an ordinary dense factorisation.
The builder asserts its claims: every entry is an exact double by construction of floats, and the whole system is
refactored from the doubles alone by potrf_exact, whose totals must have the planted classes and roundings."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

GAPS = (1, 30, 110, 250)               # exact_cases.TRSV_GAPS: bits between the half unit and the deciding unit
CLEAR, TIE, NEAR = 1, 2, 3             # potrf_exact(detail=True).kind: expected in registers, never there, either
A2 = float(2 ** 27 + 1)                # the 2 x 2 case: G = [[1, a], [a, a^2 + 3]], a^2 = 2^54 + 2^28 + 1
G2 = np.array([[1.0, A2], [A2, float(2 ** 54 + 2 ** 28 + 4)]])
# ... and its sibling: a^2 = 2^56 + 6 2^28 + 9 rounds UP to g = a^2 + 7: the exact radicand 7 is positive by less than a
# unit (16) of the leading term, a routine that rounds the product first sees 0 and reports a breakdown
A7 = float(2 ** 28 + 3)
G7 = np.array([[1.0, A7], [A7, float((2 ** 28 + 3) ** 2 + 7)]])


def _round(total):
    """the one rounding of an exact total: float() of a Fraction rounds to nearest even; beyond the range it is +-inf"""
    try:
        return float(total)
    except OverflowError:
        return float("inf") if total > 0 else float("-inf")


def _kind(t, v):
    """how far the exact total t is from a tie of the doubles around its rounding v"""
    if t == 0:
        return CLEAR
    if not math.isfinite(v) or abs(v) < 2.0 ** -960 or abs(v) >= 2.0 ** 1019:
        return TIE                      # outside the range the register certificate takes on
    err, half = abs(t - Fraction(v)), Fraction(math.ulp(v)) / 2
    pow2 = math.frexp(abs(v))[0] == 0.5
    if pow2 and abs(t) < abs(v):
        half /= 2
    if err == 0:
        return CLEAR
    if err == half:
        return TIE
    return CLEAR if (not pow2 and err <= half * (1 - Fraction(1, 2 ** 20))) else NEAR


def potrf_exact(G, uplo="U", detail=False):
    """(R, info): the definition in Fraction arithmetic on the `uplo` triangle of G (the other triangle is not read and
    comes back as it is).  float() does the one rounding, math.sqrt the root, the quotient of two np.float64 the
    division; zero entries are skipped; a non-finite entry decides the totals it meets in IEEE arithmetic.  detail: also a
    namespace with V (the rounded totals) and kind (CLEAR / TIE / NEAR per fixed entry, 0 elsewhere), both in the upper
    orientation."""
    G = np.asarray(G, dtype=np.float64)
    p = G.shape[0]
    up = uplo in ("U", "u")
    out = G.copy()
    get = (lambda j, i: G[j, i]) if up else (lambda j, i: G[i, j])

    def put(j, i, v):
        if up:
            out[j, i] = v
        else:
            out[i, j] = v

    nz = [dict() for _ in range(p)]     # column i: {k: Fraction(r_ki)} of its fixed finite non-zero entries
    bad = [dict() for _ in range(p)]    # column i: {k: r_ki} of its fixed non-finite entries
    rf = np.zeros((p, p))               # the fixed entries, upper orientation (what a non-finite entry meets)
    V, kind = np.zeros((p, p)), np.zeros((p, p), dtype=np.int8)
    info = 0
    with np.errstate(all="ignore"):
        for j in range(p):
            row = nz[j]
            for i in range(j, p):
                g = float(get(j, i))
                # a non-finite operand decides the total in IEEE arithmetic: Inf - Inf and 0 * Inf are NaN
                special = [] if math.isfinite(g) else [g]
                special += [-float(np.float64(rf[k, j]) * np.float64(rf[k, i])) for k in sorted(set(bad[j]) | set(bad[i]))
                            if k < j]
                if special:
                    t, v = None, float(np.sum(np.array(special)))
                else:
                    col = nz[i]
                    t = Fraction(g)
                    if i == j:
                        for f in row.values():
                            t -= f * f
                    elif row and col:
                        for k, f in row.items():
                            c = col.get(k)
                            if c is not None:
                                t -= f * c
                    v = _round(t)
                V[j, i], kind[j, i] = v, (TIE if t is None else _kind(t, v))
                if i == j:
                    if not v > 0:
                        put(j, j, v)
                        info = j + 1
                        break
                    rjj = np.float64(math.sqrt(v))
                    put(j, j, rjj)
                else:
                    r = np.float64(v) / rjj
                    put(j, i, r)
                    rf[j, i] = r
                    if not math.isfinite(r):
                        bad[i][j] = float(r)
                    elif r != 0:
                        nz[i][j] = Fraction(float(r))
            if info:
                break
    if detail:
        return out, info, SimpleNamespace(V=V, kind=kind)
    return out, info


def fixed_entries(p, info):
    """how many entries a call fixed: all, or the rows before the breakdown at pivot info - 1 and its radicand"""
    if info == 0:
        return p * (p + 1) // 2
    j = info - 1
    return j * (2 * p - j + 1) // 2 + 1


def embedded(p, at, g2=G2):
    """the 2 x 2 case (or its sibling G7) at rows / columns at = (a0, a1) of an otherwise diagonal G (diagonal j + 1)"""
    G = np.diag(np.arange(1.0, p + 1.0))
    a0, a1 = at
    G[a0, a0], G[a0, a1], G[a1, a0], G[a1, a1] = g2[0, 0], g2[0, 1], g2[1, 0], g2[1, 1]
    return G


# ---- planted systems -------------------------------------------------------------------------------------------------
OFF_SEQ = ("tie", "tie_odd", "carry", "near+", "near-", "ctrl+", "ctrl-")
DIAG_SEQ = ("tie", "near", "carry", "ctrl+", "tie_odd", "near", "ctrl-", "near", "near")
BLOCKS = {40: (5, 13, 10), 64: (29, 27), 65: (9, 48), 130: (36, 83)}   # m per block (a block has 4 + m rows)


def _mant(rng, cls):
    m = int(rng.integers(2 ** 52, 2 ** 53 - 4))
    if cls == "carry":
        return 2 ** 53 - 1
    if cls == "tie_odd":
        return m | 1
    return m & ~1 if cls == "tie" else m


def _f(x):
    """a Fraction that must be a double"""
    v = float(x)
    assert Fraction(v) == x, x
    return v


def _block(rng, m, dcls, dgap, off):
    """one block: (4 + m) x (4 + m) doubles and the plants [(row, col, class, gap, want)] in block coordinates"""
    n = 4 + m
    Gb = np.zeros((n, n))
    Gb[:4, :4] = np.eye(4)
    plants = []
    # the diagonal radicand and the few-bit column 0 of B
    M = _mant(rng, dcls.rstrip("+-"))
    n0 = int(rng.choice([3, 5, 7, 9, 11, 13]))
    if dcls in ("tie", "tie_odd", "carry"):
        beta, n2, bd, T0 = Fraction(2), 4, Fraction(0), Fraction(2 * M + 1)
        want = 2 * M + (2 if dcls != "tie" else 0)
    elif dcls == "near":
        g = dgap + (dgap & 1)
        beta, n2, bd, T0 = Fraction(2), 4, Fraction(1, 2 ** (g // 2)), Fraction(2 * M + 1) - Fraction(1, 2 ** g)
        want = 2 * M
    else:
        up = dcls == "ctrl+"
        beta, n2, bd, T0 = Fraction(4 if up else 2), 5, Fraction(0), Fraction(8 * M + 4 + (2 if up else -2))
        want = 8 * M + (8 if up else 0)
    col0 = (Fraction(n0), beta, Fraction(n2), bd)   # bd: the diagonal's own deciding unit; no other column meets it
    for k in range(4):
        Gb[k, 4] = Gb[4, k] = _f(col0[k])
    Gb[4, 4] = _f(T0 + sum(c * c for c in col0))
    plants.append((4, 4, "d:" + dcls, dgap if dcls == "near" else 0, float(want)))
    # the off-diagonal totals of the planted row
    for li in range(1, m):
        cls, gap = off[li - 1]
        s = -1 if rng.integers(2) else 1
        M = _mant(rng, cls.rstrip("+-"))
        delta = Fraction(0)
        if cls.startswith("near"):
            delta = Fraction(1 if cls[-1] == "+" else -1, 2 ** (gap + 1))
        elif cls.startswith("ctrl"):
            delta = Fraction(1 if cls[-1] == "+" else -1, 4)
        T = s * (Fraction(M) + Fraction(1, 2) + delta)
        q, r2, r3 = -int(rng.integers(2 ** 10, 2 ** 20)), -4 * int(rng.integers(0, 5)), -int(rng.integers(0, 9))
        x = (s * (Fraction(q) + Fraction(1, 2)), (-s * delta if delta else Fraction(s * r2)) / beta, Fraction(s * r3))
        for k in range(3):
            Gb[k, 4 + li] = Gb[4 + li, k] = _f(x[k])
        Gb[4, 4 + li] = Gb[4 + li, 4] = _f(T + sum(col0[k] * x[k] for k in range(3)))
        up = cls in ("tie_odd", "carry", "near+", "ctrl+")
        plants.append((4, 4 + li, cls, gap if cls.startswith("near") else 0, float(s * (M + (1 if up else 0)))))
        Gb[4 + li, 4 + li] = float(2 ** 60 + int(rng.integers(0, 2 ** 52)) * 2 ** 8)
    return Gb, plants


@lru_cache(maxsize=None)
def planted(p, pure=False, seed=0):
    """The planted system of size p (a key of BLOCKS).  pure: every near-tie becomes a quarter-unit control, so that no
    entry of the system is left to either side of the register certificate (asserted: kind has no NEAR).  Returns a
    namespace: G (symmetric, both triangles), R and info from potrf_exact, kind, plants [(row, col, class, gap, want)]
    and counts {class: n}."""
    rng = np.random.default_rng(1000 * p + seed)
    G = np.eye(p)
    plants, at, di, oi = [], 0, list(BLOCKS).index(p) * 2, 0
    for m in BLOCKS[p]:
        dcls = DIAG_SEQ[di % len(DIAG_SEQ)]
        dgap = GAPS[di % 4]
        di += 1
        off = []
        for _ in range(m - 1):
            off.append((OFF_SEQ[oi % 7], GAPS[(oi // 7) % 4]))
            oi += 1
        if pure:
            dcls = "ctrl-" if dcls == "near" else dcls
            off = [(c.replace("near", "ctrl"), g) for c, g in off]
        Gb, pl = _block(rng, m, dcls, dgap, off)
        n = 4 + m
        G[at:at + n, at:at + n] = Gb
        plants += [(at + r, at + c, cls, gap, want) for r, c, cls, gap, want in pl]
        at += n
    assert at <= p and (G == G.T).all()
    R, info, d = potrf_exact(G, "U", detail=True)
    assert info == 0
    counts = {}
    for r, c, cls, gap, want in plants:
        name = cls.split(":")[-1]
        assert d.V[r, c] == want, (r, c, cls, gap, d.V[r, c], want)
        k = d.kind[r, c]
        if name.startswith("ctrl"):
            assert k == CLEAR, (r, c, cls)
        elif name.startswith("near"):
            assert k == (NEAR if gap > 9 else k), (r, c, cls, gap)
        else:
            assert k == TIE, (r, c, cls)
        counts[cls] = counts.get(cls, 0) + 1
    if pure:
        assert not (d.kind == NEAR).any()
    return SimpleNamespace(p=p, G=G, R=R, info=info, kind=d.kind, V=d.V, plants=plants, counts=counts)


# ---- breakdowns ------------------------------------------------------------------------------------------------------
def breakdown_pivots(p):
    return sorted({j for j in (0, 3, 4, 63, 64, 65, p - 1) if j < p})


def breakdown(p, j, what, seed=0):
    """G = R0^T R0 for R0 = [[1, a^T], [0, diag(s)]] with small integers (every total exact: r_0i = a_i, the other
    off-diagonal totals 0, the radicands s_i^2), and the radicand of pivot j made 0 ("zero"), -1 ("neg") or NaN
    ("nan")."""
    rng = np.random.default_rng(seed + 7 * p + j)
    a = rng.integers(1, 9, p - 1).astype(np.float64)
    s = rng.integers(2, 9, p - 1).astype(np.float64)
    G = np.zeros((p, p))
    G[0, 0] = 1.0
    G[0, 1:] = G[1:, 0] = a
    G[1:, 1:] = np.outer(a, a) + np.diag(s * s)
    rad = G[j, j] - (a[j - 1] ** 2 if j else 0.0)
    G[j, j] += {"zero": -rad, "neg": -rad - 1.0, "nan": np.nan}[what]
    return G


# ---- ordinary matrices -----------------------------------------------------------------------------------------------
def gram(p, seed=0, bits=53):
    """X^T X for an integer-valued X with (2 p + 3) rows of `bits`-bit entries, computed exactly as Python integers and
    rounded once per entry: what ExBDOT gives"""
    rng = np.random.default_rng(seed + 31 * p + bits)
    n = 2 * p + 3
    X = [[int(rng.integers(-2 ** (bits - 1), 2 ** (bits - 1))) for _ in range(p)] for _ in range(n)]
    G = np.zeros((p, p))
    for i in range(p):
        for j in range(i, p):
            G[i, j] = G[j, i] = float(sum(X[r][i] * X[r][j] for r in range(n)))
    return G


def banded(p, seed=0):
    """a diagonally dominant symmetric G of bandwidth 5 (two off-diagonals a side) with full-mantissa entries"""
    rng = np.random.default_rng(seed + p)
    G = np.diag(1024.0 + rng.random(p))
    for o in (1, 2):
        v = rng.random(p - o) * 2 - 1
        G += np.diag(v, o) + np.diag(v, -o)
    return G


def restate(G):
    """a second, plain restatement of the definition for small cases (upper, dense loops, no skipping)"""
    G = np.asarray(G, dtype=np.float64)
    p = G.shape[0]
    R = G.copy()
    for j in range(p):
        t = Fraction(float(G[j, j])) - sum(Fraction(float(R[k, j])) ** 2 for k in range(j))
        v = _round(t)
        if not v > 0:
            R[j, j] = v
            return R, j + 1
        R[j, j] = math.sqrt(v)
        for i in range(j + 1, p):
            t = Fraction(float(G[j, i])) - sum(Fraction(float(R[k, j])) * Fraction(float(R[k, i])) for k in range(j))
            R[j, i] = np.float64(_round(t)) / np.float64(R[j, j])
    return R, 0


# ---- the square root, the division and the range ---------------------------------------------------------------------
def root_values():
    """512 radicands: neighbours of perfect squares, perfect squares, 2^-1074, the largest double, 2^-1022 and its
    predecessor, then random doubles over the whole range"""
    rng = np.random.default_rng(512)
    v = np.ldexp(rng.random(512) + 1.0, rng.integers(-1000, 1000, 512))
    k = rng.integers(3, 2 ** 26, 120).astype(np.float64)
    v[:120] = np.nextafter(k * k, np.where(np.arange(120) % 2 == 0, np.inf, 0.0))    # neighbours of perfect squares
    v[120:160] = k[:40] * k[:40]
    v[160], v[161], v[162], v[163] = 5e-324, np.finfo(np.float64).max, 2.0 ** -1022, np.nextafter(2.0 ** -1022, 0.0)
    return v


def range_cases():
    """Inside the product domain of the solves (a product of two non-zero entries is at least 2^-968 in magnitude, so that
    its error term is a double): totals and radicands that land among the subnormals, a total beyond the largest double,
    and an infinite radicand."""
    out = []
    # r_01 r_02 = 2^-968 (1 + 3 2^-52 + 2^-103) against g_12 = its rounding: the total is the error term, -2^-1071
    G = np.eye(3)
    G[0, 1], G[0, 2] = (1 + 2.0 ** -52) * 2.0 ** -484, (1 + 2.0 ** -51) * 2.0 ** -484
    G[1, 2] = G[0, 1] * G[0, 2]
    out.append(("subnormal total", G))
    # r_01^2 lies 2^27 - 1 units of 2^-1072 below the double g_11: the radicand is that, a subnormal
    m = 2 ** 52 + 2 ** 26 - 1
    G = np.eye(2)
    G[0, 1] = float(Fraction(m, 2 ** 536))
    G[1, 1] = float(Fraction(m * m + 2 ** 27 - 1, 2 ** 1072))
    assert Fraction(G[1, 1]) - Fraction(G[0, 1]) ** 2 == Fraction(2 ** 27 - 1, 2 ** 1072)
    out.append(("subnormal radicand", G))
    # a total beyond the range: +Inf, which the last radicand then meets (-Inf: a breakdown at the last pivot)
    big = 1.5 * 2.0 ** 1023
    G = np.diag([1.0, big, big])
    G[0, 1], G[0, 2], G[1, 2] = -1.5 * 2.0 ** 511, 1.5 * 2.0 ** 511, big
    out.append(("overflow", G))
    # +Inf passes as a radicand; its row becomes zeros
    G = np.diag([1.0, np.inf, 9.0, 16.0])
    G[0, 1], G[1, 2], G[1, 3], G[2, 3] = 3.0, 5.0, -7.0, 2.0
    out.append(("inf", G))
    out = [(name, np.triu(G) + np.triu(G, 1).T) for name, G in out]
    # ... and the same inside a larger matrix, beyond the first tile
    for name, G in list(out):
        big = np.diag(np.arange(2.0, 72.0))
        q = G.shape[0]
        big[66:66 + q, 66:66 + q] = G
        out.append((name + "@66", big))
    return out
