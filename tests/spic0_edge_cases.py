"""Edge cases for ExSpIC0: totals at the ends of the double range off the diagonal, radicands and roots over the whole range,
planted ties in long rows, wide source rows, the small structures and value sets for replays after a breakdown.  Nothing
here calls the code under test: every expectation comes from spic0_cases.ic0_exact, plain_ic0 and apply_exact.

`transplant(row, pad, wide, reader)` carries one row of range_block_cases.rows() (T = b - sum_k a_k x_k over the support
values x = 2^511, 2^-537, v, w, 1, 2^-600) into a symmetric CSR matrix.  IC(0) forms l_ik l_jk, so both factors of a product
are entries of L and each row takes its share of the scaling:

    rows 0 .. pad - 1          IDLE: a power of 4 on the diagonal (the root an exact power of two) and nothing else
    rows pad + k, k = 0 .. 5   SUPPORT: 1 on the diagonal, so l_kk = 1 and every l_.k is the stored value itself
    `wide` rows                WIDE: a small integer in every support column (l = the integer) and a diagonal that makes the
                               radicand a perfect square, with exact arithmetic
    the TARGET  j = s          x_k 2^-g_k in support column k (in [1, 2): g_k is the exponent of x_k) for the a_k the row
                               has, the diagonal dia^2 + sum_k (x_k 2^-g_k)^2 rounded once: l_jj = |dia| (asserted)
    the CARRIER i = s + 1      a_k 2^g_k in support column k, b in column s, a small integer in every idle column (l = integer
                               / power of two, exact) and the diagonal 2^40

(mirrors on the other side).  Both scalings are exact and their product is a_k x_k as a Fraction (asserted), the target
stores no idle column and a wide row neither the target nor the carrier, so the carrier's total in column s is exactly
row_total(row) and the fixed entry is fl(Round(T) / |dia|): the one IEEE division, on subnormal and huge numerators.  It is
the last entry of the carrier's L part (step kk = length - 2 of a carrier that owns `length` entries); `pad_for` gives the
pad for a length, LENGTHS puts it into every slot class of the several-entries form, at kk = 64 and at the 512-entry limit.
When the wave settles it, ic_resolve strides misses (the idle columns) and hits (the support columns).

The carrier's own radicand squares the a_k 2^g_k.  In the 2^1000 and overflow classes the square overflows: the radicand
is -Inf, the diagonal NaN and info[1] names the carrier.  In the subnormal classes the square lies below 2^-1074, outside
the product domain the kernels document, and far below the half unit of 2^40: it cannot decide the rounding.  ic0_exact
decides both.  The oracle's limbs hold neither, so the reference-rounding model exists for the other classes only
(`model(c, True)` is None elsewhere).

With wide > 0 the support row k has the wide rows, then (k, j) and (k, i) right of its diagonal: l_jk is fetched from index
`wide` of kc and the mirror post found at wide + 1 (62 .. 201: 1 to 4 passes of the wave).  `reader=True`: wide row t leaves
out support column k where t % 6 == k, so the indices differ per k and the searches of the wide rows hit and miss.

`padded_dense`, `planted` put a dense block behind idle rows with a stored ZERO in every idle column (l = 0, every product
0): the totals are unchanged and the entries move into long rows."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import potrf_cases as P
import range_block_cases as R
import spic0_cases as C
import spilu0_cases as S

NSUP = R.NSUP
LENGTHS = (8, 63, 64, 65, 66, 128, 129, C.MAX_ROW)   # entries the carrier owns; 66: the range entry itself at kk = 64
WIDES = (62, 63, 64, 200)
LEFT_OUT = ()                                        # rows of range_block_cases.rows() that cannot be carried: none
LEAD = 255
CARRIER_DIAGONAL = 2.0 ** 40


def _small(i):
    return float((1 + i % 7) * (1 if i % 2 else -1))


def _idle(i):
    """the diagonal of idle row i: a power of 4"""
    return 4.0 ** (i % 3)


def _sym(rows, i, j, v):
    rows[i][j] = rows[j][i] = v


def pad_for(row, length):
    pad = length - (len(row[4]) + 2)
    assert pad >= 0
    return pad


def transplant(row, pad=0, wide=0, reader=False):
    """the case that carries `row` (module docstring)"""
    name, cls, b, dia, ent = row
    sup = R.support()
    w0 = pad + NSUP
    s = w0 + wide
    i = s + 1
    rows = [dict() for _ in range(i + 1)]
    for t in range(pad):
        rows[t][t] = _idle(t)
        _sym(rows, i, t, _small(t))
    for k in range(NSUP):
        rows[pad + k][pad + k] = 1.0
    for t in range(wide):
        q = 2 + t % 5
        tot = q * q
        for k in range(NSUP):
            if not (reader and t % 6 == k):
                n = _small(3 * t + k)
                _sym(rows, w0 + t, pad + k, n)
                tot += int(n) ** 2
        rows[w0 + t][w0 + t] = float(tot)
    squares = Fraction(0)
    for k, a in ent.items():
        g = math.frexp(sup[k])[1] - 1
        x, y = math.ldexp(sup[k], -g), math.ldexp(a, g)
        assert 1.0 <= x < 2.0 and math.isfinite(y), (name, k)
        assert R.F(x) * 2 ** g == R.F(sup[k]) and R.F(y) == R.F(a) * Fraction(2) ** g, (name, k)
        assert R.F(x) * R.F(y) == R.F(a) * R.F(sup[k]), (name, k)
        _sym(rows, s, pad + k, x)
        _sym(rows, i, pad + k, y)
        squares += R.F(x) ** 2
    rows[s][s] = P._round(R.F(dia) ** 2 + squares)
    _sym(rows, i, s, b)
    rows[i][i] = CARRIER_DIAGONAL
    csr = S.from_rows(rows)
    crow = csr[0]
    mine = sorted(c for c in rows[i] if c <= i)
    e = mine.index(s)
    t = R.row_total(row)
    c = P._round(t)
    with np.errstate(all="ignore"):
        want = float(np.float64(c) / np.float64(abs(dia)))
    tag = f"{name} [pad {pad}, wide {wide}{', reader' if reader else ''}]"
    return SimpleNamespace(name=tag, row=name, cls=cls, pad=pad, wide=wide, reader=reader, csr=csr, s=s, carrier=i, target=s,
                           at=int(crow[i]) + e, e=e, length=len(mine), total=t, rounded=c, want=want, dia=abs(dia),
                           sign=math.copysign(1.0, dia),
                           ks=tuple(sorted(ent)), m=i + 1)


@lru_cache(maxsize=None)
def range_cases(length=0, wide=0, reader=False):
    """the 15 rows of range_block_cases.rows(), with a carrier that owns `length` entries (0: no idle row in front)"""
    out = tuple(transplant(row, pad_for(row, length) if length else 0, wide, reader) for row in R.rows())
    assert len(out) == 15 and not LEFT_OUT
    return out


def variants():
    """every (length, wide, reader) the tests run: the row classes, the wide sources, the reader"""
    return tuple([(n, 0, False) for n in LENGTHS] + [(0, w, False) for w in WIDES] + [(0, WIDES[-1], True)])


# ---- models ------------------------------------------------------------------------------------------------------------
_MODEL = {}
_oracle_round = lru_cache(maxsize=None)(S.reference_round)


class NotHeld(Exception):
    """a total that the oracle's canonical limbs do not hold"""


def reference_round(t):
    try:
        return _oracle_round(t)
    except AssertionError:
        raise NotHeld(t) from None


def flush_round(t):
    """nearest even, then subnormals flushed to zero: a defect the cases must be able to see"""
    v = P._round(t)
    return math.copysign(0.0, v) if abs(v) < 2.0 ** -1022 else v


def _settle(d, at, total):
    return d.ties + (1 if at is not None and R.settles(total) and d.kind[at] != C.TIE else 0)


def model_of(key, csr, reference=False, at=None, total=None):
    """(ll, info0, info1, detail) of a matrix, once per process.  detail.settle: the least number of entries that the
    accumulator must round (the model's ties, which include every entry outside the certificate's range, and the entry
    `at` where settles(total) holds).  reference: the model with the reference rounding, detail None; None altogether
    where the oracle's limbs do not hold a total."""
    key = (key, reference)
    if key not in _MODEL:
        if reference:
            try:
                _MODEL[key] = C.ic0_exact(*csr, rounder=reference_round) + (None,)
            except NotHeld:
                _MODEL[key] = None
        else:
            ll, i0, i1, d = C.ic0_exact(*csr, detail=True)
            d.settle = _settle(d, at, total)
            _MODEL[key] = (ll, i0, i1, d)
    return _MODEL[key]


def model(c, reference=False):
    return model_of(c.name, c.csr, reference, c.at, c.total)


def behind(lead, csr):
    """blockdiag(lead, csr) as CSR"""
    (c0, j0, v0), (c1, j1, v1) = lead, csr
    m0 = len(c0) - 1
    return np.concatenate([c0, c1[1:] + c0[-1]]), np.concatenate([j0, j1 + m0]), np.concatenate([v0, v1])


@lru_cache(maxsize=None)
def lead_model(reference=False):
    """the model of tridiagonal(LEAD), the healthy block in front: (ll, detail)"""
    ll, i0, i1, d = C.ic0_exact(*C.tridiagonal(LEAD), detail=True)
    assert (i0, i1) == (0, 0)
    if reference:
        ll = C.ic0_exact(*C.tridiagonal(LEAD), rounder=reference_round)[0]
    return ll, d


def behind_model(c, reference=False):
    """the model of behind(tridiagonal(LEAD), c.csr), composed: the off-diagonal blocks store nothing, so the two factors
    do not meet (test_spic0_edge_cases.py holds the composition to the model of the whole)"""
    got = model(c, reference)
    if got is None:
        return None
    ll, i0, i1, d = got
    lll, ld = lead_model(reference)
    assert i0 == 0
    if d is not None:
        d = SimpleNamespace(terms=ld.terms + d.terms, owned=ld.owned + d.owned, wide=ld.wide + d.wide, ties=ld.ties + d.ties,
                            nears=ld.nears + d.nears, settle=ld.ties + d.settle)
    return np.concatenate([lll, ll]), 0, (i1 + LEAD if i1 else 0), d


# ---- dense blocks behind idle rows -----------------------------------------------------------------------------------------
def padded_dense(Gm, pad, rows_padded=None, pattern=None):
    """the CSR of the symmetric Gm on `pattern` (default: dense) behind `pad` idle rows; the rows of `rows_padded`
    (default: all) store a zero in every idle column"""
    q = Gm.shape[0]
    pattern = pattern or [range(q)] * q
    rows = [{t: _idle(t)} for t in range(pad)]
    for r in range(q):
        rows.append({pad + c: float(Gm[r, c]) for c in pattern[r]})
    for r in (range(q) if rows_padded is None else rows_padded):
        for t in range(pad):
            _sym(rows, pad + r, t, 0.0)
    return S.from_rows(rows)


def tie_entry():
    """the total of (2, 1) is 3 - (2^-26)^2 = 3 - 2^-52, half way between 3 - 2^-51 and 3"""
    e = 2.0 ** -26
    return np.array([[1.0, e, e], [e, 1.0, 3.0], [e, 3.0, 64.0]])


def partial_sums():
    """the total of (3, 2) is 5 - a^2 - 1 with a^2 = 2^-51 + 2^-54: exactly it rounds to 4 - 2^-51, rounded after the first
    product (5 - 2^-50) it is 4 - 2^-50"""
    a = 3 * 2.0 ** -27
    return np.array([[1.0, 0.0, a, a], [0.0, 1.0, 1.0, 1.0], [a, 1.0, 4.0, 5.0], [a, 1.0, 5.0, 64.0]])


DENSE_PADS = (0, 61, 64, 508)
DENSE_NAMES = ("subnormal total", "subnormal radicand", "overflow", "inf", "a tie", "partial sums")
DENSE_STOPPED = ("overflow",)         # ExPOTRF stops at the breakdown, ExSpIC0 goes on: ic0_exact alone decides


@lru_cache(maxsize=None)
def dense_matrix(name):
    """the four small cases of potrf_cases.range_cases() and two of the same size that hold a tie and a partial sum"""
    own = {"a tie": tie_entry, "partial sums": partial_sums}
    return own[name]() if name in own else dict(P.range_cases())[name]


@lru_cache(maxsize=None)
def dense_case(name, pad):
    Gm = dense_matrix(name)
    return SimpleNamespace(name=f"{name} [pad {pad}]", G=Gm, q=Gm.shape[0], pad=pad, csr=padded_dense(Gm, pad))


def dense_model(name, pad, reference=False):
    c = dense_case(name, pad)
    return model_of(("dense", c.name), c.csr, reference)


def root_diagonal():
    """the 512 radicands of potrf_cases.root_values() as a diagonal matrix: no L part"""
    return S.from_rows([{i: float(v)} for i, v in enumerate(P.root_values())])


def sloppy_root(x):
    """a defect the root values must be able to see: the fp32 root refined by one Newton step in fp64"""
    with np.errstate(all="ignore"):
        y = np.float64(np.sqrt(np.float32(x)))
        return float(np.float64(0.5) * (y + np.float64(x) / y))


@lru_cache(maxsize=None)
def long_breakdown(what, owned):
    """a last-but-one row that owns `owned` entries: small integers a_t in the columns of owned - 1 rows with a 1 on the
    diagonal (l_rt = a_t exactly), and a diagonal that makes the radicand exactly 0 ("zero") or -1 ("neg").  Where the
    512-entry limit leaves room, a row behind it carries the broken pivot onwards."""
    r = owned - 1
    rows = [{t: 1.0} for t in range(r)] + [dict()]
    tot = 0
    for t in range(r):
        _sym(rows, r, t, _small(t))
        tot += int(_small(t)) ** 2
    rows[r][r] = float(tot) - {"zero": 0.0, "neg": 1.0}[what]
    if owned + 1 <= C.MAX_ROW:
        rows.append({r + 1: 9.0})
        _sym(rows, r + 1, r, 3.0)
    return SimpleNamespace(name=f"breakdown {what} [{owned}]", csr=S.from_rows(rows), row=r, owned=owned)


# ---- planted ties in long rows ---------------------------------------------------------------------------------------------
# length: the systems (p, pad, seed) run for it.  A length is the number of stored entries of the rows of the FIRST block of
# spic0_cases.planted(p) (9 rows for p = 40, 40 for p = 130); for MAX_ROW the pad is the largest that the second block of
# planted(130) allows: its rows store 512 entries, the first block's 465.  A planted entry lies at position pad + 4 of the
# part its row owns.  Rows of 12 entries hold one block of planted(40) only: two systems (two seeds) give the counts.
PLANTED = {12: ((40, 3, 0), (40, 3, 1)), 64: ((130, 24, 0),), 65: ((130, 25, 0),), 130: ((130, 90, 0),),
           C.MAX_ROW: ((130, 425, 0),)}
# ... and the slots 2 to 5 of the several-entries form, on the small system
PLANTED_MIDDLE = {192: ((40, 183, 0),), 256: ((40, 247, 0),), 320: ((40, 311, 0),), 384: ((40, 375, 0),)}
PLANTED_ALL = {**PLANTED, **PLANTED_MIDDLE}
TAIL = "subnormal radicand"           # the 2 x 2 block behind every planted system


def planted_rows(p):
    """the rows of spic0_cases.planted(p) that lie in a planted block (the rest are 1 x 1 blocks)"""
    return sum(4 + n for n in P.BLOCKS[p])


@lru_cache(maxsize=None)
def planted_base(p, seed=0):
    """spic0_cases.planted(p), or the same make from another seed"""
    if seed == 0:
        return C.planted(p)[0]
    return C.block_pattern(P.planted(p, seed=seed).G, [4 + n for n in P.BLOCKS[p]])


@lru_cache(maxsize=None)
def planted_base_model(p, seed=0):
    return C.ic0_exact(*planted_base(p, seed), detail=True)


@lru_cache(maxsize=None)
def planted(p, pad, seed=0):
    """planted_base(p, seed) behind `pad` idle rows; every row of a planted block stores a zero in every idle column.
    Behind it the 2 x 2 "subnormal radicand" block of potrf_cases.range_cases(), padded in the same way, so that the long
    rows also hold a subnormal total"""
    crow, col, val = planted_base(p, seed)
    m = len(crow) - 1
    rows = [{t: _idle(t)} for t in range(pad)]
    for r in range(m):
        rows.append({int(col[q]) + pad: float(val[q]) for q in range(int(crow[r]), int(crow[r + 1]))})
    Gm = dense_matrix(TAIL)
    for r in range(2):
        rows.append({pad + m + c: float(Gm[r, c]) for c in range(2)})
    for r in list(range(planted_rows(p))) + [m, m + 1]:
        for t in range(pad):
            _sym(rows, pad + r, t, 0.0)
    return S.from_rows(rows)


def planted_model(spec, reference=False):
    return model_of(("planted",) + tuple(spec), planted(*spec), reference)


# ---- small structures ------------------------------------------------------------------------------------------------------
def one_row():
    return S.from_rows([{0: 3.0}])


def diagonal(m=300):
    """nothing is ever fetched: no row has an L part"""
    return S.from_rows([{i: float(i % 9 + 1)} for i in range(m)])


def negative_zero():
    """A stored -0.0 at (1, 0) (and (0, 1)) and at (2, 2), with no product under either.  The exact paths round the exact
    total 0, which is +0.0: l_10 = +0.0 / 2 = +0.0 and l_22 = sqrt(+0.0) = +0.0.  The plain fp64 form of fpe = 1 keeps the
    stored sign: l_10 = -0.0 / 2 = -0.0 and l_22 = sqrt(-0.0) = -0.0.  Both report the radicand of row 2, which is not > 0:
    info[1] = 3.  The two models differ in those sign bits (and in the mirror of l_10) alone."""
    return S.from_rows([{0: 4.0, 1: -0.0}, {0: -0.0, 1: 9.0}, {2: -0.0}])


SMALL = {"one row": one_row, "diagonal": diagonal, "negative zero": negative_zero}
SMALL_INFO = {"one row": 0, "diagonal": 0, "negative zero": 3}


# ---- value sets on one pattern (capture and replay) --------------------------------------------------------------------------
def replay_pattern():
    """support row 0, target 1, carrier 2 (a dense 3 x 3 block) and a band of five rows behind it"""
    rows = [{0: 0.0}, {0: 0.0, 1: 0.0}, {0: 0.0, 1: 0.0, 2: 0.0}] + [{r - 1: 0.0, r: 0.0} for r in range(3, 8)]
    for r in range(8):
        for c in list(rows[r]):
            rows[c][r] = 0.0
    return S.from_rows(rows)[:2]


def replay_sets():
    """[(name, val)] on replay_pattern(), in the order of the replays: healthy, a zero radicand in row 1, healthy again (other
    values), then two range rows with one product: the tie at the overflow threshold and a subnormal total"""
    crow, col = replay_pattern()
    m = len(crow) - 1

    def values(low):
        """low: {(i, j): v} for j <= i"""
        return np.array([low[(max(r, int(c)), min(r, int(c)))] for r in range(m) for c in col[crow[r]:crow[r + 1]]])

    def base(scale, d):
        low = {(r, r): d + r for r in range(m)}
        low.update({(r, r - 1): -scale * (1.0 + r / 16.0) for r in range(1, m)})
        low[(2, 0)] = 0.375 * scale
        return low
    healthy, other = base(1.0, 6.0), base(1.25, 9.5)
    broken = dict(healthy)
    broken[(0, 0)], broken[(1, 0)], broken[(1, 1)] = 1.0, 2.0, 4.0          # the radicand 4 - 2^2
    out = [("healthy", values(healthy)), ("zero radicand", values(broken)), ("healthy again", values(other))]
    for name in ("tie at the overflow threshold", "subnormal total, quotient a tie"):
        c = transplant(next(r for r in R.rows() if r[0] == name))
        (k,) = c.ks
        D = C.dense_of(*c.csr)
        low = dict(healthy)
        low[(0, 0)], low[(1, 0)], low[(1, 1)] = 1.0, D[c.s, k], D[c.s, c.s]
        low[(2, 0)], low[(2, 1)], low[(2, 2)] = D[c.carrier, k], D[c.carrier, c.s], CARRIER_DIAGONAL
        out.append((name, values(low)))
    return out
