"""Cases that hold the batched ExGETRF / ExGETRS / ExPOTRF / ExPOTRS to the ends of the double range.  Nothing here calls
the code under test: every expectation comes from getrf_cases.getrf_exact, potrf_cases.potrf_exact and the Fraction
substitution of exact_cases (trsv_exact, through getrs_model and bjacobi_cases.solve_model; `trsv_ieee` below is the same
substitution, dense, with the rule the two factor models already state for a non-finite operand: it decides the totals it
meets in IEEE arithmetic, 0 * Inf and Inf - Inf being NaN).

The factor cases for ExGETRF transplant a row of exact_cases.range_rows_trsv (T = b - sum_k a_k x_k over the support values
x = 2^511, 2^-537, v, w, 1, 2^-600) into a small matrix, by the trick of getrf_cases.planted and zero_pivot:

    A = [[ Delta, Delta B ],      Delta a diagonal of powers of two with |C_ik| <= Delta_k: no interchange in the first
         [ C,     D       ]]      steps, l = C Delta^-1 and u = Delta B are exact, the trailing totals are D - C B exactly.

form "cand": the row's b is D_00, its entries are row 0 of C, the support values column 0 of B: T is a CANDIDATE of column s.
             Beside it sits one plain candidate: 1 where T is large (T is the pivot, l = 1 / T), the row's own diagonal where
             T is small (T is the non-pivot candidate, l = T / diagonal: what ExTRSV's row gives).
form "U":    the same row against column 1 of B: T is u_{s,s+1}, under the pivot `diagonal` and the multiplier (+0) / diagonal.
Whatever lands on a subnormal, an infinity or a zero is multiplied by zeros alone afterwards (the product domain of the
solves: a product of two non-zero entries is at least 2^-968 in magnitude, or exact); an Inf in U then meets 0 * Inf, so
the last candidate is NaN and info = q: the model decides.  `shift` puts that many empty support columns in front, so that
with the sizes of EMBED the range products meet each of the four slots of the kernel's inner loop.

The six classes a case carries (`cls`): 1 the overflow threshold, 2 the expansion guard at 2^1000, 3 subnormals and the
lower limit 2^-960 of the register certificate, 4 a zero by cancellation of inexact products, 5 a wide-range cancellation
that hangs on an error term, 6 a pivot decision that exact rounding alone gets right."""
import math
from fractions import Fraction
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

import bjacobi_cases as J
import exact_cases as E
import getrf_cases as G
import potrf_cases as P

NPAT = J.NPAT
NSUP = 6                                   # support values of range_rows_trsv
H, LO, V, WC, ONE, SM = range(NSUP)
DMAX = float(np.finfo(np.float64).max)
TINY = 5e-324
_LOW, _HIGH, _DOMAIN = Fraction(1, 2 ** 960), Fraction(2 ** 1020), Fraction(1, 2 ** 968)
# (p, q - base size): the sizes a case is embedded at as the trailing block of blockdiag(dominant(p - q), case); p - q
# covers the four residues mod 4 (asserted in the CPU tests)
EMBED = ((9, 0), (20, 2), (32, 1), (33, 1), (64, 3))
# rows of `rows()` whose scaling by Delta would overflow or lose bits: left out by name
LEFT_OUT = ()


def F(x):
    return Fraction(float(x))


def is_tie(t):
    """the exact total t lies half way between two neighbouring doubles (the overflow threshold counts as out of range)"""
    v = P._round(t)
    if not math.isfinite(v) or Fraction(v) == t:
        return False
    d = t - Fraction(v)
    o = math.nextafter(v, math.inf if d > 0 else -math.inf)
    return math.isfinite(o) and Fraction(o) - t == d


def settles(t):
    """what spmv_round_fast (spmv_common.hip.h) documents as never decided in registers: a tie, or a non-zero total below
    2^-960 or at or above 2^1020 in magnitude"""
    return t != 0 and (abs(t) < _LOW or abs(t) >= _HIGH or is_tie(t))


def in_domain(a, x):
    """the documented product domain: a product of two non-zero entries is at least 2^-968 in magnitude, or exact"""
    if a == 0 or x == 0 or not (math.isfinite(a) and math.isfinite(x)):
        return True
    return abs(F(a) * F(x)) >= _DOMAIN or Fraction(float(np.float64(a) * np.float64(x))) == F(a) * F(x)


# ---- the rows --------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def support():
    r = E.range_rows_trsv(0)
    return tuple(float(x) for x in r.b[:NSUP])


@lru_cache(maxsize=None)
def rows():
    """(name, class, b, diagonal, {support column: entry}): the rows of range_rows_trsv and a few of the same make"""
    r = E.range_rows_trsv(0)
    sup = support()
    v, w = sup[V], sup[WC]
    cls = {"overflow": 1, "1000": 2, "subnormal": 3, "zero": 4}
    out = []
    for name in r.names:
        i = r.rows[name]
        c = next(k for key, k in cls.items() if key in name)
        out.append((name, c, float(r.b[i]), float(r.L[i, i]), {k: float(r.L[i, k]) for k in range(NSUP) if r.L[i, k] != 0}))
    fl = v * w
    out += [
        # 2^-960 (1 - 2^-53), the double below the limit: exact, and still never decided in registers
        ("total just below 2^-960", 3, 2.0 ** -960, 3.0, {ONE: 2.0 ** -1013}),
        # 2^-960 (1 + 2^-52), the double above it: exact and inside the certificate's range
        ("total just above 2^-960", 3, 2.0 ** -960, -3.0, {ONE: -2.0 ** -1012}),
        # v w against fl(v w) 1: the two largest of six products differ by the error term of v w, about 2^-53, over
        # terms at 2^-100, 2^-200, 2^-250 (b), 2^-300 and 2^-400: no four-term expansion holds them
        ("wide-range cancellation", 5, 2.0 ** -250, 5.0,
         {V: w, ONE: -fl, H: 2.0 ** -611, LO: 2.0 ** 237, WC: math.ldexp(v, -200), SM: 2.0 ** 200}),
    ]
    return tuple(out)


def row_total(row):
    name, c, b, dia, ent = row
    sup = support()
    return F(b) - sum((F(a) * F(sup[k]) for k, a in ent.items()), Fraction(0))


def _delta(a):
    """the smallest power of two that is at least |a|"""
    m, e = math.frexp(abs(a))
    return math.ldexp(1.0, e - 1 if m == 0.5 else e)


def _case(name, cls, form, A, at, want=None, **kw):
    return SimpleNamespace(name=f"{name} [{form}]", row=name, cls=cls, form=form, A=A, at=at, want=want, **kw)


def transplant(row, form, shift=0):
    """the (NSUP + shift + 2)-square matrix that carries `row` as a candidate ("cand") or in the row of U ("U"); None if the
    scaling by Delta would overflow or lose bits"""
    name, cls, b, dia, ent = row
    sup = support()
    s = NSUP + shift
    q = s + 2
    A = np.zeros((q, q))
    A[:s, :s] = np.eye(s)
    col = s if form == "cand" else s + 1
    for k, a in ent.items():
        d = _delta(a)
        u = d * sup[k]
        if not math.isfinite(u) or Fraction(u) != F(d) * F(sup[k]) or Fraction(a / d) * F(d) != F(a):
            return None
        A[shift + k, shift + k], A[shift + k, col], A[s, shift + k] = d, u, a
    t = row_total(row)
    c = P._round(t)
    if form == "cand":
        A[s, s] = b
        if abs(c) > abs(dia):            # T is the pivot: l = 1 / T, which then meets a zero of U
            assert abs(c) >= 1.0
            A[s + 1, s], A[s, s + 1], A[s + 1, s + 1] = 1.0, 0.0, 1.0
            return _case(name, cls, form, A, (s, s), c, l=float(np.float64(1.0) / np.float64(c)), pivot=True, total=t, shift=shift)
        assert abs(c) < abs(dia)         # the diagonal is the pivot (rows swapped): l = T / diagonal
        A[s + 1, s], A[s, s + 1], A[s + 1, s + 1] = dia, 1.0, 0.0
        with np.errstate(all="ignore"):
            l = float(np.float64(c) / np.float64(dia))
        return _case(name, cls, form, A, (s + 1, s), l, l=l, pivot=False, total=t, shift=shift)
    A[s, s], A[s, s + 1], A[s + 1, s], A[s + 1, s + 1] = dia, b, 0.0, 1.0
    return _case(name, cls, form, A, (s, s + 1), c, l=math.copysign(0.0, dia), pivot=None, total=t, shift=shift)


def rounding_decides(form, shift=0):
    """Class 6.  Row X has the total beta - v w + fl(v w) 1 = beta - e (e the error term of v w), beta a power of two a few
    bits above |e|: plain fp64 gives beta exactly, the exact total rounds to another double.  Row Y holds beta itself.  In
    plain arithmetic the two candidates tie and the first index wins; exactly rounded the larger one wins.  The rows are
    ordered so that the two answers differ.  form "U": the same total in the row of U (a U entry takes no part in a pivot
    search: there the class is the total alone)."""
    sup = support()
    v, w = sup[V], sup[WC]
    fl = v * w
    e = F(v) * F(w) - F(fl)
    assert e != 0
    beta = math.ldexp(1.0, math.frexp(float(abs(e)))[1] + 8)
    row = ("rounding decides the pivot", 6, beta, beta, {V: w, ONE: -fl})
    t = row_total(row)
    c = P._round(t)
    assert t == F(beta) - e and c != beta and float(np.float64(beta) - np.float64(w) * np.float64(v) + np.float64(fl)) == beta
    if form == "U":
        return transplant(("rounding decides the pivot", 6, beta, 1.0, row[4]), "U", shift)
    s = NSUP + shift
    q = s + 2
    A = np.zeros((q, q))
    A[:s, :s] = np.eye(s)
    x_first = abs(c) < beta              # exactly, Y (second) wins; plainly the tie goes to X (first)
    rx, ry = (s, s + 1) if x_first else (s + 1, s)
    for k, a in row[4].items():
        d = _delta(a)
        A[shift + k, shift + k], A[shift + k, s], A[rx, shift + k] = d, d * sup[k], a
    A[rx, s], A[ry, s] = beta, beta
    A[rx, s + 1], A[ry, s + 1] = 0.5, 0.25
    return _case(row[0], 6, "cand", A, (s + 1, s), None, pivot=None, total=t, shift=shift, exact_pivot=s + 2, plain_pivot=s + 1)


def hand_made():
    """the small matrices that need no support: an overflow tie and its neighbour in two and three rows, a subnormal total in
    U and, transposed, a subnormal candidate whose quotient rounds among the subnormals, and a pivot chosen among subnormal
    candidates"""
    x, y = (1 + 2.0 ** -52) * 2.0 ** -484, (1 + 2.0 ** -51) * 2.0 ** -484
    M = np.array([[1.0, x, y], [x, 3.0, x * y], [0.0, 0.0, 1.0]])
    return (
        _case("2 x 2 overflow tie", 1, "cand", np.array([[1.0, 2.0 ** 1022], [-2.0 ** -52, DMAX]]), (1, 1), math.inf),
        _case("3 x 3 below the overflow tie", 1, "cand",
              np.array([[1.0, 0.0, 2.0 ** 1022], [0.0, 1.0, 2.0 ** -537], [-2.0 ** -52, 2.0 ** -537, DMAX]]), (2, 2), DMAX),
        _case("3 x 3 subnormal total", 3, "U", M, (1, 2), -2.0 ** -1071),
        _case("3 x 3 subnormal candidate and quotient", 3, "cand", np.ascontiguousarray(M.T), (2, 1), -3 * 2.0 ** -1074),
        _case("2 x 2 pivot among subnormal candidates", 3, "cand", np.array([[3 * TINY, 1.0], [-4 * TINY, 1.0]]), (1, 0), -0.75),
    )


@lru_cache(maxsize=None)
def getrf_cases(shift=0):
    """every factor case for ExGETRF with `shift` empty support columns in front (the hand-made ones have none)"""
    out, left = [], []
    for row in rows():
        for form in ("cand", "U"):
            c = transplant(row, form, shift)
            if c is None:
                left.append(row[0])
            else:
                out.append(c)
    assert tuple(sorted(set(left))) == tuple(sorted(LEFT_OUT)), left
    out += [rounding_decides("cand", shift), rounding_decides("U", shift)]
    out += list(hand_made())
    return tuple(out)


# ---- models of the factor cases --------------------------------------------------------------------------------------
def lu_totals(A, W, ipiv, info):
    """{(i, j): the exact total behind entry (i, j) of W}, from the identity P A = L U on the doubles of W: the candidate of
    the row that ends at i for j < i, u_ij for j >= i.  Entries with a non-finite operand are left out; a breakdown is
    taken at the last step only."""
    p = A.shape[0]
    assert info in (0, p)
    PA = np.array(A, dtype=np.float64, copy=True)
    for j in range(p):
        pv = int(ipiv[j]) - 1
        if pv != j:
            PA[[j, pv]] = PA[[pv, j]]
    fin = np.isfinite(W) & np.isfinite(PA)
    Wf = [[F(W[i, j]) if fin[i, j] else None for j in range(p)] for i in range(p)]
    out = {}
    for i in range(p):
        for j in range(p):
            m = min(i, j)
            if not (np.isfinite(PA[i, j]) and fin[i, :m].all() and fin[:m, j].all()):
                continue
            out[i, j] = F(PA[i, j]) - sum((Wf[i][k] * Wf[k][j] for k in range(m) if Wf[i][k] and Wf[k][j]), Fraction(0))
    return out


def chol_totals(Gm, R, info):
    """{(j, i): the exact total behind the fixed entry (j, i), j <= i, of the upper factor R}; entries with a non-finite
    operand are left out"""
    p = Gm.shape[0]
    last = p if info == 0 else info - 1
    fin = np.isfinite(R)
    out = {}
    for j in range(min(last + 1, p)):
        for i in range(j, p if j < last else j + 1):
            if not (math.isfinite(Gm[j, i]) and fin[:j, j].all() and fin[:j, i].all()):
                continue
            out[j, i] = F(Gm[j, i]) - sum((F(R[k, j]) * F(R[k, i]) for k in range(j) if R[k, j] and R[k, i]), Fraction(0))
    return out


def lu_entry(name, A, case=None):
    """getrf_cases._entry with `settle`: the least number of outputs the accumulator must have rounded"""
    e = G._entry(name, A)
    tot = lu_totals(A, e.W, e.ipiv, e.info)
    e.settle = sum(1 for t in tot.values() if settles(t))
    e.totals, e.case = tot, case
    return e


def chol_entry(name, Gm):
    R, info, d = P.potrf_exact(Gm, "U", detail=True)
    tot = chol_totals(Gm, R, info)
    e = J._entry(name, Gm, R, info, int((d.kind == P.TIE).sum()))
    e.settle, e.totals = sum(1 for t in tot.values() if settles(t)), tot
    return e


@lru_cache(maxsize=None)
def _dominant_entry(d):
    e = G._entry(f"dominant({d})", G.dominant(d, 8))
    assert e.info == 0
    return e


def _compose(dom, e, name):
    """the entry of blockdiag(dom.A, e.A), composed from the two factorisations: the off-diagonal blocks hold zeros, so no
    candidate of a leading column lies in a trailing row, and the multipliers there are (+0) / u_jj"""
    d, q = dom.A.shape[0], e.A.shape[0]
    p = d + q
    A, W = np.zeros((p, p)), np.zeros((p, p))
    A[:d, :d], A[d:, d:] = dom.A, e.A
    W[:d, :d], W[d:, d:] = dom.W, e.W
    W[d:, :d] = np.float64(0.0) / np.diag(dom.W)[None, :]
    info = e.info + d if e.info else 0
    return SimpleNamespace(name=name, A=A, W=W, ipiv=np.concatenate([dom.ipiv, e.ipiv + d]).astype(np.int32), info=info,
                           ties=dom.ties + e.ties, settle=dom.ties + e.settle, roundings=G.roundings(p, info), case=e.case,
                           totals=e.totals, parts=(dom, e))


def embed_lu(e, p):
    """the entry of blockdiag(dominant(p - q), case)"""
    d = p - e.A.shape[0]
    return _compose(_dominant_entry(d), e, f"{e.name} @{d}") if d else e


@lru_cache(maxsize=None)
def getrf_entries(shift=0):
    return tuple(lu_entry(c.name, c.A, c) for c in getrf_cases(shift))


@lru_cache(maxsize=None)
def getrf_at(p):
    """every ExGETRF case at size p: alone where p is the size of the case, else embedded behind dominant(p - q)"""
    if p == NSUP + 2:
        return tuple(e for e in getrf_entries(0))
    shift = dict(EMBED)[p]
    return tuple(embed_lu(e, p) for e in getrf_entries(shift))


@lru_cache(maxsize=None)
def _dominant_shuffled(d):
    dom = _dominant_entry(d)
    e = G._entry(dom.name + ", shuffled", G.shuffled(dom.A, 7))
    assert e.info == 0 and G.J_same(e.W, dom.W) and e.ties == dom.ties
    return e


def _shuffled_small(e):
    S = G.shuffled(e.A, 7)
    W, ipiv, info = G.getrf_exact(S)
    if info != e.info or not G.J_same(W, e.W):
        return None
    return SimpleNamespace(name=e.name + ", shuffled", A=S, W=W, ipiv=ipiv, info=info, ties=e.ties, settle=e.settle,
                           roundings=e.roundings, case=e.case, totals=e.totals)


def shuffled_entry(e):
    """the row-shuffled copy of an entry (an embedded one: the rows of either diagonal block among themselves), or None
    where the model says that the factors do not survive the shuffle"""
    if not hasattr(e, "parts"):
        return _shuffled_small(e)
    dom, small = e.parts
    s = _shuffled_small(small)
    return None if s is None else _compose(_dominant_shuffled(dom.A.shape[0]), s, e.name + ", shuffled")


# ---- ExPOTRF ---------------------------------------------------------------------------------------------------------
def root_diagonal(p, which):
    """a diagonal matrix of p of potrf_cases.root_values(): 0 neighbours of perfect squares, 1 those and the squares, 2 the
    window that ends with 2^-1074, DBL_MAX, 2^-1022 and its predecessor"""
    v = P.root_values()
    lo = (0, 110, 164 - p)[which]
    return np.diag(v[lo:lo + p])


@lru_cache(maxsize=None)
def potrf_at(p):
    """the entries for the batched ExPOTRF at size p: the range cases of potrf_cases (q = 2, 3, 4) alone (p = q) or as the
    trailing block behind a leading part of a random Gram matrix, and for p >= 4 the three diagonals of roots"""
    out = []
    for name, Gc in P.range_cases():
        q = Gc.shape[0]
        if "@" in name or q > p or (p <= 4 and q != p):
            continue
        e = chol_entry(name, Gc)
        d = p - q
        if d:
            Gg, Rg, kind = J.gram64(1)
            Gm, R = np.zeros((p, p)), np.zeros((p, p))
            Gm[:d, :d], Gm[d:, d:] = Gg[:d, :d], Gc
            R[:d, :d], R[d:, d:] = Rg[:d, :d], e.R
            lead = int((kind[:d, :d] == P.TIE).sum())
            f = J._entry(f"{name} @{d}", Gm, R, e.info + d if e.info else 0, lead + e.ties)
            f.settle, f.totals = lead + e.settle, e.totals
            e = f
        out.append(e)
    if p >= 4:
        out += [chol_entry(f"roots {w}", root_diagonal(p, w)) for w in (0, 1, 2)]
    return tuple(out)


# ---- the apply side --------------------------------------------------------------------------------------------------
def trsv_ieee(L, b, unit=False):
    """exact_cases.trsv_exact, dense: a row whose b, entries or earlier x are all finite has the exact total (zero products
    skipped) rounded once; a non-finite operand decides the total in IEEE arithmetic (0 * Inf and Inf - Inf are NaN), as
    in getrf_exact and potrf_exact.  Returns (x, totals), a total being None where IEEE arithmetic decided."""
    L, b = np.asarray(L, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = len(b)
    x, totals, xf = np.zeros(n), [None] * n, [None] * n
    with np.errstate(all="ignore"):
        for i in range(n):
            bad = [j for j in range(i) if not (math.isfinite(L[i, j]) and math.isfinite(x[j]))]
            if bad or not math.isfinite(b[i]):
                special = ([] if math.isfinite(b[i]) else [float(b[i])]) + [-float(np.float64(L[i, j]) * np.float64(x[j])) for j in bad]
                r = float(np.sum(np.array(special)))
            else:
                T = F(b[i])
                for j in np.nonzero(L[i, :i])[0].tolist():
                    if x[j] != 0:
                        if xf[j] is None:
                            xf[j] = F(x[j])
                        T -= F(L[i, j]) * xf[j]
                totals[i] = T
                r = P._round(T)
            x[i] = r if unit else float(np.float64(r) / np.float64(L[i, i]))
    return x, totals


def _neutral(L, b, i):
    L[i, :i], L[i, i], b[i] = 0.0, 1.0, 1.0


def _outside(L, b):
    """the rows of the system that multiply two non-zero doubles outside the product domain"""
    x, _ = trsv_ieee(L, b)
    return [i for i in range(len(b)) if not all(in_domain(L[i, j], x[j]) for j in range(i))]


VARIANTS = ("full", "safe", "half")


@lru_cache(maxsize=None)
def range_block(lead, variant):
    """(L, B): range_rows_trsv(lead) as a lower system in substitution order with NPAT right-hand sides.
      full: column 0 is b, with the row that overflows (the last: nothing consumes it within a sweep); columns 1 .. 4 are
            -b, b, -b, b with 1 in that row's place, so that its total stays finite;
      safe: the overflowing row made a row of the identity; b, -b, b, -b, b;
      half: b / 2, -b / 2, ...: every total halves (the overflow tie becomes a tie at 2^1023); the rows whose products
            would leave the product domain (a product below 2^-968 that is no longer exact) made rows of the identity."""
    r = E.range_rows_trsv(lead)
    L, b = r.L.copy(), r.b.copy()
    n = r.n
    sign = np.array([1.0, -1.0, 1.0, -1.0, 1.0])
    dropped = []
    if variant == "safe":
        _neutral(L, b, n - 1)
        dropped = [n - 1]
    if variant == "half":
        b = b / 2
        assert (b * 2 == r.b).all()
        while True:
            out = _outside(L, b)
            if not out:
                break
            for i in out:
                _neutral(L, b, i)
                dropped.append(i)
    B = np.outer(b, sign)
    if variant == "full":
        B[n - 1, 1:] = sign[1:]
    names = {i: nm for nm, i in r.rows.items()}
    assert not _outside(L, B[:, 0]) and not _outside(L, B[:, 1])
    return SimpleNamespace(L=L, B=B, n=n, lead=lead, rows=r.rows, dropped=tuple(names[i] for i in dropped), want=r.want)


def _count(totals):
    return sum(1 for t in totals if t is not None and settles(t))


# ExPOTRS: an entry is (name, sys): sys(rows) gives the lower system (L, B) of a block of `rows` rows in substitution order.
# Sweep '1' stores F = L^T; sweep '2' stores the index reversal F = L[::-1, ::-1] and meets B reversed.
def _prefix(L, B):
    return lambda rows: (L[:rows, :rows], B[:rows])


@lru_cache(maxsize=None)
def potrs_seven(p, sweep, turn=0):
    """healthy, range, planted, range, healthy, range, NaN for a sweep ('1' or '2'); p = lead + 18.  `turn` rotates the three
    variants of the range block through the three places."""
    lead = p - (NSUP + 12)
    base = J.solve_seven(p, sweep)

    def healthy(blk):
        if sweep == "1":
            return lambda rows: (np.ascontiguousarray(blk.F[:rows, :rows].T), blk.B[:rows])
        return lambda rows: (np.ascontiguousarray(blk.F[:rows, :rows][::-1, ::-1]), blk.B[:rows][::-1])

    def rng(variant):
        c = range_block(lead, variant)
        return SimpleNamespace(name=f"range {variant}", key=("range", lead, variant), sys=_prefix(c.L, c.B))
    nanL = np.full((p, p), np.nan)
    plant = base[5] if sweep == "1" else base[6]
    v = [VARIANTS[(t + turn) % 3] for t in range(3)]
    return (SimpleNamespace(name="healthy 0", key=("healthy", p, sweep, 0), sys=healthy(base[0])), rng(v[0]),
            SimpleNamespace(name="planted", key=("planted", p, sweep), sys=healthy(plant)), rng(v[1]),
            SimpleNamespace(name="healthy 1", key=("healthy", p, sweep, 1), sys=healthy(base[1])), rng(v[2]),
            SimpleNamespace(name="nan", key=("nan", p), sys=_prefix(nanL, base[2].B)))


_MODELS = {}


def _solve(entry, rows, unit=False):
    """(X [rows, NPAT] in substitution order, settle [NPAT]) of an entry's system, cached"""
    key = (entry.key, rows, unit)
    if key not in _MODELS:
        L, B = entry.sys(rows)
        X, st = np.zeros((rows, NPAT)), np.zeros(NPAT, dtype=np.int64)
        for c in range(NPAT):
            X[:, c], tot = trsv_ieee(L, B[:, c], unit)
            st[c] = _count(tot)
        _MODELS[key] = (X, st)
    return _MODELS[key]


def potrs_case(entries, p, n, k, sweep, uplo):
    """block b is entries[b % len(entries)], column j its pattern j % NPAT: (factors [nb, p, p] for `uplo` with NaN wherever
    nothing must be read, X0, the expected X, the least number of settled roundings)"""
    nb = -(-n // p)
    cols = np.arange(k) % NPAT
    mask = J.tri_mask(p, uplo)
    full = np.full((nb, p, p), np.nan)
    X0, want, settle = np.zeros((n, k)), np.zeros((n, k)), 0
    for b in range(nb):
        rows = min(p, n - b * p)
        e = entries[b % len(entries)]
        L, B = e.sys(rows)
        X, st = _solve(e, rows)
        Fu = L.T if sweep == "1" else L[::-1, ::-1]
        M = np.full((p, p), np.nan)
        M[:rows, :rows] = Fu if uplo == "U" else Fu.T
        full[b][mask] = M[mask]
        rev = slice(None) if sweep == "1" else slice(None, None, -1)
        X0[b * p:b * p + rows] = B[rev][:, cols]
        want[b * p:b * p + rows] = X[rev][:, cols]
        settle += int(st[cols].sum())
    return full, X0, want, settle


# ExGETRS: an entry is (name, lu): lu(rows) gives (LU [rows, rows], ipiv [rows], B [rows, NPAT]) of a block of `rows` rows.
def getrs_ieee(LU, ipiv, b):
    """getrf_cases.getrs_model with trsv_ieee in the place of trsv_exact: (x, the totals of both sweeps)"""
    rows = len(b)
    x = np.array(b, dtype=np.float64, copy=True)
    for j in range(rows):
        pv = int(ipiv[j]) - 1
        if 0 <= pv < rows and pv != j:
            x[j], x[pv] = x[pv], x[j]
    LU = np.asarray(LU, dtype=np.float64)[:rows, :rows]
    y, t1 = trsv_ieee(np.tril(LU, -1) + np.eye(rows), x, unit=True)
    zr, t2 = trsv_ieee(np.ascontiguousarray(np.triu(LU)[::-1, ::-1]), y[::-1])
    return zr[::-1].copy(), list(t1) + list(t2)


def unswap(ipiv, B):
    """the right-hand sides that the interchanges of ipiv turn into B"""
    X = np.array(B, copy=True)
    for j in range(len(ipiv) - 1, -1, -1):
        pv = int(ipiv[j]) - 1
        if pv != j:
            X[[j, pv]] = X[[pv, j]]
    return X


def pair_pivots(p):
    """rows 2m and 2m + 1 change places: a cut at an even row keeps every interchange inside the block"""
    ip = np.arange(1, p + 1, dtype=np.int32)
    ip[0:p - 1:2] += 1
    return ip


def random_pivots(p, seed):
    rng = np.random.default_rng([p, seed, 96])
    return np.array([int(rng.integers(j, p)) + 1 for j in range(p)], dtype=np.int32)


@lru_cache(maxsize=None)
def getrs_range(lead, variant, direction):
    """the range block as a factored block.  forward: L is its strictly lower part under a unit diagonal, U a diagonal of
    small odd integers of both signs, the rows interchanged in pairs and the right-hand sides permuted so that the
    interchanges restore them.  backward: U is the reversed system, L = I, no interchange; a short block is the reversal of
    the leading part of the system."""
    c = range_block(lead, variant)
    n = c.n
    if direction == "forward":
        dia = np.array([(3.0, -5.0, 7.0, -9.0, 11.0)[i % 5] for i in range(n)])
        LU = np.tril(c.L, -1) + np.diag(dia)
        ip = pair_pivots(n)
        X0 = unswap(ip, c.B)
        lu = lambda rows: (LU[:rows, :rows], ip[:rows], X0[:rows])
    else:
        ident = np.arange(1, n + 1, dtype=np.int32)
        lu = lambda rows: (np.ascontiguousarray(c.L[:rows, :rows][::-1, ::-1]), ident[:rows], c.B[:rows][::-1])
    return SimpleNamespace(name=f"range {variant} {direction}", key=("range", lead, variant, direction), lu=lu, block=c)


@lru_cache(maxsize=None)
def getrs_planted(p, part):
    """the leading p rows of a planted ExTRSV system as the L part (its unit variant; U = I) or, reversed, as the U part
    (L = I) of a block, under random interchanges that the permuted right-hand sides undo; column j is b 2^j"""
    unit = part == "L"
    c = E.planted_trsv_case(40, 40, 20, False, unit) if p <= 40 else E.planted_trsv_case(64, 400, 53, False, unit)
    L, b = c.L[:p, :p], c.b[:p]
    scale = 2.0 ** np.arange(NPAT)
    ip = random_pivots(p, 3 if unit else 4)
    if unit:
        LU, B = np.tril(L, -1) + np.eye(p), np.outer(b, scale)
    else:
        LU, B = np.ascontiguousarray(L[::-1, ::-1]), np.outer(b[::-1], scale)
    X0 = unswap(ip, B)
    return SimpleNamespace(name=f"planted {part}", key=("planted", p, part), lu=lambda rows: (LU[:rows, :rows], ip[:rows], X0[:rows]),
                           case=c)


@lru_cache(maxsize=None)
def getrs_seven(p, turn=0):
    """healthy, range, planted, range, healthy, range, NaN; p = lead + 18.  `turn` rotates the six range blocks (three variants,
    two directions) and the two planted parts through their places."""
    lead = p - (NSUP + 12)
    base = G.solve_seven(p)

    def healthy(s):
        blk = base[s]
        return SimpleNamespace(name=f"healthy {s}", key=("healthy", p, s), lu=lambda rows: (blk.LU[:rows, :rows], blk.ipiv[:rows], blk.B[:rows]))
    six = [(v, d) for d in ("forward", "backward") for v in VARIANTS]
    pick = [six[(2 * t + turn) % 6] for t in range(3)]
    nan = SimpleNamespace(name="nan", key=("nan", p), lu=lambda rows: (np.full((rows, rows), np.nan), np.arange(1, rows + 1, dtype=np.int32),
                                                                      base[2].B[:rows]))
    return (healthy(0), getrs_range(lead, *pick[0]), getrs_planted(p, "LU"[turn % 2]), getrs_range(lead, *pick[1]), healthy(1),
            getrs_range(lead, *pick[2]), nan)


def _getrs_solve(entry, rows):
    key = (entry.key, rows, "getrs")
    if key not in _MODELS:
        LU, ip, B = entry.lu(rows)
        X, st = np.zeros((rows, NPAT)), np.zeros(NPAT, dtype=np.int64)
        for c in range(NPAT):
            X[:, c], tot = getrs_ieee(LU, ip, B[:, c])
            st[c] = _count(tot)
        _MODELS[key] = (X, st)
    return _MODELS[key]


def getrs_case(entries, p, n, k):
    """(LU [nb, p, p], ipiv [nb, p], X0, the expected X, the least number of settled roundings): block b is
    entries[b % len(entries)], column j its pattern j % NPAT; the unused part of a short last block is NaN, its pivots
    garbage"""
    nb = -(-n // p)
    cols = np.arange(k) % NPAT
    LU, ipiv = np.full((nb, p, p), np.nan), np.zeros((nb, p), dtype=np.int32)
    X0, want, settle = np.zeros((n, k)), np.zeros((n, k)), 0
    for b in range(nb):
        rows = min(p, n - b * p)
        e = entries[b % len(entries)]
        lu, ip, B = e.lu(rows)
        X, st = _getrs_solve(e, rows)
        LU[b, :rows, :rows] = lu
        ipiv[b, :rows] = ip
        ipiv[b, rows:] = -(2 ** 31) + 5
        X0[b * p:b * p + rows] = B[:, cols]
        want[b * p:b * p + rows] = X[:, cols]
        settle += int(st[cols].sum())
    return LU, ipiv, X0, want, settle
