"""The cases of tests/blas1_cases.py dealt over R ranks (or over the parts of a host-pointer call) adversarially.

Nothing here touches the GPU, the library or the oracle.  A case is cut into R shards whose concatenation has the same
exact total: total, expected double, digits and canonical limbs are those of the case.  What changes is what every rank
exports before the merge (exblas_amd/csrc/comm.hip; host_reduce in capi.hip): partial totals that are negative under a
positive total (a signed top digit over a run of 0xffffffff digits), beyond 2^1024 under a finite total, a deciding
half or sticky unit alone on a rank, LOW / HIGH extension sets that are non-zero on some ranks and cancel in the sum.

Partitions (all deterministic in the case index):
  contiguous   the terms in order, cut like exblas_shard_range
  round_robin  term i on rank i % R
  by_sign      positive terms on the lowest ranks, negative ones on the highest
  one_rank     all terms on rank index % R, every other shard empty
  last_alone   the last term on the last rank, the rest on rank 0 (in families A and F the last term is the half,
               quarter, +-1-unit or sub-unit part)
Ballast: k copies of +G on rank a and k copies of -G on rank b != a; the total does not change.
  ("main", s, k)  G = term(2^53 - 1, s), s in {0, 1000, 2044}: 53 ones at the bottom, in the middle, at the top (DBL_MAX / 2);
                  for ExDOT
                  the pair (+-G, 1.0).  With s = 2044 and k = 3 a rank's partial total passes 2^1024.
  ("low", k)      ExDOT (+-m 2^-537, 2^-538), m a full 53-bit odd mantissa in [1, 2): products below 2^-968
  ("high", k)     ExDOT (+-2^600, m 2^500): products beyond 2^1024
Every constructor asserts, in integer / Fraction arithmetic, that the multiset of the case's terms plus ballast equals
the union of the shards, that the per-rank totals add up to the total, and that the ballast sums to 0.
"""
import collections
import functools
import math
from fractions import Fraction

import numpy as np

import blas1_cases as B
from helpers import FPE_VARIANTS_DOT, FPE_VARIANTS_SUM

PARTITIONS = ("contiguous", "round_robin", "by_sign", "one_rank", "last_alone")
BIG_PARTITIONS = ("contiguous", "by_sign")       # for the D cases with 32768 terms and more
BIG_TERMS = 32768
BALLAST_S = (0, 1000, 2044)
BALLAST_K = (1, 3)
SUM_BALLAST = (None,) + tuple(("main", s, k) for s in BALLAST_S for k in BALLAST_K)
DOT_BALLAST = SUM_BALLAST + tuple((w, k) for w in ("low", "high") for k in BALLAST_K)
M_ODD = float.fromhex("0x1.b7e151628aed3p+0")   # 53 bits, odd, in [1, 2)
LOW_LIMIT = Fraction(1, 1 << 968)                # a product of non-zero operands below this goes to the LOW accumulator
HIGH_LIMIT = 1 << 1024                           # a product of finite operands from here on goes to the HIGH accumulator
assert 1.0 <= M_ODD < 2.0 and (B.units(M_ODD) >> 1022) & 1 == 1 and B.units(M_ODD).bit_length() == 1075


@functools.lru_cache(maxsize=None)
def _u(x):
    return B.units(x)


def shard_range(n, rank, world):
    """exblas_shard_range: even cuts"""
    def cut(r):
        return n if r >= world else ((n * r) // world) & ~1
    return cut(rank), cut(rank + 1)


class Shards:
    """one case dealt over R ranks.  a (and b for ExDOT): R float64 arrays; T: the exact total in units of 2^-1074 (an int
    for ExSUM, a Fraction for ExDOT); T_r: the per-rank totals; want / flags: the expected double and flag word;
    low_r / high_r: per rank, the exact sum (Fraction, in units) of the products below 2^-968 / from 2^1024 on, None
    where the rank holds no such product; last_alone: the rank of the case's last term holds nothing else"""
    __slots__ = ("case", "index", "R", "partition", "ballast", "a", "b", "T", "T_r", "want", "flags", "low_r", "high_r",
                 "last_alone", "name")

    def __repr__(self):
        return f"<{self.name or self.case!r} #{self.index} R={self.R} {self.partition} ballast={self.ballast}>"

    @property
    def is_dot(self):
        return self.b is not None

    def digits_r(self):
        """[R, 68]: every rank's expected exported main digit set (ExSUM)"""
        assert not self.is_dot
        return B.digits_matrix(self.T_r)

    def concatenated(self):
        a = np.concatenate(self.a)
        return (a, np.concatenate(self.b)) if self.is_dot else a


def _value(item):
    """the exact value of a term or a product, in units of 2^-1074 (int for a term, Fraction for a product)"""
    x, y = item
    return _u(x) if y is None else Fraction(x) * Fraction(y) * B.ONE


def _deal(items, R, partition, index):
    """-> R lists of item positions"""
    n = len(items)
    if partition == "contiguous":
        return [list(range(*shard_range(n, r, R))) for r in range(R)]
    if partition == "round_robin":
        return [list(range(r, n, R)) for r in range(R)]
    if partition == "one_rank":
        return [list(range(n)) if r == index % R else [] for r in range(R)]
    if partition == "last_alone":
        if R == 1:
            return [list(range(n))]
        return [list(range(n - 1))] + [[] for _ in range(R - 2)] + [[n - 1] if n else []]
    assert partition == "by_sign"
    pos = [i for i, it in enumerate(items) if math.copysign(1.0, it[0]) * (1.0 if it[1] is None else math.copysign(1.0, it[1])) > 0]
    in_pos = set(pos)
    neg = [i for i in range(n) if i not in in_pos]
    if R == 1:
        return [pos + neg]
    lo_ranks = (R + 1) // 2                       # ranks [0, lo_ranks) hold the positive terms, the others the negative ones
    out = [pos[slice(*shard_range(len(pos), r, lo_ranks))] for r in range(lo_ranks)]
    out += [neg[slice(*shard_range(len(neg), r, R - lo_ranks))] for r in range(R - lo_ranks)]
    return out


def ballast_items(ballast, dot):
    """-> (k, the +G item, the -G item)"""
    if ballast is None:
        return 0, None, None
    if ballast[0] == "main":
        _, s, k = ballast
        g = B.term((1 << 53) - 1, s)
        return k, (g, 1.0 if dot else None), (-g, 1.0 if dot else None)
    assert dot
    which, k = ballast
    if which == "low":
        return k, (math.ldexp(M_ODD, -537), math.ldexp(1.0, -538)), (-math.ldexp(M_ODD, -537), math.ldexp(1.0, -538))
    return k, (math.ldexp(1.0, 600), math.ldexp(M_ODD, 500)), (-math.ldexp(1.0, 600), math.ldexp(M_ODD, 500))


def ballast_ranks(index, R):
    a = index % R
    return (a, (a + 1 + (index // R) % (R - 1)) % R) if R > 1 else (0, 0)


def _finish(sh, items, shards, ball):
    """fill the arrays and the per-rank exact figures of `sh`, and hold the construction to its claims"""
    dot = sh.b is not None
    assert collections.Counter(items) + collections.Counter(ball) == collections.Counter(it for s in shards for it in s)
    assert sum((_value(it) for it in ball), 0) == 0, "the ballast does not cancel"
    sh.a = [np.array([it[0] for it in s], dtype=np.float64) for s in shards]
    sh.T_r = [sum((_value(it) for it in s), 0) for s in shards]
    assert sum(sh.T_r, 0) == sh.T, "the per-rank totals do not add up to the total"
    sh.low_r, sh.high_r = [None] * sh.R, [None] * sh.R
    if dot:
        sh.b = [np.array([it[1] for it in s], dtype=np.float64) for s in shards]
        for r, s in enumerate(shards):
            vals = [_value(it) for it in s]
            low = [v for v in vals if 0 < abs(v) < LOW_LIMIT * B.ONE]
            high = [v for v in vals if abs(v) >= HIGH_LIMIT * B.ONE]
            sh.low_r[r] = sum(low, Fraction(0)) if low else None
            sh.high_r[r] = sum(high, Fraction(0)) if high else None
    return sh


def deal(case, index, R, partition, ballast=None):
    """`case` (of blas1_cases families A - D, or F) over R ranks"""
    dot = case.a is not None
    items = [(float(x), float(y)) for x, y in zip(case.a, case.b)] if dot else [(x, None) for x in case.terms]
    sh = Shards()
    for s in Shards.__slots__:
        setattr(sh, s, None)
    sh.case, sh.index, sh.R, sh.partition, sh.ballast = case, index, R, partition, ballast
    sh.T = case.exact * B.ONE if dot else case.T
    sh.want = case.want
    sh.b = [] if dot else None
    parts = _deal(items, R, partition, index)
    assert sorted(i for part in parts for i in part) == list(range(len(items)))
    shards = [[items[i] for i in part] for part in parts]
    last_rank = [r for r, part in enumerate(parts) if part and part[-1] == len(items) - 1]
    k, plus, minus = ballast_items(ballast, dot)
    ra, rb = ballast_ranks(index, R)
    ball = [plus] * k + [minus] * k
    # +G in front of what rank a holds (it is added first), -G behind what rank b holds
    shards[ra] = [plus] * k + shards[ra]
    shards[rb] = shards[rb] + [minus] * k
    _finish(sh, items, shards, ball)
    sh.last_alone = bool(last_rank) and len(shards[last_rank[0]]) == 1
    sh.flags = B.dot_flags(items + ball, case.exact) if dot else 0
    if dot and ballast is None:
        assert sh.flags == case.flags
    return sh


def explicit(name, R, per_rank, want, flags, dot=True):
    """a hand-made case: per_rank[r] is the list of (x, y) pairs (or of terms) of rank r; non-finite operands allowed
    (then no exact total is kept)"""
    sh = Shards()
    for s in Shards.__slots__:
        setattr(sh, s, None)
    sh.name, sh.index, sh.R, sh.partition, sh.want, sh.flags = name, 0, R, "explicit", want, flags
    sh.a = [np.array([(p[0] if dot else p) for p in s], dtype=np.float64) for s in per_rank]
    sh.b = [np.array([p[1] for p in s], dtype=np.float64) for s in per_rank] if dot else None
    return sh


# ---------------------------------------------------------------------------------------------
# the non-finite table (include/exblas_hip.h: flags are the OR over the ranks; NaN if a NaN was seen or both infinities
# were, otherwise the infinity)
# ---------------------------------------------------------------------------------------------
def nonfinite_table(R=3):
    inf, nan = math.inf, math.nan
    fill = [[(1.5, 1.0), (-0.25, 1.0)], [(3.0, 1.0)], [(2.0 ** -30, 1.0), (7.0, 1.0)]]

    def rows(extra):
        out = [list(f) for f in fill[:R]] + [[] for _ in range(R - 3)]
        for r, p in extra:
            out[r].insert(1, p)
        return out
    over = (math.ldexp(1.0, 600), math.ldexp(1.0, 500))
    table = [("+Inf on one rank", rows([(1, (inf, 1.0))]), inf, 1, True),
             ("-Inf on one rank", rows([(R - 1, (-inf, 1.0))]), -inf, 2, True),
             ("NaN on one rank", rows([(0, (nan, 1.0))]), nan, 4, True),
             ("+Inf on rank 0, -Inf on the last rank", rows([(0, (inf, 1.0)), (R - 1, (-inf, 1.0))]), nan, 3, True),
             ("0 * Inf on one rank", rows([(1, (0.0, inf))]), nan, 4, False),
             ("finite overflowing pair on rank 0, +Inf operand on rank 1", rows([(0, over), (1, (inf, 2.0))]), inf,
              B.FLAG_PINF | B.FLAG_POVER | B.FLAG_PHIGH_EXACT, False)]
    out = []
    for name, per_rank, want, flags, as_sum in table:
        out.append(explicit("dot: " + name, R, per_rank, want, flags))
        if as_sum:
            out.append(explicit("sum: " + name, R, [[p[0] for p in s] for s in per_rank], want, flags, dot=False))
    return out


# ---------------------------------------------------------------------------------------------
# word 71 of the summed set: the under / overflow counters, 1 and 65536 per rank
# ---------------------------------------------------------------------------------------------
COUNTER_R, COUNTER_UNDER, COUNTER_OVER = 64, 40, 3


def counter_case():
    """64 ranks: 40 hold a product below 2^-968 (half a unit each), 3 a finite overflowing product (2^1100 + 2^1100 -
    2^1101 = 0); the main part is a tie of Family A with an odd mantissa, which the 20 units move off the tie"""
    h = B.family_a([1100], kinds=("tie",), signs=(1,))[1]
    assert h.mant == "odd"
    per_rank = [[] for _ in range(COUNTER_R)]
    for i, x in enumerate(h.terms):
        per_rank[7 + 9 * i].append((x, 1.0))
    for r in range(COUNTER_UNDER):
        per_rank[(3 * r + 1) % COUNTER_R].append((math.ldexp(1.0, -537), math.ldexp(1.0, -538)))
    assert len({(3 * r + 1) % COUNTER_R for r in range(COUNTER_UNDER)}) == COUNTER_UNDER
    for r, p in ((0, (math.ldexp(1.0, 600), math.ldexp(1.0, 500))), (31, (math.ldexp(1.0, 600), math.ldexp(1.0, 500))),
                 (63, (-math.ldexp(1.0, 600), math.ldexp(1.0, 501)))):
        per_rank[r].append(p)
    exact = sum((Fraction(x) * Fraction(y) for s in per_rank for x, y in s), Fraction(0))
    assert exact * B.ONE == h.T + COUNTER_UNDER // 2
    sh = explicit("flag counters", COUNTER_R, per_rank, B.X.round_nearest_even(exact), 8 | 16 | 32 | 64)
    sh.T = exact * B.ONE
    sh.low_r = [Fraction(1, 2) if any(0 < abs(Fraction(x) * Fraction(y)) < LOW_LIMIT for x, y in s) else None for s in per_rank]
    sh.high_r = [Fraction(1) if any(abs(Fraction(x) * Fraction(y)) >= HIGH_LIMIT for x, y in s) else None for s in per_rank]
    assert sum(v is not None for v in sh.low_r) == COUNTER_UNDER and sum(v is not None for v in sh.high_r) == COUNTER_OVER
    return sh


# ---------------------------------------------------------------------------------------------
# the batches that the GPU tests run: the same lists in the worker process and in the test that checks its output
# ---------------------------------------------------------------------------------------------
Job = collections.namedtuple("Job", "shards fpe ee")


def _settings(case, j, ballasts):
    """partition and ballast of the j-th case of a batch: 5 partitions and 7 (11) ballast settings are coprime, so the
    cases of a kind walk through every pair of them"""
    big = case.terms is not None and len(case.terms) >= BIG_TERMS
    return (BIG_PARTITIONS[j % 2] if big else PARTITIONS[j % len(PARTITIONS)]), ballasts[j % len(ballasts)]


def deal_batch(cases, R, offset=0, variants=None):
    out = []
    for i, c in enumerate(cases):
        dot = c.a is not None
        partition, ballast = _settings(c, i + offset, DOT_BALLAST if dot else SUM_BALLAST)
        v = variants or (FPE_VARIANTS_DOT if dot else FPE_VARIANTS_SUM)
        fpe, ee = v[(i + offset) % len(v)]
        out.append(Job(deal(c, i, R, partition, ballast), fpe, ee))
    return out


@functools.lru_cache(maxsize=None)
def _f_low():
    return B.family_f_low()


@functools.lru_cache(maxsize=None)
def _f_high():
    return B.family_f_high()


@functools.lru_cache(maxsize=None)
def sum_sample(count):
    return tuple(B.stride_sample(B.sum_cases(), count))


@functools.lru_cache(maxsize=None)
def dot_sample(count):
    """a cut of Family F that keeps all of family_f_high; from 1000 cases on it leaves no kind of family_f_low out (there
    are more than 600 kinds), below that it is evenly strided"""
    high, low = _f_high(), _f_low()
    want = max(1, count - len(high))
    return tuple((B.stride_sample(low, want) if count >= 1000 else low[::max(1, len(low) // want)]) + high)


def pipeline_sequence(R):
    """16 reductions; the two accumulator slots alternate, so each slot sees back to back: a case with HIGH products, one
    with no out-of-range product, one with LOW products only, a plain ExSUM -- twice"""
    f = _f_low() + _f_high()
    EX = B.FLAG_POVER | B.FLAG_PHIGH_EXACT
    LOW = B.FLAG_PUNDER | B.FLAG_PLOW_EXACT
    high = [c for c in f if c.flags == EX and math.isfinite(c.want)]
    low = [c for c in f if c.flags == LOW]
    plain = [B._dot_case("plain " + c.kind, [(x, 1.0) for x in c.terms], p=c.p, mant=c.mant)
             for c in B.family_a([1100, 1500], kinds=("tie", "exact"), signs=(1, -1))]
    sums = B.family_a([777, 1999], kinds=("tie", "tie-1"), signs=(1, -1))
    assert all(c.flags == 0 for c in plain) and len(high) >= 4 and len(low) >= 4
    seq = []
    for rnd in range(2):
        for kind, pool in (("high", high), ("none", plain), ("low", low), ("sum", sums)):
            for slot in range(2):
                i = len(seq)
                c = pool[(5 * rnd + 3 * slot + 1) % len(pool)]
                ballast = {"high": ("high", 3), "none": None, "low": ("low", 1), "sum": ("main", 2044, 3)}[kind]
                if rnd == 1 and kind == "none":
                    ballast = ("main", 1000, 1)
                fpe, ee = ((8, True), (0, False), (4, False), (6, True))[(i + rnd) % 4]
                seq.append(Job(deal(c, i, R, PARTITIONS[(i + 2) % len(PARTITIONS)], ballast), fpe, ee))
                assert seq[-1].shards.flags == {"high": EX, "none": 0, "low": LOW, "sum": 0}[kind]
    assert len(seq) == 16
    return seq


@functools.lru_cache(maxsize=None)
def batches(sum_count=1000, dot_count=1000, r8_count=200, finish_count=50):
    """name -> list of Job (every Job of a batch has the same rank count)"""
    s, d = sum_sample(sum_count), dot_sample(dot_count)
    s8, d8 = sum_sample(r8_count), dot_sample(r8_count)
    fin = list(B.stride_sample(s, finish_count // 2))[:finish_count // 2] + list(d[::max(1, len(d) // (finish_count // 2))])[:finish_count // 2]
    out = {"sum_r2": deal_batch(s, 2), "sum_r3": deal_batch(s, 3, offset=3), "sum_r8": deal_batch(s8, 8, offset=1),
           "dot_r2": deal_batch(d, 2), "dot_r3": deal_batch(d, 3, offset=4), "dot_r8": deal_batch(d8, 8, offset=2),
           "finish_r3": deal_batch(fin, 3, offset=6), "pipe_r2": pipeline_sequence(2),
           "counters_r64": [Job(counter_case(), 8, True)],
           "nonfinite_r3": [Job(sh, *((8, True), (0, False), (4, False))[i % 3]) for i, sh in enumerate(nonfinite_table(3))]}
    return out


def host_batches(nv, count=300):
    """the ExSUM and the ExDOT cases of one device list of the host-pointer merge"""
    return deal_batch(sum_sample(count), nv, offset=nv), deal_batch(dot_sample(count), nv, offset=nv + 1)


def real_rank_batch(world, count=60):
    """the fixed batch that real ranks run (tests/test_gpu_multirank.py): ExSUM and ExDOT, by_sign and last_alone, with
    ballast"""
    s = B.family_a(range(B.P_MIN, B.P_MAX + 1, 97)) + B.family_b() + B.family_c()     # (small lists: every rank builds them)
    d = B.family_f_low(positions=(3 * 32 + 31, 40 * 32 + 5)) + B.family_f_high()
    s, d = s[::len(s) // (count // 2)][:count // 2], d[::len(d) // (count // 2 - 6)][:count // 2 - 6] + d[-6:]
    out = []
    for i, c in enumerate(s + d):
        dot = c.a is not None
        ballasts = (DOT_BALLAST if dot else SUM_BALLAST)[1:]
        v = FPE_VARIANTS_DOT if dot else FPE_VARIANTS_SUM
        out.append(Job(deal(c, i, world, ("by_sign", "last_alone")[i % 2], ballasts[i % len(ballasts)]), *v[i % len(v)]))
    assert len(out) == count
    return out
