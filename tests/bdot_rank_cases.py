"""The constructions of tests/bdot_cases.py with their ROWS dealt over R shards adversarially -- the block counterpart of
tests/rank_cases.py, for the row-sharded ExBDOT (exbdot_export_dev + exbdot_round_dev, exbdot_allreduce).

Nothing here touches the GPU, the library or the oracle.  A block pair is cut into R row shards whose stacking has the
same exact inner products: the expected doubles are those of the construction.  What changes is what every shard exports
before the merge: per output the exact total of the shard's products, as 68 digits.  All arithmetic is on Python
integers in units of 2^-1074 (every product of a construction is a whole number of units: asserted against Fractions).

Constructions (built once, `constructions()`):
  d_short, d_long  planted_d on bdot_cases.sample(24) in panels of at most 64 columns: the first (Family A, at most three
                   terms a column) has n = 70 rows, the one panel that is kept beyond it holds the columns of 32 768 to
                   32 771 terms
  g                planted_g on the first 12 cases of the sample with the shifts (0, -3, 40, -200, 7); only the outputs
                   in `keep` have an exact total
  ints             integer_blocks(rng, 200, 5, 5), mode 'G'
Partitions of the rows (deterministic in the job index):
  contiguous   the rows in order, cut like exblas_shard_range
  round_robin  row i on shard i % R
  one_rank     all rows on shard index % R, every other shard empty
  last_alone   the last row on the last shard, the rest on shard 0 (in planted_d every fourth column ends on the last row,
               and the last term of a Family A case is its half, quarter or +-1-unit part)
Ballast: k rows (+g, .., +g | y_row) on shard a and k rows (-g, .., -g | y_row) on shard b != a, g a full odd 53-bit
  mantissa times 2^500, y_row[j] = (1 + (j + 1) / 1024) 2^523.  Each product is negated exactly, so a pair cancels whatever
  its TwoProd error is; every product is finite (below 2^1024) and k = 3 copies take a shard's partial total beyond 2^1024.
"""
import collections
import functools
import math
from fractions import Fraction

import numpy as np

import bdot_cases as D
import blas1_cases as B
from rank_cases import M_ODD, ballast_ranks, shard_range

PARTITIONS = ("contiguous", "round_robin", "one_rank", "last_alone")
BALLAST_K = (0, 1, 3)
G_SHIFTS = (0, -3, 40, -200, 7)
G_CASES = 12
NEAR_TIE = ("tie", "tie+1", "tie-1", "below")
BALLAST_G = math.ldexp(M_ODD, 500)
HIGH_LIMIT_UNITS = 1 << (1024 + B.U)
RANKS = (2, 3, 8)


def ballast_y(q):
    y = np.array([math.ldexp(1.0 + (j + 1) / 1024.0, 523) for j in range(q)])
    assert all(math.isfinite(BALLAST_G * v) and 3 * Fraction(BALLAST_G) * Fraction(float(v)) >= 1 << 1024 for v in y)
    return y


def _product_units(x, y):
    """x * y exactly, as a whole number of units of 2^-1074 (asserted)"""
    v = B.units(x) * B.units(y)
    assert v % B.ONE == 0, "a product is not a whole number of units"
    return v >> B.U


class Construction:
    """name, mode, X, Y, n, p, q; outputs: their number ('D': p, 'G': p * q, output i * q + j); want / keep: the expected
    doubles and which of them are held (flat); kinds: per output the (family, kind) of its case or None; vals[o]: {row:
    the exact product of that row in units} over the rows where it is non-zero, for the kept outputs; T[o]: their sum"""

    def __init__(self, name, mode, X, Y, want, keep, kinds):
        self.name, self.mode, self.X, self.Y = name, mode, X, Y
        self.n, self.p, self.q = X.shape[0], X.shape[1], Y.shape[1]
        self.outputs = self.p if mode == "D" else self.p * self.q
        self.want, self.keep, self.kinds = np.asarray(want, dtype=np.float64).ravel(), np.asarray(keep, dtype=bool).ravel(), kinds
        assert self.want.shape == self.keep.shape == (self.outputs,) and len(kinds) == self.outputs
        self.vals, self.T = [None] * self.outputs, [None] * self.outputs
        for o in np.nonzero(self.keep)[0]:
            i, j = self.columns(o)
            rows = np.nonzero((X[:, i] != 0) & (Y[:, j] != 0))[0]
            self.vals[o] = {int(r): _product_units(float(X[r, i]), float(Y[r, j])) for r in rows}
            self.T[o] = sum(self.vals[o].values())
            assert B.X.round_nearest_even(Fraction(self.T[o], B.ONE)) == self.want[o] or math.isnan(self.want[o])

    def columns(self, o):
        return (int(o), int(o)) if self.mode == "D" else (int(o) // self.q, int(o) % self.q)

    def __repr__(self):
        return f"<{self.name} {self.mode} {self.n} x {self.p}, {self.q}>"


@functools.lru_cache(maxsize=None)
def constructions():
    sample = D.sample(24)
    assert len(sample) == 106
    panels = [sample[i:i + D.MAX_COLS] for i in range(0, len(sample), D.MAX_COLS)]
    long_panels = [pn for pn in panels if max(len(c.terms) for c in pn) >= 32771]
    panels = [pn for pn in panels if pn not in long_panels] + long_panels[:1]
    out = []
    for name, pn in zip(("d_short", "d_long"), panels):
        d = D.planted_d(pn)
        out.append(Construction(name, "D", d.X, d.Y, d.want, np.ones(d.k, dtype=bool), [(c.family, c.kind) for c in pn]))
    assert len(out) == 2 and out[0].n == 3 + D.PAD_ROWS and out[1].n == 32771 + D.PAD_ROWS
    cases = sample[:G_CASES]
    g = D.planted_g(cases, G_SHIFTS)
    out.append(Construction("g", "G", g.X, g.Y, g.want, g.keep, [(c.family, c.kind) for c in cases for _ in G_SHIFTS]))
    c = D.integer_blocks(np.random.default_rng(11), 200, 5, 5)
    out.append(Construction("ints", "G", c.X, c.Y, c.want, np.ones((5, 5), dtype=bool), [None] * 25))
    for con, T in ((out[0], [c.T for c in panels[0]]), (out[1], [c.T for c in panels[1]])):
        assert con.T == T
    for o in range(25):
        assert Fraction(out[3].T[o], B.ONE) == c.G[o // 5, o % 5]
    return tuple(out)


def _deal_rows(n, R, partition, index):
    if partition == "contiguous":
        return [list(range(*shard_range(n, r, R))) for r in range(R)]
    if partition == "round_robin":
        return [list(range(r, n, R)) for r in range(R)]
    if partition == "one_rank":
        return [list(range(n)) if r == index % R else [] for r in range(R)]
    assert partition == "last_alone"
    if R == 1:
        return [list(range(n))]
    return [list(range(n - 1))] + [[] for _ in range(R - 2)] + [[n - 1]]


class Shards:
    """one construction dealt over R shards.  rows[r]: the construction's rows of shard r, in order; X[r], Y[r]: the
    shard's blocks (ballast rows included: +g in front on shard `ra`, -g behind on shard `rb`); T_r[r][o]: the exact total
    of shard r for the kept output o (None elsewhere)"""

    def __init__(self, con, index, R, partition, k):
        self.con, self.index, self.R, self.partition, self.k = con, index, R, partition, k if R > 1 else 0
        self.rows = _deal_rows(con.n, R, partition, index)
        assert sorted(i for part in self.rows for i in part) == list(range(con.n))
        self.ra, self.rb = ballast_ranks(index, R)
        yb = ballast_y(con.q)
        self.X, self.Y = [], []
        for r, part in enumerate(self.rows):
            x, y = [con.X[part]], [con.Y[part]]
            if self.k and r == self.ra:
                x.insert(0, np.full((self.k, con.p), BALLAST_G))
                y.insert(0, np.tile(yb, (self.k, 1)))
            if self.k and r == self.rb:
                x.append(np.full((self.k, con.p), -BALLAST_G))
                y.append(np.tile(yb, (self.k, 1)))
            self.X.append(np.ascontiguousarray(np.concatenate(x)))
            self.Y.append(np.ascontiguousarray(np.concatenate(y)))
        owner = np.empty(con.n, dtype=np.int64)
        for r, part in enumerate(self.rows):
            owner[part] = r
        self.T_r = [[None] * con.outputs for _ in range(R)]
        for o in np.nonzero(con.keep)[0]:
            tot = [0] * R
            for row, v in con.vals[o].items():
                tot[owner[row]] += v
            if self.k:
                gy = _product_units(BALLAST_G, float(yb[con.columns(o)[1]]))
                tot[self.ra] += self.k * gy
                tot[self.rb] -= self.k * gy
            assert sum(tot) == con.T[o], "the per-shard totals do not add up to the total"
            for r in range(R):
                self.T_r[r][o] = tot[r]

    def __repr__(self):
        return f"<{self.con.name} #{self.index} R={self.R} {self.partition} ballast k={self.k}>"

    def digits_r(self, r):
        """[outputs, 68]: the digit sets shard r is expected to export (rows of zeros where the output is not kept)"""
        return B.digits_matrix([0 if t is None else t for t in self.T_r[r]])

    def stacked(self, order=None):
        order = range(self.R) if order is None else order
        return np.concatenate([self.X[r] for r in order]), np.concatenate([self.Y[r] for r in order])


def jobs(R):
    """every construction under every partition, the ballast walking through none, k = 1 and k = 3"""
    out = []
    for ci, con in enumerate(constructions()):
        for pi, partition in enumerate(PARTITIONS):
            out.append(Shards(con, len(out), R, partition, BALLAST_K[(ci + pi) % len(BALLAST_K)]))
    return out


def multiset_of(con, X, Y, o):
    """the non-zero exact products of output o over the rows of the blocks X, Y, as a Counter"""
    i, j = con.columns(o)
    rows = np.nonzero((X[:, i] != 0) & (Y[:, j] != 0))[0]
    return collections.Counter(_product_units(float(X[r, i]), float(Y[r, j])) for r in rows)


def corners(sh):
    """which of the corners this deal reaches, as a set of names"""
    con, out = sh.con, set()
    if any(len(x) == 0 for x in sh.X):
        out.add("empty shard")
    for o in np.nonzero(con.keep)[0]:
        tot = [sh.T_r[r][o] for r in range(sh.R)]
        if con.T[o] > 0 and min(tot) < 0:
            out.add("negative under positive")
        if max(abs(t) for t in tot) >= HIGH_LIMIT_UNITS and math.isfinite(con.want[o]):
            out.add("beyond 2^1024 under finite")
        kind = con.kinds[o]
        if kind is not None and kind[0] == "A" and kind[1] != "exact" and con.vals[o]:
            # the last term of a Family A case is the half, quarter or +-1 unit: alone when its shard holds nothing else
            # for this output, ballast included
            last_row = max(con.vals[o])
            r = next(r for r, part in enumerate(sh.rows) if last_row in part)
            alone = not any(row in con.vals[o] for row in sh.rows[r] if row != last_row) and not (sh.k and r in (sh.ra, sh.rb))
            if alone and len(con.vals[o]) > 1:
                assert tot[r] == con.vals[o][last_row]
                out.add("deciding unit alone")
    return out
