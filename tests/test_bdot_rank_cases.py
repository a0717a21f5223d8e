"""CPU suite: the row-sharded ExBDOT constructions (tests/bdot_rank_cases.py) held to exact arithmetic -- the union of the
shards is the construction's multiset of products plus a ballast that cancels, the per-shard totals add up, and every
corner the GPU tests rely on is reached for every rank count."""
import collections
import math
from fractions import Fraction

import numpy as np
import pytest

import bdot_cases as D
import bdot_rank_cases as S
import blas1_cases as B


def test_constructions_are_what_the_issue_counts():
    d_short, d_long, g, ints = S.constructions()
    assert (d_short.mode, d_short.n, d_short.p) == ("D", 70, 64)
    assert (d_long.mode, d_long.n, d_long.p) == ("D", 32771 + 67, 42)
    assert (g.mode, g.p, g.q) == ("G", 12, 5) and (ints.mode, ints.n, ints.p, ints.q) == ("G", 200, 5, 5)
    # planted_g: at least half of the block's outputs are kept, and no tie or near-tie kind of its cases is lost
    assert int(g.keep.sum()) == 34 and 2 * int(g.keep.sum()) >= g.outputs
    kinds = {k for k in g.kinds if k[1] in S.NEAR_TIE}
    assert kinds and kinds == {g.kinds[o] for o in np.nonzero(g.keep)[0] if g.kinds[o][1] in S.NEAR_TIE}
    assert d_short.keep.all() and d_long.keep.all() and ints.keep.all()


def test_ballast_products_are_finite_exact_negations():
    y = S.ballast_y(64)
    for v in y:
        p = S.BALLAST_G * float(v)
        assert math.isfinite(p) and (-S.BALLAST_G) * float(v) == -p
        exact = Fraction(S.BALLAST_G) * Fraction(float(v))
        assert exact < 1 << 1024 <= 3 * exact
    assert B.units(S.BALLAST_G) >> (500 + B.U - 52) & 1 == 1 and (B.units(S.BALLAST_G) >> (500 + B.U - 52)).bit_length() == 53


@pytest.mark.parametrize("R", S.RANKS)
def test_deals_hold_in_exact_arithmetic_and_reach_every_corner(R):
    reached = collections.Counter()
    jobs = S.jobs(R)
    assert {(sh.partition, sh.k) for sh in jobs} >= {(p, k) for p in S.PARTITIONS for k in S.BALLAST_K}
    for sh in jobs:
        con = sh.con
        assert [len(x) for x in sh.X] == [len(y) for y in sh.Y]
        assert sum(len(x) for x in sh.X) == con.n + 2 * sh.k
        kept = np.nonzero(con.keep)[0]
        # the whole check per output on the small constructions, on a few columns of the long panel (its shards are
        # row subsets of one array: the row bookkeeping is asserted for all of them in the constructor)
        for o in (kept if con.n < 1000 else kept[:: max(1, len(kept) // 4)]):
            j = con.columns(o)[1]
            gy = S._product_units(S.BALLAST_G, float(S.ballast_y(con.q)[j]))
            want = collections.Counter(con.vals[o].values()) + collections.Counter({gy: sh.k, -gy: sh.k})
            got = collections.Counter()
            for r in range(R):
                part = S.multiset_of(con, sh.X[r], sh.Y[r], o)
                assert sum(v * c for v, c in part.items()) == sh.T_r[r][o], (sh, o, r)
                got += part
            assert +got == +want, (sh, o)      # (Counter addition drops nothing here: every count is positive)
            assert sum(sh.T_r[r][o] for r in range(R)) == con.T[o]
            if con.n < 1000:
                assert Fraction(con.T[o], B.ONE) == D.exact_inner(con.X[:, con.columns(o)[0]], con.Y[:, j])
        for name in S.corners(sh):
            reached[name] += 1
    for name in ("negative under positive", "beyond 2^1024 under finite", "deciding unit alone", "empty shard"):
        assert reached[name] >= 1, (R, name, dict(reached))


def test_stacking_in_any_order_is_the_same_multiset():
    sh = S.jobs(3)[1]
    con = sh.con
    X0, Y0 = sh.stacked()
    X1, Y1 = sh.stacked((2, 0, 1))
    for o in np.nonzero(con.keep)[0][:8]:
        assert S.multiset_of(con, X0, Y0, o) == S.multiset_of(con, X1, Y1, o)
