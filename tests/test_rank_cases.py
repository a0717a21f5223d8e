"""CPU tests of tests/rank_cases.py: the dealt cases meet their own claims, the oracle and MPFR return the case's double
on the concatenated shards, and the corners that the constructions exist for are counted -- none may be empty."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import blas1_cases as B
import rank_cases as RC
from helpers import same_double


@pytest.fixture(scope="module")
def dealt():
    """every partition x ballast on a strided sample of A - D (2 and 3 ranks) and on a cut of F (3 ranks): the three
    assertions of the constructors (multiset, per-rank totals, ballast) run inside RC.deal"""
    sums, dots = [], []
    sample = B.stride_sample(B.sum_cases(), 150)
    for i, c in enumerate(sample):
        big = len(c.terms) >= RC.BIG_TERMS
        combos = list(itertools.product(RC.BIG_PARTITIONS if big else RC.PARTITIONS, RC.SUM_BALLAST))
        for k, (partition, ballast) in enumerate(combos if not big else combos[i % 3::3]):
            sums.append(RC.deal(c, i + k, 2 + (i + k) % 2, partition, ballast))
    for i, c in enumerate(RC.dot_sample(300)):
        for k, (partition, ballast) in enumerate(itertools.product(RC.PARTITIONS, RC.DOT_BALLAST)):
            if (i + k) % 5 == 0 or ballast is not None and ballast[0] in ("low", "high") and (i + k) % 2 == 0:
                dots.append(RC.deal(c, i + k, 3, partition, ballast))
    return sums, dots


def test_shard_range_is_the_library_s():
    from exblas_amd.dist import shard_range
    for n in (0, 1, 2, 3, 7, 8, 1001, 32769):
        for world in (1, 2, 3, 8, 64):
            assert [RC.shard_range(n, r, world) for r in range(world)] == [shard_range(n, r, world) for r in range(world)]


def test_every_partition_meets_every_ballast(dealt):
    sums, dots = dealt
    for what, shards, ballasts in (("sum", sums, RC.SUM_BALLAST), ("dot", dots, RC.DOT_BALLAST)):
        seen = {(s.case.family, s.partition, s.ballast) for s in shards}
        for family in {s.case.family for s in shards}:
            for partition in RC.PARTITIONS:
                for ballast in ballasts:
                    assert (family, partition, ballast) in seen, (what, family, partition, ballast)
    assert {(s.case.family, s.case.kind) for s in sums} == {(c.family, c.kind) for c in B.sum_cases()}
    for s in sums[::7]:
        assert (s.digits_r().astype(object) * [1 << (32 * l) for l in range(B.NDIG)]).sum() == s.T


def test_the_gpu_batches(capsys):
    """the lists that the GPU tests run: their sizes, and that the dealing leaves nothing out"""
    b = RC.batches()
    sizes = {k: len(v) for k, v in b.items()}
    with capsys.disabled():
        print(f"\nrank_cases batches: {sizes}")
    assert sizes["sum_r2"] == sizes["sum_r3"] >= 1000 and 150 <= sizes["sum_r8"] <= 400
    assert sizes["dot_r2"] == sizes["dot_r3"] >= 1000 and 150 <= sizes["dot_r8"] <= 400
    assert sizes["finish_r3"] == 50 and sizes["pipe_r2"] >= 12 and sizes["counters_r64"] == 1
    kinds = {(c.family, c.kind) for c in B.sum_cases()}
    for name in ("sum_r2", "sum_r3", "sum_r8"):
        jobs = b[name]
        assert {(j.shards.case.family, j.shards.case.kind) for j in jobs} == kinds, name
        for family in "ABCD":
            mine = [j for j in jobs if j.shards.case.family == family]
            small = [j for j in mine if len(j.shards.case.terms) < RC.BIG_TERMS]
            assert {j.shards.partition for j in small} == set(RC.PARTITIONS), (name, family)
            assert {j.shards.ballast for j in mine} == set(RC.SUM_BALLAST), (name, family)
            assert {(j.fpe, j.ee) for j in mine} == set(RC.FPE_VARIANTS_SUM), (name, family)
        assert all(j.shards.partition in RC.BIG_PARTITIONS for j in jobs if len(j.shards.case.terms) >= RC.BIG_TERMS)
    high_kinds = {c.kind for c in B.family_f_high()}
    for name in ("dot_r2", "dot_r3", "dot_r8"):
        jobs = b[name]
        assert {j.shards.case.kind for j in jobs} >= high_kinds
        assert {(j.shards.partition, j.shards.ballast) for j in jobs} == set(itertools.product(RC.PARTITIONS, RC.DOT_BALLAST)), name
    assert {c.kind for c in B.family_f()} == {j.shards.case.kind for j in b["dot_r2"]}
    for world in (1, 2, 3):
        assert len(RC.real_rank_batch(world)) == 60


def test_oracle_and_mpfr_on_the_concatenated_shards(oracle, dealt):
    """the shards hold the case's total: oracle.exsum on every dealt sum, oracle.exdot where no product leaves the range
    that the oracle's accumulator holds (it restates the reference's kernels, which have both limits), MPFR on all"""
    sums, dots = dealt
    have_mpfr = oracle.mpfr() is not None
    for s in sums[::3]:
        x = s.concatenated()
        assert same_double(oracle.exsum(x, 0), s.want), s
        if have_mpfr:
            # (as a dot product with ones: the MPFR sum oracle keeps 2098 bits like the reference's test, one too few for a
            # running total of 3 x 2^1023 over a unit of 2^-1074; the dot oracle keeps 4196)
            assert same_double(oracle.mpfr_exdot(x, np.ones(len(x))), s.want), s
    plain = 0
    for s in dots:
        a, b = s.concatenated()
        if s.flags == 0:
            plain += 1
            assert same_double(oracle.exdot(a, b, 0), s.want), s
        if have_mpfr:
            assert same_double(oracle.mpfr_exdot(a, b), s.want), s
    for job in RC.batches()["pipe_r2"]:
        s = job.shards
        if s.is_dot and s.flags == 0:
            plain += 1
            assert same_double(oracle.exdot(*s.concatenated(), 0), s.want), s
    assert plain > 0


def test_coverage_counts(capsys):
    """what the dealing is for, counted over the batches that the GPU tests run; every count must be non-zero"""
    b = RC.batches()
    sums = [j.shards for name in ("sum_r2", "sum_r3", "sum_r8") for j in b[name]]
    dots = [j.shards for name in ("dot_r2", "dot_r3", "dot_r8") for j in b[name]]
    counts = {
        "some T_r < 0 < T": sum(1 for s in sums + dots if s.T > 0 and any(t < 0 for t in s.T_r)),
        "some |T_r| > DBL_MAX while |T| <= DBL_MAX": sum(1 for s in sums + dots if abs(s.T) <= B.DBL_MAX_UNITS
                                                        and any(abs(t) > B.DBL_MAX_UNITS for t in s.T_r)),
        "the rank of the last term holds nothing else": sum(1 for s in sums + dots if s.last_alone),
        "F: LOW sum zero, two ranks' LOW parts non-zero": sum(1 for s in dots if _cancels(s.low_r)),
        "F: HIGH sum zero, two ranks' HIGH parts non-zero": sum(1 for s in dots if _cancels(s.high_r)),
        "F: the all-reduced LOW sum is negative": sum(1 for s in dots if sum((v for v in s.low_r if v is not None), Fraction(0)) < 0),
        "empty shards": sum(1 for s in sums + dots for x in s.a if len(x) == 0),
    }
    with capsys.disabled():
        print()
        for k, v in counts.items():
            print(f"rank_cases coverage: {v:6d}  {k}")
    for k, v in counts.items():
        assert v > 0, k


def _cancels(parts):
    held = [v for v in parts if v is not None and v != 0]
    return len(held) >= 2 and sum(held, Fraction(0)) == 0


def test_non_finite_table_and_counter_case():
    table = RC.nonfinite_table(3)
    assert len(table) == 10
    for sh in table:
        a = np.concatenate(sh.a)
        b = np.concatenate(sh.b) if sh.is_dot else np.ones(len(a))
        with np.errstate(invalid="ignore", over="ignore"):
            vals = np.where(np.isfinite(a) & np.isfinite(b), 0.0, a * b)    # what the non-finite OPERANDS give
        pinf, ninf, nan = np.isposinf(vals).any(), np.isneginf(vals).any(), np.isnan(vals).any()
        assert (sh.flags & 7) == pinf * 1 + ninf * 2 + nan * 4, sh
        want = math.nan if nan or (pinf and ninf) else (math.inf if pinf else -math.inf)
        assert same_double(sh.want, want), sh
    c = RC.counter_case()
    assert c.R == 64 and c.flags == 8 | 16 | 32 | 64 and math.isfinite(c.want)
