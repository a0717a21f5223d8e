"""CPU tests of the constructed ExSUM / ExDOT cases (tests/blas1_cases.py): the constructions meet their own conditions,
and the oracle and MPFR return the integer reference's bits, so that a wrong expectation is caught without a GPU.  The
integer reference shares no code with the library or the oracle; where the two disagree the oracle is wrong."""
import math
from fractions import Fraction

import numpy as np
import pytest

import blas1_cases as B
from helpers import digits_from_int, exact_int_from_canon, exact_int_from_digits, same_double


def test_case_counts(capsys):
    """the counts per family, kind and sign, printed once (also without -s): none may be empty"""
    cases = list(B.sum_cases()) + B.family_e() + B.family_f()
    counts = B.kind_counts(cases)
    fam = {}
    for (family, kind, sign), n in sorted(counts.items()):
        fam.setdefault(family, {}).setdefault(kind if family != "F" else kind.split(" ")[0], {}).setdefault(sign, 0)
        fam[family][kind if family != "F" else kind.split(" ")[0]][sign] += n
    with capsys.disabled():
        print()
        for family, kinds in fam.items():
            total = sum(sum(s.values()) for s in kinds.values())
            print(f"blas1_cases family {family}: {total} cases" + ("" if family in "AF" else f" in {len(kinds)} kinds"))
            if family in "AF":
                for kind, s in kinds.items():
                    print(f"    {kind:14s} {s}")
    assert sum(sum(s.values()) for s in fam["A"].values()) == 85860
    for kind in B.A_KINDS:
        assert fam["A"][kind].get("+", 0) > 0 and fam["A"][kind].get("-", 0) > 0, kind
    for family in "BCDEF":
        for kind, s in fam[family].items():
            assert sum(s.values()) > 0
        assert any("+" in s for s in fam[family].values()) and any("-" in s for s in fam[family].values()), family
    a = [c for c in B.sum_cases() if c.family == "A"]
    lz_limb = {((c.p >> 5), 31 - (c.p & 31)) for c in a}
    assert lz_limb >= {(t, lz) for t in range(2, 65) for lz in range(32)}          # every leading-zero count in every limb
    sticky_far = max((c.p - 53) // 32 for c in a if c.kind in ("+1", "-1", "tie+1", "tie-1"))
    assert sticky_far >= 63                                                        # a deciding bit 63 digits below the half bit
    with capsys.disabled():
        print(f"blas1_cases family A: {len(lz_limb)} leading-bit positions, {sum(c.kind == 'tie' for c in a)} ties, "
              f"{sum(math.isinf(c.want) for c in a)} round to +-Inf, {sum(len(c.terms) for c in a)} doubles")


def test_canon_and_digits_round_trip():
    rng = np.random.default_rng(5)
    values = [0, 1, -1, (1 << 2124) + 12345, -(1 << 2124) - 12345, B.CANON_LIMIT - 1, -B.CANON_LIMIT, B.DBL_MAX_UNITS, -B.DBL_MAX_UNITS]
    values += [int(rng.integers(-(1 << 62), 1 << 62)) << int(rng.integers(0, 2060)) for _ in range(300)]
    values += [c.T for c in B.sum_cases()[::97]]
    for T in values:
        canon = B.canon_from_int(T)
        assert exact_int_from_canon(canon) == T << 18
        assert ((canon[:-1] >= 0) & (canon[:-1] < 1 << 52)).all()
        assert exact_int_from_digits(digits_from_int(T)) == T
    assert (B.canon_matrix(values) == np.array([B.canon_from_int(T) for T in values])).all()
    wide = values + [1 << (32 * 67), -(1 << (32 * 67)), B.DIGITS_LIMIT - 1, -B.DIGITS_LIMIT]
    assert (B.digits_matrix(wide) == np.array([digits_from_int(T) for T in wide])).all()
    with pytest.raises(AssertionError):
        B.canon_from_int(B.CANON_LIMIT)
    assert not B.canon_fits(1 << (32 * 67)) and B.canon_fits(-(1 << 2112))
    assert B.units(5e-324) == 1 and B.units(-1.0) == -B.ONE and B.units(1.7976931348623157e308) == B.DBL_MAX_UNITS


def test_oracle_agrees_on_every_sum_case(oracle):
    """A - D: oracle.exsum returns `want` and canon_from_int(T) on every case"""
    bad = []
    for i, c in enumerate(B.sum_cases()):
        got, limbs = oracle.exsum(np.array(c.terms), 0, limbs=True)
        if not same_double(got, c.want) or not (limbs == B.canon_from_int(c.T)).all():
            bad.append((i, c, got, c.want))
    assert not bad, (len(bad), bad[:5])
    # the expansion variants on a sample (not on D: the oracle's expansions restate the reference's, which have no guard
    # against huge values and overflow there)
    for c in [c for c in B.sum_cases()[::499] if c.family != "D"]:
        for fpe, ee in ((4, False), (8, True)):
            got, limbs = oracle.exsum(np.array(c.terms), fpe, ee, limbs=True)
            assert same_double(got, c.want) and (limbs == B.canon_from_int(c.T)).all(), (c, fpe, ee)


def test_oracle_rounds_the_limb_sets(oracle):
    """E: the sets add up to T; where T fits the canonical limbs the oracle's rounding of them is `want`"""
    fits = 0
    for c in B.family_e():
        assert sum(exact_int_from_digits(row[:B.NDIG]) for row in c.sets) == c.T
        assert exact_int_from_digits(digits_from_int(c.T)) == c.T and abs(int(digits_from_int(c.T)[-1])) < 1 << 40
        if B.canon_fits(c.T):
            fits += 1
            assert same_double(oracle.round_limbs(B.canon_from_int(c.T)), c.want), c
    assert fits >= 60


def test_mpfr_agrees(oracle):
    """MPFR at 4196 bits on all of B - D, a strided sample of A, and a strided sample of F that leaves no kind out"""
    assert oracle.mpfr() is not None, "this test needs the MPFR oracle (oracle/libmpfr_oracle.so)"
    sums = [c for c in B.sum_cases() if c.family != "A"] + B.stride_sample([c for c in B.sum_cases() if c.family == "A"], 2000)
    for c in sums:
        assert same_double(oracle.mpfr_exsum(np.array(c.terms)), c.want), c
    f = B.family_f()
    sample = B.stride_sample(f, 2000)
    assert len(sample) >= 2000 and {c.kind for c in sample} == {c.kind for c in f}
    for c in sample:
        assert same_double(oracle.mpfr_exdot(c.a, c.b), c.want), (c, c.want)
        assert c.want == B.X.round_nearest_even(sum((Fraction(float(x)) * Fraction(float(y)) for x, y in zip(c.a, c.b)), Fraction(0)))
