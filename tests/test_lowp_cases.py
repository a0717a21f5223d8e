"""Holds the builders of tests/lowp_cases.py to their claims, and the library's CPU rounding (exblas_round_digits_host,
the host compilation of round_digits_to) to the Python-integer model.  No GPU."""
import numpy as np
import pytest

import blas1_cases as B
import lowp_cases as L


def cast_bits(v, name):
    """the pattern numpy (float32, float16) or torch (bfloat16) gives when it converts the double v"""
    if name == "bfloat16":
        import torch
        return int(torch.tensor(v, dtype=torch.float64).to(torch.bfloat16).view(torch.int16)) & 0xffff
    with np.errstate(over="ignore"):
        return int(np.array(v, dtype=np.float64).astype(name).reshape(1).view({"float32": np.uint32, "float16": np.uint16}[name])[0])


def doubles_for(name, count=3000, seed=1):
    """doubles over the format's whole range (subnormal results, overflow) that need one rounding only"""
    prec, emin, emax, width = L.FORMATS[name]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(count) * np.exp2(rng.integers(emin - prec - 2, emax + 3, count))
    edge = [0.0, 2.0 ** emin, 2.0 ** (emin - prec + 1), 2.0 ** (emin - prec), 2.0 ** (emin - prec) * 1.5, 2.0 ** (emax + 1),
            (2 - 2.0 ** -prec) * 2.0 ** emax, np.nextafter((2 - 2.0 ** -prec) * 2.0 ** emax, 0)]
    x = np.concatenate([x, edge, -np.array(edge[1:])])
    if name == "bfloat16":      # torch converts a double through float32: one rounding only for doubles that ARE float32
        with np.errstate(over="ignore"):
            x = x.astype(np.float32).astype(np.float64)
        x = x[np.isfinite(x)]
    return x


@pytest.mark.parametrize("name", L.NARROW)
def test_round_to_agrees_with_the_casts_on_doubles(name):
    for v in doubles_for(name):
        assert L.round_to(B.units(v), name) == cast_bits(v, name), (name, float(v).hex())


@pytest.mark.parametrize("name", L.NARROW)
def test_traps_differ_from_the_cast(name):
    """the builder asserts that the single rounding differs from double-then-cast; here the cast is numpy's / torch's"""
    tr = L.traps(name)
    assert len(tr) >= 12
    for T, one, two in tr:
        d = np.array([L.round_to(T, "float64")], dtype=np.uint64).view(np.float64)[0]
        assert cast_bits(d, name) == two != one == L.round_to(T, name)


def test_units_of_every_dtype_and_of_products():
    import torch
    rng = np.random.default_rng(2)
    x = rng.standard_normal(500) * np.exp2(rng.integers(-20, 12, 500))
    for name in L.NARROW:
        t = torch.from_numpy(x).to(getattr(torch, name))
        want = sum(B.units(float(v)) for v in t.double())
        assert L.units(t) == want
        if name != "bfloat16":
            assert L.units(t.numpy()) == want
        u = torch.from_numpy(x[::-1].copy()).to(getattr(torch, name))
        assert L.units(t, u) == sum(B.units(float(a) * float(b)) for a, b in zip(t.double(), u.double()))   # exact doubles
    assert L.units(x) == B.total_of(x)
    for name in L.NARROW:                                   # both ends of the product range
        a, b = L.dot_range_pairs(name)
        ta, tb = L.as_torch(a, name), L.as_torch(b, name)
        prods = ta.double() * tb.double()
        prec, emin, emax, width = L.FORMATS[name]
        assert float(prods.abs().min()) == 2.0 ** (2 * (emin - prec + 1)) and float(prods.abs().max()) > 2.0 ** (2 * emax + 1)
        assert L.units(ta, tb) == sum(B.units(float(p)) for p in prods)
    assert 2 * (L.FORMATS["float32"][1] - 23) == -298


def test_digits_of_matches_the_blas1_helpers():
    for T in L.random_totals(3, 1)[::7]:
        assert (L.digits_of(T) == B.digits_matrix([T])[0]).all()


@pytest.mark.parametrize("name", L.ALL)
def test_planted_totals_cover_their_kinds(name):
    """every kind in both signs, in normal binades and (narrow formats) in the subnormal range; `want`, written down from
    the construction, is what the model gives"""
    P = L.planted(name)
    kinds = {(c.kind, c.T < 0, c.subnormal) for c in P}
    for neg in (False, True):
        for kind in ("exact", "tie_even", "tie_odd", "tie+1", "tie-1"):
            assert (kind, neg, False) in kinds, (kind, neg)
            if name != "float64":
                assert (kind, neg, True) in kinds, (kind, neg, "subnormal")
        for kind in ("below_overflow", "at_overflow"):
            assert (kind, neg, False) in kinds
        if name != "float64":
            for kind in ("sub_max+half", "half_min", "half_min+1"):
                assert (kind, neg, True) in kinds
    assert ("zero", False, False) in kinds
    prec, emin, emax, width = L.FORMATS[name]
    inf = (2 * emax + 1) << (prec - 1)
    for c in P:
        assert L.round_to(c.T, name) == c.want, c
        if c.kind == "at_overflow":
            assert c.want & ~(1 << (width - 1)) == inf
        if c.kind == "below_overflow":
            assert c.want & ~(1 << (width - 1)) == inf - 1
        if c.kind in ("tie+1", "tie-1"):
            assert c.T % 2 == 1 or name == "float64"        # the sticky bit sits in the lowest digit
    if name == "float16":
        assert any(c.kind == "at_overflow" and c.T == 65520 << L.U for c in P)
    if name == "float32":
        assert any(c.kind == "at_overflow" and c.T == ((1 << 128) - (1 << 103)) << L.U for c in P)


MUTANT_CATCHERS = {"sticky_next_digit": {"tie+1", "half_min+1"}, "ties_away": {"tie_even", "half_min"},
                   "flush_subnormal": {"exact", "tie_even", "tie_odd", "tie+1", "tie-1", "half_min+1"},
                   "overflow_late": {"at_overflow"}}


@pytest.mark.parametrize("mutant", L.MUTANTS)
@pytest.mark.parametrize("name", L.NARROW)
def test_planted_totals_kill_the_mutants(name, mutant):
    """Four wrong roundings and the planted kinds that tell each from the right one (MUTANT_CATCHERS):
      sticky_next_digit  the sticky bit taken from the digit below the half bit only -- caught by tie+1 (one unit of
                         2^-1074 above a tie whose half bit lies 29 digits or more higher) and half_min+1;
      ties_away          ties rounded away from zero -- caught by tie_even and half_min (the tie between 0 and the
                         smallest subnormal goes to 0);
      flush_subnormal    a subnormal result flushed to zero -- caught by every subnormal case with a non-zero result;
      overflow_late      the overflow threshold one ulp late, the tie at 2^(emax+1) - ulp/2 kept finite -- caught by
                         at_overflow alone (below_overflow and max pass either way).
    The same totals go through the library in test_round_digits_host_*: a library with one of these faults fails there."""
    killers = {c.kind for c in L.planted(name) if L.round_to(c.T, name, mutant) != c.want}
    assert killers, (name, mutant)
    assert killers <= MUTANT_CATCHERS[mutant] | ({"sub_max+half"} if mutant == "flush_subnormal" else set()), killers
    assert MUTANT_CATCHERS[mutant] & killers


@pytest.mark.parametrize("name", L.NARROW)
def test_inputs_realise_their_totals(name):
    """input_cases asserts the sums; here: subnormal inputs and the largest finite value occur, and every trap of every
    target has float32 inputs wherever its bits are within float32's reach"""
    prec, emin, emax, width = L.FORMATS[name]
    cases = L.input_cases(name)
    pats = {p & ~(1 << (width - 1)) for _, _, ps in cases for p in ps}
    assert any(0 < p < 1 << (prec - 1) for p in pats), "no subnormal input"
    assert ((2 * emax + 1) << (prec - 1)) - 1 in pats, "the largest finite value is missing"
    assert {k for k, _, _ in cases} >= {"exact", "tie_even", "tie_odd", "tie+1", "tie-1", "max", "2max", "cancel"}
    assert sum(L.realise(T, "float32") is not None for T, _, _ in L.traps(name)) >= 8
    assert L.realise(1, name) is None and L.realise(1 << (emax + L.U + 1), name) is None


# ---------------------------------------------------------------------------------------------
# the library's CPU rounding
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_round():
    import exblas_amd
    return lambda T, name: exblas_amd.round_digits_host(L.digits_of(T), name)


@pytest.mark.parametrize("name", L.ALL)
def test_round_digits_host_on_planted_totals_and_traps(host_round, name):
    for target in L.ALL:                                    # the totals planted for one format, rounded into every format
        for c in L.planted(name):
            assert host_round(c.T, target) == L.round_to(c.T, target), (c, target)
    for c in L.planted(name):
        assert host_round(c.T, name) == c.want, c
    if name != "float64":
        for T, one, two in L.traps(name):
            assert host_round(T, name) == one, (name, T)


@pytest.mark.parametrize("name", L.ALL)
def test_round_digits_host_on_random_totals_at_every_bit_position(host_round, name):
    for T in L.random_totals(5):
        assert host_round(T, name) == L.round_to(T, name), (name, T.bit_length())


def test_round_digits_host_float64_is_the_finalize_rounding(host_round):
    """for float64 the routine must return what round_exact_bits returns: the expectations of blas1_cases"""
    from helpers import bits
    cases = [B.Case("A", "exact", T) for T in L.random_totals(6, 1)[::5]]
    cases += [B.Case("A", "tie", c.T) for c in L.planted("float64")]
    for c in cases:
        want = int(bits([c.want])[0]) & (2**64 - 1)
        if c.want == 0 and c.T < 0:
            want = 1 << 63                                  # (Fraction-based rounding has no -0)
        assert host_round(c.T, "float64") == want, c
        assert want == L.round_to(c.T, "float64") or c.want == 0
