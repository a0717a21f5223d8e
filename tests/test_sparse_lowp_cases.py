"""CPU suite (no GPU): the constructed rows of the narrow ExSpMV / ExSpMM (tests/sparse_lowp_cases.py) against their own
claims, and the interval certificate behind the in-register rounding (exblas_round_interval_host) against the integer
model: sound on every planted and trap total and on seeded random (res, bound) pairs, complete at a margin of 4 bounds."""
from fractions import Fraction

import numpy as np
import pytest

import lowp_cases as L
import sparse_lowp_cases as S


@pytest.fixture(scope="module")
def ex():
    import exblas_amd
    exblas_amd.load_library()
    return exblas_amd


@pytest.mark.parametrize("dtype", S.NARROW)
def test_rows_are_what_they_claim(dtype):
    """Row() has asserted that each row's exact total is its T and that `want`, written down from the construction, is the
    integer model's rounding; here: every kind the issue lists occurs in both signs, and every entry is a finite value of
    the dtype against a power of two the table holds."""
    rows = S.all_rows(dtype)
    kinds = {(r.kind.split(":")[0], r.T < 0) for r in rows}
    for k in ("exact", "tie_even", "tie_odd", "tie+u", "tie-u", "below_overflow", "at_overflow", "sub_max+half", "half_min",
              "half_min+u", "half_min-u", "trap"):
        assert (k, False) in kinds and (k, True) in kinds, k
    assert any(r.kind == "cancel" and len(r.entries) >= 2 for r in rows)
    ones = (1 << L.FORMATS[dtype][0]) - 1
    assert any(r.kind.startswith("tie") and ((abs(r.T) >> (abs(r.T).bit_length() - L.FORMATS[dtype][0])) == ones)
               and not r.kind.endswith("sub") for r in rows)                  # the all-ones carry
    tab = S.table(dtype)
    lo = S.lo_exp(dtype)
    for r in rows:
        for pat, b in r.entries:
            assert L._finite(pat, dtype) and 0 <= b - lo < len(tab)
            assert L.value_units(tab[b - lo], dtype) == (1 << (b + L.U))
    assert sum(r.must_acc for r in rows) >= 8


@pytest.mark.parametrize("dtype", S.NARROW)
def test_traps_separate_the_two_roundings(dtype):
    traps = S.trap_rows(dtype)
    assert len(traps) >= 8
    for r in traps:
        depth = int(r.kind.split(":")[1])
        assert 56 <= depth <= 100
        assert r.want == L.round_to(r.T, dtype) != L.double_then_cast(r.T, dtype)
        assert r.must_acc
    if dtype == "float16":      # the head is two float16 values, the perturbation the smallest subnormal squared
        assert all(len(r.entries) == 3 and r.entries[-1][1] == -24 and abs(r.T).bit_length() - 1 - L.U in (14, 15)
                   for r in traps)


def test_row_total_pairs_and_alpha():
    """the exact total for every accepted pair, alpha included, in the fine unit"""
    for vt, xt in S.PAIRS:
        v = [L.encode(vt, False, L.U, (1 << (L.FORMATS[vt][0] - 1)) | 1), L.encode(vt, True, L.U - 2, 1 << (L.FORMATS[vt][0] - 1))]
        x = [L.encode(xt, False, L.U + 1, (1 << (L.FORMATS[xt][0] - 1)) | 1), L.encode(xt, False, L.U, 1 << (L.FORMATS[xt][0] - 1))]
        pv, px = L.FORMATS[vt][0] - 1, L.FORMATS[xt][0] - 1
        want = (Fraction(1) + Fraction(1, 1 << pv)) * 2 * (Fraction(1) + Fraction(1, 1 << px)) - Fraction(1, 4)
        assert Fraction(S.row_total(v, vt, x, xt), 1 << S.UF) == want
        assert Fraction(S.row_total(v, vt, x, xt, alpha=0.5), 1 << S.UF) == want / 2
    # a rounded alpha: fl64(0.3 * 3) is not 0.9
    t = S.row_total([L.encode("float32", False, L.U, 1 << 23)], "float32", [L.encode("float32", False, L.U + 1, 3 << 22)],
                    "float32", alpha=0.3)
    assert Fraction(t, 1 << S.UF) == Fraction(np.float64(0.3) * np.float64(3.0))


def _check(ex, res, bound, dtype, must_refuse=False):
    got = ex.round_interval_host(res, bound, dtype)
    lo, hi = S.endpoint_patterns(res, bound, dtype)
    if got is not None:
        assert got == lo == hi, (dtype, res, bound, got, lo, hi)             # sound: both ends round to it
    assert not (must_refuse and got is not None), (dtype, res, bound)
    if res != 0.0:
        p, lower, upper = S.cell(Fraction(res), dtype)
        a, b = abs(Fraction(res)), Fraction(bound)
        far = a - lower > 4 * b and (upper is None or upper - a > 4 * b)
        if far:
            assert got is not None, (dtype, res, bound)                     # complete at the margin
            assert got == (p | (S.sign_bit(dtype) if res < 0 else 0))
    return got


@pytest.mark.parametrize("dtype", S.NARROW)
def test_round_interval_on_planted_and_trap_totals(ex, dtype):
    """res = RN64(T) with the true |T - res| as the bound: never a pattern other than round_to(T); 0 on every trap and on
    every tie with bound > 0"""
    decided = 0
    for r in S.all_rows(dtype):
        if r.T == 0:
            assert ex.round_interval_host(0.0, 0.0, dtype) == 0
            continue
        res, b = S.double_of(r.T)
        kind = r.kind.split(":")[0]
        near_tie = kind in ("tie+u", "tie-u", "trap", "half_min+u", "half_min-u", "below_overflow", "above_overflow")
        got = _check(ex, res, b, dtype, must_refuse=b > 0 and near_tie)
        if got is not None:
            assert got == r.want, r
            decided += 1
        if b == 0:
            assert got == r.want, r              # an exact sum is decided here, ties (to even) included
    assert decided > 50


@pytest.mark.parametrize("dtype", S.NARROW + ("float64",))
def test_round_interval_refuses_what_it_cannot_know(ex, dtype):
    for res, b in ((float("inf"), 0.0), (float("nan"), 0.0), (1.0, float("nan")), (1.0, -1.0), (1.0, float("inf")),
                   (0.0, 1e-300)):
        assert ex.round_interval_host(res, b, dtype) is None
    assert ex.round_interval_host(0.0, 0.0, dtype) == 0
    assert ex.round_interval_host(-1.0, 0.0, dtype) == L.round_to(-(1 << L.U), dtype)
    with pytest.raises(TypeError):
        ex.round_interval_host(1.0, 0.0, "int32")
    import ctypes
    assert ex.load_library().exblas_round_interval_host(1.0, 0.0, 9, ctypes.byref(ctypes.c_uint64())) < 0
    assert ex.load_library().exblas_round_interval_host(1.0, 0.0, 1, None) < 0


def test_round_interval_float64(ex):
    """float64: the spacing test of the fp64 kernels -- sound (the bound stays below half the distance to a neighbour)"""
    for res in (1.0, 1.5, -3.0, 2.0 ** -900, 2.0 ** 1000):
        ulp = np.spacing(abs(res))
        pat = int(np.array([res]).view(np.uint64)[0])
        assert ex.round_interval_host(res, 0.0, "float64") == pat
        assert ex.round_interval_host(res, ulp / 16, "float64") == pat
        assert ex.round_interval_host(res, ulp / 2, "float64") is None
    assert ex.round_interval_host(1.0, 2.0 ** -54, "float64") is None       # below a power of two the spacing halves
    assert ex.round_interval_host(1.0, 2.0 ** -56, "float64") == int(np.array([1.0]).view(np.uint64)[0])


@pytest.mark.parametrize("dtype", S.NARROW)
def test_round_interval_random(ex, dtype):
    """seeded random (res, bound): the whole exponent range of the format, its subnormals, the overflow threshold, values
    next to boundaries, bounds from 0 to beyond a quantum"""
    prec, emin, emax, width = L.FORMATS[dtype]
    rng = np.random.default_rng([17, prec])
    n, certified, refused = 4000, 0, 0
    for i in range(n):
        mode = i % 4
        if mode == 0:                                   # anywhere, subnormal and overflow ranges included
            e = int(rng.integers(emin - prec - 6, emax + 4))
            res = float(np.ldexp(1.0 + rng.random(), e))
        elif mode == 1:                                 # next to a rounding boundary of the format
            e = int(rng.integers(emin - prec + 1, emax + 1))
            q = max(e, emin) - (prec - 1)
            m = int(rng.integers(1 << (prec - 1), 1 << prec)) if e >= emin else int(rng.integers(0, 1 << (prec - 1)))
            res = float(np.ldexp(m + 0.5, q))
            k = int(rng.integers(-3, 4))
            for _ in range(abs(k)):
                res = float(np.nextafter(res, np.inf if k > 0 else 0.0))
        elif mode == 2:                                 # around the overflow threshold
            res = float(np.ldexp(2.0 - 2.0 ** -prec, emax)) * (1.0 + float(rng.integers(-4, 5)) * 2.0 ** -50)
        else:                                           # around zero and the smallest subnormal
            res = float(np.ldexp(rng.random() * 3, emin - prec))
        if rng.integers(2):
            res = -res
        if res == 0.0:
            continue
        choice = int(rng.integers(5))
        bound = 0.0 if choice == 0 else abs(res) * float(2.0 ** -int(rng.integers(1, 70)))
        if choice == 4:
            bound = float(np.spacing(abs(res))) * float(rng.integers(1, 4))
        got = _check(ex, res, bound, dtype)
        certified += got is not None
        refused += got is None
    assert certified > n // 4 and refused > n // 20


@pytest.mark.parametrize("dtype", L.ALL)
def test_round_window_is_round_digits(ex, dtype):
    """the accumulator rounding of the narrow products (leading bit, 64 bits, sticky: round_window_host) against the integer
    model and the digit walk (round_digits_host): every planted and trap total of the format, the row totals of the sparse
    cases, and totals with the leading bit at every position of the 68 digits"""
    totals = [c.T for c in L.planted(dtype)] + L.random_totals(31, per_position=1)
    if dtype in S.NARROW:
        totals += [t[0] for t in L.traps(dtype)] + [r.T for r in S.all_rows(dtype)]
    for T in totals:
        d = L.digits_of(T)
        got = ex.round_window_host(d, dtype)
        assert got == L.round_to(T, dtype) == ex.round_digits_host(d, dtype), (dtype, T)
    with pytest.raises(ValueError):
        ex.round_window_host(np.zeros(67, dtype=np.int64), dtype)
    assert ex.load_library().exblas_round_window_host(None, 1, None) == 1
