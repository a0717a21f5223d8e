"""The builders of tests/gemm_decision_cases.py: the spans, top exponents and positions they claim, the bound that makes
the int64 base result exact, the derivation of non-finite outputs, and the coverage of the case tables.  CPU only."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_cases as X
import gemm_decision_cases as D
from helpers import bits

ALL_K = sorted(set(D.CONTIG_K) | set(D.STRIDED_K))


def _as_ints(vec):
    """finite doubles -> Python integers in units of 2^-1074, through Fraction (independent of D._int_exp)"""
    return [int(Fraction(float(x)) * 2 ** 1074) for x in vec]


def _span(vec):
    return X.span_bits(np.array([_as_ints(vec)], dtype=object), 1)


def _top(vec):
    return max(abs(i).bit_length() for i in _as_ints(vec)) - 1 - 1074


def test_seam_geometry_is_what_the_launch_code_gives():
    assert [D.contig_positions(k) for k in D.CONTIG_K] == [[0], [0, 254], [0, 255, 256, 1023, 1024],
                                                           [0, 255, 256, 1023, 1024, 2048]]
    assert [(D.ysplit(k), D.slice_len(k)) for k in D.STRIDED_K] == [(1, 255), (8, 33), (32, 65)]
    assert [D.strided_positions(k) for k in D.STRIDED_K] == [[0, 254], [0, 32, 33, 231, 256], [0, 64, 65, 2015, 2048]]
    for k in D.STRIDED_K:                                   # the last slice that holds anything, walked as the kernel walks
        per, ys = D.slice_len(k), D.ysplit(k)
        starts = [y * per for y in range(ys) if y * per < k]
        assert starts[-1] in D.strided_positions(k) and min(k, starts[-1] + per) - 1 == k - 1
    assert [D.contiguous(o, t) for o, t in D.LAYOUTS] == [True, False, False, True]
    assert sorted((t if o == "A" else D.partner_trans(o, t), D.partner_trans(o, t) if o == "A" else t)
                  for o, t in D.LAYOUTS) == [("N", "N"), ("N", "T"), ("T", "N"), ("T", "T")]
    assert len(D.SEAM_IDS) == 14
    assert D.VECTORS == ((1, 0), (257, 0), (257, 255), (257, 256))


@pytest.mark.parametrize("k", ALL_K)
def test_base_is_exact_in_int64_and_inside_every_domain(k):
    b = D.base(k)
    mant = max(int(np.abs(b.P).max()).bit_length(), int(np.abs(b.Q).max()).bit_length())
    assert mant <= 20 and k <= 2049 and 2 * mant + (k - 1).bit_length() <= 52      # every sum is below 2^52
    assert int(np.abs(b.c).max()) < 2 ** 52
    rows = [0, 255, 256]
    assert (X.gemm_exact(X.obj(b.P[rows]), X.obj(b.Q.T)) == X.obj(b.c[rows])).all()
    assert (bits(b.want) == bits(b.c.astype(np.float64))).all()
    assert (b.P != 0).all() and np.abs(b.P).max() <= 127 and np.abs(b.Q).max() <= 127
    for l in b.probed:
        assert tuple(b.Q[:, l]) == D.PARTNER_AT_PROBE
    assert set(D.contig_positions(k)) | set(D.strided_positions(k)) == set(b.probed)
    if k > 1:
        assert (b.P[:, 1] % 2 == 1).all() and 1 not in b.probed
        assert (b.Q[:, 2] == b.Q[:, 3]).all() and not {2, 3} & set(b.probed)
    assert b.bits_q == max(_span(q) for q in b.Qf)
    assert 1 <= b.bits_p[1] <= b.bits_p[257] <= 7 and b.bits_q <= 7
    for v in (0, 255, 256):
        assert D.vector_facts(b.Pf[v]) == (_span(b.Pf[v]), _top(b.Pf[v]), False) and b.spans[v] == _span(b.Pf[v])
    assert max(b.spans) == b.bits_p[257] and b.spans[0] == b.bits_p[1] and len(b.spans) == 257


def test_exact_dot_and_derive():
    rng = np.random.default_rng(5)
    x = np.ldexp(rng.integers(-2 ** 52, 2 ** 52, 40).astype(np.float64), rng.integers(-300, 300, 40))
    y = np.ldexp(rng.integers(-2 ** 52, 2 ** 52, 40).astype(np.float64), rng.integers(-300, 300, 40))
    x[3], y[7] = 0.0, -0.0
    x[9], y[9] = 3 * 2.0 ** -1074, 4.0
    v, e = D.exact_dot(x, y)
    assert Fraction(v) * Fraction(2) ** e == sum(Fraction(float(p)) * Fraction(float(q)) for p, q in zip(x, y))
    assert D.derive(x, y) == float(Fraction(v) * Fraction(2) ** e)
    assert D.derive([D.SUBNORMAL, 5.0, -5.0], [4.0, 9.0, 9.0]) == 12 * 2.0 ** -1074
    assert math.isnan(D.derive([math.nan, 1.0], [0.0, 1.0]))
    assert math.isnan(D.derive([math.inf, 1.0], [0.0, 1.0]))            # Inf x 0
    assert math.isnan(D.derive([math.inf, math.inf], [1.0, -1.0]))      # both infinities
    assert D.derive([math.inf, 2.0], [-2.0, 1e300]) == -math.inf
    assert D.derive([-math.inf, -math.inf], [-2.0, -3.0]) == math.inf
    assert D.derive([1.0, -1.0], [3.0, 3.0]) == 0.0 and not math.copysign(1.0, D.derive([1.0, -1.0], [3.0, 3.0])) < 0


def test_decision_rules():
    assert D.i8_digits(126, 7) == (16, 2) and D.i8_digits(127, 7) is None and D.i8_digits(7, 127) is None
    assert D.i8_digits(0, 7) == (1, 2) and D.i8_digits(61, 7) == (8, 2) and D.i8_digits(62, 7) == (8, 2)
    assert D.i8_digits(53, 53) == (7, 7) and D.i8_digits(55, 53) == (8, 8) and D.i8_digits(78, 70) == (10, 10) and D.i8_digits(70, 64) == (9, 9)
    assert D.i8_digits(86, 80) == (12, 12) and D.i8_digits(20, 7) == (3, 2)
    assert D.expected_info(3, 84, 7, 257) == [1, 4, 4] and D.expected_info(3, 7, 7, 257) == [1, 2, 2]
    assert D.expected_info(4, 0, 7, 257) == [4, 1, 7, X.crt_moduli_needed(1, 7, 257)]
    assert D.expected_info(4, 126, 7, 257)[:3] == [4, 126, 7]
    assert (D.I8_ERANGE, D.MFMA_ERANGE, D.I8_SPAN, D.MFMA_SPAN) == (300, 400, 126, 84)


@pytest.mark.parametrize("k", ALL_K)
def test_planted_vectors_are_what_they_claim(k):
    b = D.base(k)
    for v in (0, 255, 256):
        for pos in b.probed:
            for kind in D.FLAG_KINDS:
                vec = D.lone_special(b, v, pos, kind)
                assert D.vector_facts(vec) == (None, None, True)
                if kind == "subnormal":
                    assert abs(vec[pos]) == D.SUBNORMAL and 0 < abs(vec[pos]) < 2.0 ** -1022
                    rest = np.delete(vec, pos)
                    assert all(D.derive(rest, np.delete(q, pos)) == 0.0 for q in b.Qf)      # the rest cancels exactly
                    for j, q in enumerate(b.Qf):                                            # partners: 0 or a power of two >= 1
                        assert q[pos] == 0 or (abs(q[pos]) >= 1 and math.frexp(q[pos])[0] in (0.5, -0.5))
                        assert D.derive(vec, q) == vec[pos] * q[pos]
                else:
                    diff = np.flatnonzero(bits(vec) != bits(b.Pf[v]))
                    assert diff.tolist() == [pos] and not np.isfinite(vec[pos])
                    got = [D.derive(vec, q) for q in b.Qf]
                    sign = -1.0 if kind == "-inf" else 1.0
                    assert math.isnan(got[1]) and (math.isnan(got[0]) if kind == "nan" else got[0] == sign * math.inf)
                    assert math.isnan(got[2]) if kind == "nan" else got[2] == -sign * math.inf
            top, low = D.lone_setter(b, v, pos, "top"), D.lone_setter(b, v, pos, "low")
            for vec in (top, low):
                assert np.flatnonzero(bits(vec) != bits(b.Pf[v])).tolist() == [pos]
                assert D.vector_facts(vec) == (_span(vec), _top(vec), False)
            assert abs(top[pos]) == 2.0 ** 60 and _top(top) == 60 and np.abs(np.delete(top, pos)).max(initial=0) < 2 ** 8
            assert abs(low[pos]) == 3 * 2.0 ** -60 and _top(low) <= 6
            if k > 1:
                assert _span(top) == 61 and _span(low) == _top(np.delete(b.Pf[v], pos)) + 1 + 60
            else:
                assert _span(top) == 1 and _span(low) == 2
    for v in (0, 255, 256):
        for t in (300, -300, 301, -301, 400, -401):
            vec = D.scaled_vector(b, v, t)
            assert _top(vec) == t and _span(vec) == _span(b.Pf[v])
            assert all(abs(D.exact_dot(vec, q)[1]) < 900 for q in b.Qf)


def test_span_and_alpha_cases():
    b = D.base(257)
    for v in (0, 255, 256):
        for pos in b.probed:
            for nbits in (84, 85, 126, 127):
                vec = D.span_vector(b, v, pos, nbits)
                assert _span(vec) == nbits == D.vector_facts(vec)[0] and _top(vec) == nbits - 1
                assert D.seen_bits(b, 257, v, vec, "A") == (nbits, b.bits_q) and D.seen_bits(b, 257, v, vec, "B") == (b.bits_q, nbits)
                assert np.flatnonzero(bits(vec) != bits(b.Pf[v])).tolist() == [pos]
            cases = {name: (alpha, vec, ok) for name, alpha, vec, ok in D.alpha_cases(b, v, pos)}
            assert len(cases) == 11

            def seen(name):                                  # the vector as the scan sees it: fl(alpha a)
                with np.errstate(all="ignore"):
                    return D.vector_facts(cases[name][0] * cases[name][1])

            want_top = {"299 x 2": 300, "299 x 4": 301, "1.25 x 3": 300, "1.5 x 3": 301, "-299 / 2": -300, "-299 / 4": -301}
            for name, t in want_top.items():
                assert _top(cases[name][1]) == (299 if t > 0 else -299) and seen(name)[1:] == (t, False)
                assert cases[name][2] == (abs(t) <= D.I8_ERANGE)
                assert seen(name)[0] <= 10
            assert [cases[n][1][pos] / 2.0 ** 299 for n in ("1.25 x 3", "1.5 x 3")] == [1.25, 1.5]
            for name in ("overflow", "underflow", "zero x inf", "nan"):
                assert seen(name) == (None, None, True) and not cases[name][2]
            for name in ("overflow", "underflow"):                          # A itself is finite and normal
                assert (np.isfinite(cases[name][1]) & ((cases[name][1] == 0) | (np.abs(cases[name][1]) >= 2.0 ** -1022))).all()
            assert seen("zero") == (0, None, False) and cases["zero"][2]
            assert cases["overflow"][1][pos] == -2.0 ** 1000 and cases["underflow"][1][pos] * 2.0 ** -73 == 3 * 2.0 ** -1073


def test_with_vector_recomputes_only_what_the_vector_reaches():
    b = D.base(255)
    v, pos = 255, 254
    vec = D.lone_setter(b, v, pos, "top")
    for operand in ("A", "B"):
        w = D.with_vector(b, 257, v, vec, operand)
        w = w if operand == "A" else w.T
        keep = np.arange(257) != v
        assert (bits(w[keep]) == bits(b.want[keep])).all()
        full = [X.round_nearest_even(sum(Fraction(float(p)) * Fraction(float(q)) for p, q in zip(vec, qv))) for qv in b.Qf]
        assert w[v].tolist() == full and (bits(w[v]) != bits(b.want[v])).tolist() == [True, False, True]
    w3 = D.with_vector(b, 257, 0, b.Pf[0], "A", alpha=3.0)
    assert (w3 == 3.0 * b.want).all()
    assert D.with_vector(b, 1, 0, b.Pf[0], "B").shape == (3, 1)
    assert np.isnan(D.with_vector(b, 257, 0, b.Pf[0], "A", alpha=math.nan)).all()
    z = D.with_vector(b, 257, 3, D.lone_special(b, 3, 0, "+inf"), "A", alpha=0.0)
    assert np.isnan(z[3]).all() and (bits(np.delete(z, 3, axis=0)) == 0).all()
    c0 = D.c_template(4, 3, 1.0)
    assert (c0[:, 3:] == -7.0).all() and np.isnan(D.c_template(4, 3, 0.0)[:, :3]).all()
    s = np.arange(12.0).reshape(4, 3)
    assert (D.with_beta(s, 1.0, c0) == c0[:, :3] + s).all() and D.with_beta(s, 0.0, c0) is not None


@pytest.mark.parametrize("operand,trans,k", D.SEAM_IDS)
def test_probe_table_coverage(operand, trans, k):
    probes = D.seam_probes(operand, trans, k)
    pos = D.positions(operand, trans, k)
    assert len(probes) == 3 * len(pos) * len(D.VECTORS)
    for p in pos:
        here = [q for q in probes if q.pos == p]
        assert sorted(q.kind for q in here if q.kind in D.FLAG_KINDS) == sorted(D.FLAG_KINDS)    # every kind of flag
        for Vv in D.VECTORS:                                                                      # on every vector:
            kinds = [q.kind for q in here if (q.V, q.v) == Vv]
            assert len(kinds) == 3 and "top" in kinds and "low" in kinds and set(kinds) & set(D.FLAG_KINDS)
    for group in (D.FLAG_KINDS, ("top",), ("low",), ("top", "low")):
        assert {q.path for q in probes if q.kind in group} == {2, 4}, group
    assert {q.variant for q in probes} <= set(range(7)) and {q.beta for q in probes} == {0.0, 1.0}
    assert all(q.beta == 0.0 for q in probes if q.kind in D.FLAG_KINDS)
