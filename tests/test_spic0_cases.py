"""CPU suite: the ExSpIC0 model (spic0_cases.ic0_exact) against ExPOTRF's model and a naive restatement, its planted
classes, its sensitivity to wrong routines, the breakdown and defect cases, and the counter bounds the GPU tests rely on.
Nothing here needs a GPU."""
import math

import numpy as np
import pytest

import potrf_cases as P
import spic0_cases as C
from helpers import assert_bits as _same, bits as _bits


def _lower(csr, ll):
    """the lower triangle of the densified factor"""
    return np.tril(C.dense_of(csr[0], csr[1], ll))


@pytest.mark.parametrize("name", list(C.DENSE) + list(C.PLANTED))
def test_model_lower_triangle_is_potrf_exact_on_dense_and_planted_cases(name):
    csr = C.SOUND[name]()
    Gm = C.dense(C.DENSE[name])[1] if name in C.DENSE else C.planted(int(name[7:]))[1].G
    ll, i0, i1, _ = C.expected(name)
    R, info = P.potrf_exact(Gm, "L")
    assert (i0, i1, info) == (0, 0, 0)
    # a stored zero of the block pattern and the zero outside it: potrf_exact skips both, their totals are the same
    assert (_bits(_lower(csr, ll)) == _bits(np.tril(R))).all(), name


@pytest.mark.parametrize("name", C.NAIVE)
def test_model_agrees_with_the_naive_restatement(name):
    csr = C.SOUND[name]()
    _same(C.restate(*csr), C.expected(name)[0], name)


@pytest.mark.parametrize("name", list(C.SOUND))
def test_factor_is_mirrored_and_every_position_is_fixed(name):
    csr = C.SOUND[name]()
    ll = C.expected(name)[0]
    D = C.dense_of(csr[0], csr[1], ll)
    mask = C.dense_of(csr[0], csr[1], np.ones(len(ll))) != 0
    assert (mask == mask.T).all()
    assert (_bits(D[mask]) == _bits(D.T[mask])).all() or np.isnan(D[mask]).any()
    if name in C.HEALTHY:
        assert np.isfinite(ll).all() and (C.dense_of(csr[0], csr[1], ll).diagonal() > 0).all()


def test_planted_ties_and_near_ties_are_present_off_the_diagonal_and_on_it():
    tot = {"ties_l": 0, "ties_d": 0, "nears_l": 0, "nears_d": 0}
    for name in C.PLANTED:
        d = C.expected(name)[3]
        for k in tot:
            tot[k] += getattr(d, k)
        c = C.planted(int(name[7:]))[1]
        # every plant of potrf_cases is a stored entry of the block pattern with the class potrf_exact gives it
        csr = C.SOUND[name]()
        kinds = C.dense_of(csr[0], csr[1], d.kind.astype(np.float64))
        for r, col, cls, gap, want in c.plants:
            assert kinds[col, r] == c.kind[r, col], (name, r, col, cls)
    print(tot)
    assert tot["ties_l"] >= 50 and tot["nears_l"] >= 20 and tot["ties_d"] >= 2 and tot["nears_d"] >= 2, tot


@pytest.mark.parametrize("name", C.PLANTED)
def test_wrong_routines_differ_on_a_planted_entry(name):
    csr = C.SOUND[name]()
    want = C.expected(name)[0]
    for wrong in (dict(round_products=True), dict(rounder=C.round_away)):
        got = C.ic0_exact(*csr, **wrong)[0]
        assert (_bits(got) != _bits(want)).any(), (name, wrong)


@pytest.mark.parametrize("name", list(C.BREAKDOWN_INFO))
def test_breakdowns_have_their_info(name):
    ll, i0, i1, _ = C.expected(name)
    assert (i0, i1) == (0, C.BREAKDOWN_INFO[name])
    csr = C.SOUND[name]()
    r = i1 - 1
    d = int(csr[0][r]) + int(np.searchsorted(csr[1][int(csr[0][r]):int(csr[0][r + 1])], r))
    if name.startswith("breakdown"):
        rad = {"breakdown_zero": 0.0, "breakdown_neg": -1.0}[name]
        assert (ll[d] == 0.0) if rad == 0.0 else math.isnan(ll[d])
        assert not np.isfinite(ll[int(csr[0][r + 1]):]).all()          # the broken pivot travels on
        assert np.isfinite(ll[:int(csr[0][r])][csr[1][:int(csr[0][r])] <= np.repeat(np.arange(r), np.diff(csr[0][:r + 1]))]).all()
    else:
        assert math.isnan(ll[d])


def test_defects_have_their_info_and_phase_one_comes_first():
    for name, csr in C.defects().items():
        ll, i0, i1 = C.ic0_exact(*csr)
        assert i0 > 0 and i1 == 0 and (_bits(ll) == _bits(csr[2])).all(), name
        if name in C.DEFECT_INFO:
            assert i0 == C.DEFECT_INFO[name], (name, i0)
    crow, col, _ = C.defects()["phase 1 after a missing mirror"]
    assert C.mirror_defect(crow, col, 12) == 4 and C.structure(crow, col, 12) == 10


def test_values_above_the_diagonal_are_never_read():
    csr = C.SOUND["random"]()
    crow, col, val = csr
    rows = np.repeat(np.arange(len(crow) - 1), np.diff(crow))
    junk = val.copy()
    junk[col > rows] = np.nan
    _same(C.ic0_exact(crow, col, junk)[0], C.expected("random")[0], "NaN above the diagonal")
    assert (_bits(C.plain_ic0(crow, col, junk)) == _bits(C.plain_ic0(crow, col, val))).all()


@pytest.mark.parametrize("name", list(C.SOUND))
def test_the_model_meets_the_counter_bounds(name):
    """what the GPU test asserts of the counters, met by the model's own classes: out[0] + out[1] == owned entries,
    out[2] == terms, TIE <= out[1], and on healthy cases out[1] <= TIE + NEAR (a routine that rounds every CLEAR entry
    in registers and every other one from the accumulator meets both)"""
    csr = C.SOUND[name]()
    d = C.expected(name)[3]
    rows = np.repeat(np.arange(len(csr[0]) - 1), np.diff(csr[0]))
    owned = int((csr[1] <= rows).sum())
    assert d.owned == owned and d.terms > 0
    lowkinds = d.kind[csr[1] <= rows]
    assert (lowkinds > 0).all()                            # every owned entry is classified
    ideal_acc = int((lowkinds != C.CLEAR).sum())
    assert d.ties <= ideal_acc <= d.ties + d.nears
    print(name, "owned", owned, "terms", d.terms, "ties", d.ties, "nears", d.nears, "wide rows", d.wide, "ranged", d.ranged)
    if name in C.HEALTHY:
        assert d.ranged and d.nears + d.ties == ideal_acc


def test_plain_restatement_is_another_routine():
    """fpe = 1's fixed-order form rounds every product and every difference: it must differ somewhere"""
    csr = C.SOUND["stencil27"]()
    assert (_bits(C.plain_ic0(*csr)) != _bits(C.expected("stencil27")[0])).any()
