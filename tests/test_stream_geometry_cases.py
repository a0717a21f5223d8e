"""CPU suite: tests/stream_geometry_cases.py is held to its own claims -- every seam class of the streaming ExSUM / ExDOT
loops is in every geometry's plan for every variant (or is shown to be out of reach there), the data families spill or
do not spill as they are meant to, the lone-element totals decode, and the expected totals are the exact sums."""
from fractions import Fraction

import numpy as np
import pytest

import stream_geometry_cases as G
from helpers import exact_int_from_canon, exact_sum_int

NUM_CUS = (64, 256, 304)

# The only classes a plan may lack, and why; each is checked below to be out of reach by a scan over every size.
#   reentry, reentry3  a workgroup needs 69 (200) tiles to meet the expansion a second (third) time after its first
#                  spill: within 3.2M doubles only grids up to 22 (7) can, and at the cap these geometries have 63 or more
#   tiles2, tiles3 below the cap the grid grows with n (one tile each); at the cap of a small grid a workgroup has dozens
#   tiles3, tiles4 default geometry: three or four rounds of a grid of 511 .. 1217 workgroups are beyond 3.2M doubles
#   both_exits     needs two workgroups
#   slots2, slots3, trips2  strided kernels at a small grid: the grid is only small from n = num_cu x 256 on, many trips
#   slots4, last4, trips2, trips3  strided kernels at the default grid: 4T and 8T elements at inc >= 2 are beyond 3.2M
EXCUSABLE = {"vector": {"reentry", "reentry3", "tiles2", "tiles3", "tiles4", "both_exits"},
             "strided": {"slots2", "slots3", "slots4", "last4", "trips2", "trips3"}}


@pytest.fixture(scope="module")
def plans():
    return {(cu, g): G.build_plan(cu, g) for cu in NUM_CUS for g in G.GEOMETRY_NAMES}


_REACH = {}


def _reachable_vector(num_cu, geometry, routine, knob):
    """every seam class some size within the limit reaches: every tile count; beyond the first tiles, where the grid no
    longer depends on the remainder, three remainders and two head / tail pairs stand for all"""
    key = (num_cu, geometry, routine, knob)
    if key in _REACH:
        return _REACH[key]
    env = G.geometries(num_cu)[geometry]
    out = set()
    for nt in range(0, G.LIMIT // G.TILE + 1):
        for rem in (G.REMAINDERS if nt <= 8 else (0, 257, 1023)):
            for head, tail in (((0, 0), (0, 1), (1, 0), (1, 1)) if nt <= 8 else ((0, 0), (1, 1))):
                if head and routine == G.DOT:
                    continue
                n = head + 2 * (nt * G.TILE_V + rem) + tail
                if 0 < n <= G.LIMIT - 2:
                    grid = G.launch_model(num_cu, env, routine, n, fpe=knob)[1]
                    s = G.seams(n, head, grid)
                    out |= G.seam_classes(s)
                    for attempt, name in ((2, "reentry"), (3, "reentry3")):
                        if G.reentry_possible(grid, s["ntiles"], attempt):       # (any grid: the plan's limit of 4 is its choice)
                            out.add(name)
    _REACH[key] = out
    return out


def _reachable_strided(num_cu, env, routine, inc):
    out = set()
    nmax = (G.LIMIT - 2) // inc
    cap_n = num_cu * int(env.get("EXBLAS_BLOCKS_PER_CU", 8)) * G.BLOCK
    T = G.launch_model(num_cu, env, routine, cap_n, aligned=False, strided=True)[1] * G.BLOCK
    ns = set(range(1, 1200)) | {nmax}
    ns |= {m * T + d for m in range(1, nmax // T + 2) for d in (-1, 0, 1)}
    for n in ns:
        if 0 < n <= nmax:
            grid = G.launch_model(num_cu, env, routine, n, aligned=False, strided=True)[1]
            out |= G.strided_classes(G.seams_strided(n, grid))
    return out


@pytest.mark.parametrize("num_cu", NUM_CUS)
@pytest.mark.parametrize("geometry", G.GEOMETRY_NAMES)
def test_every_seam_class_is_in_every_plan(plans, num_cu, geometry):
    env = G.geometries(num_cu)[geometry]
    entries, coverage = plans[num_cu, geometry]
    for routine in (G.SUM, G.DOT):
        for var, held in coverage[routine, "vector"].items():
            knob = 0 if (routine == G.SUM and var[0] < 2) else 8
            missing = (G.all_vector_classes(routine) | {"reentry", "reentry3"}) - held
            assert missing <= EXCUSABLE["vector"], (geometry, routine, var, missing)
            if missing:
                reach = _reachable_vector(num_cu, geometry, routine, knob)
                assert not (missing & reach), (geometry, routine, var, "in reach but not planned", missing & reach)
        incs = (2, 3) if routine == G.SUM else (1, 2, 3)
        reach = set().union(*[_reachable_strided(num_cu, env, routine, inc) for inc in incs])
        for var, held in coverage[routine, "strided"].items():
            missing = G.all_strided_classes() - held
            assert missing <= EXCUSABLE["strided"], (geometry, routine, var, missing)
            assert not (missing & reach), (geometry, routine, var, "in reach but not planned", missing & reach)
    # the coverage table is what the entries hold, not what the builder says
    for routine in (G.SUM, G.DOT):
        seen = {v: set() for v in G.VARIANTS[routine]}
        for e in entries:
            if e["routine"] != routine or e["kind"] != "plain":
                continue
            kernel, grid = G.entry_launch(num_cu, env, e)
            if kernel in (G.K_EXSUM, G.K_EXDOT):
                s = G.seams(e["n"], e["offa"] & 1 if routine == G.SUM else 0, grid)
                seen[e["fpe"], bool(e["ee"])] |= G.seam_classes(s)
                if e["family"] == G.WTN:
                    assert grid <= 4 and G.reentry_possible(grid, s["ntiles"]) and e["wtn"] == G.WTN_TILES * grid * G.TILE
                    seen[e["fpe"], bool(e["ee"])].add("reentry")
                    if G.reentry_possible(grid, s["ntiles"], 3):
                        seen[e["fpe"], bool(e["ee"])].add("reentry3")
        for var, held in coverage[routine, "vector"].items():
            assert held <= seen[var], (geometry, routine, var, held - seen[var])
    # sizes: within the limit, about 150 vector sizes per routine, lone cases for every variant
    assert G.plan_length(entries) <= G.LIMIT
    for routine in (G.SUM, G.DOT):
        sizes = {(e["n"], e["offa"]) for e in entries if e["routine"] == routine and e["kind"] == "plain"
                 and G.entry_launch(num_cu, env, e)[0] in (G.K_EXSUM, G.K_EXDOT)}
        assert 100 <= len(sizes) <= 260, (geometry, routine, len(sizes))
        lone = {(e["fpe"], bool(e["ee"])) for e in entries if e["routine"] == routine and e["kind"] == "lone" and e["inca"] == 1}
        assert lone == set(G.VARIANTS[routine])
    assert len(entries) <= 2200


@pytest.mark.parametrize("num_cu", NUM_CUS)
def test_issue_geometry_table(num_cu):
    """the grids the geometries are named after, from n = num_cu x 2048 on"""
    geo = G.geometries(num_cu)
    n = (num_cu + 40) * G.TILE
    want = {"one_per_cu": (num_cu - 1 if num_cu % 2 == 0 else num_cu, num_cu), "three_wg": (3, 3), "four_wg": (4, 4), "one_wg": (1, 1)}
    for name, (gs, gd) in want.items():
        assert G.launch_model(num_cu, geo[name], G.SUM, n) == (G.K_EXSUM, gs)
        assert G.launch_model(num_cu, geo[name], G.DOT, n) == (G.K_EXDOT, gd)
    assert G.launch_model(num_cu, geo["default"], G.SUM, 4 * num_cu * G.TILE) == (G.K_EXSUM, 2 * num_cu - 1)
    assert G.launch_model(num_cu, geo["default"], G.SUM, 4 * num_cu * G.TILE, fpe=0) == (G.K_EXSUM, 3 * num_cu - 1 + num_cu % 2)
    assert G.launch_model(num_cu, geo["default"], G.DOT, 5 * num_cu * G.TILE) == (G.K_EXDOT, 4 * num_cu + 1)
    # below the cap of 4 per compute unit: one workgroup per tile, made odd above num_cu
    assert G.launch_model(num_cu, geo["default"], G.DOT, 300 * G.TILE)[1] == {64: 257, 256: 301, 304: 300}[num_cu]
    assert G.launch_model(num_cu, geo["default"], G.DOT, 1000, aligned=False)[0] == G.K_EXDOT_STRIDED
    assert G.launch_model(num_cu, geo["default"], G.SUM, 1000, strided=True) == (G.K_EXSUM_STRIDED, 4)
    assert [G.env_ngroups(geo[g]) for g in G.GEOMETRY_NAMES] == [32, 32, 1000, 3, 1]


def test_seams_of_the_sizes_the_issue_names():
    # 256 .. 262 tiles at a grid of 3: 85 / 86 tiles each, both exits in one launch
    both = [G.seams(nt * G.TILE, 0, 3) for nt in range(256, 263)]
    assert all(s["tile_counts"] <= {85, 86, 87, 88} for s in both) and any(s["exit_first"] and s["exit_second"] for s in both)
    # a remainder of 1023 vectors: two strides at a grid of 3, four at a grid of 1
    assert G.seams(2 * 1023, 0, 3)["rem_strides"] == 2 and G.seams(2 * 1023, 0, 1)["rem_strides"] == 4
    # one workgroup per compute unit (255): 1 -> 2, 2 -> 3, 3 -> 4 tiles at 255, 510, 765 tiles
    for k in (1, 2, 3):
        assert G.seams(255 * k * G.TILE, 0, 255)["tile_counts"] == {k}
        assert G.seams((255 * k + 1) * G.TILE, 0, 255)["tile_counts"] == {k, k + 1}
    s = G.seams(1 + 2 * (5 * 1024 + 300) + 1, 1, 4)
    assert (s["ntiles"], s["rem"], s["head"], s["tail"], s["tile_counts"], s["idle"]) == (5, 300, 1, 1, {1, 2}, False)
    assert G.seams(2 * 1024, 0, 7)["idle"] and G.seams(100, 1, 1)["ntiles"] == 0
    # strided: T = grid x 256
    assert G.seams_strided(768, 3) == {"slots": 1, "last_slots": 1, "trips": 1, "edge": "0"}
    assert G.seams_strided(4 * 768 + 1, 3) == {"slots": 4, "last_slots": 1, "trips": 2, "edge": "p1"}
    assert G.seams_strided(4 * 768 - 1, 3) == {"slots": 4, "last_slots": 4, "trips": 1, "edge": "m1"}


@pytest.fixture(scope="module")
def small_data():
    return G.Data((G.THIRD_ATTEMPT_TILES * 4 + 5) * G.TILE)


def test_a_longer_buffer_begins_with_the_shorter_one(small_data):
    """what the tests below show of the families holds for the buffers of every plan"""
    longer = G.Data(small_data.length + 5 * G.TILE)
    for fam in (G.NARROW, G.WIDE):
        for field in ("x", "y", "k"):
            assert (getattr(longer.fam[fam], field)[:small_data.length] == getattr(small_data.fam[fam], field)).all()


def _attempts(states):
    """(tile index, state) of the tiles that tried the expansion"""
    return [(i, s) for i, s in enumerate(states) if s != "bypassed"]


@pytest.mark.parametrize("nfpe", [2, 3, 4, 6, 8])
def test_families_spill_as_meant(small_data, nfpe):
    """A plain TwoSum cascade of one wavefront under the kernels' bypass rule, workgroup 1 of 3, misaligned head.
    wide: residues outlive the expansion within four tiles, whatever its size.  narrow: never."""
    grid, nt = 3, G.SECOND_ATTEMPT_TILES * 3 + 3
    streams = {f: G.wave_stream(small_data.operand(f, "x"), 1, grid, 1, nt) for f in (G.NARROW, G.WIDE)}
    states, _ = G.cascade_states(streams[G.NARROW], nfpe)
    assert set(states) == {"absorbed"} and len(states) == 70
    states, _ = G.cascade_states(streams[G.WIDE], nfpe)
    assert "spilled" in states[:4]
    first = states.index("spilled")
    assert states[first + 1:first + 1 + G.BYPASS_MIN] == ["bypassed"] * G.BYPASS_MIN


@pytest.mark.parametrize("grid", [1, 3, 4])
def test_wide_then_narrow_is_absorbed_after_a_bypass(small_data, grid):
    """wide_then_narrow, every wavefront of every workgroup at the share the plans give it (200 tiles each and three more,
    misaligned head).  The first spill comes within four tiles; 64 tiles later the expansion is tried again on narrow
    data with the stale wide terms still in it.  The narrow elements displace the stale terms of the scales below 2^0,
    which leave as residues: that attempt spills for every size and the span doubles to 127.  The third attempt, 128
    tiles on, meets an expansion whose low terms have made room:
      N = 8  every wavefront absorbs it and every later tile (the span is reset), stale wide and new narrow terms
             sharing the expansion until the flush;
      N = 6  some wavefronts absorb it, the others spill a third time;
      N <= 4 no wavefront does: a small expansion is full of stale terms above the narrow ones.  These variants are
             EXCUSED from the absorbed re-entry; they take the stale re-entries and the doubling span."""
    nt = G.THIRD_ATTEMPT_TILES * grid + 3
    assert G.reentry_possible(grid, nt, 3) and (nt + 1) * G.TILE + 2 <= min(G.LIMIT, small_data.length)
    x = small_data.operand(G.WTN, "x", wtn=G.WTN_TILES * grid * G.TILE)
    absorbed = {n: 0 for n in (2, 3, 4, 6, 8)}
    waves = 0
    for wg in range(grid):
        for wave in range(4):
            stream = G.wave_stream(x, 1, grid, wg, nt, wave)
            waves += 1
            for nfpe in absorbed:
                states, stale = G.cascade_states(stream, nfpe)
                tries = _attempts(states)
                first = next(k for k, (_, s) in enumerate(tries) if s == "spilled")
                (i1, s1), (i2, s2), (i3, s3) = tries[first:first + 3]
                assert i1 < 4 and i2 == i1 + 1 + G.BYPASS_MIN and i3 == i2 + 2 * G.BYPASS_MIN + 2, (nfpe, wg, wave, tries[:6])
                assert i2 >= G.WTN_TILES and s2 == "spilled" and stale[i2] and stale[i3]      # narrow data, stale expansion
                if s3 == "absorbed":
                    assert all(s == "absorbed" for s in states[i3:]) and len(states) > i3 + 3
                    absorbed[nfpe] += 1
    assert absorbed[8] == waves and 0 < absorbed[6] <= waves and absorbed[2] == absorbed[3] == absorbed[4] == 0, (absorbed, waves)


def test_lone_totals_decode():
    names = [nm for nm, _ in G.lone_positions(1 + 2 * (9 * 1024 + 1023) + 1, 1, 3)]
    assert names == ["head", "after_head", "tile0_last", "round1_first", "round1_last", "last_full_first", "last_full_last",
                     "rem_first", "rem_last", "rem_stride2_first", "tail"]
    tot = G.lone_total(len(names))
    counts, report = G.lone_decode(tot, names)
    assert counts == [1] * len(names) and report == "every seam once"
    one = lambda j: (1 << (G.LONE_BITS * j)) << 1074                               # noqa: E731
    # the second remainder stride skipped; the tail added by each of 767 workgroups... each failure names its seam
    assert G.lone_decode(tot - one(9), names)[1] == "rem_stride2_first counted 0 times"
    assert G.lone_decode(tot + 766 * one(10), names)[1] == "tail counted 767 times"
    assert G.lone_decode(tot + one(2) - one(5), names)[1] == "tile0_last counted 2 times; last_full_first counted 0 times"
    assert G.lone_decode(tot + 1, names)[0] is None and G.lone_decode(-tot, names)[0] is None
    # positions are distinct, inside the case, and where the kernel's index arithmetic puts them
    pos = dict(G.lone_positions(1 + 2 * (9 * 1024 + 1023) + 1, 1, 3))
    assert pos["round1_first"] == 1 + 2 * 3 * 1024 and pos["last_full_last"] == 2 * 9 * 1024 and pos["tail"] == 2 * (9 * 1024 + 1023) + 1
    assert pos["rem_stride2_first"] == 1 + 2 * (9 * 1024 + 768) and len(set(pos.values())) == len(pos)
    spos = dict(G.lone_positions_strided(5 * 768 + 1, 3))
    assert spos == {"first": 0, "slot0_last": 767, "slot1_first": 768, "slot2_first": 1536, "slot3_first": 2304,
                    "trip0_last": 3071, "trip1_first": 3072, "last": 3840}


def test_lone_background_cancels_exactly(small_data):
    """the operands lone_build makes sum (ExSUM) / multiply and sum (ExDOT) to the seam values alone, and so does every
    double2 of the background on its own: a loop that drops or repeats whole vectors cannot hide behind the background"""
    n, grid = 1 + 2 * (5 * 1024 + 1023) + 1, 3
    for head in (1, 0):
        named = G.lone_positions(n, head, grid)
        pos, vals = [p for _, p in named], G.lone_values(len(named))
        fam = small_data.fam[G.WIDE]
        a = G.lone_build(np, fam.x, n, head, pos, vals, True)
        assert exact_sum_int(a) == G.lone_total(len(pos))
        ya = G.lone_build(np, fam.y, n, head, pos, vals, True)
        xb = G.lone_build(np, fam.x, n, head, pos, [1.0] * len(pos), False)
        tot = sum(Fraction(p) * Fraction(q) for p, q in zip(ya.tolist(), xb.tolist()))
        assert tot * 2 ** 1074 == G.lone_total(len(pos)) and all(ya[p] * xb[p] == v for p, v in zip(pos, vals))
        m = (n - head) // 2
        seam_vec = {(p - head) // 2 for p in pos if p >= head}
        quiet = np.array([q not in seam_vec for q in range(m)])
        va, vy, vx = (t[head:head + 2 * m].reshape(m, 2) for t in (a, ya, xb))
        assert (va[quiet, 0] == -va[quiet, 1]).all() and (va[quiet, 0] != 0).all()
        assert (vy[quiet, 0] == -vy[quiet, 1]).all() and (vx[quiet, 0] == vx[quiet, 1]).all() and (vx[quiet, 0] != 0).all()
        assert a[n - 1] == vals[-1] and (head == 0 or a[0] == vals[0])            # the scalar ends carry seams only


def _python_total(data, e):
    """the total of a short entry, element by element in Python integers"""
    if e["family"] == G.WTN:
        x, y = data.operand(G.WTN, "x", e["wtn"]), data.operand(G.WTN, "y", e["wtn"])
    else:
        x, y = data.fam[e["family"]].x, data.fam[e["family"]].y
    n = 3 * e["n"] if e["kind"] == "acc" else e["n"]
    xs = x[e["offb"] if e["routine"] == G.DOT else e["offa"]:][::e["incb"] if e["routine"] == G.DOT else e["inca"]][:n]
    if e["routine"] == G.SUM:
        return exact_sum_int(xs)
    ys = y[e["offa"]:][::e["inca"]][:n]
    tot = 0
    for p, q in zip(ys.tolist(), xs.tolist()):
        tot += Fraction(p) * Fraction(q)
    tot *= 2 ** 1074
    assert tot.denominator == 1
    return tot.numerator


def test_expected_totals_are_the_exact_sums(small_data):
    mk = lambda **kw: dict(dict(kind="plain", routine=G.SUM, family=G.WIDE, fpe=8, ee=1, n=0, inca=1, incb=1, offa=0,   # noqa: E731
                                offb=0, wtn=0, pos=[]), **kw)
    cases = [mk(n=5000, offa=1, offb=1), mk(n=4097, offa=2047, offb=2047), mk(n=300, offa=5, offb=5, family=G.NARROW),
             mk(n=3000, inca=3, offa=1), mk(n=9000, family=G.WTN, wtn=4096, offa=1, offb=1),
             mk(n=9000, family=G.WTN, wtn=4096, offa=5000, offb=5000), mk(n=2100, kind="acc", offa=3, offb=3),
             mk(routine=G.DOT, n=4500, offa=2, offb=2), mk(routine=G.DOT, n=2500, family=G.NARROW),
             mk(routine=G.DOT, n=2000, inca=3, incb=1, offa=1, offb=1), mk(routine=G.DOT, n=2000, offa=1, offb=0),
             mk(routine=G.DOT, n=2000, offa=0, offb=1), mk(routine=G.DOT, n=7000, family=G.WTN, wtn=6144),
             mk(routine=G.DOT, n=1500, kind="acc", family=G.NARROW)]
    memo = {}
    for e in cases:
        assert G.expected_total(small_data, e, memo) == _python_total(small_data, e), e
    assert G.exact_double(3 << 1074) == 3.0 and G.exact_double((1 << 1127) + (1 << 1074)) == 2.0 ** 53
    assert G.exact_double((1 << 1127) + (3 << 1074)) == 2.0 ** 53 + 4


def test_expected_totals_agree_with_the_oracle(small_data, oracle):
    """full-length cases against the C oracle's superaccumulator (its canonical limbs are in units of 2^-1092)"""
    n = 212 * G.TILE - 3
    for fam in (G.NARROW, G.WIDE):
        f = small_data.fam[fam]
        r, limbs = oracle.exsum(f.x[1:1 + n], 0, False, limbs=True)
        tot = small_data.total(G.SUM, fam, 1, n)
        assert exact_int_from_canon(limbs) == tot << 18 and r == G.exact_double(tot)
        r, limbs = oracle.exdot(f.y[2:2 + n], f.x[2:2 + n], 0, False, limbs=True)
        tot = small_data.total(G.DOT, fam, 2, n)
        assert exact_int_from_canon(limbs) == tot << 18 and r == G.exact_double(tot)
