"""Sizes, data and expected totals that put every positional seam of the streaming ExSUM / ExDOT kernels
(exblas_amd/csrc/blas1_common.hip.h: k_blas1_stream and k_blas1_strided, here with the fp64 front ends SumF64 and DotF64
of blas1.hip) under test in every launch geometry.
Pure numpy / Python: no GPU, no oracle.  tests/test_stream_geometry_cases.py holds this module to its coverage claims,
tests/test_gpu_stream_geometry.py runs the plans (tests/stream_geometry_worker.py, one child process per geometry).

`launch_model` is a RESTATEMENT of the launchers' geometry rules at this commit.  Its only job is choosing sizes; the GPU
test asserts that the grid the library reports (exblas_last_blas1_info) equals the model's, so a change of geometry fails
with "update the model" instead of silently losing coverage.

Nothing here is measured and nothing has a tolerance: every total is an exact Python integer in units of 2^-1074."""
import json
from fractions import Fraction

import numpy as np

from helpers import FPE_VARIANTS_DOT, FPE_VARIANTS_SUM

BLOCK, U = 256, 4
TILE_V = BLOCK * U            # double2 vectors per tile
TILE = 2 * TILE_V             # doubles per tile (and per stream)
LIMIT = 3_200_000             # no operand is longer than this many doubles
BYPASS_MIN = 63               # fpe.hip.h: tiles that skip the expansion after the first spill
K_EXSUM, K_EXSUM_STRIDED, K_EXDOT, K_EXDOT_STRIDED = 1, 2, 3, 4
SUM, DOT = 0, 1
NARROW, WIDE, WTN = 0, 1, 2
FAMILIES = ("narrow", "wide", "wide_then_narrow")
NSCALES, SCALE_BITS, SCALE_ZERO = 12, 96, 5      # scale index s stands for 2^(96 (s - 5)): 2^-480 .. 2^576
WTN_TILES = 8                 # wide_then_narrow: this many wide tiles in every workgroup's share, narrow after
REMAINDERS = (0, 1, 255, 256, 257, 767, 768, 769, 1023)
VARIANTS = {SUM: list(FPE_VARIANTS_SUM), DOT: list(FPE_VARIANTS_DOT) + [(1, False), (2, False)]}   # dot 1, 2: N = 0


# ---------------------------------------------------------------------------------------------------------------------
# launch geometry (restatement of blas1_common.hip.h: grid_for, run_stream, run_strided, launch_blas1)
# ---------------------------------------------------------------------------------------------------------------------
def geometries(num_cu):
    """name -> environment of the child process"""
    one = {"EXBLAS_BPC_SUM": "1", "EXBLAS_BPC_DOT": "1", "EXBLAS_BPC_SA": "1", "EXBLAS_BLOCKS_PER_CU": "1"}
    return {
        "default": {},
        "one_per_cu": dict(one),
        "three_wg": dict(one, EXBLAS_GRID_ADJ=str(3 - num_cu), EXBLAS_NGROUPS="1000"),
        "four_wg": dict(one, EXBLAS_GRID_ADJ=str(4 - num_cu), EXBLAS_NGROUPS="3"),
        "one_wg": dict(one, EXBLAS_GRID_ADJ=str(1 - num_cu), EXBLAS_NGROUPS="1"),
    }


GEOMETRY_NAMES = ("default", "one_per_cu", "three_wg", "four_wg", "one_wg")


def env_ngroups(env):
    return max(1, int(env.get("EXBLAS_NGROUPS", 32)))


def _grid_for(num_cu, env, work, per_block, bpc):
    want = max(1, -(-work // per_block))
    cap = num_cu * bpc
    return max(1, cap + int(env.get("EXBLAS_GRID_ADJ", 0))) if want >= cap else want


def launch_model(num_cu, env, routine, n, aligned=True, strided=False, fpe=8):
    """(kernel, grid) of one ExSUM / ExDOT call of n > 0 elements.  RESTATEMENT of the launchers, see the module's
    docstring.  aligned: every operand pointer is a multiple of 16 (matters to ExDOT only); strided: an increment other
    than 1; fpe: ExSUM with fpe < 2 (superaccumulators only) has a resident-blocks knob of its own."""
    per_cu = int(env.get("EXBLAS_BLOCKS_PER_CU", 8))
    if routine == SUM:
        if strided:
            return K_EXSUM_STRIDED, _grid_for(num_cu, env, n, BLOCK, per_cu)
        bpc = int(env.get("EXBLAS_BPC_SA", 3)) if fpe < 2 else int(env.get("EXBLAS_BPC_SUM", 2))
        grid = _grid_for(num_cu, env, n, TILE, bpc)
        if grid == num_cu * bpc and grid > 1 and grid % 2 == 0:
            grid -= 1                      # an odd grid at the cap
        return K_EXSUM, grid
    if strided or not aligned:
        return K_EXDOT_STRIDED, _grid_for(num_cu, env, n, BLOCK, per_cu)
    bpc = min(int(env.get("EXBLAS_BPC_DOT", 48)), max(4, (n // TILE) // (5 * num_cu)))
    grid = _grid_for(num_cu, env, n, TILE, bpc)
    if grid > num_cu and grid % 2 == 0:
        grid += 1                          # an odd grid above one workgroup per compute unit
    return K_EXDOT, grid


# ---------------------------------------------------------------------------------------------------------------------
# which seams a call exercises
# ---------------------------------------------------------------------------------------------------------------------
def seams(n, head, grid):
    """The positional facts of one fp64 k_blas1_stream launch (head: 1 when ExSUM's pointer is 8 mod 16, else 0)."""
    head = 1 if (head and n > 0) else 0
    nv = (n - head) >> 1
    ntiles = nv // TILE_V
    q, r = divmod(ntiles, grid)            # tile t goes to workgroup t mod grid: r workgroups have q + 1 tiles, the rest q
    counts = {q, q + 1} if r else {q}
    rem = nv - ntiles * TILE_V
    return {
        "ntiles": ntiles,
        "tile_counts": counts,
        "exit_first": any(c % 2 == 1 for c in counts),            # an odd number of tiles leaves at the first break
        "exit_second": any(c and c % 2 == 0 for c in counts),
        "idle": 0 in counts,
        "rem": rem,
        "rem_strides": -(-rem // (grid * BLOCK)),
        "head": head,
        "tail": (n - head) & 1,
    }


def seams_strided(n, grid):
    """fp64 k_blas1_strided: how many of the four u slots the last trip uses, how many slots any trip uses,
    the loop trips of the busiest lane, and where n sits relative to a multiple of T = grid x 256"""
    T = grid * BLOCK
    trips = -(-n // (4 * T))
    last = -(-(n - (trips - 1) * 4 * T) // T)
    edge = {T - 1: "m1", 0: "0", 1: "p1"}.get(n % T, "in")
    return {"slots": min(4, -(-n // T)), "last_slots": last, "trips": trips, "edge": edge}


def seam_classes(s):
    """names of the seam classes of one vector-kernel launch"""
    out = {f"head{s['head']}", f"tail{s['tail']}", f"strides{min(s['rem_strides'], 4)}"}
    if s["rem"] in REMAINDERS:
        out.add(f"rem{s['rem']}")
    if s["exit_first"]:
        out.add("exit_first")
    if s["exit_second"]:
        out.add("exit_second")
    if s["exit_first"] and s["exit_second"]:
        out.add("both_exits")
    if s["idle"]:
        out.add("idle_workgroup")
    if s["ntiles"] == 0:
        out.add("no_tile")
    for c in s["tile_counts"]:
        if c:
            out.add(f"tiles{min(c, 4)}")
    return out


def strided_classes(s):
    return {f"slots{s['slots']}", f"last{s['last_slots']}", f"trips{min(s['trips'], 3)}", f"edge_{s['edge']}"}


def all_vector_classes(routine):
    out = {"tail0", "tail1", "exit_first", "exit_second", "both_exits", "idle_workgroup", "no_tile"}
    out |= {f"rem{r}" for r in REMAINDERS} | {f"strides{k}" for k in range(5)} | {f"tiles{k}" for k in range(1, 5)}
    return out | ({"head0", "head1"} if routine == SUM else {"head0"})


def all_strided_classes():
    return ({f"slots{k}" for k in range(1, 5)} | {f"last{k}" for k in range(1, 5)} | {f"trips{k}" for k in range(1, 4)}
            | {"edge_m1", "edge_0", "edge_p1", "edge_in"})


# ---------------------------------------------------------------------------------------------------------------------
# data: one long buffer per family and operand; expected totals from exact integer block sums
# ---------------------------------------------------------------------------------------------------------------------
class Family:
    """x[i] = mx[i] * 2^(96 (k[i] - 5)) is ExSUM's operand and ExDOT's second one; y[i] = my[i] ExDOT's first.  Mantissas
    are below 2^40 in magnitude, so every element is exact, every ExDOT product an inexact double with a non-zero error
    term (80 bits), and all of it stays far inside [2^-968, 2^1000)."""
    CHUNK = 2048

    def __init__(self, wide, length, seed):
        # one generator per array: a longer buffer begins with the shorter one, so what the CPU test shows of a family
        # holds for the buffers of every plan
        draw = lambda j, lo, hi: np.random.default_rng([seed, j]).integers(lo, hi, length, dtype=np.int64)   # noqa: E731
        if wide:       # odd 40-bit integers on twelve scales 96 bits apart: more than an 8-term expansion holds
            self.mx = (draw(0, 1 << 38, 1 << 39) * 2 + 1) * (draw(1, 0, 2) * 2 - 1)
            self.my = (draw(2, 1 << 38, 1 << 39) * 2 + 1) * (draw(3, 0, 2) * 2 - 1)
            self.k = draw(4, 0, NSCALES)
        else:          # integers below 2^40: they never spill any expansion
            self.mx = draw(0, -(1 << 40) + 1, 1 << 40)
            self.my = draw(2, -(1 << 40) + 1, 1 << 40)
            self.k = np.full(length, SCALE_ZERO, dtype=np.int64)
        self.x = np.ldexp(self.mx.astype(np.float64), (SCALE_BITS * (self.k - SCALE_ZERO)).astype(np.int32))
        self.y = self.my.astype(np.float64)
        self.length = length
        self.scales = sorted(set(self.k.tolist()))
        self._tables = {}

    @staticmethod
    def _terms(routine, mx, my):
        """int64 terms w_j below 2^41 and shifts with element = sum_j w_j << shift_j (exactly)"""
        if routine == SUM:
            return [(mx, 0)]
        xh, xl, yh, yl = mx >> 20, mx & 0xfffff, my >> 20, my & 0xfffff
        return [(xh * yh, 40), (xh * yl + xl * yh, 20), (xl * yl, 0)]

    @classmethod
    def direct_total(cls, routine, mx, my, k):
        """exact total of elements given as mantissas and scale indices, in units of 2^-1074"""
        tot = 0
        for w, shift in cls._terms(routine, mx, my):
            for s in np.unique(k).tolist():
                tot += int(w[k == s].sum()) << (shift + SCALE_BITS * (s - SCALE_ZERO) + 1074)
        return tot

    def _table(self, routine):
        """per term and scale: exact prefix sums over chunks of CHUNK elements (Python integers)"""
        if routine not in self._tables:
            nb = self.length // self.CHUNK
            tab = []
            for w, shift in self._terms(routine, self.mx, self.my):
                for s in self.scales:
                    part = np.where(self.k == s, w, 0)[:nb * self.CHUNK].reshape(nb, self.CHUNK).sum(axis=1)
                    pre = [0]
                    for v in part.tolist():
                        pre.append(pre[-1] + v)
                    tab.append((w, shift, s, pre))
            self._tables[routine] = tab
        return self._tables[routine]

    def total(self, routine, lo, hi):
        """exact total of the contiguous elements [lo, hi) (ExDOT: both operands at the same offset)"""
        assert 0 <= lo <= hi <= self.length
        c0, c1 = -(-lo // self.CHUNK), hi // self.CHUNK
        if c0 >= c1:
            return self.direct_total(routine, self.mx[lo:hi], self.my[lo:hi], self.k[lo:hi])
        e0, e1 = slice(lo, c0 * self.CHUNK), slice(c1 * self.CHUNK, hi)
        tot = 0
        for w, shift, s, pre in self._table(routine):
            v = pre[c1] - pre[c0] + int(w[e0][self.k[e0] == s].sum()) + int(w[e1][self.k[e1] == s].sum())
            tot += v << (shift + SCALE_BITS * (s - SCALE_ZERO) + 1074)
        return tot


class Data:
    """the families' buffers of one plan (generated once, every case is a slice)"""

    def __init__(self, length, seed=20261020):
        self.length = length
        self.fam = {NARROW: Family(False, length, seed), WIDE: Family(True, length, seed + 1)}

    def total(self, routine, family, off, n, inca=1, offb=None, incb=1, wtn=0):
        """exact total (units of 2^-1074) of one case.  wide_then_narrow: the wide buffer below index `wtn`, the narrow
        one from there on."""
        offb = off if offb is None else offb
        if inca == 1 and incb == 1 and offb == off:
            if family != WTN:
                return self.fam[family].total(routine, off, off + n)
            cut = min(max(wtn, off), off + n)
            return self.fam[WIDE].total(routine, off, cut) + self.fam[NARROW].total(routine, cut, off + n)
        assert family != WTN
        f = self.fam[family]
        ix, iy = off + inca * np.arange(n), offb + incb * np.arange(n)
        if routine == SUM:
            return Family.direct_total(SUM, f.mx[ix], None, f.k[ix])
        return Family.direct_total(DOT, f.mx[iy], f.my[ix], f.k[iy])     # a = y (plain), b = x (scaled)

    def operand(self, family, which, wtn=0):
        """the float64 buffer of a family: which = 'x' (scaled) or 'y'"""
        if family != WTN:
            return getattr(self.fam[family], which)
        return np.concatenate([getattr(self.fam[WIDE], which)[:wtn], getattr(self.fam[NARROW], which)[wtn:]])


def exact_double(total):
    """the correctly rounded double of a total in units of 2^-1074"""
    return float(Fraction(total, 1 << 1074))


# ---------------------------------------------------------------------------------------------------------------------
# lone-element cases: a background that cancels inside every double2, 2^(12 j) at seam position j
# ---------------------------------------------------------------------------------------------------------------------
def lone_positions(n, head, grid):
    """[(seam name, element index)] of a vector-kernel launch, distinct positions only (the first name wins)"""
    s = seams(n, head, grid)
    nt, nv = s["ntiles"], (n - s["head"]) >> 1
    el = lambda vec, c: s["head"] + 2 * vec + c                                    # noqa: E731
    cand = []
    if s["head"]:
        cand += [("head", 0), ("after_head", 1)]
    if nt > 0:
        cand += [("tile0_first", el(0, 0)), ("tile0_last", el(TILE_V - 1, 1))]
    if nt > grid:
        cand += [("round1_first", el(grid * TILE_V, 0)), ("round1_last", el((grid + 1) * TILE_V - 1, 1))]
    if nt > 1:
        cand += [("last_full_first", el((nt - 1) * TILE_V, 0)), ("last_full_last", el(nt * TILE_V - 1, 1))]
    if s["rem"]:
        cand += [("rem_first", el(nt * TILE_V, 0)), ("rem_last", el(nv - 1, 1))]
    if s["rem_strides"] > 1:
        cand += [("rem_stride2_first", el(nt * TILE_V + grid * BLOCK, 0))]
    if s["tail"]:
        cand += [("tail", n - 1)]
    return _distinct(cand)


def lone_positions_strided(n, grid):
    T = grid * BLOCK
    cand = [("first", 0), ("slot0_last", T - 1), ("slot1_first", T), ("slot2_first", 2 * T), ("slot3_first", 3 * T),
            ("trip0_last", 4 * T - 1), ("trip1_first", 4 * T), ("last", n - 1)]
    return _distinct([(name, p) for name, p in cand if 0 <= p < n])


def _distinct(cand):
    seen, out = set(), []
    for name, p in cand:
        if p not in seen:
            seen.add(p)
            out.append((name, p))
    return out


LONE_BITS = 12     # seam j carries 2^(12 j): a position counted up to 4095 times (once per workgroup, say) is still readable


def lone_values(npos):
    return [2.0 ** (LONE_BITS * j) for j in range(npos)]


def lone_total(npos):
    """what a launch that counts every seam position once returns, in units of 2^-1074"""
    return sum(1 << (LONE_BITS * j) for j in range(npos)) << 1074


def lone_decode(total, names):
    """-> (counts per seam or None when the total is no sum of c_j 2^(12 j) with 0 <= c_j < 4096, report string)"""
    if total < 0 or total & ((1 << 1074) - 1) or (total >> 1074) >> (LONE_BITS * len(names)):
        return None, f"the total {total >> 1074 if not total & ((1 << 1074) - 1) else total} decodes to no seam counts of {names}"
    v = total >> 1074
    counts = [(v >> (LONE_BITS * j)) & ((1 << LONE_BITS) - 1) for j in range(len(names))]
    bad = [f"{nm} counted {c} times" for nm, c in zip(names, counts) if c != 1]
    return counts, "; ".join(bad) if bad else "every seam once"


def lone_head(e):
    """the scalar head element of a lone entry's launch (k_blas1_stream<SumF64> with a pointer 8 mod 16)"""
    return e["offa"] & 1 if (e["routine"] == SUM and e["inca"] == 1) else 0


def lone_build(xp, base, n, head, positions, values, negate):
    """The operand of a lone-element case from `base`.  The background cancels inside every double2 the kernels load:
    element head + 2q is base[q], element head + 2q + 1 its negation (`negate`; the other ExDOT operand repeats base[q]),
    the scalar head and tail are zero.  So a loop that drops or repeats whole vectors, tiles or strides still leaves a
    background of zero and the total names the seam positions alone.  The vector of a seam position is zeroed, then
    `values` are written at the positions.  xp: numpy for the CPU test, torch in the worker."""
    m = (n - head) // 2
    out = xp.zeros_like(base[:n])
    assert len(out) == n
    out[head:head + 2 * m:2] = base[:m]
    out[head + 1:head + 2 * m:2] = -base[:m] if negate else base[:m]
    for p in positions:
        if head <= p < head + 2 * m:
            q = (p - head) // 2
            out[head + 2 * q] = 0
            out[head + 2 * q + 1] = 0
        else:
            out[p] = 0
    for p, v in zip(positions, values):
        out[p] = v
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the plan of one geometry
# ---------------------------------------------------------------------------------------------------------------------
# an entry: dict(kind, routine, family, fpe, ee, n, inca, incb, offa, offb, wtn, pos) -- kind "plain" | "acc" | "lone"
def _cap_tiles(num_cu, env, routine, fpe):
    """tiles from which the grid sits at its cap (and EXBLAS_GRID_ADJ applies)"""
    if routine == SUM:
        bpc = int(env.get("EXBLAS_BPC_SA", 3)) if fpe < 2 else int(env.get("EXBLAS_BPC_SUM", 2))
    else:
        bpc = min(int(env.get("EXBLAS_BPC_DOT", 48)), 4)      # (max(4, .) holds below 20 tiles per compute unit)
    return num_cu * bpc


def vector_candidates(num_cu, env, routine, fpe=8):
    """[(n, head, grid, seams)]: the cross of head x tail x remainder x the tile counts that flip each exit parity"""
    cap = _cap_tiles(num_cu, env, routine, fpe)
    g = launch_model(num_cu, env, routine, (cap + 8) * TILE, fpe=fpe)[1]          # the grid at the cap
    tiles = {0, 1, 2, 3, cap - 2, cap - 1}
    tiles |= {cap + j for j in range(0, 8)}                                       # small grids: every parity mix
    tiles |= {m * g + d for m in (1, 2, 3, 4) for d in (-1, 0, 1)}                # 1 -> 2, 2 -> 3, 3 -> 4 tiles each
    if g <= 4:      # room for a workgroup to meet the expansion again after one bypass span, and after two
        tiles |= {max(SECOND_ATTEMPT_TILES * g, cap) + 3, max(THIRD_ATTEMPT_TILES * g, cap) + 3}
    out = []
    for nt in sorted(t for t in tiles if t >= 0):
        for rem in REMAINDERS:
            for head in ((0, 1) if routine == SUM else (0,)):
                for tail in (0, 1):
                    n = head + 2 * (nt * TILE_V + rem) + tail
                    if n <= 0 or n + 2 > LIMIT:
                        continue
                    grid = launch_model(num_cu, env, routine, n, fpe=fpe)[1]
                    out.append((n, head, grid, seams(n, head, grid)))
    return out


def strided_candidates(num_cu, env, routine, inc):
    """[(n, grid, seams_strided)] with n at T-1, T, T+1, 4T-1, 4T, 4T+1, 5T+1 where T = grid x 256 lets it, and the
    same distances from a multiple of 4T where the grid is only small from n = num_cu x 256 on"""
    cap = num_cu * int(env.get("EXBLAS_BLOCKS_PER_CU", 8))
    T = launch_model(num_cu, env, routine, cap * BLOCK, aligned=False, strided=True)[1] * BLOCK
    base = 0 if T >= cap * BLOCK else -(-(cap * BLOCK) // (4 * T)) * 4 * T
    ns = {1, 255, 256, 257, 1000} | {base + m * T + d for m in (1, 2, 3, 4, 5, 8) for d in (-1, 0, 1)}
    out = []
    for n in sorted(ns):
        if n > 0 and n * inc + 2 <= LIMIT:
            grid = launch_model(num_cu, env, routine, n, aligned=False, strided=True)[1]
            out.append((n, grid, seams_strided(n, grid)))
    return out


def _cover(cands, classes_of, want):
    """a small subset of the candidates that holds every class of `want` some candidate holds (greedy set cover)"""
    left = want & set().union(*[classes_of(c) for c in cands]) if cands else set()
    chosen = []
    while left:
        best = max(cands, key=lambda c: len(classes_of(c) & left))
        chosen.append(best)
        left -= classes_of(best)
    return chosen


def _thin(cands, keep, count):
    """`keep` plus evenly spaced others, `count` in all at the most"""
    rest = [c for c in cands if c not in keep]
    step = max(1, -(-len(rest) // max(1, count - len(keep))))
    return keep + rest[::step]


# A workgroup that spills within its first four tiles (wide data does) skips 63 tiles and tries the expansion again; if
# that attempt spills too it skips 127 and tries a third time.  Tiles per workgroup that reach the attempt with some to spare:
SECOND_ATTEMPT_TILES = 4 + (BYPASS_MIN + 1) + 1             # 69
THIRD_ATTEMPT_TILES = 4 + (BYPASS_MIN + 1) + (2 * BYPASS_MIN + 2) + 4     # 200


def reentry_possible(grid, ntiles, attempt=2):
    """every workgroup has the tiles to reach its second (third) expansion attempt after spilling in its first tiles"""
    return ntiles // grid >= (SECOND_ATTEMPT_TILES if attempt == 2 else THIRD_ATTEMPT_TILES)


def build_plan(num_cu, geometry):
    """-> (entries, coverage) of one geometry.  coverage[(routine, 'vector' | 'strided')][variant] = classes held."""
    env = geometries(num_cu)[geometry]
    entries, coverage = [], {}

    def add(kind, routine, family, var, n, inca=1, incb=1, offa=0, offb=0, wtn=0, pos=()):
        entries.append(dict(kind=kind, routine=routine, family=family, fpe=var[0], ee=int(var[1]), n=n, inca=inca, incb=incb,
                            offa=offa, offb=offb, wtn=wtn, pos=[list(p) for p in pos]))

    for routine in (SUM, DOT):
        variants = VARIANTS[routine]
        cov = coverage.setdefault((routine, "vector"), {v: set() for v in variants})
        by_knob = {}
        for var in variants:                         # (ExSUM without an expansion has a geometry knob of its own)
            knob = 0 if (routine == SUM and var[0] < 2) else 8
            if knob not in by_knob:
                cands = vector_candidates(num_cu, env, routine, knob)
                cls = lambda c: seam_classes(c[3])                                 # noqa: E731
                by_knob[knob] = (cands, _cover(cands, cls, all_vector_classes(routine)))
        i = 0
        for knob, (cands, cover) in sorted(by_knob.items()):
            mine = [v for v in variants if (0 if (routine == SUM and v[0] < 2) else 8) == knob]
            thinned = _thin(cands, cover, 150 if knob == 8 else 40)
            jobs = [(c, v) for c in cover for v in mine] + [(c, mine[j % len(mine)]) for j, c in enumerate(thinned)]
            for (n, head, grid, s), var in jobs:
                family = (NARROW, WIDE, WTN)[i % 3]
                i += 1
                wtn = WTN_TILES * grid * TILE
                if family == WTN and not (grid <= 4 and reentry_possible(grid, s["ntiles"])):
                    family = WIDE                    # no re-entry to aim at: the wide prefix would be the whole case
                add("plain", routine, family, var, n, offa=head, offb=head if routine == SUM else 0, wtn=wtn)
                cov[var] |= seam_classes(s)
        # wide_then_narrow where every workgroup meets the expansion again with stale contents: after the first bypass
        # span (that attempt spills again, the span doubles) and after the second (absorbed by the larger expansions)
        for var in variants:
            knob = 0 if (routine == SUM and var[0] < 2) else 8
            for attempt, name in ((2, "reentry"), (3, "reentry3")):
                for n, head, grid, s in by_knob[knob][0]:
                    if grid <= 4 and reentry_possible(grid, s["ntiles"], attempt) and s["rem"] == 257 and s["tail"] and (head or routine == DOT):
                        add("plain", routine, WTN, var, n, offa=head, offb=head if routine == SUM else 0, wtn=WTN_TILES * grid * TILE)
                        cov[var].add(name)
                        break
        # strided kernels: inc 2 and 3, and (ExDOT) inc 1 with offsets of unequal parity
        cov = coverage.setdefault((routine, "strided"), {v: set() for v in variants})
        shapes = [(2, 2, 0, 0), (3, 3, 1, 0)] if routine == SUM else [(2, 2, 0, 0), (3, 1, 1, 1), (1, 1, 1, 0), (1, 1, 0, 1)]
        for inca, incb, offa, offb in shapes:
            cands = strided_candidates(num_cu, env, routine, max(inca, incb))
            for j, (n, grid, s) in enumerate(cands):
                for var in variants:
                    add("plain", routine, (WIDE, NARROW)[(i + j) % 2], var, n, inca, incb, offa, offb)
                    cov[var] |= strided_classes(s)
            i += 1
        # lone elements on a cancelling background, every variant: the largest seam list the geometry allows
        for var in variants:
            knob = 0 if (routine == SUM and var[0] < 2) else 8
            cap = _cap_tiles(num_cu, env, routine, knob)
            g = launch_model(num_cu, env, routine, (cap + 8) * TILE, fpe=knob)[1]
            nt = max(cap, g) + 3
            head = 1 if routine == SUM else 0
            n = head + 2 * (nt * TILE_V + 1023) + 1
            grid = launch_model(num_cu, env, routine, n, fpe=knob)[1]
            add("lone", routine, WIDE if var[0] else NARROW, var, n, offa=head, pos=lone_positions(n, head, grid))
        inc = 2
        cands = strided_candidates(num_cu, env, routine, inc)
        n, grid, _ = max(cands, key=lambda c: len(lone_positions_strided(c[0], c[1])))
        for var in variants:
            add("lone", routine, WIDE, var, n, inc, inc, pos=lone_positions_strided(n, grid))
    # the accumulators are left zeroed for the next call: three accumulate calls and one finish per family (the cut of
    # wide_then_narrow inside the second call)
    for routine in (SUM, DOT):
        for j, family in enumerate((NARROW, WIDE, WTN)):
            add("acc", routine, family, VARIANTS[routine][3 + j], 3 * TILE + 77, offa=0, offb=0, wtn=4 * TILE + 500)
    return entries, coverage


def entry_launch(num_cu, env, e):
    """(kernel, grid) the model expects of an entry (an "acc" entry: of its last launch)"""
    strided = e["inca"] != 1 or e["incb"] != 1
    aligned = e["offa"] % 2 == 0 and e["offb"] % 2 == 0
    return launch_model(num_cu, env, e["routine"], e["n"], aligned=aligned, strided=strided, fpe=e["fpe"])


def plan_length(entries):
    """doubles the families' buffers need"""
    need = 0
    for e in entries:
        n = 3 * e["n"] if e["kind"] == "acc" else e["n"]
        need = max(need, e["offa"] + n * e["inca"], e["offb"] + n * e["incb"])
    assert need + 2 <= LIMIT, need
    return -(-need // Family.CHUNK) * Family.CHUNK


def expected_total(data, e, memo=None):
    """the exact total of an entry; memo: a dict shared by the entries of a plan (the variants share their sizes)"""
    if e["kind"] == "lone":
        return lone_total(len(e["pos"]))
    n = 3 * e["n"] if e["kind"] == "acc" else e["n"]
    key = (e["routine"], e["family"], e["offa"], n, e["inca"], e["offb"], e["incb"], e["wtn"] if e["family"] == WTN else 0)
    memo = {} if memo is None else memo
    if key not in memo:
        memo[key] = data.total(e["routine"], e["family"], e["offa"], n, e["inca"], e["offb"], e["incb"], e["wtn"])
    return memo[key]


def plan_json(entries):
    return json.dumps(entries)


# ---------------------------------------------------------------------------------------------------------------------
# a plain TwoSum cascade of one wavefront (what the spill / bypass claims of the families rest on)
# ---------------------------------------------------------------------------------------------------------------------
def wave_stream(x, head, grid, wg, ntiles, wave=0):
    """[tiles of this workgroup, 64 lanes, 8 elements]: what one wavefront of k_blas1_stream<SumF64> absorbs, tile by tile"""
    lanes = wave * 64 + np.arange(64)
    out = []
    for t in range(wg, ntiles, grid):
        vec = t * TILE_V + np.arange(U)[None, :] * BLOCK + lanes[:, None]           # [64, U]
        idx = head + 2 * vec[:, :, None] + np.arange(2)[None, None, :]
        out.append(x[idx.reshape(64, 2 * U)])
    return np.array(out)


def cascade_states(stream, nfpe):
    """Per tile: 'absorbed', 'spilled' or 'bypassed' under the kernels' rule (a spill sends the next `span` tiles past
    the expansion, span 63 doubling with each spill in a row, reset by an absorbed tile), with Knuth's TwoSum on numpy
    doubles.  Also returns whether the expansion was non-zero at each attempt."""
    a = np.zeros((nfpe, 64))
    left, span, states, stale = 0, BYPASS_MIN, [], []
    for tile in stream:
        if left > 0:
            left -= 1
            states.append("bypassed")
            stale.append(None)
            continue
        stale.append(bool((a != 0).any()))
        x = tile.copy()
        for i in range(nfpe):
            for j in range(x.shape[1]):
                s = a[i] + x[:, j]
                bb = s - a[i]
                x[:, j] = (a[i] - (s - bb)) + (x[:, j] - bb)
                a[i] = s
            if not (x != 0).any():
                break
        if (x != 0).any():
            states.append("spilled")
            left, span = span, min(2 * span + 1, 4095)
        else:
            states.append("absorbed")
            span = BYPASS_MIN
    return states, stale
