"""GPU suite that holds the batched ExGETRF / ExGETRS / ExPOTRF / ExPOTRS to the ends of the double range: the cases of
range_block_cases.py (never the code under test decides an expectation), bit for bit, a NaN being a NaN, on the paths 0, 1, 2
and 3, with the variant and the layout rotating from call to call.

  * neighbours in one wave: a batch cycles healthy, range, planted, range, healthy, range, NaN at G + 1 and 4 G + 1 matrices
    (NB + 1 and 4 NB + 1 blocks), every one of them held to its own model, with the counters of the same call;
  * every range case alone, at batch 1 and in a wave filled with copies of it, and the row-shuffled copy where the model
    says that the factors survive the shuffle;
  * the apply at k = 1, 3, 5, 65 with a last block cut above the range rows and inside them; 'B' against '1' then '2';
  * the single routines as second witnesses (expotrf_dev, extrsm_dev, extrsv_dev twice) and the reference rounding mode.

The counters: cnt[0] + cnt[1] is the model's number of roundings; cnt[1] is at least the number of totals that
spmv_round_fast (spmv_common.hip.h) documents as never decided in registers: ties, and non-zero totals below 2^-960 or at
or above 2^1020 in magnitude (range_block_cases.settles).

The six classes of ExGETRF cases, each as a candidate and in the row of U: 1 the overflow threshold, 2 the expansion guard at
2^1000, 3 subnormals and the limit 2^-960, 4 a zero by cancellation, 5 a wide-range cancellation, 6 a pivot that exact
rounding decides."""
import numpy as np
import pytest

import bjacobi_cases as J
import getrf_cases as G
import range_block_cases as R
import test_gpu_getrf_batched as TGF
import test_gpu_getrs_batched as TGS
import test_gpu_potrf_batched as TPF
import test_gpu_potrs_batched as TPS

pytestmark = pytest.mark.gpu
ALL = np.ones((1, 1), dtype=bool)
KS = (1, 3, 5, 65)
CLASS_NAMES = {1: "overflow threshold", 2: "guard at 2^1000", 3: "subnormals and 2^-960", 4: "zero by cancellation",
               5: "wide-range cancellation", 6: "rounding decides the pivot"}


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    _reset(exblas_amd)


def _reset(ex):
    for name in ("getrf_batched", "getrs_batched", "potrf_batched", "potrs_batched", "potrf", "trsm"):
        getattr(ex, f"set_{name}_path")(0)
    ex.load_library().exblas_set_round_mode(0)


def _settle(e):
    """the least number of roundings the accumulator settles: a healthy or planted entry has its ties"""
    return getattr(e, "settle", e.ties)


def _wave(p):
    return max(64 // J.pw_of(p), 1)


def _fill(p):
    """the batch that fills a wave with copies of one matrix; beyond p = 32, where a wave holds one, the four waves of a
    workgroup item"""
    return _wave(p) if _wave(p) > 1 else 4


def _sevens(cases, healthy0, planted, healthy1, nan):
    """healthy, range, planted, range, healthy, range, NaN, over all the range cases three at a time"""
    n = len(cases)
    return [(healthy0, cases[(3 * g) % n], planted, cases[(3 * g + 1) % n], healthy1, cases[(3 * g + 2) % n], nan)
            for g in range(-(-n // 3))]


# ---------------------------------------------------------------------------------------------
# ExGETRF
# ---------------------------------------------------------------------------------------------
def _lu_call(ex, p, batch, path, t, seven):
    layout, pad, gap = G.LAYOUTS[t % len(G.LAYOUTS)]
    fpe, ee = G.VARIANTS[t % 3]
    A, want, pivots, infos, entries = G.factor_batch(p, batch, seven)
    ex.set_getrf_batched_path(path)
    got, piv, inf, cnt = TGF._factor(ex, A, layout, pad, gap, fpe, ee)
    what = (p, batch, path, layout, pad, gap, fpe, [e.name for e in seven[:7]])
    assert (inf == infos).all(), (what, inf[:16], infos[:16])
    assert (piv == pivots).all(), (what, np.argwhere(piv != pivots)[:4].tolist())
    J.same_bits(got, want, ALL, what)
    assert cnt[0] + cnt[1] == sum(e.roundings for e in entries), (what, cnt)
    assert cnt[1] >= sum(_settle(e) for e in entries), (what, cnt)
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return got


@pytest.mark.parametrize("p", [q for q, _ in R.EMBED])
def test_getrf_range_matrices_beside_healthy_and_planted_ones(ex, p):
    cases = R.getrf_at(p)
    assert {(e.case.cls, e.case.form) for e in cases} == {(c, f) for c in CLASS_NAMES for f in ("cand", "U")}
    base = G.factor_seven(p)
    assert base[0].name == "planted" and base[6].name == "nan" and base[0].ties >= 1
    try:
        t = p
        for seven in _sevens(cases, base[1], base[0], base[2], base[6]):
            for path in (0, 1, 2, 3):
                for batch in (_wave(p) + 1, 4 * _wave(p) + 1):
                    _lu_call(ex, p, batch, path, t, seven)
                    t += 1
    finally:
        ex.set_getrf_batched_path(0)


@pytest.mark.parametrize("p", [R.NSUP + 2] + [q for q, _ in R.EMBED])
def test_getrf_every_range_case_alone_and_shuffled(ex, p):
    """p = 8: every case at its own size (the hand-made ones are 2 x 2 and 3 x 3)"""
    kept = 0
    try:
        t = p
        for e in R.getrf_at(p):
            q = e.A.shape[0]
            s = R.shuffled_entry(e)
            kept += s is not None
            for path in (0, 1, 2, 3):
                for batch in (1, _fill(q)):
                    _lu_call(ex, q, batch, path, t, (e,) * 7)
                    t += 1
                if s is not None:          # the same factors under other pivots
                    got = _lu_call(ex, q, _fill(q), path, t, (s, e, s, s, e, s, e))
                    J.same_bits(got[0], got[1], ALL, ("shuffled", e.name))
        print("getrf alone", p, len(R.getrf_at(p)), "cases,", kept, "shuffled copies kept")
    finally:
        ex.set_getrf_batched_path(0)


# ---------------------------------------------------------------------------------------------
# ExPOTRF
# ---------------------------------------------------------------------------------------------
def _chol_call(ex, p, batch, path, t, seven):
    uplo, layout, pad, gap = J.LAYOUTS[t % len(J.LAYOUTS)]
    fpe, ee = J.VARIANTS[t % 3]
    full, want, infos, entries = J.factor_batch(p, batch, uplo, seven)
    ex.set_potrf_batched_path(path)
    got, inf, cnt = TPF._factor(ex, full, uplo, layout, pad, gap, fpe, ee)
    what = (p, batch, path, uplo, layout, pad, gap, fpe, [e.name for e in seven[:7]])
    assert (inf == infos).all(), (what, inf[:16], infos[:16])
    J.same_bits(got, want, J.tri_mask(p, uplo), what)
    assert cnt[0] + cnt[1] == sum(e.fixed for e in entries), (what, cnt)
    assert cnt[1] >= sum(_settle(e) for e in entries), (what, cnt)
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return got, inf


@pytest.mark.parametrize("p", [2, 3, 4, 9, 20, 32, 33, 64])
def test_potrf_range_cases_and_roots_alone_beside_neighbours_and_through_the_single_routine(ex, p):
    cases = R.potrf_at(p)
    names = [e.name.split(" @")[0] for e in cases]
    roots = ["roots 0", "roots 1", "roots 2"]
    assert names == {2: ["subnormal radicand"], 3: ["subnormal total", "overflow"], 4: ["inf"] + roots}.get(
        p, ["subnormal total", "subnormal radicand", "overflow", "inf"] + roots)
    base = J.factor_seven(p)
    try:
        t = p
        sevens = [(e,) * 7 for e in cases]
        if p >= 9:
            assert base[1].name == "planted" and base[6].name == "nan"
            sevens += _sevens(cases, base[0], base[1], base[3], base[6])
        for seven in sevens:
            alone = seven[0] is seven[1]
            for path in (0, 1, 2, 3):
                for batch in ((1, _fill(p)) if alone else (_wave(p) + 1, 4 * _wave(p) + 1)):
                    _chol_call(ex, p, batch, path, t, seven)
                    t += 1
        # the single routine gives every range matrix the same bits
        ex.set_potrf_batched_path(0)
        for e in cases:
            one, info = TPF._single(ex, e)
            assert info == e.info
            J.same_bits(one, e.R, J.tri_mask(p, "U"), ("expotrf_dev", p, e.name))
    finally:
        ex.set_potrf_batched_path(0)


# ---------------------------------------------------------------------------------------------
# the apply
# ---------------------------------------------------------------------------------------------
def _blocks(k):
    nb = max(64 // min(J.pw_of(k), 64), 1)
    return nb + 1, 4 * nb + 1


def _rotated(seven, nb):
    """the seven, turned so that the last of nb blocks is a range block"""
    off = next(o for o in range(7) if (nb - 1 + o) % 7 in (1, 3, 5))
    return tuple(seven[(i + off) % 7] for i in range(7))


def _tails(p):
    """the rows of the last block: whole, cut above the range rows, cut inside them"""
    lead = p - (R.NSUP + 12)
    return p, lead + R.NSUP, lead + R.NSUP + 6


def _potrs_call(ex, entries, p, n, k, sweep, path, t):
    uplo, layout, pad, gap = J.LAYOUTS[t % len(J.LAYOUTS)]
    fpe, ee = J.VARIANTS[t % 3]
    full, X0, want, settle = R.potrs_case(entries, p, n, k, sweep, uplo)
    ex.set_potrs_batched_path(path)
    got, cnt = TPS._apply(ex, full, X0, uplo, layout, pad, gap, (0, 3, 1)[t % 3], sweep, fpe, ee)
    what = (p, n, k, sweep, path, uplo, layout, pad, gap, fpe, [e.name for e in entries])
    J.same_bits(got, want, np.ones_like(got, dtype=bool), what)
    assert cnt[0] + cnt[1] == n * k, (what, cnt)
    assert cnt[1] >= settle, (what, cnt, settle)
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return got


@pytest.mark.parametrize("sweep", ["1", "2"])
@pytest.mark.parametrize("p", [18, 32, 64])
def test_potrs_range_blocks_beside_healthy_and_planted_ones(ex, p, sweep):
    try:
        t = p
        for k in KS:
            for nb in _blocks(k):
                for path in (0, 1, 2, 3):
                    seven = _rotated(R.potrs_seven(p, sweep, t % 3), nb)
                    n = (nb - 1) * p + _tails(p)[t % 3]
                    _potrs_call(ex, seven, p, n, k, sweep, path, t)
                    t += 1
    finally:
        ex.set_potrs_batched_path(0)


@pytest.mark.parametrize("p", [18, 32, 64])
def test_potrs_every_range_block_alone_both_sweeps_in_one_launch_and_extrsm(ex, p):
    try:
        t = p
        for sweep in ("1", "2"):
            seven = R.potrs_seven(p, sweep)
            for e in (seven[1], seven[3], seven[5]):
                for path in (0, 1, 2, 3):
                    for k, nb in ((1, 1), (5, 8), (3, 16)):
                        got = _potrs_call(ex, (e,), p, nb * p, k, sweep, path, t)
                        t += 1
                # ExTRSM on the block: the same bits
                L, B = e.sys(p)
                Fu = np.ascontiguousarray(L.T if sweep == "1" else L[::-1, ::-1])
                X0 = B if sweep == "1" else B[::-1]
                one = TPS._trsm_block(ex, Fu, X0[:, :3], sweep)
                J.same_bits(one, got[:p, :3], np.ones((p, 3), dtype=bool), ("extrsm_dev", p, sweep, e.name))
        # 'B' on the block without the overflowing row, beside healthy ones: '1' followed by '2'
        seven = R.potrs_seven(p, "1")
        safe = next(e for e in seven if e.name == "range safe")
        entries = (seven[0], safe, seven[4], safe)
        for path, k, (uplo, layout, pad, gap) in zip((0, 1, 2, 3), (1, 3, 65, 5), J.LAYOUTS):
            ex.set_potrs_batched_path(path)
            nb = _blocks(k)[0]
            full, X0, want1, _ = R.potrs_case(entries, p, nb * p, k, "1", uplo)
            both, _ = TPS._apply(ex, full, X0, uplo, layout, pad, gap, 2, "B")
            one, _ = TPS._apply(ex, full, X0, uplo, layout, pad, gap, 2, "1")
            two, _ = TPS._apply(ex, full, one, uplo, layout, pad, gap, 0, "2")
            J.same_bits(one, want1, np.ones_like(one, dtype=bool), ("the first sweep of B", p, path))
            J.same_bits(both, two, np.ones_like(both, dtype=bool), ("B against 1 then 2", p, path))
    finally:
        ex.set_potrs_batched_path(0)


def _getrs_call(ex, entries, p, n, k, path, t):
    layout, pad, gap = G.LAYOUTS[t % len(G.LAYOUTS)]
    fpe, ee = G.VARIANTS[t % 3]
    LU, ipiv, X0, want, settle = R.getrs_case(entries, p, n, k)
    ex.set_getrs_batched_path(path)
    got, cnt = TGS._apply(ex, LU, ipiv, X0, layout, pad, gap, (0, 3, 1)[t % 3], fpe, ee)
    what = (p, n, k, path, layout, pad, gap, fpe, [e.name for e in entries])
    J.same_bits(got, want, np.ones_like(got, dtype=bool), what)
    assert cnt[0] + cnt[1] == 2 * n * k, (what, cnt)
    assert cnt[1] >= settle, (what, cnt, settle)
    if fpe == 0 or path == 1:
        assert cnt[0] == 0, (what, cnt)
    return got, (LU, ipiv, X0)


@pytest.mark.parametrize("p", [18, 32, 64])
def test_getrs_range_blocks_beside_healthy_and_planted_ones(ex, p):
    """the forward blocks carry the range rows in L under interchanges, the backward blocks in U; the column that keeps the
    overflowing row of a forward block is NaN above it (0 * Inf), and that column alone"""
    try:
        t = p
        for k in KS:
            for nb in _blocks(k):
                for path in (0, 1, 2, 3):
                    seven = _rotated(R.getrs_seven(p, t % 2), nb)
                    n = (nb - 1) * p + _tails(p)[t % 3]
                    _getrs_call(ex, seven, p, n, k, path, t)
                    t += 1
    finally:
        ex.set_getrs_batched_path(0)


@pytest.mark.parametrize("p", [18, 32, 64])
def test_getrs_every_range_and_planted_block_alone_and_extrsv_twice(ex, p):
    lead = p - (R.NSUP + 12)
    blocks = [R.getrs_range(lead, v, d) for d in ("forward", "backward") for v in R.VARIANTS]
    blocks += [R.getrs_planted(p, "L"), R.getrs_planted(p, "U")]
    try:
        t = p
        for e in blocks:
            if e.name.startswith("planted"):
                assert R._getrs_solve(e, p)[1].min() >= 3          # the ties of the model
            for path in (0, 1, 2, 3):
                for k, nb in ((1, 1), (5, 8), (3, 16)):
                    got, (LU, ipiv, X0) = _getrs_call(ex, (e,), p, nb * p, k, path, t)
                    t += 1
            for j in range(3):            # ExTRSV twice on the column: the same bits
                one = TGS._trsv_twice(ex, LU[0], ipiv[0], X0[:p, j])
                J.same_bits(one, got[:p, j], np.ones(p, dtype=bool), ("extrsv_dev twice", p, e.name, j))
    finally:
        ex.set_getrs_batched_path(0)


# ---------------------------------------------------------------------------------------------
# the reference rounding mode, once per kernel
# ---------------------------------------------------------------------------------------------
def test_reference_rounding_mode_on_the_range_cases(ex):
    """every output goes through the accumulator (nothing is rounded in registers), the four paths agree bit for bit, and a
    planted tie of the batch rounds the other way than to nearest even"""
    lib = ex.load_library()
    lib.exblas_set_round_mode(1)
    p = 32
    try:
        runs = {"getrf": [], "potrf": [], "potrs": [], "getrs": []}
        lu = _sevens(R.getrf_at(p), G.factor_seven(p)[1], G.factor_seven(p)[0], G.factor_seven(p)[2], G.factor_seven(p)[6])[0]
        ch = _sevens(R.potrf_at(p), J.factor_seven(p)[0], J.factor_seven(p)[1], J.factor_seven(p)[3], J.factor_seven(p)[6])[0]
        A, lu_want, _, infos, lu_ent = G.factor_batch(p, 7, lu)
        full, ch_want, ch_infos, ch_ent = J.factor_batch(p, 7, "U", ch)
        Fs, X0s, s_want, _ = R.potrs_case(R.potrs_seven(p, "1"), p, 7 * p, 5, "1", "U")
        LU, ipiv, X0g, g_want, _ = R.getrs_case(R.getrs_seven(p, 0), p, 7 * p, 5)
        for path in (0, 1, 2, 3):
            fpe = (8, 0, 4, 8)[path]
            ex.set_getrf_batched_path(path)
            got, piv, inf, cnt = TGF._factor(ex, A, "col", 1, 2, fpe, True)
            assert cnt == (0, sum(e.roundings for e in lu_ent), 0, 0) and (inf == infos).all()
            runs["getrf"].append(np.concatenate([got.ravel(), piv.ravel().astype(np.float64)]))
            ex.set_potrf_batched_path(path)
            got, inf, cnt = TPF._factor(ex, full, "U", "row", 1, 2, fpe, True)
            assert cnt == (0, sum(e.fixed for e in ch_ent), 0, 0) and (inf == ch_infos).all()
            runs["potrf"].append(np.triu(got).ravel())
            ex.set_potrs_batched_path(path)
            got, cnt = TPS._apply(ex, Fs, X0s, "U", "col", 1, 2, 1, "1", fpe, True)
            assert cnt == (0, 7 * p * 5, 0, 0)
            runs["potrs"].append(got.ravel())
            ex.set_getrs_batched_path(path)
            got, cnt = TGS._apply(ex, LU, ipiv, X0g, "row", 1, 2, 1, fpe, True)
            assert cnt == (0, 2 * 7 * p * 5, 0, 0)
            runs["getrs"].append(got.ravel())
        nearest = {"getrf": lu_want.ravel(), "potrf": np.triu(np.nan_to_num(ch_want)).ravel(), "potrs": s_want.ravel(), "getrs": g_want.ravel()}
        for name, r in runs.items():
            for other in r[1:]:
                J.same_bits(other, r[0], np.ones_like(other, dtype=bool), ("reference mode, the paths", name))
            a = np.nan_to_num(r[0][:nearest[name].size], nan=0.0, posinf=1.0, neginf=-1.0)
            b = np.nan_to_num(nearest[name], nan=0.0, posinf=1.0, neginf=-1.0)
            assert (a.view(np.int64) != b.view(np.int64)).any(), ("the modes never differed", name)
    finally:
        _reset(ex)
