"""CPU tests of the constructed ExGEMV / ExGEMM cases, their sparse views and the ExTRSV systems (tests/exact_cases.py): the constructions meet their own
conditions, and the oracle (and MPFR where built) returns the integer reference's bits on every output.  The integer
reference shares no code with the library or the oracle; where the two disagree the oracle is wrong."""
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest

import exact_cases as X

PLANTED_GEMM = [(40, 48, 35, 54, "tail"), (40, 48, 300, 100, "split"), (40, 48, 9000, 118, "head"),
                (37, 50, 9000, 54, "split"), (13, 21, 300, 118, "tail"), (16, 16, 5, 100, "head")]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_round_nearest_even_and_classes():
    assert X.round_nearest_even(2**53 + 1) == 2.0**53 and X.round_nearest_even(2**53 + 3) == 2.0**53 + 4
    assert X.round_nearest_even(Fraction(3, 2**1075)) == 2 * 5e-324 and X.round_nearest_even(Fraction(1, 2**1075)) == 0.0
    assert X.round_nearest_even(2**1024 - 2**971) == np.finfo(np.float64).max
    assert X.round_nearest_even(2**1024 - 2**970) == np.inf and X.round_nearest_even(-(2**1024)) == -np.inf
    assert X.classify(0)[0] == "zero" and X.classify(-(2**53 - 1) << 70)[0] == "exact"
    assert X.classify((2**52 << 1) + 1) == ("tie", False) and X.classify(-((2**52 + 1) << 4) - 8) == ("tie", True)
    assert X.classify(((2**53 - 1) << 4) + 8) == ("carry", True)
    assert X.classify((2**52 << 4) + 9)[0] == "tie+1" and X.classify((2**52 << 4) + 7)[0] == "tie-1"
    assert X.classify((2**52 << 4) + 3)[0] == "other"
    with pytest.raises(AssertionError):
        X.to_f64(X.obj([2**66 + 1]))                       # would silently round
    with pytest.raises(AssertionError):
        X.to_f64(X.obj([3]), -1075)                        # leaves the double range


def test_moduli_table_and_worst_case_parameters():
    bits = X.crt_bits()
    assert X.crt_moduli(5) == [256, 255, 253, 251, 247] and len(bits) == X.CRT_LMAX + 1 == 40
    assert bits[1:5] == [8, 15, 23, 31] and bits[39] == 285
    assert bits[1:] == [8, 15, 23, 31, 39, 47, 55, 63, 71, 79, 87, 94, 102, 110, 117, 125, 132, 140, 147, 155, 162, 170,
                        177, 184, 191, 198, 206, 213, 220, 226, 233, 240, 247, 253, 260, 266, 273, 279, 285]
    ks = set()
    for L in range(2, 37):
        na, nb, k = X.crt_worst_params(L)
        assert X.crt_need(na, nb, k) == bits[L] and X.crt_moduli_needed(na, nb, k) == L
        assert 1 <= nb <= na <= 126 and (k > 1 or na <= 53)
        ks.add(k)
    assert {1, 2, 3, 16, 17, 8192, 8193} <= ks            # powers of two, one more, and the k-pass boundary


@pytest.mark.parametrize("m,n,k,S,layout", PLANTED_GEMM)
def test_planted_gemm_vs_oracle(oracle, m, n, k, S, layout):
    c = X.planted_gemm(m, n, k, S, seed=1, layout=layout)
    count = X.planted_mix(c)
    assert (np.array([int(v) for v in c.a.ravel()], dtype=object) == c.a_int.ravel()).all()
    assert (np.array([int(v) for v in c.b.ravel()], dtype=object) == c.b_int.ravel()).all()
    if m >= 16:
        assert count["zero"] >= n and count["exact"] > 0
    assert (c.bits_a, c.bits_b) == (S + 4, S)              # 122 bits at S = 118: inside the 126 the int8 paths accept
    # H and the deciding unit sit where the layout says (different k passes from k > 8192 on)
    assert {"tail": c.pos["H"] == k - 2 and c.pos["d"] == k - 1, "split": c.pos["H"] == 0 and c.pos["d"] == k - 1,
            "head": c.pos["d"] == 0 and c.pos["H"] == k - 1}[layout]
    plain = c.a @ c.b                                       # what the suite's random data never shows: fp64 is wrong here
    assert (plain != c.want).sum() > m * n // 8
    for ta, tb in (("N", "N"), ("T", "T")):
        a, lda = X.gemm_operand(c.a, ta, 1)
        b, ldb = X.gemm_operand(c.b, tb, 2)
        got = oracle.exgemm(ta, tb, m, n, k, 1.0, a, lda, b, ldb, 0.0, np.zeros(m * n), n, 0, mode=oracle.ROUND_EXACT)
        bad = _bits(got) != _bits(c.want.reshape(-1))
        assert not bad.any(), (ta, tb, c.classes.reshape(-1)[bad][:8], got[bad][:4], c.want.reshape(-1)[bad][:4])
    if oracle.mpfr() is not None:
        dots = oracle.mpfr_exgemm_dots(m, n, k, c.a.reshape(-1), k, c.b.reshape(-1), n)
        assert (_bits(dots) == _bits(c.want)).all()


@pytest.mark.parametrize("outputs,inner,S,layout,plant,beta", [
    (40, 3001, 54, "split", None, 0), (48, 300, 100, "tail", "H", 1), (33, 3001, 118, "head", "d", 1),
    (40, 35, 118, "split", "H", -0.75), (64, 2900, 54, "tail", "d", -0.75)])
def test_planted_gemv_vs_oracle(oracle, outputs, inner, S, layout, plant, beta):
    c = X.planted_gemv(outputs, inner, S, seed=2, layout=layout, plant=plant, beta=beta)
    X.planted_mix(c)
    assert [int(v) for v in c.g.ravel()] == c.g_int.ravel().tolist() and [int(v) for v in c.x] == c.x_int.tolist()
    if plant:
        assert [int(v) for v in c.y0] == c.y0_int.tolist() and (c.y0 != 0).sum() >= outputs // 3
    for trans in ("N", "T"):
        m, n, a, lda, xs, ys = X.gemv_operands(c.g, c.x, c.y0, trans, pad=3, offa=2, incx=2, offx=1, incy=3, offy=2)
        got = oracle.exgemv(trans, m, n, 1.0, a, lda, xs, c.beta, ys, 0, incx=2, incy=3, offa=2, offx=1, offy=2,
                            mode=oracle.ROUND_EXACT)
        assert (_bits(got[2::3]) == _bits(c.want)).all(), (trans, c.classes[_bits(got[2::3]) != _bits(c.want)][:8])
        if oracle.mpfr() is not None:
            m, n, a, lda, xs, ys = X.gemv_operands(c.g, c.x, c.y0, trans)
            assert (_bits(oracle.mpfr_exgemv(trans, m, n, 1.0, a, lda, xs, c.beta, ys)) == _bits(c.want)).all(), trans


def test_crt_worst_cases_vs_oracle(oracle):
    seen = set()
    for L in range(2, 37):
        c = X.crt_worst_case(L)
        assert X.crt_need(c.na, c.nb, c.k) == X.crt_bits()[L]
        # the operands really span na and nb bits, and every base-256 digit of the full entries is 255
        assert (c.bits_a, c.bits_b) == (c.na, c.nb)
        M = 1
        for p in X.crt_moduli(L):
            M *= p
        assert 4 * c.top < M and (c.classes == "max").sum() >= 4
        assert {int(v) for v in c.c_int.ravel()} >= {c.top, -c.top, 1, -1}
        seen |= set(c.classes.ravel())
        want = c.want.reshape(-1)
        got = oracle.exgemm("N", "N", c.m, c.n, c.k, 1.0, c.a.reshape(-1), c.k, c.b.reshape(-1), c.n, 0.0,
                            np.zeros(c.m * c.n), c.n, 0, mode=oracle.ROUND_EXACT)
        assert (_bits(got) == _bits(want)).all(), (L, c.classes.reshape(-1)[_bits(got) != _bits(want)][:8])
        if oracle.mpfr() is not None:
            dots = oracle.mpfr_exgemm_dots(c.m, c.n, c.k, c.a.reshape(-1), c.k, c.b.reshape(-1), c.n)
            assert (_bits(dots) == _bits(c.want)).all(), L
    assert {"max", "zero", "exact", "other"} <= seen


@pytest.mark.parametrize("k", [8192, 8193])
def test_crt_wrap_case_vs_oracle(oracle, k):
    c = X.crt_wrap_case(k)
    body = np.array([[int(v) % 256 for v in row] for row in c.a_int]), np.array([[int(v) % 256 for v in row] for row in c.b_int])
    assert (body[0] == 128).sum() == c.m * k - 1 and (body[1] == 128).sum() == c.n * k - 1
    assert (c.bits_a, c.bits_b) == (12, 12)
    got = oracle.exgemm("N", "N", c.m, c.n, k, 1.0, c.a.reshape(-1), k, c.b.reshape(-1), c.n, 0.0, np.zeros(c.m * c.n),
                        c.n, 0, mode=oracle.ROUND_EXACT)
    assert (_bits(got) == _bits(c.want.reshape(-1))).all()


@pytest.mark.parametrize("inner", [12, 3000])
def test_range_rows_gemv_vs_oracle(oracle, inner):
    r = X.range_rows_gemv(inner)
    tiny, dmax = 5e-324, np.finfo(np.float64).max
    by_name = dict(zip(r.names, zip(r.want, r.want_with_y)))
    assert by_name["subnormal 15 units"][0] == 15 * tiny and by_name["subnormal -2 units"][0] == -2 * tiny
    assert by_name["largest subnormal"][0] == (2**52 - 1) * tiny and by_name["smallest normal"][0] == 2.0**-1022
    assert by_name["partial sums overflow"][0] == 2.0**1023 and by_name["DBL_MAX"][0] == dmax
    assert by_name["tie at the overflow threshold"][0] == np.inf
    assert by_name["just below the overflow tie"] == (dmax, dmax)
    assert by_name["negative tie at the overflow threshold"] == (-dmax, -np.inf)
    assert by_name["huge products cancel, 3 units remain"][0] == 3 * tiny
    assert not np.isnan(r.want).any() and not np.isnan(r.want_with_y).any()
    for trans in ("N", "T"):
        for beta, want in ((0.0, r.want), (1.0, r.want_with_y)):
            m, n, a, lda, xs, ys = X.gemv_operands(r.g, r.x, r.y0, trans, pad=1)
            got = oracle.exgemv(trans, m, n, 1.0, a, lda, xs, beta, ys, 0, mode=oracle.ROUND_EXACT)
            assert (_bits(got) == _bits(want)).all(), (trans, beta, [r.names[i] for i in np.nonzero(_bits(got) != _bits(want))[0]])
            if oracle.mpfr() is not None:
                m, n, a, lda, xs, ys = X.gemv_operands(r.g, r.x, r.y0, trans)
                assert (_bits(oracle.mpfr_exgemv(trans, m, n, 1.0, a, lda, xs, beta, ys)) == _bits(want)).all(), (trans, beta)


# ---------------------------------------------------------------------------------------------
# sparse views (ExSpMV / ExSpMM): the oracle is called per row / per output, on the stored entries and the gathered x
# ---------------------------------------------------------------------------------------------
from test_gpu_spmm import _oracle_outputs  # noqa: E402  (plain helpers: nothing in them touches the GPU)
from test_gpu_spmv import _oracle_rows  # noqa: E402


def _mpfr_rows(oracle, crow, col, val, xs, beta, y0):
    out = np.empty(len(crow) - 1)
    for i in range(len(out)):
        a, b = int(crow[i]), int(crow[i + 1])
        out[i] = oracle.mpfr_exgemv("N", 1, b - a, 1.0, val[a:b], 1, np.ascontiguousarray(xs[col[a:b]]), beta, y0[i:i + 1])[0]
    return out


@pytest.mark.parametrize("cls", X.COMPLETE_CLASSES)
def test_complete_to(cls):
    rng = np.random.default_rng(5)
    for T in [0, 1, -1, 2**53 - 1, -(2**53 - 1), 2**105 + 12345, -(2**400 + 2**17 + 1)] + \
             [int(rng.integers(-2**62, 2**62)) << int(rng.integers(0, 300)) for _ in range(40)]:
        for gap in (1, 2, 20, 29, 30, 31, 70, 84):
            fix = X.complete_to(T, cls, gap)               # (asserts the class of the total itself)
            assert all(abs(t) >> ((abs(t) & -abs(t)).bit_length() - 1) < 2**53 for t in fix.terms)
            assert (T << fix.scale) + sum(fix.terms) == fix.total and (T < 0) == (fix.total < 0)
            low = abs(fix.total).bit_length() - 54         # bits below the half unit
            assert len(fix.terms) <= -(-low // 53) + (2 if cls == "carry" else 1)
            got = X.classify(fix.total >> fix.unit)
            assert got[0] == {"tie_odd": "tie"}.get(cls, cls)
            if cls in ("tie", "tie_odd"):
                assert got[1] == (cls == "tie_odd")
            # the deciding unit is `gap` bits below the half unit: half an ulp of the rounded total is 2^(unit + gap)
            assert (abs(fix.total).bit_length() - 54) - fix.unit == gap
            X.to_f64(X.obj(fix.terms))


@pytest.mark.parametrize("outputs,inner,S,layout,plant,beta", [
    (40, 27, 54, "split", None, 0), (48, 70, 63, "head", "H", 1), (33, 300, 118, "tail", "d", -0.75),
    (32, 4200, 64, "split", "d", 1)])
def test_csr_from_rows_vs_oracle(oracle, outputs, inner, S, layout, plant, beta):
    c = X.planted_gemv(outputs, inner, S, seed=3, layout=layout, plant=plant, beta=beta)
    X.planted_mix(c)
    y0 = c.y0 if beta else np.full(outputs, np.nan)
    seen = set()
    for kw in (dict(), dict(itype=np.int32, spread=True), dict(zeros="drop"), dict(dup=c.pos["lead"]),
               dict(itype=np.int32, zeros="drop", dup=c.pos["lead"], spread=True, shuffle=True, n_cols=3 * outputs * inner)):
        crow, col, val, xs, n_cols = X.csr_from_rows(c.g, c.x, seed=4, **kw)
        assert crow.dtype == col.dtype == kw.get("itype", np.int64) and len(xs) == n_cols >= inner
        assert n_cols >= kw.get("n_cols", 0) and 0 <= col.min() and col.max() < n_cols
        lens = np.diff(crow)
        if kw.get("zeros") != "drop":
            assert (lens == inner + (1 if "dup" in kw else 0)).all()
        else:
            assert lens.min() <= 5 and len(set(lens.tolist())) > 1       # the carry rows: 4 non-zeros
        ref = np.zeros(n_cols, dtype=bool)
        ref[col] = True
        assert np.isnan(xs[~ref]).all() and (~ref).sum() >= n_cols // 7 and not np.isnan(xs[ref]).any()
        for i in range(outputs):                            # injective within a row (but for the duplicate), unsorted
            cc = col[crow[i]:crow[i + 1]]
            assert len(set(cc.tolist())) == len(cc) - (1 if "dup" in kw else 0)
        assert (np.diff(col[crow[0]:crow[1]]) < 0).any()
        if not kw.get("shuffle") and kw.get("zeros") != "drop":   # the layout's positions are the stored positions
            assert (val[crow[5]:crow[5] + inner][[c.pos["H"], c.pos["d"]]] == c.g[5, [c.pos["H"], c.pos["d"]]]).all()
        if kw.get("spread"):
            assert set(col[crow[0]:crow[1]].tolist()).isdisjoint(col[crow[1]:crow[2]].tolist())
        # the converter's round trip in Python integers (beta y0 apart), then the oracle on the stored entries
        prod = X.csr_dense_int(crow, col, val, xs)
        assert (prod == X.gemv_exact(c.g_int, c.x_int)).all()
        got = _oracle_rows(oracle, crow, col, val, xs, 1.0, c.beta, y0, mode=oracle.ROUND_EXACT)
        assert (_bits(got) == _bits(c.want)).all(), (kw, c.classes[_bits(got) != _bits(c.want)][:8])
        if oracle.mpfr() is not None and inner <= 300:
            assert (_bits(_mpfr_rows(oracle, crow, col, val, xs, c.beta, c.y0)) == _bits(c.want)).all(), kw
        seen.add(_bits(got).tobytes())
    assert len(seen) == 1                                   # drop, dup and spread do not change the result


@pytest.mark.parametrize("rows,kcols,inner,S,layout,plant,beta", [
    (27, 1, 5, 54, "tail", None, 0), (40, 3, 27, 63, "split", "H", 1), (33, 17, 64, 64, "head", "d", -0.75),
    (20, 33, 65, 90, "split", None, 0), (17, 65, 1025, 118, "head", "H", -0.75)])
def test_planted_spmm_vs_oracle(oracle, rows, kcols, inner, S, layout, plant, beta):
    c = X.planted_spmm(rows, kcols, inner, S, seed=5, layout=layout, plant=plant, beta=beta)
    count = X.planted_mix(c)
    if kcols >= 16:
        assert count["zero"] >= rows and (c.classes[:, 3] == "zero").all() and (c.classes[:, kcols - 2] == "exact").any()
    assert c.want.shape == (rows, kcols) and (c.c_int == X.gemm_exact(c.g_int, c.x_int) +
                                               [[Fraction(c.beta) * int(v) for v in r] for r in c.y0_int]).all()
    assert np.isnan(c.y0).all() if beta == 0 else (c.y0 != 0).sum() >= rows * kcols // 3
    for kw in (dict(), dict(itype=np.int32, zeros="drop", dup=c.pos["lead"], spread=True)):
        crow, col, val, Xd, n_cols = X.csr_from_rows(c.g, c.x, seed=6, **kw)
        assert Xd.shape == (n_cols, kcols)
        got = _oracle_outputs(oracle, crow, col, val, Xd, 1.0, c.beta, c.y0, mode=oracle.ROUND_EXACT)
        bad = _bits(got) != _bits(c.want)
        assert not bad.any(), (kw, c.classes[bad][:8])
    if oracle.mpfr() is not None and inner <= 65:
        for j in range(kcols):
            y0 = np.ascontiguousarray(c.y0[:, j]) if beta else np.zeros(rows)
            w = _mpfr_rows(oracle, crow, col, val, np.ascontiguousarray(Xd[:, j]), c.beta, y0)
            assert (_bits(w) == _bits(c.want[:, j])).all(), j


@pytest.mark.parametrize("outputs,inner,S,layout,beta", [
    (40, 6, 54, "tail", 0), (64, 27, 63, "split", -0.75), (45, 300, 64, "head", 0), (30, 5000, 118, "split", -0.75),
    (35, 70, 90, "tail", -0.75)])
def test_planted_inexact_vs_oracle(oracle, outputs, inner, S, layout, beta):
    c = X.planted_inexact(outputs, inner, S, seed=7, layout=layout, beta=beta)
    X.planted_mix(c)
    assert (X.gemv_exact(c.g_int, c.x_int, Fraction(beta), c.y0_int) == c.c_exact).all()
    assert np.isnan(c.y0).all() if beta == 0 else (np.abs(c.y0) >= 2.0**104).all()
    assert all(int(v) == int(r) << u for v, r, u in zip(c.c_exact, c.c_int, c.unit))
    plain = c.g @ c.x + (beta * c.y0 if beta else 0.0)
    assert (plain != c.want).sum() > outputs // 8          # fp64 is wrong here
    seen = set()
    for kw in (dict(), dict(itype=np.int32, zeros="drop", dup=c.pos["lead"], spread=True)):
        crow, col, val, xs, n_cols = X.csr_from_rows(c.g, c.x, seed=8, **kw)
        got = _oracle_rows(oracle, crow, col, val, xs, 1.0, c.beta, c.y0, mode=oracle.ROUND_EXACT)
        assert (_bits(got) == _bits(c.want)).all(), (kw, c.classes[_bits(got) != _bits(c.want)][:8])
        if oracle.mpfr() is not None and inner <= 300:
            y0 = c.y0 if beta else np.zeros(outputs)
            assert (_bits(_mpfr_rows(oracle, crow, col, val, xs, c.beta, y0)) == _bits(c.want)).all(), kw
        seen.add(_bits(got).tobytes())
    assert len(seen) == 1


def test_adversarial_rows_vs_oracle(oracle):
    a = X.adversarial_rows(1500, seed=9)
    assert a.lens.min() >= 1 and a.lens.max() <= 200 and {63, 64, 65} <= set(a.lens.tolist())
    cls = a.classes
    for name in ("tie", "carry", "tie+1", "tie-1", "other"):
        assert (cls == name).sum() >= 50, name
    assert 4 * ((cls == "tie") | (cls == "carry")).sum() >= a.count
    ref = np.zeros(a.n_cols, dtype=bool)
    ref[a.col] = True
    assert np.isnan(a.xs[~ref]).all() and not np.isnan(a.xs[ref]).any() and len(set(a.col.tolist())) == len(a.col)
    for i in (0, 1, 2, 3, 700, 1499):                       # the expected values, recomputed from the stored doubles
        s = sum(Fraction(float(v)) * Fraction(float(w)) for v, w in
                zip(a.val[a.crow[i]:a.crow[i + 1]], a.xs[a.col[a.crow[i]:a.crow[i + 1]]]))
        assert s == Fraction(a.exact[i][0]) * Fraction(2) ** a.exact[i][1] and X.round_nearest_even(s) == a.want[i]
    got = _oracle_rows(oracle, a.crow, a.col, a.val, a.xs, 1.0, 0.0, np.full(a.count, np.nan), mode=oracle.ROUND_EXACT)
    bad = _bits(got) != _bits(a.want)
    assert not bad.any(), (cls[bad][:8], np.nonzero(bad)[0][:8])
    if oracle.mpfr() is not None:
        assert (_bits(_mpfr_rows(oracle, a.crow, a.col, a.val, a.xs, 0.0, np.zeros(a.count))) == _bits(a.want)).all()
    for scale in (-1.0, 2.0, 0.5):                          # the columns ExSpMM runs: exact scalings of x
        w = _oracle_rows(oracle, a.crow, a.col, a.val, a.xs * scale, 1.0, 0.0, np.zeros(a.count), mode=oracle.ROUND_EXACT)
        assert (_bits(w) == _bits(a.want * scale)).all(), scale


def test_range_rows_as_csr_vs_oracle(oracle):
    for inner in (12, 20000):
        r = X.range_rows_gemv(inner)
        for kw in (dict(), dict(zeros="drop", itype=np.int32)):
            crow, col, val, xs, n_cols = X.csr_from_rows(r.g, r.x, seed=10, **kw)
            for beta, want in ((0.0, r.want), (1.0, r.want_with_y)):
                got = _oracle_rows(oracle, crow, col, val, xs, 1.0, beta, r.y0, mode=oracle.ROUND_EXACT)
                assert (_bits(got) == _bits(want)).all(), (inner, kw, beta)


# ---------------------------------------------------------------------------------------------
# ExTRSV: planted totals along the substitution chain, the control system and the range rows
# ---------------------------------------------------------------------------------------------
TRSV_ORIENT = (("L", "N"), ("U", "N"), ("L", "T"), ("U", "T"))
TRSV_ORACLE_VARIANTS = ((0, False), (4, True), (8, True))


def _trsv_vs_oracle(oracle, L, b, want, diag, what, mpfr=True):
    for uplo, trans in TRSV_ORIENT:
        a, lda, xs, idx = X.trsv_operands(L, b, uplo, trans, diag, lda_pad=3, offa=2, incx=2, offx=1)
        for fpe, ee in TRSV_ORACLE_VARIANTS:
            rc, got = oracle.extrsv(uplo, trans, diag, len(b), a, lda, xs, fpe, ee, incx=2, offa=2, offx=1,
                                    mode=oracle.ROUND_EXACT)
            bad = _bits(got[idx]) != _bits(want)
            assert rc == 0 and not bad.any(), (what, uplo, trans, fpe, ee, np.nonzero(bad)[0][:8])
            keep = np.ones(len(got), dtype=bool)
            keep[idx] = False
            assert np.isnan(got[keep]).all()
        if mpfr and oracle.mpfr() is not None:
            a, lda, xs, idx = X.trsv_operands(L, b, uplo, trans, diag)
            got = oracle.mpfr_extrsv(uplo, trans, diag, len(b), a, lda, xs, True)
            assert (_bits(got[idx]) == _bits(want)).all(), (what, uplo, trans, "mpfr")


def test_trsv_exact_and_operands():
    L = np.array([[2.0, 0, 0], [1.0, 4.0, 0], [0.5, -3.0, -8.0]])
    b = np.array([6.0, 7.0, 1.5])
    x, tot = X.trsv_exact(L, b)
    assert x.tolist() == [3.0, 1.0, -0.375] and tot == [6, 4, 3]
    assert X.trsv_exact(L, b, unit=True)[0].tolist() == [6.0, 1.0, 1.5]
    # a total that is a tie (1 + 2^-53 -> 1), then an inexact quotient: the IEEE division of the rounded total
    x, tot = X.trsv_exact(np.array([[1.0, 0], [-2.0 ** -53, 3.0]]), np.array([1.0, 1.0]))
    assert tot[1] == 1 + Fraction(1, 2**53) and x[1] == 1.0 / 3.0
    for uplo, trans in TRSV_ORIENT:
        for diag in "NU":
            a, lda, xs, idx = X.trsv_operands(L, b, uplo, trans, diag, lda_pad=2, offa=3, incx=3, offx=1)
            assert lda == 5 and len(a) == 3 + 15 and len(xs) == 1 + 6 + 1 and (xs[idx] == b).all()
            A = a[3:].reshape(3, 5)[:, :3].T                # A[r, c]
            op = A.T if trans == "T" else A
            fwd = (uplo == "L") != (trans == "T")
            assert idx.tolist() == ([1, 4, 7] if fwd else [7, 4, 1])
            logical = op if fwd else op[::-1, ::-1]
            low = np.tril(np.ones((3, 3), bool), -1 if diag == "U" else 0)
            assert (logical[low] == L[low]).all() and np.isnan(logical[~low]).all()
            assert np.isnan(A[np.triu_indices(3, 1) if uplo == "L" else np.tril_indices(3, -1)]).all()
            assert np.isnan(a[:3]).all() and np.isnan(a[3:].reshape(3, 5)[:, 3:]).all() and np.isnan(xs).sum() == len(xs) - 3


@pytest.mark.parametrize("unit", [False, True])
@pytest.mark.parametrize("n,W,mbits,filler", X.TRSV_CASES)
def test_planted_trsv_vs_oracle(oracle, n, W, mbits, filler, unit):
    c = X.planted_trsv(n, seed=21, W=W, mbits=mbits, filler=filler, unit=unit)   # (asserts its own conditions)
    p = c.planted
    assert c.counts == X.planted_mix(SimpleNamespace(classes=c.classes[p], tie_up=c.tie_up[p], c_int=c.c_int[p]))
    assert c.counts["tie"] + c.counts["carry"] + c.counts["tie+1"] + c.counts["tie-1"] == p.sum() >= (n * 5) // 8
    assert set(c.gap[p].tolist()) == set(X.TRSV_GAPS) and (c.want[~p] == 1.0).all()
    big = np.nonzero(c.cancel)[0]                           # the exactly cancelling pairs: 2^120 / 2^150 times the total
    assert 8 * len(big) >= p.sum() and not c.cancel[~p].any()
    for i in big[:6]:
        top = np.abs(c.L[i, :i]).max()
        assert (c.L[i, :i] == top).sum() == 1 and (c.L[i, :i] == -top).sum() == 1
        assert 2.0 ** (c.cancel[i] - 2) < top / abs(float(c.totals[i])) < 2.0 ** (c.cancel[i] + 2)
    # the expected x and the totals follow from the doubles alone, and each total is of the class it is labelled with
    x, tot = X.trsv_exact(c.L, c.b, unit)
    assert (_bits(x) == _bits(c.want)).all() and tot == c.totals
    for i in np.nonzero(p)[0][:: max(1, int(p.sum()) // 40)]:
        T = c.totals[i]
        a = abs(T.numerator) << max(0, 60 - abs(T.numerator).bit_length())
        half = 1 << (a.bit_length() - 54)
        r = a % (2 * half)
        dev = {"tie": 0, "carry": 0, "tie+1": 1, "tie-1": -1}[c.classes[i]]
        assert (r - half) * (1 << int(c.gap[i])) == dev * half, (i, c.classes[i])
        if c.classes[i] == "carry":
            assert a >> (a.bit_length() - 53) == 2**53 - 1
    if filler:
        cols = p.copy()                                     # dense but for the anchor columns
        assert (c.L[np.ix_(p, cols)][np.tril_indices(int(p.sum()), -1)] != 0).all()
    if n > X.TRSV_BLOCK:                                    # closing terms in the row's own block and in earlier ones
        flags = [f for f in c.own if f]
        assert any(all(f) for f in flags) and any(not any(f) for f in flags)
    plain = np.zeros(n)                                     # fp64 substitution is wrong here
    for i in range(n):
        plain[i] = (c.b[i] - c.L[i, :i] @ plain[:i]) / (1.0 if unit else c.L[i, i])
    assert (plain != c.want).sum() > n // 8
    diag = "U" if unit else "N"
    _trsv_vs_oracle(oracle, c.L, c.b, c.want, diag, (n, W, "planted"))
    # the control: every planted b_i a quarter unit of its total further from the tie
    moved = c.b_control != c.b
    assert (moved == p).all()
    xc, totc = X.trsv_exact(c.L, c.b_control, unit)
    first = int(np.nonzero(p)[0][0])
    q = abs(totc[first] - c.totals[first])
    assert q * 4 == Fraction(np.spacing(abs(X.round_nearest_even(c.totals[first])))) or c.classes[first] == "carry"
    assert np.isfinite(xc).all() and (_bits(xc) != _bits(c.want)).any()
    _trsv_vs_oracle(oracle, c.L, c.b_control, xc, diag, (n, W, "control"), mpfr=False)


@pytest.mark.parametrize("lead", [0, 58, 70])
def test_range_rows_trsv_vs_oracle(oracle, lead):
    r = X.range_rows_trsv(lead)                             # (asserts the values it was built for)
    first = min(r.rows.values())                            # lead = 58: the range rows open the second block of 64
    assert first == lead + 6 and (first % X.TRSV_BLOCK == 0) == (lead == 58)
    assert r.n == lead + 18 and np.isinf(r.want).sum() == 1 and np.isinf(r.want[-1])
    assert (np.abs(r.want[np.isfinite(r.want)]) >= 2.0**1000 / 8).sum() >= 5
    sub = np.abs(r.want) < 2.0**-1022
    assert (sub & (r.want != 0)).sum() >= 4 and (r.want == 0).sum() == 2
    _trsv_vs_oracle(oracle, r.L, r.b, r.want, "N", ("range", lead))
