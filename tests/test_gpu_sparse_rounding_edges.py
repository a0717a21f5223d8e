"""ExSpMV / ExSpMM on constructed ties in every row class (tests/exact_cases.py), bit for bit.

`spmv_round_fast` decides most sparse results in registers and only has to be sound; random 53-bit mantissas never put
a row on a tie or next to one, so nothing random can show an unsound acceptance.  These inputs put exact ties (to even
downwards and upwards, carrying into the next binade), sums one deciding unit off a tie (that unit 20 to 84 bits below
the half unit: both sides of the test's 2^-30 margin), subnormal and DBL_MAX results and non-finite terms into every
kernel that rounds a row: eight lanes per short row, one wave per medium row, the split rows and their finish, both
forms of the ExSpMM main kernel, both forms of its deferred finish, and every forced path -- with the deciding half
unit or unit in a stored entry, in a TwoProd error term or in y.

Expected bits: the Python-integer reference in the exact rounding mode, the oracle per row / per output in the
reference rounding mode; for rows with non-finite terms what GPU ExGEMV 'N' gives for the row as a 1 x len matrix (the
routines' contract).  No tolerance, nothing filtered at run time, no expected value from ExSpMV / ExSpMM themselves.

The counters (`last_spmv_info`, `last_spmm_info`) keep the file from passing vacuously; what is asserted of them is
derived, not measured (`_spmv_counters`, `_spmm_counters`):
  accounting    registers + accumulator == rows (outputs) of the unsplit rows, the split rows are exactly those the path says
  forced        path 1, fpe = 0 and the reference rounding mode decide nothing in registers
  soundness     no tie passes the register test: registers <= unsplit outputs - (ties + carries)
  non-vacuity   a sum 2^-20 or 2^-29 of a half unit off a tie (S = 54, 63) is inside the documented acceptance rule
                (|q| < h (1 - 2^-30), nothing spills: the planted rows span S + 24 <= 87 bits): on paths 0 and 2, exact
                rounding mode, fpe >= 2, unsplit rows with their zeros stored, registers >= (tie+1) + (tie-1) outputs
Each test prints the counters it saw per path (pytest -s)."""
import functools

import numpy as np
import pytest

import exact_cases as X
from test_gpu_spmm import _dev as spmm_dev, _oracle_outputs
from test_gpu_spmv import _dev as spmv_dev, _oracle_rows

pytestmark = pytest.mark.gpu

S_ALL = (54, 63, 64, 65, 90, 118)
S_LONG = (54, 64, 118)
FPE = [(fpe, ee) for fpe in (0, 2, 4, 8) for ee in (False, True)]
ALPHAS = (1.0, -1.0, 2.0 ** -7, 2.0 ** 40)
PATHS = (0, 1, 2, 3)
SPMV_SPLIT, SPMV_CHUNK = 16384, 4096          # ExSpMV: rows longer than 16384 entries are split into chunks of 4096
SPMM_SPLIT = 1024                             # ExSpMM: rows longer than 1024 entries are split
# how the rows are stored, rotated over the cases (the first one is the plain form the counters are predicted for)
STORE = (dict(), dict(itype=np.int32), dict(zeros="drop"), dict(dup="lead", itype=np.int32), dict(spread=True),
         dict(zeros="drop", dup="lead", spread=True, shuffle=True))


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_spmv_path(0)
    exblas_amd.set_spmm_path(0)
    exblas_amd.load_library().exblas_set_round_mode(0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _gemv_case(outputs, inner, S, layout, plant=None, beta=0):
    case = X.planted_gemv(outputs, inner, S, seed=11, layout=layout, plant=plant, beta=beta)
    X.planted_mix(case)
    return case


def _spmm_case(rows, kcols, inner, S, layout, plant=None, beta=0):
    case = X.planted_spmm(rows, kcols, inner, S, seed=12, layout=layout, plant=plant, beta=beta)
    X.planted_mix(case)
    return case


def _inexact_case(outputs, inner, S, layout, beta):
    case = X.planted_inexact(outputs, inner, S, seed=13, layout=layout, beta=beta)
    X.planted_mix(case)
    return case


@functools.lru_cache(maxsize=None)
def _adversarial():
    return X.adversarial_rows(20000, seed=14)


def _store(case, kw, seed, x=None):
    kw = dict(kw)
    if kw.get("dup") == "lead":
        kw["dup"] = case.pos["lead"]
    return X.csr_from_rows(case.g, case.x if x is None else x, seed=seed, **kw)


def _ties(classes):
    return (classes == "tie") | (classes == "carry")


def _near(classes):
    return (classes == "tie+1") | (classes == "tie-1")


def _spmv_counters(info, lens, classes, path, mode, fpe, S=None, plain=False):
    """module docstring; `classes` per row, `lens` the stored lengths.  Returns the counters for the report."""
    rows = len(lens)
    split = np.ones(rows, dtype=bool) if path == 3 else (lens > SPMV_SPLIT) if path != 2 else np.zeros(rows, dtype=bool)
    assert info[2] == split.sum() and info[0] + info[1] == rows - info[2], (info, path)
    chunk = 16 if path == 3 else SPMV_CHUNK
    assert info[3] == ((lens[split] + chunk - 1) // chunk).sum(), (info, path)
    if path == 1 or fpe == 0 or mode == 1:
        assert info[0] == 0, (info, path, fpe, mode)
    assert info[0] <= (~split).sum() - (_ties(classes) & ~split).sum(), ("a tie was decided in registers", info, path)
    if path in (0, 2) and mode == 0 and fpe >= 2 and S in (54, 63) and plain:
        assert info[0] >= (_near(classes) & ~split).sum(), ("near-ties inside the acceptance rule fell back", info, path, S)
    return tuple(info)


def _spmm_counters(info, lens, classes, k, path, mode, fpe, S=None, plain=False):
    """as _spmv_counters, per output; `classes` is rows x k"""
    rows = len(lens)
    split = np.ones(rows, dtype=bool) if path == 3 else (lens > SPMM_SPLIT) if path != 2 else np.zeros(rows, dtype=bool)
    assert info[2] == split.sum() and info[0] + info[1] == (rows - info[2]) * k, (info, path)
    if path == 1 or fpe == 0 or mode == 1:
        assert info[0] == 0, (info, path, fpe, mode)
    ties = int(_ties(classes)[~split].sum())
    assert info[1] >= ties and info[0] <= (~split).sum() * k - ties, ("a tie was decided in registers", info, path)
    if path in (0, 2) and mode == 0 and fpe >= 2 and S in (54, 63) and plain:
        assert info[0] >= _near(classes)[~split].sum(), ("near-ties inside the acceptance rule fell back", info, path, S)
    return tuple(info)


def _same(got, want, classes, what):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), (what, int(bad.sum()), sorted(set(np.asarray(classes)[bad].tolist())), np.argwhere(bad)[:4].tolist(),
                           np.asarray(got)[bad][:3], np.asarray(want)[bad][:3])


def _spmv_sweep(ex, oracle, csr, want, classes, beta, y0, S, plain, alpha=1.0, paths=PATHS, fpes=FPE, tag=()):
    """One stored matrix through the forced paths, the (fpe, early_exit) variants on path 0 and both rounding modes."""
    lib = ex.load_library()
    crow, col, val, xs, n_cols = csr
    m, lens = len(crow) - 1, np.diff(crow).astype(np.int64)
    xa = xs / alpha                                        # a power of two: fl(alpha * xa) == xs exactly
    assert (xa[~np.isnan(xs)] * alpha == xs[~np.isnan(xs)]).all()
    seen = {}
    try:
        for path in paths:
            ex.set_spmv_path(path)
            got = spmv_dev(ex, crow, col, val, xa, m, n_cols, alpha, beta, y0)
            seen[path] = _spmv_counters(ex.last_spmv_info(), lens, classes, path, 0, 8, S, plain)
            _same(got, want, classes, tag + ("path", path))
        ex.set_spmv_path(0)
        for fpe, ee in fpes:
            got = spmv_dev(ex, crow, col, val, xa, m, n_cols, alpha, beta, y0, fpe, ee)
            _spmv_counters(ex.last_spmv_info(), lens, classes, 0, 0, fpe, S, plain)
            _same(got, want, classes, tag + ("fpe", fpe, ee))
        want_ref = _oracle_rows(oracle, crow, col, val, xa, alpha, beta, y0, mode=oracle.ROUND_REFERENCE)
        assert not np.isnan(want_ref).any()
        lib.exblas_set_round_mode(1)
        for path in paths:
            ex.set_spmv_path(path)
            fpe, ee = FPE[(path + len(tag)) % len(FPE)]
            got = spmv_dev(ex, crow, col, val, xa, m, n_cols, alpha, beta, y0, fpe, ee)
            _spmv_counters(ex.last_spmv_info(), lens, classes, path, 1, fpe)
            _same(got, want_ref, classes, tag + ("reference mode, path", path))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_spmv_path(0)
    return seen


def _spmm_sweep(ex, oracle, csr, want, classes, beta, y0, S, plain, alpha=1.0, paths=PATHS, fpes=FPE, tag=(), pads=(3, 5)):
    lib = ex.load_library()
    crow, col, val, xs, n_cols = csr
    m, k, lens = len(crow) - 1, xs.shape[1], np.diff(crow).astype(np.int64)
    xa = xs / alpha
    assert (xa[~np.isnan(xs)] * alpha == xs[~np.isnan(xs)]).all()
    seen = {}
    try:
        for path in paths:
            ex.set_spmm_path(path)
            got = spmm_dev(ex, crow, col, val, xa, m, n_cols, alpha, beta, y0, xpad=pads[0], ypad=pads[1])
            seen[path] = _spmm_counters(ex.last_spmm_info(), lens, classes, k, path, 0, 8, S, plain)
            _same(got, want, classes, tag + ("path", path))
        ex.set_spmm_path(0)
        for fpe, ee in fpes:
            got = spmm_dev(ex, crow, col, val, xa, m, n_cols, alpha, beta, y0, fpe, ee, xpad=pads[1], ypad=pads[0])
            _spmm_counters(ex.last_spmm_info(), lens, classes, k, 0, 0, fpe, S, plain)
            _same(got, want, classes, tag + ("fpe", fpe, ee))
        want_ref = _oracle_outputs(oracle, crow, col, val, xa, alpha, beta, y0, mode=oracle.ROUND_REFERENCE)
        assert not np.isnan(want_ref).any()
        lib.exblas_set_round_mode(1)
        for path in paths:
            ex.set_spmm_path(path)
            fpe, ee = FPE[(path + len(tag)) % len(FPE)]
            got = spmm_dev(ex, crow, col, val, xa, m, n_cols, alpha, beta, y0, fpe, ee, xpad=0, ypad=1)
            _spmm_counters(ex.last_spmm_info(), lens, classes, k, path, 1, fpe)
            _same(got, want_ref, classes, tag + ("reference mode, path", path))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_spmm_path(0)
    return seen


def _apart(case, csr, least):
    """the leading entry, the half unit and the deciding unit of every row lie more than `least` stored entries apart"""
    crow, col, val, xs, n_cols = csr
    p = sorted(case.pos[name] for name in ("lead", "H", "d"))
    assert (np.diff(crow) == case.g.shape[1]).all()        # stored with their zeros: positions are stored positions
    assert min(p[1] - p[0], p[2] - p[1]) > least, (p, least)
    return p


# ---------------------------------------------------------------------------------------------
# ExSpMV
# ---------------------------------------------------------------------------------------------
SPMV_LENGTHS = (5, 8, 9, 16, 17, 27, 64,                   # eight lanes per row, two entries per lane and step
                65, 256, 257, 300, 4097, 16384,            # one wave per row, four per lane and step
                16385, 70000)                              # split rows: five chunks (one entry in the last), 18 chunks


@pytest.mark.parametrize("length", SPMV_LENGTHS)
def test_exspmv_planted_ties(ex, oracle, length):
    """Every row is a planted class.  Every S (the deciding unit S - 34 bits below the half unit) and layout per length;
    each case in its plain form (int64, zeros stored, one column map) and in one other stored form (int32, zeros
    dropped, the leading entry stored twice, a column map per row, entries shuffled), alpha rotating with x pre-scaled
    by its exact inverse; y holds NaN (beta = 0)."""
    outputs = 64 if length <= 300 else 32
    report = {}
    for si, S in enumerate(S_ALL if length <= 300 else S_LONG):
        for li, layout in enumerate(X.LAYOUTS):
            case = _gemv_case(outputs, length, S, layout)
            y0 = np.full(outputs, np.nan)
            plain = _store(case, STORE[0], seed=si)
            if length >= 3000 and layout != "tail":
                _apart(case, plain, SPMV_CHUNK if length > SPMV_SPLIT else 1000)
            n = 3 * si + li
            report[(S, layout)] = _spmv_sweep(ex, oracle, plain, case.want, case.classes, 0.0, y0, S, True,
                                              alpha=ALPHAS[n % 4], tag=(length, S, layout))
            kw = STORE[1 + n % 5]
            if length >= 3000:                             # a map per row of a long row is a large x: the other forms there
                kw = STORE[1 + n % 3]
            other = _store(case, kw, seed=n)
            quick = length > 300
            _spmv_sweep(ex, oracle, other, case.want, case.classes, 0.0, y0, S, False, alpha=ALPHAS[(n + 1) % 4],
                        paths=PATHS[n % 2::2] if quick else PATHS, fpes=FPE[n % 4::4] if quick else FPE,
                        tag=(length, S, layout, tuple(sorted(kw))))
    print("\nexspmv planted", length, {k: v for k, v in report.items() if k[1] == "split"})


BETA_LENGTHS = (27, 64, 300, 16384, 16385, 20000)


@pytest.mark.parametrize("plant,beta", [("H", 1), ("d", 1), ("H", -0.75), ("d", -0.75)])
@pytest.mark.parametrize("length", BETA_LENGTHS)
def test_exspmv_half_unit_or_deciding_unit_in_y(ex, oracle, length, plant, beta):
    """The half unit (H) or the deciding unit (d) comes from beta * y: exactly (beta = 1) or through TwoProd (beta = -3/4:
    3 term from y, -2 term from the row), in the sub == 0 lane of k_spmv_rows<8> / <64>, in k_spmv_long_finish (two_prod_safe and
    wave_add_double) and, on path 1, in the accumulator finish."""
    outputs = 64 if length <= 300 else 32
    report = {}
    for si, S in enumerate(S_LONG if length > 300 else (54, 63, 64, 118)):
        layout = X.LAYOUTS[(si + (plant == "d")) % 3]
        case = _gemv_case(outputs, length, S, layout, plant, beta)
        assert (case.y0 != 0).sum() >= outputs // 3
        plain = _store(case, STORE[0], seed=si)
        report[S] = _spmv_sweep(ex, oracle, plain, case.want, case.classes, case.beta, case.y0, S, True,
                                alpha=ALPHAS[(si + 1) % 4], fpes=FPE[si % 2::2], tag=(length, S, layout, plant, beta))
        kw = STORE[1 + si % 3]
        _spmv_sweep(ex, oracle, _store(case, kw, seed=si), case.want, case.classes, case.beta, case.y0, S, False,
                    paths=(0, 3), fpes=FPE[3::4], tag=(length, S, layout, plant, beta, tuple(sorted(kw))))
    print("\nexspmv beta", length, plant, beta, report)


# ---------------------------------------------------------------------------------------------
# ExSpMM
# ---------------------------------------------------------------------------------------------
SPMM_K = (1, 2, 3, 8, 17, 32,                              # the narrow main kernel, G = 1 .. 32 lanes per row
          33, 64, 65, 130)                                 # WIDE: one row x 64 columns per wave, ragged last tiles
SPMM_LENGTHS = (27, 64, 65,                                # both forms of the deferred finish (8 lanes / 64 lanes per output)
                1024, 1025,                                # the split threshold
                5000)                                      # several chunks of 1024 per lane group


@pytest.mark.parametrize("length", SPMM_LENGTHS)
@pytest.mark.parametrize("kcols", SPMM_K)
def test_exspmm_planted_ties(ex, oracle, kcols, length):
    """planted_spmm: every output a planted class, at least 40 % of them ties (several rounds of the deferred finish per
    bitmap word), padded ldx / ldy with the sentinel check; the half unit or the deciding unit in Y for two S of three."""
    rows = 37 if length <= 65 else 19
    report = {}
    for si, S in enumerate(S_ALL if length <= 65 else S_LONG):
        n = si + SPMM_K.index(kcols) + SPMM_LENGTHS.index(length)
        layout = X.LAYOUTS[n % 3]
        plant, beta = ((None, 0), ("H", 1), ("d", -0.75), (None, 0), ("d", 1), ("H", -0.75))[n % 6]
        case = _spmm_case(rows, kcols, length, S, layout, plant, beta)
        ties = _ties(case.classes)
        assert 10 * ties.sum() >= 4 * ties.size
        plain = _store(case, STORE[0], seed=n)
        quick = length > 65 and kcols > 32
        report[(S, plant, beta)] = _spmm_sweep(ex, oracle, plain, case.want, case.classes, case.beta, case.y0, S, True,
                                               alpha=ALPHAS[n % 4], fpes=FPE[n % 4::4] if quick else FPE,
                                               tag=(kcols, length, S, layout, plant, beta))
        kw = STORE[1 + n % (3 if length > 65 else 5)]
        _spmm_sweep(ex, oracle, _store(case, kw, seed=n), case.want, case.classes, case.beta, case.y0, S, False,
                    alpha=ALPHAS[(n + 1) % 4], paths=PATHS[n % 2::2], fpes=FPE[(n + 2) % 4::4],
                    tag=(kcols, length, S, layout, plant, beta, tuple(sorted(kw))), pads=(58, 1))
    print("\nexspmm planted", kcols, length, report)


# ---------------------------------------------------------------------------------------------
# products with a non-zero TwoProd error term
# ---------------------------------------------------------------------------------------------
COLUMN_SCALES = (1.0, -1.0, 2.0, 0.5, -4.0)               # exact scalings of x: a tie stays a tie, the sign flips


def _columns(x, k):
    return np.stack([x * COLUMN_SCALES[j % 5] for j in range(k)], axis=1)


@pytest.mark.parametrize("beta", [0, -0.75])
@pytest.mark.parametrize("length", [27, 300, 20000])
def test_inexact_products(ex, oracle, length, beta):
    """planted_inexact: the leading products are 80 to 106 bits wide, so the planted class of a row depends on TwoProd
    error terms (they enter the expansion at slot N - 3, apart from the products); with beta = -3/4 the product
    beta * y has such an error term as well, in each of the five places that add the beta term.  ExSpMV on short,
    medium and split rows, ExSpMM at k = 5 and k = 40 with the columns x (and y) times (1, -1, 2, 1/2, -4)."""
    outputs = 60 if length <= 300 else 30
    for si, S in enumerate(S_ALL if length <= 300 else S_LONG):
        layout = X.LAYOUTS[si % 3]
        case = _inexact_case(outputs, length, S, layout, beta)
        for kw in (STORE[0], STORE[1 + si % 5 if length <= 300 else 1 + si % 3]):
            csr = _store(case, kw, seed=si)
            _spmv_sweep(ex, oracle, csr, case.want, case.classes, case.beta, case.y0, None, False, fpes=FPE[si % 2::2],
                        tag=("inexact", length, S, layout, beta, tuple(sorted(kw))))
        for k in (5, 40):
            Xc = _columns(case.x, k)
            want = _columns(case.want, k)
            classes = np.repeat(case.classes[:, None], k, axis=1)
            csr = _store(case, STORE[(si + k) % 4], seed=si, x=Xc)
            _spmm_sweep(ex, oracle, csr, want, classes, case.beta, _columns(case.y0, k), None, False,
                        fpes=FPE[(si + 1) % 2::4], tag=("inexact", length, S, layout, beta, k))


# ---------------------------------------------------------------------------------------------
# results at the ends of the double range
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inner", [12, 3000, 20000])
def test_result_range_rows(ex, oracle, inner):
    """range_rows_gemv as CSR: subnormal sums, the largest subnormal, the smallest normal, DBL_MAX, the tie at the
    overflow threshold and huge products that cancel, as short, medium and split rows; beta in {0, 1}, every path."""
    r = X.range_rows_gemv(inner)
    nr = len(r.names)
    none = np.full(nr, "other", dtype=object)              # (no class: the counters are only held to their accounting)
    for kw in (STORE[0], STORE[2]):
        csr = X.csr_from_rows(r.g, r.x, seed=inner, **kw)
        for beta, want, sums in ((0.0, r.want, r.exact), (1.0, r.want_with_y, r.exact_with_y)):
            y0 = r.y0 if beta else np.full(nr, np.nan)
            _spmv_sweep(ex, oracle, csr, want, none, beta, y0, None, False, tag=("range", inner, beta, tuple(r.names)))
            want_neg = np.array([X.round_nearest_even(-s) for s in sums])
            for k in (5, 40):
                sign = np.array([1.0 if j % 2 == 0 else -1.0 for j in range(k)])
                csr2 = X.csr_from_rows(r.g, r.x[:, None] * sign[None, :], seed=inner, **kw)
                want2 = np.where(sign[None, :] > 0, want[:, None], want_neg[:, None])
                Y0 = r.y0[:, None] * sign[None, :] if beta else np.full((nr, k), np.nan)
                _spmm_sweep(ex, oracle, csr2, want2, np.repeat(none[:, None], k, axis=1), beta, Y0, None, False,
                            fpes=FPE[1::3], tag=("range", inner, beta, k, tuple(r.names)))


# ---------------------------------------------------------------------------------------------
# overflowing and non-finite terms
# ---------------------------------------------------------------------------------------------
def _nonfinite_rows(length, seed):
    """(values, x, beta, y) rows of `length` entries: small integers against small integers, except at two positions
    chosen away from the first lane of the row and, in a split row, from its first chunk."""
    rng = np.random.default_rng([seed, length])
    far, near = length - 3, max(3, length // 2 + 5)        # 40: lanes 5 and 1 of eight; 500: lanes 52 and 63; 20000: chunks 4, 2
    dmax = np.finfo(np.float64).max
    rows = []

    def row(special, beta=0.0, y=np.nan, sign=0):
        v = rng.integers(-8, 9, length).astype(np.float64)
        x = rng.integers(-8, 9, length).astype(np.float64)
        if sign:                                           # the rest of the row has one sign
            v, x = np.abs(v) * sign, np.abs(x)
        for p, (a, b) in special.items():
            v[p], x[p] = a, b
        rows.append((v, x, beta, y))

    row({near: (2.0 ** 600, 2.0 ** 500), far: (-(2.0 ** 600), 2.0 ** 500)})      # two overflowing products that cancel
    row({far: (2.0 ** 600, 2.0 ** 500), near: (2.0 ** 600, -(2.0 ** 400))})      # one that does not (and a huge finite one)
    row({far: (-(2.0 ** 1000), 2.0 ** 30)})
    row({far: (np.inf, 1.0)})                                                    # a true Inf
    row({far: (np.inf, 1.0), near: (1.0, -np.inf)})                              # ... and its opposite
    row({far: (3.0, np.inf), near: (0.0, 2.0)})
    row({far: (np.nan, 1.0)})                                                    # a NaN
    row({near: (0.0, np.inf)})                                                   # 0 * Inf
    row({far: (-(2.0 ** 1000), 2.0 ** 23)}, 2.0, 1.5 * 2.0 ** 1023, -1)           # beta * y overflows, the row is negative
    row({far: (2.0 ** 1000, 2.0 ** 23)}, 2.0, -dmax, 1)
    row({}, 2.0, dmax, -1)
    # -3/4 times a finite double cannot overflow: the largest finite product, and an infinite y
    row({far: (-(2.0 ** 1000), 2.0 ** 23)}, -0.75, -dmax, -1)
    row({far: (2.0 ** 1000, 2.0 ** 23)}, -0.75, np.inf, 1)
    row({far: (-(2.0 ** 1000), 2.0 ** 23)}, -0.75, -np.inf, -1)
    row({near: (2.0 ** 600, 2.0 ** 500)}, -0.75, np.inf, 1)
    return rows, (near, far)


@pytest.mark.parametrize("length", [40, 500, 20000])
def test_overflowing_and_nonfinite_terms(ex, oracle, length):
    """Products that overflow (2^600 * 2^500), true Inf and NaN entries and a beta * y that overflows, in a lane other
    than the row's first and a chunk other than its first, in short, medium and split rows.  The contract: the bits of
    GPU ExGEMV 'N' on the row as a 1 x len matrix -- and the same bits on paths 0 .. 3 (the short path forms beta * y
    with two_prod, the split rows' finish with two_prod_safe).  ExSpMM at k = 2 with the columns x and -x.
    beta = 2 overflows on a finite y; -3/4 times a finite double cannot, so that beta runs on +-Inf in y and on
    -DBL_MAX, whose product is the largest finite one with a non-zero error term (the expansion's 2^1000 guard)."""
    import torch
    lib = ex.load_library()
    rows, (near, far) = _nonfinite_rows(length, 15)
    assert near % 8 != 0 and far % 8 != 0 and near % 64 != 0 and far % 64 != 0
    assert length <= SPMV_CHUNK or (near >= SPMV_CHUNK and far >= SPMV_CHUNK and near // SPMV_CHUNK != far // SPMV_CHUNK)
    m = len(rows)
    try:
        for mode in (0, 1):
            lib.exblas_set_round_mode(mode)
            for beta in sorted({r[2] for r in rows}):
                sel = [r for r in rows if r[2] == beta]
                g, xr = np.stack([r[0] for r in sel]), np.stack([r[1] for r in sel])
                y0 = np.array([r[3] for r in sel])
                ms = len(sel)
                want = np.empty((ms, 2))
                for i in range(ms):
                    for j, sg in enumerate((1.0, -1.0)):
                        Y = torch.from_numpy(np.array([y0[i] * sg])).cuda()
                        ex.exgemv_dev("N", 1, length, 1.0, torch.from_numpy(g[i].copy()).cuda(), 1,
                                      torch.from_numpy(xr[i] * sg).cuda(), beta, Y, 8, True)
                        want[i, j] = Y.cpu().numpy()[0]
                # every row has its own x: one column map per row (n_cols = ms * length and some)
                crow = np.arange(ms + 1, dtype=np.int64) * length
                rng = np.random.default_rng(length)
                n_cols = ms * length + 77
                col = rng.permutation(n_cols)[:ms * length].astype(np.int64)
                xs = np.full(n_cols, np.nan)
                xs[col] = xr.reshape(-1)
                val = g.reshape(-1)
                X2 = np.stack([xs, -xs], axis=1)
                for path in PATHS:
                    ex.set_spmv_path(path)
                    ex.set_spmm_path(path)
                    for it in (np.int64, np.int32):
                        got = spmv_dev(ex, crow.astype(it), col.astype(it), val, xs, ms, n_cols, 1.0, beta, y0)
                        info = ex.last_spmv_info()
                        assert info[0] + info[1] == ms - info[2], info
                        _same(got, want[:, 0], np.arange(ms), ("exspmv", length, mode, beta, path))
                        Y0 = np.stack([y0, -y0], axis=1) if beta else np.full((ms, 2), np.nan)
                        got = spmm_dev(ex, crow.astype(it), col.astype(it), val, X2, ms, n_cols, 1.0, beta, Y0)
                        info = ex.last_spmm_info()
                        assert info[0] + info[1] == (ms - info[2]) * 2, info
                        _same(got, want, np.repeat(np.arange(ms)[:, None], 2, axis=1), ("exspmm", length, mode, beta, path))
    finally:
        lib.exblas_set_round_mode(0)
        ex.set_spmv_path(0)
        ex.set_spmm_path(0)
    assert m == 15


@pytest.mark.parametrize("m", [1, 2, 5, 513])
def test_exgemv_reference_with_an_infinite_x(ex, m):
    """The reference of the contract, held to IEEE itself: ExGEMV 'N' on m rows (odd m: the kernel whose last lane has no
    second row) against an x with one infinite entry.  Row i is +-Inf by the sign of A(i, k) x_k, and NaN where
    A(i, k) = 0 -- in that row only.  (Row 0 of an odd m used to come out NaN: found by the rows above.)"""
    import torch
    rng = np.random.default_rng(m)
    n, k = 40, 29
    a = rng.integers(1, 9, (m, n)).astype(np.float64) * rng.choice((-1.0, 1.0), (m, n))
    if m > 2:
        a[m // 2, k] = 0.0
    x = rng.integers(-8, 9, n).astype(np.float64)
    for xk in (np.inf, -np.inf):
        x[k] = xk
        with np.errstate(invalid="ignore"):
            want = a[:, k] * xk                            # +-Inf, NaN for the zero
        assert np.isnan(want).sum() == (m > 2) and np.isinf(want).sum() == m - (m > 2)
        A = torch.from_numpy(np.asfortranarray(a).reshape(-1, order="F").copy()).cuda()
        for fpe, ee in ((8, True), (4, False), (0, False)):
            Y = torch.full((m,), np.nan, dtype=torch.float64, device="cuda")
            ex.exgemv_dev("N", m, n, 1.0, A, m, torch.from_numpy(x).cuda(), 0.0, Y, fpe, ee)
            got = Y.cpu().numpy()
            assert (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(want)] == want[~np.isnan(want)]).all(), \
                (m, xk, fpe, ee, np.nonzero(np.isnan(got) != np.isnan(want))[0][:5])


# ---------------------------------------------------------------------------------------------
# the wide net
# ---------------------------------------------------------------------------------------------
def _first_rows(a, bad_rows):
    out = []
    for i in bad_rows[:3]:
        lo, hi = int(a.crow[i]), int(a.crow[i + 1])
        out.append((int(i), a.classes[i], a.exact[i], [v.hex() for v in a.val[lo:hi]], [v.hex() for v in a.xs[a.col[lo:hi]]]))
    return out


def test_adversarial_rows(ex, oracle):
    """20000 rows of 1 to 200 entries (lengths straddling 64): integers of 1 to 53 bits over exponent windows of 60 to
    400 bits, exact cancellation planted, every second row closed onto a tie, a carry or one unit off a tie with the
    deciding unit 1 to 70 bits below the half unit.  One matrix, ExSpMV and ExSpMM (k = 4: x, -x, 2 x, x / 2), paths
    0, 1 and 2; the expected bits are Fraction's.  This is the net for what the planted rows cannot isolate (the tail
    clause of spmv_round_fast: after two VecSum passes the planted rows' tails are tiny or zero)."""
    a = _adversarial()
    m, lens, cls = a.count, a.lens.astype(np.int64), a.classes
    assert 4 * _ties(cls).sum() >= m and (lens < 64).any() and (lens == 64).any() and (lens > 64).any()
    y0 = np.full(m, np.nan)
    scales = (1.0, -1.0, 2.0, 0.5)
    X4 = np.stack([a.xs * s for s in scales], axis=1)
    want4 = np.stack([np.where(a.want == 0, 0.0, a.want * s) for s in scales], axis=1)   # an exact zero sum is +0.0
    assert (np.abs(a.want[a.want != 0]) > 2.0 ** -1000).all() and np.isfinite(a.want).all()   # the scalings are exact
    cls4 = np.repeat(cls[:, None], 4, axis=1)
    report = {}
    try:
        for path in (0, 1, 2):
            ex.set_spmv_path(path)
            ex.set_spmm_path(path)
            for it in (np.int64, np.int32):
                got = spmv_dev(ex, a.crow.astype(it), a.col.astype(it), a.val, a.xs, m, a.n_cols, 1.0, 0.0, y0)
                report["exspmv", path] = _spmv_counters(ex.last_spmv_info(), lens, cls, path, 0, 8)
                bad = np.nonzero(_bits(got) != _bits(a.want))[0]
                assert bad.size == 0, ("exspmv", path, bad.size, sorted(set(cls[bad].tolist())), _first_rows(a, bad))
                got = spmm_dev(ex, a.crow.astype(it), a.col.astype(it), a.val, X4, m, a.n_cols, 1.0, 0.0, np.full((m, 4), np.nan))
                report["exspmm", path] = _spmm_counters(ex.last_spmm_info(), lens, cls4, 4, path, 0, 8)
                bad = np.nonzero((_bits(got) != _bits(want4)).any(axis=1))[0]
                assert bad.size == 0, ("exspmm", path, bad.size, sorted(set(cls[bad].tolist())), _first_rows(a, bad))
    finally:
        ex.set_spmv_path(0)
        ex.set_spmm_path(0)
    print("\nadversarial rows", {c: int((cls == c).sum()) for c in sorted(set(cls.tolist()))}, report)
