"""ExSUM / ExDOT on float32, float16 and bfloat16 inputs and the single rounding into a narrow format, on the GPU.

Tier 1 holds every entry (_dev, _ctx, host, accumulate + finish, exsum_to / exdot_to) to Python integers
(tests/lowp_cases.py) at the sizes where the streaming kernel changes behaviour: n = 0 .. 9, every pointer offset from a
16-byte boundary, one workgroup tile t (4096 float32 / 8192 16-bit elements) minus / plus one and 2 t + 1, ExDOT with
equal and unequal misalignment, increments 2 and 3 -- through the superaccumulator-only kernel (fpe 0) and both
expansion kernels (fpe 4, 8), with the kernel id of exblas_last_blas1_info asserted.  Tier 2 compares the whole record
with the fp64 path on the widened data at sizes where a workgroup streams 1, 2, 3 and 4 tiles (the grid is read back,
no CU count is assumed), on order-1, wide-range and cancelling data.  Every comparison is bit for bit."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import lowp_cases as L
from helpers import exact_int_from_digits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = {"float32": 4096, "float16": 8192, "bfloat16": 8192}
PER16 = {"float32": 4, "float16": 8, "bfloat16": 8}
K_SUM, K_SUM_STRIDED, K_DOT, K_DOT_STRIDED = 5, 6, 7, 8
OUT_EXACT, OUT_FLAGS, OUT_DIGITS = 0, 2, 48


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    return exblas_amd


def tdt(name):
    import torch
    return getattr(torch, name)


def place(src, off):
    """a CUDA copy of the CPU tensor src whose first element lies `off` elements past a 16-byte boundary"""
    import torch
    buf = torch.zeros(src.numel() + 16, dtype=src.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + src.numel()]
    v.copy_(src)
    assert src.numel() == 0 or v.data_ptr() % 16 == (off * src.element_size()) % 16   # (an empty view has no address)
    return v


def random_cpu(rng, n, name, family="mixed"):
    """n finite values of the dtype as a CPU tensor: subnormals, both signs, most of the dtype's exponent range"""
    import torch
    lo = {"float32": -140, "float16": -24, "bfloat16": -130}[name]
    hi = {"float32": 120, "float16": 14, "bfloat16": 120}[name]
    x = rng.standard_normal(n)
    if family != "order1":
        x = x * np.exp2(rng.integers(lo, hi, n))
    return torch.from_numpy(x).to(tdt(name))


def narrow_bits(t):
    """the bit pattern of a 0-d / 1-d narrow (or float64) tensor's elements as Python ints"""
    import torch
    it = {8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()]
    mask = (1 << (8 * t.element_size())) - 1
    return [int(v) & mask for v in t.reshape(-1).view(it).cpu().tolist()]


def check_record(ex, rec, T, what, flags=0):
    r = ex.read_record(rec)
    assert r.flags == flags, (what, r.flags)
    assert (r.digits == L.digits_of(T)).all(), (what, "digits")
    assert int(r.words[OUT_EXACT]) & (2**64 - 1) == L.round_to(T, "float64"), (what, "OUT_EXACT")


# ---------------------------------------------------------------------------------------------
# Tier 1
# ---------------------------------------------------------------------------------------------
def sizes(name):
    t = TILE[name]
    return [0, 1, 2, 3, 7, 8, 9, t - 1, t, t + 1, 2 * t + 1]


@pytest.mark.parametrize("name", L.NARROW)
def test_exsum_dev_sizes_offsets_and_kernels(ex, name):
    """every size x every offset from a 16-byte boundary x fpe 0 (superaccumulators), 4 and 8 (expansions): digits, the
    double, the flags, the rounded narrow result, and kernel 5"""
    rng = np.random.default_rng(11)
    for n in sizes(name):
        src = random_cpu(rng, n, name)
        T = L.units(src)
        for off in range(PER16[name]):
            x = place(src, off)
            for fpe in (0, 4, 8):
                rec = ex.exsum_lp_dev(x, fpe=fpe)
                check_record(ex, rec, T, (name, n, off, fpe))
                if n:
                    assert ex.last_blas1_info()[0] == K_SUM
            got = narrow_bits(ex.round_records_dev(rec, tdt(name)))[0]
            assert got == L.round_to(T, name), (name, n, off, hex(got))


@pytest.mark.parametrize("name", L.NARROW)
def test_exdot_dev_sizes_offsets_and_kernels(ex, name):
    """as above for ExDOT: equal misalignment of the operands takes the vector kernel (7), unequal the strided one (8)"""
    rng = np.random.default_rng(12)
    per = PER16[name]
    for n in sizes(name):
        a, b = random_cpu(rng, n, name), random_cpu(rng, n, name)
        T = L.units(a, b)
        for off in range(per):
            for offb, kernel in ((off, K_DOT), ((off + 1 + off % (per - 1)) % per, K_DOT_STRIDED)):
                assert (offb == off) == (kernel == K_DOT)
                x, y = place(a, off), place(b, offb)
                for fpe in (0, 4, 8):
                    rec = ex.exdot_lp_dev(x, y, fpe=fpe)
                    check_record(ex, rec, T, (name, n, off, offb, fpe))
                    if n:
                        assert ex.last_blas1_info()[0] == kernel, (name, n, off, offb)
        got = narrow_bits(ex.round_records_dev(rec, tdt(name)))[0]
        assert got == L.round_to(T, name), (name, n)


@pytest.mark.parametrize("name", L.NARROW)
def test_increments(ex, name):
    """increments 2 and 3 take the strided kernels (6, 8)"""
    rng = np.random.default_rng(13)
    t = TILE[name]
    for n in (1, 9, t + 1):
        for inc in (2, 3):
            a, b = random_cpu(rng, n * inc, name), random_cpu(rng, n * 2, name)
            x, y = place(a, 1), place(b, 0)
            for fpe in (0, 8):
                check_record(ex, ex.exsum_lp_dev(x, fpe=fpe, inca=inc, n=n), L.units(a[::inc]), (name, n, inc, fpe))
                assert ex.last_blas1_info()[0] == K_SUM_STRIDED
                check_record(ex, ex.exdot_lp_dev(x, y, fpe=fpe, incx=inc, incy=2, n=n), L.units(a[::inc], b[::2]),
                             (name, n, inc, fpe, "dot"))
                assert ex.last_blas1_info()[0] == K_DOT_STRIDED


@pytest.mark.parametrize("name", L.NARROW)
def test_every_entry(ex, name):
    """_ctx, host, accumulate + finish and exsum_to / exdot_to give what _dev gives: the Python-integer total"""
    import torch
    rng = np.random.default_rng(14)
    n = TILE[name] + 5
    a, b = random_cpu(rng, n, name), random_cpu(rng, n, name)
    x, y = place(a, 3), place(b, 3)
    Ts, Td = L.units(a), L.units(a, b)
    ctx = ex.Context()
    try:
        check_record(ex, ctx.exsum_lp(x), Ts, "ctx sum")
        check_record(ex, ctx.exdot_lp(x, y, fpe=0), Td, "ctx dot")
        ctx.exsum_lp_accumulate(x[:100])
        ctx.exsum_lp_accumulate(x[100:], fpe=0)
        check_record(ex, ctx.finish(), Ts, "ctx accumulate")
        assert narrow_bits(ctx.exsum_to(x))[0] == L.round_to(Ts, name)
    finally:
        ctx.destroy()
    ex.exdot_lp_accumulate_dev(x[:7], y[:7])
    ex.exdot_lp_accumulate_dev(x[7:], y[7:])
    check_record(ex, ex.finish_dev(), Td, "accumulate dot")
    for target in L.ALL:
        out = ex.exsum_to_dev(x, tdt(target))
        assert out.dtype == tdt(target) and out.dim() == 0
        assert narrow_bits(out)[0] == L.round_to(Ts, target), (name, target)
        assert narrow_bits(ex.exdot_to_dev(x, y, tdt(target)))[0] == L.round_to(Td, target), (name, target)
    assert ex.exsum_to_dev(x).dtype == tdt(name)
    host_a = a if name == "bfloat16" else a.numpy()
    host_b = b if name == "bfloat16" else b.numpy()
    r = ex.exsum_lp(host_a)
    assert (r.digits == L.digits_of(Ts)).all() and r.flags == 0
    r = ex.exdot_lp(host_a, host_b, fpe=0)
    assert (r.digits == L.digits_of(Td)).all() and r.flags == 0
    # float64 forwards to the fp64 entry: the same record
    xd = x.double()
    assert torch.equal(ex.exsum_lp_dev(xd), ex.exsum_dev(xd))
    assert torch.equal(ex.exdot_lp_dev(xd, y.double()), ex.exdot_dev(xd, y.double()))


@pytest.mark.parametrize("name", L.NARROW)
def test_planted_input_totals(ex, name):
    """ties, near-ties, the largest finite values and subnormal inputs of the dtype itself: record and narrow result"""
    for kind, T, pats in L.input_cases(name):
        x = place(L.as_torch(pats, name), 1)
        for fpe in (0, 8):
            rec = ex.exsum_lp_dev(x, fpe=fpe)
            check_record(ex, rec, T, (name, kind, fpe))
        assert narrow_bits(ex.round_records_dev(rec, tdt(name)))[0] == L.round_to(T, name), (name, kind)


@pytest.mark.parametrize("target", L.NARROW)
def test_double_rounding_traps(ex, target):
    """float32 inputs whose exact sum rounds differently in one step than through a double: exsum_to rounds once"""
    import torch
    hit = 0
    for T, one, two in L.traps(target):
        pats = L.realise(T, "float32")
        if pats is None:
            continue
        x = place(L.as_torch(pats, "float32"), 0)
        rec = ex.exsum_lp_dev(x)
        assert narrow_bits(ex.round_records_dev(rec, tdt(target)))[0] == one != two
        through_double = rec[:1].view(torch.float64).to(tdt(target))
        assert narrow_bits(through_double)[0] == two          # the route this feature replaces
        hit += 1
    assert hit >= 8


# ---------------------------------------------------------------------------------------------
# Tier 2: the fp64 path on the widened data
# ---------------------------------------------------------------------------------------------
def family_data(name, family, n, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, device="cuda", generator=g)
    if family == "wide":
        lo, hi = (-24, 14) if name == "float16" else (-120, 120)
        x = x * torch.exp2(torch.randint(lo, hi, (n,), device="cuda", generator=g).float())
    x = x.to(tdt(name))
    if family == "cancel":
        h = n // 2
        x[h:2 * h] = -x[:h][torch.randperm(h, device="cuda", generator=g)]
    return x


def span_bits(x):
    """bits between the highest leading bit and the lowest set bit of the elements' units"""
    pats, name = L.patterns(x)
    m, s = L._split(pats, name)
    nz = m != 0
    top = max(int(abs(int(v))).bit_length() + int(sh) for v, sh in zip(m[nz], s[nz]))
    return top - int(s[nz].min())


@pytest.mark.parametrize("family", ("order1", "wide", "cancel"))
@pytest.mark.parametrize("name", L.NARROW)
def test_records_equal_fp64_path_at_1_to_4_tiles(ex, name, family):
    import torch
    t = TILE[name]
    fpe = 4 if family == "wide" else 8
    if family == "wide" and name != "float16":
        # more than an expansion of 4 holds: waves spill and enter the adaptive bypass
        assert span_bits(family_data(name, family, 4096, 5)) > 4 * 53
    probe = family_data(name, "order1", 4096 * t, 1)       # large enough to reach the grids' caps
    ex.exsum_lp_dev(probe)
    gs = ex.last_blas1_info()[1]
    ex.exdot_lp_dev(probe, probe)
    gd = ex.last_blas1_info()[1]
    del probe
    nmax = max(gs, gd + 2) * t * 4 + 13
    x, y = family_data(name, family, nmax, 21), family_data(name, "order1", nmax, 22)
    xd, yd = x.double(), y.double()
    for k in (1, 2, 3, 4):
        n = gs * t * k + 13
        rec = ex.exsum_lp_dev(x[:n], fpe=fpe)
        assert ex.last_blas1_info()[:2] == (K_SUM, gs)
        assert torch.equal(rec, ex.exsum_dev(xd[:n])), (name, family, k, "sum")
        assert torch.equal(ex.exsum_lp_dev(x[:n], fpe=0), ex.exsum_dev(xd[:n], fpe=0)), (name, family, k, "sum, fpe 0")
        for _ in range(3):                                 # (ExDOT's grid depends on n: settle on the grid n gets)
            n = gd * t * k + 13
            rec = ex.exdot_lp_dev(x[:n], y[:n], fpe=fpe)
            kernel, g2 = ex.last_blas1_info()[:2]
            if g2 == gd:
                break
            gd = g2
        assert kernel == K_DOT and g2 == gd and n <= nmax, (k, gd, g2)
        assert torch.equal(rec, ex.exdot_dev(xd[:n], yd[:n])), (name, family, k, "dot")


def test_tuning_does_not_change_the_record():
    """two launches of one input under different exblas_set_tuning block counts: the same records.  The knob is
    process-wide and cannot be put back one kernel at a time, so the launches run in a child process."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "lowp_tuning_worker.py"), ROOT], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "same records: True" in r.stdout and "grids differ: True" in r.stdout, \
        (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------------------------------------
# mixed reductions, flags, round_records, graphs
# ---------------------------------------------------------------------------------------------
def test_mixed_dtypes_fold_into_one_reduction(ex):
    import torch
    rng = np.random.default_rng(15)
    parts = [random_cpu(rng, 5000 + i, name) for i, name in enumerate(L.NARROW)]
    d = torch.from_numpy(rng.standard_normal(3001) * np.exp2(rng.integers(-300, 300, 3001)))
    T = sum(L.units(p) for p in parts) + L.units(d)
    for i, p in enumerate(parts):
        ex.exsum_lp_accumulate_dev(place(p, i + 1), fpe=(0, 4, 8)[i])
    ex.exsum_accumulate_dev(d.cuda())
    check_record(ex, ex.finish_dev(), T, "mixed")


@pytest.mark.parametrize("name", L.NARROW)
def test_product_range_ends_set_no_product_flags(ex, name):
    """products at 2^-298 (float32) and nearly 2^256: exact in the main accumulator, flag bits 3 to 6 clear"""
    a, b = L.dot_range_pairs(name)
    x, y = L.as_torch(a, name), L.as_torch(b, name)
    T = L.units(x, y)
    for reps in (1, 700):                                   # short (head / tail lanes) and through the vector loop
        xs, ys = place(x.repeat(reps), 2), place(y.repeat(reps), 2)
        for fpe in (0, 4, 8):
            check_record(ex, ex.exdot_lp_dev(xs, ys, fpe=fpe), T * reps, (name, reps, fpe))
        check_record(ex, ex.exdot_lp_dev(xs, ys[1:], n=xs.numel() - 1), L.units(xs[:-1].cpu(), ys[1:].cpu()), "strided")


@pytest.mark.parametrize("name", L.NARROW)
def test_nonfinite_tables_match_the_fp64_path(ex, name):
    import torch
    for key, (vals, (a, b), flags) in L.NONFINITE.items():
        for pad in (0, 3 * TILE[name]):
            filler = [0.5] * pad
            if vals is not None:
                x = torch.tensor(filler + vals, dtype=torch.float64).to(tdt(name)).cuda()
                rec = ex.exsum_lp_dev(x)
                assert torch.equal(rec, ex.exsum_dev(x.double())) and int(rec[OUT_FLAGS]) == flags, (name, key, pad)
                out = ex.round_records_dev(rec, tdt(name))
                assert narrow_bits(out) == narrow_bits(rec[:1].view(torch.float64).to(tdt(name))), (name, key)
            x = torch.tensor(filler + a, dtype=torch.float64).to(tdt(name)).cuda()
            y = torch.tensor(filler + b, dtype=torch.float64).to(tdt(name)).cuda()
            for fpe in (0, 8):
                rec = ex.exdot_lp_dev(x, y, fpe=fpe)
                assert torch.equal(rec, ex.exdot_dev(x.double(), y.double())) and int(rec[OUT_FLAGS]) == flags, (name, key, pad)
            out = ex.exdot_to_dev(x, y)
            assert narrow_bits(out) == narrow_bits(rec[:1].view(torch.float64).to(tdt(name))), (name, key)


@functools.lru_cache(maxsize=None)
def batch_totals():
    out = []
    for name in L.ALL:
        out += [c.T for c in L.planted(name)[::3]]
    for name in L.NARROW:
        out += [T for T, _, _ in L.traps(name)]
    return out + L.random_totals(9, 1)[::16]


def test_round_records_batch(ex):
    """[count, 128] records -- planted totals of every format, the traps, random totals (written as digit sets), records
    made by the fp64 entries, and one with a flag bit set -- rounded into every format"""
    import torch
    Ts = list(batch_totals())
    rng = np.random.default_rng(16)
    d = rng.standard_normal(777) * np.exp2(rng.integers(-200, 200, 777))
    da = torch.from_numpy(d).cuda()
    made = [ex.exsum_dev(da), ex.exdot_dev(da, da.flip(0))]
    Ts += [L.units(d), None]
    recs = torch.zeros(len(Ts) + 1, 128, dtype=torch.int64)
    for i, T in enumerate(Ts[:-2]):
        recs[i, OUT_DIGITS:OUT_DIGITS + 68] = torch.from_numpy(L.digits_of(T))
        recs[i, OUT_EXACT] = int(np.array([L.round_to(T, "float64")], dtype=np.uint64).view(np.int64)[0])
    recs = recs.cuda()
    recs[len(Ts) - 2], recs[len(Ts) - 1] = made
    Ts[-1] = exact_int_from_digits(ex.read_record(made[1]).digits)
    assert ex.read_record(made[1]).flags & 8 == 0            # (no product below 2^-1074: the digits are the total)
    inf_rec = ex.exsum_lp_dev(torch.tensor([1.0, float("-inf")], device="cuda"))
    recs[len(Ts)] = inf_rec
    for target in L.ALL:
        out = ex.round_records_dev(recs, tdt(target))
        assert out.shape == (len(Ts) + 1,) and out.dtype == tdt(target)
        got = narrow_bits(out)
        want = [L.round_to(T, target) for T in Ts]
        bad = [(i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert not bad, (target, bad[:5])
        prec, emin, emax, width = L.FORMATS[target]
        assert got[-1] == (1 << (width - 1)) | ((2 * emax + 1) << (prec - 1)), (target, hex(got[-1]))   # -Inf
        if target == "float64":
            assert got == [int(v) & (2**64 - 1) for v in recs[:, OUT_EXACT].cpu().tolist()]
    # a strided batch and a single record
    wide = torch.zeros(len(Ts) + 1, 160, dtype=torch.int64, device="cuda")
    wide[:, :128] = recs
    assert narrow_bits(ex.round_records_dev(wide[:, :128], tdt("float16"))) == narrow_bits(ex.round_records_dev(recs, tdt("float16")))
    assert ex.round_records_dev(recs[3], tdt("bfloat16")).dim() == 0


@pytest.mark.parametrize("name", L.NARROW)
def test_captured_graph_replays_on_new_data(ex, name):
    """one graph of exsum_lp + round_records, captured after a warm call, replayed three times on new data"""
    import torch
    rng = np.random.default_rng(17)
    n = 3 * TILE[name] + 77
    sets = [random_cpu(rng, n, name) for _ in range(4)]
    x = place(sets[3], 5)
    rec, out = ex.new_record_buffer(), torch.zeros((), dtype=tdt(name), device="cuda")
    ex.round_records_dev(ex.exsum_lp_dev(x, out=rec), tdt(name), out=out)           # warm
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            ex.round_records_dev(ex.exsum_lp_dev(x, out=rec), tdt(name), out=out)
    for r in range(3):
        x.copy_(sets[r])
        rec.fill_(-1)
        out.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        T = L.units(sets[r])
        check_record(ex, rec, T, (name, "replay", r))
        assert narrow_bits(out)[0] == L.round_to(T, name), (name, r)
    del g
