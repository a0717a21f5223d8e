"""ExSUM / ExDOT finalize rounding on constructed totals (tests/blas1_cases.py), bit for bit.

Every exact result of the library is rounded by finish_wave (superacc.hip.h): lane-per-limb carry propagation, sign
extension through empty limbs, a two's-complement magnitude from ballot masks and a 64-bit rounding window cut at any
offset inside a 32-bit digit; k_finalize (blas1.hip) adds the split low / high merge of the group accumulators and the
scalar fold of the ExDOT low / high accumulators.  Random data produces none of: a tie, a sticky bit three or more
digits below the window, a 67-lane carry or borrow ripple, a negative total whose borrow crosses empty limbs, a leading
bit on a digit boundary, a total in limbs 64 .. 67.  These inputs do, at every bit position.

Expected bits come from Python integers alone (exact_cases.round_nearest_even, helpers.digits_from_int,
blas1_cases.canon_from_int) in the exact rounding mode, and from the oracle's restatement of the reference's Round() on
those canonical limbs in the reference mode; ExDOT flags from the constructor.  Nothing expected is computed by
exblas_amd.  No tolerance.  Each test prints what it ran (pytest -s)."""
import functools

import numpy as np
import pytest

import blas1_cases as B
from helpers import FPE_VARIANTS_DOT, FPE_VARIANTS_SUM, expected_fields
from helpers import bits as _bits, same_bits as _same_bits

pytestmark = pytest.mark.gpu

NVEC = 33 * 2048 + 3                     # 33 full tiles of the streaming kernel, one remainder vector, one odd element
TILE_VEC, BLOCK = 1024, 256              # double2 vectors per tile, threads per workgroup (blas1.hip: BLOCK, U = 4)
PLACEMENTS = ("lane", "tiles", "edges")
A_LIMBS = (1, 2, 31, 32, 62, 63, 64, 65)
A_VARIANTS = ((0, False), (8, True))
SUM_IDS = [f"fpe{f}{'-ee' if e else ''}" for f, e in FPE_VARIANTS_SUM]
DOT_IDS = [f"fpe{f}{'-ee' if e else ''}" for f, e in FPE_VARIANTS_DOT]


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.load_library().exblas_set_round_mode(0)


@functools.lru_cache(maxsize=None)
def _expected(which):
    """(cases, want bits, reference-mode bits or None, canon [n, 41], digits [n, 68], canon-fits mask) -- computed once"""
    cases = {"sum": B.sum_cases, "bcd": lambda: tuple(c for c in B.sum_cases() if c.family != "A"),
             "a_subset": lambda: tuple(c for c in B.sum_cases() if c.family == "A" and (c.p >> 5) in A_LIMBS),
             "e": lambda: tuple(B.family_e())}[which]()
    return (cases,) + expected_fields(cases)


def _report(what, bad, cases, got, want):
    idx = np.nonzero(bad)[0]
    assert not bad.any(), (what, int(bad.sum()), [(int(i), repr(cases[i]), hex(int(got[i])), hex(int(want[i]))) for i in idx[:6]])


# ---------------------------------------------------------------------------------------------
# the segmented sweep: all of A - D as the segments of one launch
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _segments():
    import torch
    cases = B.sum_cases()
    lens = np.array([len(c.terms) for c in cases], dtype=np.int64)
    vals = np.fromiter((x for c in cases for x in c.terms), dtype=np.float64, count=int(lens.sum()))
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return torch.from_numpy(vals).cuda(), torch.from_numpy(offs).cuda()


@pytest.mark.parametrize("fpe,ee", FPE_VARIANTS_SUM, ids=SUM_IDS)
def test_segmented_sweep(ex, fpe, ee):
    """every case of A - D as one segment (one wave each: the LDS accumulator straight into finish_wave), in the exact
    mode against the integer reference and in the reference mode against the oracle's Round() of the integer limbs"""
    cases, want, ref, _, _, fits = _expected("sum")
    assert fits.all()
    dv, do = _segments()
    lib = ex.load_library()
    got = _bits(ex.exsum_segmented_dev(dv, do, fpe, ee).cpu().numpy())
    _report(("exact mode", fpe, ee), ~_same_bits(got, want), cases, got, want)
    lib.exblas_set_round_mode(1)
    try:
        got_ref = _bits(ex.exsum_segmented_dev(dv, do, fpe, ee).cpu().numpy())
    finally:
        lib.exblas_set_round_mode(0)
    _report(("reference mode", fpe, ee), ~_same_bits(got_ref, ref), cases, got_ref, ref)
    differ = int((~_same_bits(want, ref)).sum())
    assert differ > 0 and (~_same_bits(got, got_ref)).sum() == differ, "the two rounding modes must differ somewhere"
    print(f"segmented fpe={fpe} ee={ee}: {len(cases)} segments, {dv.numel()} doubles, the modes differ on {differ}")


# ---------------------------------------------------------------------------------------------
# k_finalize through exsum_dev: the terms inside a zero vector, three placements
# ---------------------------------------------------------------------------------------------
def _positions(nterms, placement):
    """where term j goes (indices into the vector the kernel is given; `edges`: that vector starts 8 bytes off a 16-byte
    boundary and is one element longer, so that it has a scalar head, a remainder vector and an odd tail element)"""
    j = np.arange(nterms, dtype=np.int64)
    if placement == "lane":
        if nterms <= 8:      # the 4 double2 loads of thread 37 in tile 2: one lane's tile, one expansion
            return 2 * (2 * TILE_VEC + 37 + ((j // 2) % 4) * BLOCK) + (j & 1)
        return 2 * TILE_VEC * 2 + j                              # contiguous from the start of tile 2: 8 per lane and tile
    if placement == "tiles":
        if nterms <= 33:     # a different tile each: different workgroups, different group accumulators
            return 2 * (((3 + 7 * j) % 33) * TILE_VEC + (11 + 5 * j) % BLOCK + (j % 4) * BLOCK) + (j & 1)
        return 2 * j + 1                                         # every other element, through all 33 tiles
    n = NVEC + 1
    first = np.array([0, n - 1, n - 3, n - 2], dtype=np.int64)  # head, odd tail, the remainder vector
    return np.concatenate([first, 1 + np.arange(max(0, nterms - 4))])[:nterms] if nterms > 4 else first[:nterms]


def _run_exsum_dev(ex, which, placement, fpe, ee):
    import torch
    cases, want, ref, canon, digits, fits = _expected(which)
    n = len(cases)
    lens = np.array([len(c.terms) for c in cases], dtype=np.int64)
    assert lens.max() + 8 < NVEC // 2
    offs = np.concatenate([[0], np.cumsum(lens)])
    vals = torch.from_numpy(np.fromiter((x for c in cases for x in c.terms), dtype=np.float64, count=int(offs[-1]))).cuda()
    pos = np.concatenate([_positions(int(k), placement) for k in lens])
    nvec = NVEC + 1 if placement == "edges" else NVEC
    assert pos.min() >= 0 and pos.max() < nvec
    for i in (0, n // 2, n - 1):
        assert len(set(pos[offs[i]:offs[i + 1]].tolist())) == lens[i], "two terms share a position"
    dpos = torch.from_numpy(pos).cuda()
    buf = torch.zeros(NVEC + 2, dtype=torch.float64, device="cuda")
    x = buf[1:1 + nvec] if placement == "edges" else buf[:nvec]
    assert (x.data_ptr() % 16 == 8) == (placement == "edges")
    rec = torch.zeros(n, ex.OUT_WORDS, dtype=torch.int64, device="cuda")
    zero = torch.zeros(int(lens.max()), dtype=torch.float64, device="cuda")
    for i in range(n):
        a, b = int(offs[i]), int(offs[i + 1])
        p = dpos[a:b]
        x.index_copy_(0, p, vals[a:b])
        ex.exsum_dev(x, fpe, ee, n=nvec, out=rec[i])
        x.index_copy_(0, p, zero[:b - a])
    out = rec.cpu().numpy()
    assert not buf.cpu().numpy().any(), "the vector was not left zero"
    what = (which, placement, fpe, ee)
    _report(what + ("exact",), ~_same_bits(out[:, ex.OUT_EXACT], want), cases, out[:, ex.OUT_EXACT], want)
    _report(what + ("flags",), out[:, ex.OUT_FLAGS] != 0, cases, out[:, ex.OUT_FLAGS], np.zeros(n, dtype=np.int64))
    _report(what + ("refmode",), fits & ~_same_bits(out[:, ex.OUT_REFMODE], ref), cases, out[:, ex.OUT_REFMODE], ref)
    got_c, got_d = out[:, ex.OUT_CANON:ex.OUT_CANON + 41], out[:, ex.OUT_DIGITS:ex.OUT_DIGITS + 68]
    bad_c = fits & (got_c != canon).any(axis=1)
    _report(what + ("canon",), bad_c, cases, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
    bad_d = (got_d != digits).any(axis=1)
    _report(what + ("digits",), bad_d, cases, np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64))
    return n


@pytest.mark.parametrize("fpe,ee", FPE_VARIANTS_SUM, ids=SUM_IDS)
def test_exsum_dev_small_carry_and_range_cases(ex, fpe, ee):
    """B, C, D through the streaming kernel and k_finalize, every variant, three placements: record fields and flags"""
    for placement in PLACEMENTS:
        n = _run_exsum_dev(ex, "bcd", placement, fpe, ee)
    print(f"exsum_dev fpe={fpe} ee={ee}: {n} cases of B, C, D x {len(PLACEMENTS)} placements")


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("fpe,ee", A_VARIANTS, ids=["fpe0", "fpe8-ee"])
def test_exsum_dev_position_sweep(ex, fpe, ee, placement):
    """the cases of A whose top digit lies in limbs 1, 2, 31, 32, 62 .. 65 (every leading-zero count in each: the first
    limbs, the middle, and both sides of the hand-over from the first to the second register at lanes 63 / 64)"""
    cases = _expected("a_subset")[0]
    assert {c.p for c in cases} == set(B.a_positions_for_limbs(A_LIMBS))     # (limb 1 from p = 53 on, limb 65 up to p = 2097)
    assert {(c.p >> 5, 31 - (c.p & 31)) for c in cases} >= {(t, lz) for t in A_LIMBS[1:-1] for lz in range(32)}
    n = _run_exsum_dev(ex, "a_subset", placement, fpe, ee)
    print(f"exsum_dev position sweep fpe={fpe} ee={ee} {placement}: {n} cases")


# ---------------------------------------------------------------------------------------------
# exblas_finalize_dev on raw limb sets
# ---------------------------------------------------------------------------------------------
def test_finalize_dev_raw_limb_sets(ex):
    """E: un-normalised sets, out of place and in place (the record written over the sets it was computed from)"""
    import torch
    cases, want, ref, canon, digits, fits = _expected("e")
    n = len(cases)
    assert {c.sets.shape[0] for c in cases} >= set(B.E_NSETS)
    for mode in ("out of place", "in place"):
        recs = []
        for c in cases:
            words = max(ex.OUT_WORDS, ex.OUT_DIGITS + c.sets.size)
            buf = torch.zeros(words, dtype=torch.int64, device="cuda")
            sets = buf[ex.OUT_DIGITS:ex.OUT_DIGITS + c.sets.size]
            sets.copy_(torch.from_numpy(c.sets.ravel()).cuda())
            if mode == "in place":
                recs.append(ex.finalize_dev(sets, out=buf)[:ex.OUT_WORDS])
            else:
                recs.append(ex.finalize_dev(sets))
                assert (sets.cpu().numpy() == c.sets.ravel()).all(), "the input sets were written"
        out = torch.stack(recs).cpu().numpy()
        _report((mode, "exact"), ~_same_bits(out[:, ex.OUT_EXACT], want), cases, out[:, ex.OUT_EXACT], want)
        _report((mode, "flags"), out[:, ex.OUT_FLAGS] != 0, cases, out[:, ex.OUT_FLAGS], np.zeros(n, dtype=np.int64))
        _report((mode, "refmode"), fits & ~_same_bits(out[:, ex.OUT_REFMODE], ref), cases, out[:, ex.OUT_REFMODE], ref)
        z = np.zeros(n, dtype=np.int64)
        _report((mode, "canon"), fits & (out[:, ex.OUT_CANON:ex.OUT_CANON + 41] != canon).any(axis=1), cases, z, z)
        _report((mode, "digits"), (out[:, ex.OUT_DIGITS:ex.OUT_DIGITS + 68] != digits).any(axis=1), cases, z, z)
    print(f"finalize_dev: {n} limb sets, {int(fits.sum())} within the canonical limbs, "
          f"{int(np.isinf([c.want for c in cases]).sum())} round to +-Inf")


# ---------------------------------------------------------------------------------------------
# ExDOT: the fraction rounding and the high fold
# ---------------------------------------------------------------------------------------------
SLOT = 16                                # doubles per case in the packed operand buffers
DOT_LAYOUTS = ("contiguous", "odd", "stride2")


@functools.lru_cache(maxsize=None)
def _dot_operands():
    """the operands of every Family F case packed three ways, on the device: (cases, {layout: (a, b, n per case)})"""
    import torch
    cases = tuple(B.family_f())
    out = {}
    for layout in DOT_LAYOUTS:
        a = np.full(len(cases) * SLOT, np.nan)
        b = np.full(len(cases) * SLOT, np.nan)
        ns = np.zeros(len(cases), dtype=np.int64)
        for i, c in enumerate(cases):
            k = len(c.a)
            assert 2 * k <= SLOT
            ca, cb = c.a, c.b
            if layout != "stride2" and (k % 2 == 1) != (layout == "odd"):      # a 0 * 0 product in front fixes the parity
                ca, cb = np.concatenate([[0.0], ca]), np.concatenate([[0.0], cb])
            ns[i] = len(ca)
            step = 2 if layout == "stride2" else 1                               # stride 2: NaN in between must not be read
            a[i * SLOT:i * SLOT + step * len(ca):step] = ca
            b[i * SLOT:i * SLOT + step * len(cb):step] = cb
        out[layout] = (torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), ns)
    return cases, out


@pytest.mark.parametrize("fpe,ee", FPE_VARIANTS_DOT, ids=DOT_IDS)
def test_exdot_fraction_rounding_and_high_fold(ex, fpe, ee):
    """F: the vector kernel with an even and with an odd length (remainder vectors, scalar tail) and the strided kernel,
    dealt over the cases so that every case meets every layout across the variants: the double and the exact flag word"""
    import torch
    cases, packed = _dot_operands()
    n = len(cases)
    shift = FPE_VARIANTS_DOT.index((fpe, ee))
    rec = torch.zeros(n, ex.OUT_WORDS, dtype=torch.int64, device="cuda")
    used = {l: 0 for l in DOT_LAYOUTS}
    for i in range(n):
        layout = DOT_LAYOUTS[(i + shift) % 3]
        a, b, ns = packed[layout]
        inc = 2 if layout == "stride2" else 1
        ex.exdot_dev(a[i * SLOT:], b[i * SLOT:], fpe, ee, incx=inc, incy=inc, n=int(ns[i]), out=rec[i])
        used[layout] += 1
    out = rec.cpu().numpy()
    want = _bits([c.want for c in cases])
    flags = np.array([c.flags for c in cases], dtype=np.int64)
    _report(("exact", fpe, ee), ~_same_bits(out[:, ex.OUT_EXACT], want), cases, out[:, ex.OUT_EXACT], want)
    _report(("flags", fpe, ee), out[:, ex.OUT_FLAGS] != flags, cases, out[:, ex.OUT_FLAGS], flags)
    print(f"exdot fpe={fpe} ee={ee}: {n} cases, layouts {used}, flag words {sorted(set(flags.tolist()))}")


# ---------------------------------------------------------------------------------------------
# the host-pointer entries
# ---------------------------------------------------------------------------------------------
def test_host_entries(ex):
    """50 cases of every family through exsum_record / exdot_record"""
    cases, want, ref, canon, digits, fits = _expected("sum")
    count = 0
    for family in "ABCD":
        idx = [i for i, c in enumerate(cases) if c.family == family]
        idx = idx[::max(1, len(idx) // 50)][:50] if family != "D" else idx
        assert len(idx) >= min(50, sum(c.family == family for c in cases))
        for k, i in enumerate(idx):
            c = cases[i]
            fpe, ee = FPE_VARIANTS_SUM[k % len(FPE_VARIANTS_SUM)]
            r = ex.exsum_record(len(c.terms), np.array(c.terms), 1, 0, fpe, ee)
            assert _same_bits(_bits([r.exact])[0], want[i]) and _same_bits(_bits([r.refmode])[0], ref[i]), (c, fpe, ee, r.exact)
            assert r.flags == 0 and (r.canon == canon[i]).all() and (r.digits == digits[i]).all(), (c, fpe, ee)
            count += 1
    f = B.family_f()
    sample = f[::len(f) // 50] + f[-12:]              # (the last cases are the sums on either side of what the digits hold)
    assert len(sample) >= 50
    for k, c in enumerate(sample):
        fpe, ee = FPE_VARIANTS_DOT[k % len(FPE_VARIANTS_DOT)]
        r = ex.exdot_record(len(c.a), c.a, 1, 0, c.b, 1, 0, fpe, ee)
        assert _same_bits(_bits([r.exact])[0], _bits([c.want])[0]) and r.flags == c.flags, (c, fpe, ee, r.exact, r.flags)
    print(f"host entries: {count} sums, {len(sample)} dots")
