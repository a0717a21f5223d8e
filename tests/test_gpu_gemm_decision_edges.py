"""ExGEMM's path decision at its edges and at the seams of the operand scan (tests/gemm_decision_cases.py), bit for bit.

The digit-slice and residue paths decide on the device from a scan of fl(alpha A) and B whether they may run; the
fp64-slice path decides on the host from the same scan.  A scan that misses one element is silent: an Inf sliced as
garbage, or a vector scale that makes the fixed-point conversion overflow.  Here one planted element (or one planted
vector) alone decides, at every position where the scan kernels change thread, load, trip, slice or workgroup, in all
four operand layouts with NaN in the padding of the leading dimension; both the reported path and every output bit
are checked, against Python integers (oracle: reference rounding mode only).  Operands stay on the device; a probe
plants its elements and restores them."""
import ctypes as C
import math

import numpy as np
import pytest

import exact_cases as X
import gemm_decision_cases as D
from helpers import assert_bits, bits
from test_gpu_blas23 import GEMM_VARIANTS

pytestmark = pytest.mark.gpu

K_EDGE = 257                                  # the edge tests: eight strided slices, 257 vectors


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    return exblas_amd


@pytest.fixture
def lib(ex):
    """the library with the forced path and the rounding mode put back whatever the test did"""
    L = ex.load_library()
    try:
        yield L
    finally:
        L.exblas_set_gemm_path(0)
        L.exblas_set_round_mode(0)


class Rig:
    """The base operands of one (probed operand, its transpose, k) on the device, padded with NaN."""

    def __init__(self, ex, lib, operand, trans, k):
        import torch
        self.torch, self.ex, self.lib = torch, ex, lib
        self.operand, self.k, self.b = operand, k, D.base(k)
        b, qtrans = self.b, D.partner_trans(operand, trans)
        pmat, qmat = (b.Pf, b.Qf.T) if operand == "A" else (b.Pf.T, b.Qf)
        p, self.ldp = X.gemm_operand(pmat, trans, 2, fill=math.nan)
        q, self.ldq = X.gemm_operand(qmat, qtrans, 1, fill=math.nan)
        self.Pd, self.Qd = torch.from_numpy(p).cuda(), torch.from_numpy(q).cuda()
        stored = self.Pd.view(-1, self.ldp)
        self.pv = stored if D.contiguous(operand, trans) else stored.t()      # pv[v, l]: element l of vector v
        self.ta, self.tb = (trans, qtrans) if operand == "A" else (qtrans, trans)

    def plant(self, v, vec):
        """writes the elements in which vec differs from the base vector; returns what restore() needs"""
        idx = np.flatnonzero(bits(vec) != bits(self.b.Pf[v]))
        self.pv[v, self.torch.from_numpy(idx).cuda()] = self.torch.from_numpy(np.ascontiguousarray(vec[idx])).cuda()
        return v, idx

    def restore(self, planted):
        v, idx = planted
        self.pv[v, self.torch.from_numpy(idx).cuda()] = self.torch.from_numpy(np.ascontiguousarray(self.b.Pf[v][idx])).cuda()

    def run(self, V, beta, variant, alpha=1.0, ctx=None):
        """one call on the first V vectors of the probed operand; returns (info words, C body, C before the call)"""
        m, n = (V, D.NPARTNER) if self.operand == "A" else (D.NPARTNER, V)
        c0 = D.c_template(m, n, beta)
        Cd = self.torch.from_numpy(c0.reshape(-1).copy()).cuda()
        Ad, lda, Bd, ldb = (self.Pd, self.ldp, self.Qd, self.ldq) if self.operand == "A" else (self.Qd, self.ldq, self.Pd, self.ldp)
        fpe, ee = GEMM_VARIANTS[variant % len(GEMM_VARIANTS)]
        (ctx.exgemm if ctx is not None else self.ex.exgemm_dev)(self.ta, self.tb, m, n, self.k, alpha, Ad, lda, Bd, ldb, beta,
                                                                 Cd, n + 2, fpe, ee)
        info = (C.c_int * 8)()
        if ctx is not None:
            assert self.lib.exblas_last_gemm_info_ctx(ctx.handle, info) == 0
        else:
            assert self.lib.exblas_last_gemm_info(info) == 0
        got = Cd.cpu().numpy().reshape(m, n + 2)
        assert (bits(got[:, n:]) == bits(c0[:, n:])).all(), "the padding of C was written"
        return list(info), got[:, :n], c0

    def probe(self, path, V, v, vec, accept, beta=0.0, variant=0, alpha=1.0, ctx=None, what=()):
        """plants vec as vector v, runs on the forced path, checks the decision and every output bit, restores"""
        b = self.b
        s = D.with_vector(b, V, v, vec, self.operand, alpha)
        planted = self.plant(v, vec)
        try:
            if ctx is None:
                self.lib.exblas_set_gemm_path(path)
            info, got, c0 = self.run(V, beta, variant, alpha, ctx)
        finally:
            self.restore(planted)
        what = (self.operand, self.ta, self.tb, self.k, path, V, v, alpha, beta, *what, info)
        if accept:
            want_info = D.expected_info(path, *D.seen_bits(b, V, v, vec, self.operand, alpha), self.k)
            assert info[:len(want_info)] == want_info, (what, want_info)
        else:
            assert info[0] == 0, what
        assert_bits(got, D.with_beta(s, beta, c0), what)
        return info


# ---------------------------------------------------------------------------------------------
# 1, 2: the scan's seams
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operand,trans,k", D.SEAM_IDS)
def test_lone_special_at_every_seam(ex, lib, operand, trans, k):
    """One NaN, +Inf, -Inf or subnormal, everything else well inside the domain: the forced int8 path must decline and
    the scalar kernel's result has NaN / the signed infinity exactly where IEEE puts them (the partner holds 4, 0, -2
    against the special); the subnormal's product is the whole result of its vector."""
    rig = Rig(ex, lib, operand, trans, k)
    for p in D.seam_probes(operand, trans, k):
        if p.kind in D.FLAG_KINDS:
            rig.probe(p.path, p.V, p.v, D.lone_special(rig.b, p.v, p.pos, p.kind), False, p.beta, p.variant, what=(p.kind, p.pos))


@pytest.mark.parametrize("operand,trans,k", D.SEAM_IDS)
def test_lone_scale_setter_at_every_seam(ex, lib, operand, trans, k):
    """The single largest element of its vector (2^60 over a base below 2^7) and the single element with the lowest
    set bit (3 * 2^-60): accepted, with the digit counts / bit counts and moduli the spans imply.  A scan that misses the
    element sizes the fixed-point window without it and the bits are wrong -- no flag is involved."""
    rig = Rig(ex, lib, operand, trans, k)
    for p in D.seam_probes(operand, trans, k):
        if p.kind in ("top", "low"):
            rig.probe(p.path, p.V, p.v, D.lone_setter(rig.b, p.v, p.pos, p.kind), True, p.beta, p.variant, what=(p.kind, p.pos))


# ---------------------------------------------------------------------------------------------
# 3, 4, 5: the rules of the int8 paths
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operand", ["A", "B"])
@pytest.mark.parametrize("sign", [1, -1])
def test_exponent_rule_per_vector(ex, lib, operand, sign):
    """a whole vector (0, 255, 256 = last) with its top exponent at exactly +-300 is accepted, at +-301 declined"""
    rigs = [Rig(ex, lib, operand, t, K_EDGE) for t in ("N", "T")]
    n = 0
    for vi, v in enumerate((0, 255, 256)):
        for edge in (D.I8_ERANGE, D.I8_ERANGE + 1):
            for path in (2, 4):
                rig = rigs[(vi + n) % 2]
                rig.probe(path, D.NVEC, v, D.scaled_vector(rig.b, v, sign * edge), edge == D.I8_ERANGE, float(n % 2), n,
                          what=(sign * edge,))
                n += 1


def test_exponent_rule_through_alpha(ex, lib):
    """the scan looks at fl(alpha A): gemm_decision_cases.alpha_cases on vectors 0, 255 and 256 of A, both layouts"""
    rigs = [Rig(ex, lib, "A", t, K_EDGE) for t in ("N", "T")]
    n = 0
    for vi, v in enumerate((256, 0, 255)):
        rig = rigs[vi % 2]
        pos = D.positions("A", "NT"[vi % 2], K_EDGE)[-1 - vi]
        for name, alpha, vec, accept in D.alpha_cases(rig.b, v, pos):
            for path in ((2, 4) if vi == 0 else ((2, 4)[(n + vi) % 2],)):
                rig.probe(path, D.NVEC, v, vec, accept, float(n % 2), n, alpha=alpha, what=(name, pos))
                n += 1


@pytest.mark.parametrize("operand", ["A", "B"])
def test_span_rule(ex, lib, operand):
    """one vector of exactly 126 bits is accepted (16 digits; the moduli the residue path needs), 127 bits declined"""
    rigs = [Rig(ex, lib, operand, t, K_EDGE) for t in ("N", "T")]
    n = 0
    for vi, v in enumerate((0, 255, 256)):
        for nbits in (D.I8_SPAN, D.I8_SPAN + 1):
            for path in (2, 4):
                rig = rigs[(vi + n) % 2]
                seams = D.positions(operand, "NT"[(vi + n) % 2], K_EDGE)
                info = rig.probe(path, D.NVEC, v, D.span_vector(rig.b, v, seams[n % len(seams)], nbits), nbits == D.I8_SPAN,
                                 float(n % 2), n, what=(nbits,))
                if nbits == D.I8_SPAN:
                    assert info[1 if operand == "A" else 2] == (16 if path == 2 else 126), info
                n += 1


# ---------------------------------------------------------------------------------------------
# 6: the fp64 slices, decided on the host from the same scan
# ---------------------------------------------------------------------------------------------
def test_fp64_slice_path_edges(ex, lib, oracle):
    """84 bits: 4 slices, 85: declined; top exponents +-400 accepted, +-401 declined; nothing but zeros: declined, exact
    zeros (the host's rule reads the exponent range of both operands together: with one of them all zero the other's
    range decides, and the result is exact zeros on whichever path); the reference rounding mode: declined, the oracle's
    bits; a lone NaN / Inf / subnormal at the last position of the last vector in each of the four layouts."""
    n = 0
    for operand, trans in D.LAYOUTS:
        rig = Rig(ex, lib, operand, trans, K_EDGE)
        b, last = rig.b, K_EDGE - 1
        for kind in ("nan", ("+inf", "-inf")[n % 2], "subnormal"):
            rig.probe(3, D.NVEC, D.NVEC - 1, D.lone_special(b, D.NVEC - 1, last, kind), False, float(n % 2), n, what=(kind,))
            n += 1
        v = (0, 255, 256, 255)[n % 4]
        pos = D.positions(operand, trans, K_EDGE)[n % 3]
        for nbits in (D.MFMA_SPAN, D.MFMA_SPAN + 1):
            info = rig.probe(3, D.NVEC, v, D.span_vector(b, v, pos, nbits), nbits == D.MFMA_SPAN, float(n % 2), n, what=(nbits,))
            assert nbits > D.MFMA_SPAN or info[:3] == [1, 4, 4]
            n += 1
        for top in (D.MFMA_ERANGE, -D.MFMA_ERANGE, D.MFMA_ERANGE + 1, -D.MFMA_ERANGE - 1):
            rig.probe(3, D.NVEC, v, D.scaled_vector(b, v, top), abs(top) == D.MFMA_ERANGE, float(n % 2), n, what=(top,))
            n += 1
    rig = Rig(ex, lib, "A", "N", K_EDGE)
    b = rig.b
    lib.exblas_set_gemm_path(3)
    for beta in (0.0, 1.0):                                          # A' = 0 * A: zeros on whichever path
        info, got, c0 = rig.run(D.NVEC, beta, 3, alpha=0.0)
        assert_bits(got, D.with_beta(np.zeros((D.NVEC, D.NPARTNER)), beta, c0), ("A' all zero", beta, info))
    saved = rig.Qd.clone()
    try:
        rig.Qd.zero_()                                               # ... and B: nothing but zeros, declined
        for beta in (0.0, 1.0):
            info, got, c0 = rig.run(D.NVEC, beta, 5, alpha=0.0)
            assert info[0] == 0, info
            assert_bits(got, D.with_beta(np.zeros((D.NVEC, D.NPARTNER)), beta, c0), ("all zero", beta, info))
    finally:
        rig.Qd.copy_(saved)
    info, got, _ = rig.run(D.NVEC, 0.0, 6)                           # back inside: accepted, two slices
    assert info[:3] == D.expected_info(3, b.bits_p[D.NVEC], b.bits_q, K_EDGE) == [1, 2, 2], info
    assert_bits(got, b.want, "base on the fp64 slices")
    lib.exblas_set_round_mode(1)
    want = oracle.exgemm("N", "N", D.NVEC, D.NPARTNER, K_EDGE, 1.0, b.Pf.reshape(-1), K_EDGE, np.ascontiguousarray(b.Qf.T).reshape(-1),
                         D.NPARTNER, 0.0, np.zeros(D.NVEC * D.NPARTNER), D.NPARTNER, 0, mode=oracle.ROUND_REFERENCE)
    info, got, _ = rig.run(D.NVEC, 0.0, 6)
    assert info[0] == 0, info
    assert_bits(got, want.reshape(D.NVEC, D.NPARTNER), "reference rounding mode")


# ---------------------------------------------------------------------------------------------
# 7: nothing is carried from one call to the next
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [2, 4])
def test_no_state_carried_between_calls(ex, lib, oracle, path):
    """On one context: accepted (a 126-bit vector: 16 digits in several passes on the digit path), declined (a lone
    NaN), accepted again (the wide vector elsewhere, then the narrow base), each with its info block and its bits; the
    last accepted product once more in the reference rounding mode against the oracle's ExGEMM."""
    lib.exblas_set_gemm_path(path)                                   # a context inherits the knobs when it is created
    ctx = ex.Context()
    try:
        rig = Rig(ex, lib, "A", ("N", "T")[path == 4], K_EDGE)
        b = rig.b
        seams = D.positions("A", ("N", "T")[path == 4], K_EDGE)
        wide = D.span_vector(b, 256, seams[-1], D.I8_SPAN)
        info = rig.probe(path, D.NVEC, 256, wide, True, 0.0, 1, ctx=ctx, what=("first",))
        assert info[1] == (16 if path == 2 else 126), info
        rig.probe(path, D.NVEC, 256, D.lone_special(b, 256, seams[-1], "nan"), False, 1.0, 2, ctx=ctx, what=("nan",))
        wide0 = D.span_vector(b, 0, seams[1], D.I8_SPAN)
        rig.probe(path, D.NVEC, 0, wide0, True, 1.0, 3, ctx=ctx, what=("again",))
        rig.probe(path, D.NVEC, 255, D.lone_special(b, 255, seams[0], "subnormal"), False, 0.0, 4, ctx=ctx, what=("subnormal",))
        info, got, _ = rig.run(D.NVEC, 0.0, 5, ctx=ctx)
        assert info[:3] == D.expected_info(path, b.bits_p[D.NVEC], b.bits_q, K_EDGE)[:3], info
        assert_bits(got, b.want, ("narrow base", path))
        # the reference rounding mode on the wide product: same decision, the oracle's bits
        a = b.Pf.copy()
        a[0] = wide0
        want = oracle.exgemm("N", "N", D.NVEC, D.NPARTNER, K_EDGE, 1.0, a.reshape(-1), K_EDGE, np.ascontiguousarray(b.Qf.T).reshape(-1),
                             D.NPARTNER, 0.0, np.zeros(D.NVEC * D.NPARTNER), D.NPARTNER, 0, mode=oracle.ROUND_REFERENCE)
        assert not np.isnan(want).any()
        planted = rig.plant(0, wide0)
        try:
            lib.exblas_set_round_mode(1)
            info, got, _ = rig.run(D.NVEC, 0.0, 6, ctx=ctx)
        finally:
            lib.exblas_set_round_mode(0)
            rig.restore(planted)
        assert info[:3] == D.expected_info(path, D.I8_SPAN, b.bits_q, K_EDGE)[:3], info
        assert_bits(got, want.reshape(D.NVEC, D.NPARTNER), ("reference rounding mode", path))
    finally:
        ctx.destroy()
