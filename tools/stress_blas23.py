"""Randomised soak of ExGEMV / ExGEMM against the oracle: python tools/stress_blas23.py [iterations] [seed].
Random shapes, transposes, alpha/beta, leading dimensions, strides and variants; bits must equal the oracle's.
After those cases (unchanged by this: it draws from a generator of its own) a `planted` family: iterations / 10 cases
(at least 4) of tests/exact_cases.py's planted ties for ExGEMV ('N' / 'T', the half unit or the deciding unit planted in
y through beta = 1 or -0.75, strides, offsets) and ExGEMM, judged by the Python integer reference."""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # noqa: F401
import exblas_amd as ex
from oracle import pyoracle as o

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 200
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
lib = ex.load_library()
lib.exblas_hip_init(-1)
gv_variants = [(0, False), (2, False), (3, False), (4, False), (6, False), (8, False), (4, True), (6, True), (8, True)]
gm_variants = [(0, False), (3, False), (4, False), (8, False), (4, True), (6, True), (8, True)]
kinds = [("fpuniform", 10, 0), ("fpuniform_signed", 40, 20), ("fpuniform_signed", 200, 100), ("lognormal", 0.0, 2.0),
         ("ill_cond", 1e16, 0)]
scalars = [0.0, 1.0, -1.0, 2.5, -0.3, 1e-3]
bits = lambda v: np.ascontiguousarray(v, dtype=np.float64).view(np.int64)  # noqa: E731
t0 = time.time()
bad = 0
fast = 0
for it in range(iters):
    kind, p0, p1 = kinds[int(rng.integers(0, len(kinds)))]
    seed = int(rng.integers(1, 1 << 30))
    if it % 3 != 2:
        m, n = int(rng.integers(1, 900)), int(rng.integers(1, 900))
        trans = str(rng.choice(["N", "T"]))
        lda = m + int(rng.integers(0, 4))
        incx, incy = int(rng.choice([1, 1, 2])), int(rng.choice([1, 1, 3]))
        offa, offx, offy = int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(0, 3))
        alpha, beta = float(rng.choice(scalars[1:])), float(rng.choice(scalars))
        rows, inner = (n, m) if trans == "T" else (m, n)
        a = o.gen(kind, lda * n + offa, seed, p0, p1)
        x = o.gen(kind, (inner - 1) * incx + 1 + offx, seed + 1, p0, p1)
        y0 = o.gen(kind, (rows - 1) * incy + 1 + offy, seed + 2, p0, p1)
        fpe, ee = gv_variants[int(rng.integers(0, len(gv_variants)))]
        want = o.exgemv(trans, m, n, alpha, a, lda, x, beta, y0, 0, incx=incx, incy=incy, offa=offa, offx=offx, offy=offy)
        y = y0.copy()
        ex.exgemv(trans, m, n, alpha, a, lda, offa, x, incx, offx, beta, y, incy, offy, fpe, ee)
        ok = (bits(y) == bits(want)).all()
        desc = f"gemv {trans} m={m} n={n} lda={lda} inc={incx},{incy} off={offa},{offx},{offy} a={alpha} b={beta}"
    else:
        m, n, k = int(rng.integers(1, 200)), int(rng.integers(1, 200)), int(rng.integers(1, 400))
        ta, tb = str(rng.choice(["N", "T"])), str(rng.choice(["N", "T"]))
        lda = (m if ta == "T" else k) + int(rng.integers(0, 3))
        ldb = (k if tb == "T" else n) + int(rng.integers(0, 3))
        ldc = n + int(rng.integers(0, 3))
        alpha, beta = float(rng.choice(scalars[1:])), float(rng.choice(scalars))
        a = o.gen(kind, (k if ta == "T" else m) * lda, seed, p0, p1)
        b = o.gen(kind, (n if tb == "T" else k) * ldb, seed + 1, p0, p1)
        c0 = o.gen(kind, m * ldc, seed + 2, p0, p1)
        fpe, ee = gm_variants[int(rng.integers(0, len(gm_variants)))]
        want = o.exgemm(ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c0, ldc, 0)
        c = c0.copy()
        ex.exgemm(ta, tb, m, n, k, alpha, a, lda, b, ldb, beta, c, ldc, fpe, ee)
        fast += lib.exblas_last_gemm_slices() >= 2
        # the padding columns of C (ldc > n) must stay untouched, the rest must match
        ok = (bits(c) == bits(want)).all()
        desc = f"gemm {ta}{tb} m={m} n={n} k={k} ld={lda},{ldb},{ldc} a={alpha} b={beta} slices={lib.exblas_last_gemm_slices()}"
    if not ok:
        bad += 1
        print(f"MISMATCH it={it} {desc} kind={kind} fpe={fpe} ee={ee}", flush=True)
    if it % 40 == 0:
        print(f"it {it}: {desc} kind={kind} fpe={fpe}{'ee' if ee else ''} [{time.time() - t0:.0f} s]", flush=True)
# planted ties: every output an exact tie, one unit off a tie or a carry into the next binade
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
try:
    import exact_cases as xc  # noqa: E402
except ImportError:                                # a tree without tests/exact_cases.py: the cases above are the whole run
    xc = None
    print("planted family not run: tests/exact_cases.py is not in this tree", flush=True)
prng = np.random.default_rng([int(sys.argv[2]) if len(sys.argv) > 2 else 1, 0x71e5])
planted = max(4, iters // 10) if xc else 0
for it in range(planted):
    S, layout = int(prng.choice([54, 61, 84, 100, 118])), str(prng.choice(xc.LAYOUTS))
    if it % 3 != 2:
        outputs = int(prng.integers(16, 600))
        inner = int(prng.integers(5, 400)) if prng.random() < 0.5 else int(prng.integers(2000, 4000))
        plant, beta = [(None, 0), ("H", 1), ("d", 1), ("H", -0.75), ("d", -0.75)][int(prng.integers(0, 5))]
        case = xc.planted_gemv(outputs, inner, S, seed=it, layout=layout, plant=plant, beta=beta)
        trans = str(prng.choice(["N", "T"]))
        incx, incy = int(prng.choice([1, 1, 2])), int(prng.choice([1, 1, 3]))
        offa, offx, offy = int(prng.integers(0, 3)), int(prng.integers(0, 3)), int(prng.integers(0, 3))
        m, n, a, lda, x, y = xc.gemv_operands(case.g, case.x, case.y0, trans, pad=int(prng.integers(0, 4)), offa=offa,
                                              incx=incx, offx=offx, incy=incy, offy=offy)
        fpe, ee = gv_variants[int(prng.integers(0, len(gv_variants)))]
        want = y.copy()
        want[offy::incy] = case.want
        ex.exgemv(trans, m, n, 1.0, a, lda, offa, x, incx, offx, case.beta, y, incy, offy, fpe, ee)
        ok = (bits(y) == bits(want)).all()
        desc = f"gemv {trans} m={m} n={n} lda={lda} inc={incx},{incy} off={offa},{offx},{offy} S={S} {layout} plant={plant} b={beta}"
    else:
        m, n, k = int(prng.integers(1, 200)), int(prng.integers(16, 200)), int(prng.integers(5, 400))
        ta, tb = str(prng.choice(["N", "T"])), str(prng.choice(["N", "T"]))
        case = xc.planted_gemm(m, n, k, S, seed=it, layout=layout)
        a, lda = xc.gemm_operand(case.a, ta, int(prng.integers(0, 3)))
        b, ldb = xc.gemm_operand(case.b, tb, int(prng.integers(0, 3)))
        fpe, ee = gm_variants[int(prng.integers(0, len(gm_variants)))]
        c = np.zeros(m * n)
        ex.exgemm(ta, tb, m, n, k, 1.0, a, lda, b, ldb, 0.0, c, n, fpe, ee)
        fast += lib.exblas_last_gemm_slices() >= 2
        ok = (bits(c) == bits(case.want.reshape(-1))).all()
        desc = f"gemm {ta}{tb} m={m} n={n} k={k} ld={lda},{ldb} S={S} {layout} slices={lib.exblas_last_gemm_slices()}"
    if not ok:
        bad += 1
        print(f"MISMATCH planted it={it} {desc} fpe={fpe} ee={ee}", flush=True)
print(f"done: {iters} cases + {planted} planted, {bad} mismatches, {fast} gemm cases on the MFMA path, {time.time() - t0:.0f} s")
sys.exit(1 if bad else 0)
