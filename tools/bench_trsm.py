"""ExTRSM benchmark: one dense lower triangle (column-major, NaN in the other triangle) of n = 2048 and 8192 with k = 4, 16
and 64 right-hand sides, solved as 'L','N' (forward) and 'L','T' (backward), three ways on the same block:
  extrsm_us          one extrsm_dev call
  loop_extrsv_us     the loop of k extrsv_dev calls on the strided columns of the block (x = X + j, incx = ldx): what a
                     caller without ExTRSM does
  exsptrsm_us        exsptrsm_dev on the densified CSR of op(A) (int32 indices), always as a LOWER system: for 'L','T',
                     where op(A) is upper, rows and columns are reversed (the same substitution, the same bits).  The
                     upper form is not used because ExSpTRSM's watchdog limits ONE poll to 2 s and walks a row in
                     storage order: the row of an upper dense matrix begins with its newest dependency, so every wave
                     behind the front sits in one poll for as long as the chain needs to reach it -- at n = 8192,
                     k = 16 (a call of more than 4 s) that poll outlasts the 2 s and the call reports a stall
each including the copy of B into X.  Before anything is timed the three results are asserted to be bit-identical.  The
three are then timed interleaved (one of each per repetition, device events around each call), --repeats (10)
repetitions after one warm round, and reported as median with the spread (min, max).  Per configuration one JSON line is
printed and appended to --out, then the table, and the verdict on n = 8192, k = 16: ExTRSM must beat the loop by more
than the run-to-run spread of the two medians (the sum of their max - min).

    python tools/bench_trsm.py [--ns 2048,8192] [--ks 4,16,64] [--trans N,T] [--repeats 10] [--out profiles/trsm_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import exblas_amd as ex  # noqa: E402


def triangle(n, seed=7):
    """A (strides (1, n): column-major) with a diagonal in [1, 2), a strict lower triangle in (-1, 1) / n, so that the
    solution stays of the order of b, and NaN above the diagonal"""
    g = torch.Generator("cuda").manual_seed(seed)
    store = (2.0 * torch.rand(n, n, dtype=torch.float64, device="cuda", generator=g) - 1.0) / n    # store[j, i] = A[i, j]
    A = store.t()
    A.diagonal().copy_(1.0 + torch.rand(n, dtype=torch.float64, device="cuda", generator=g))
    A.masked_fill_(torch.triu(torch.ones(n, n, dtype=torch.bool, device="cuda"), 1), float("nan"))
    return A


def csr_of_lower(P):
    """int32 CSR of the lower triangle of the Python-indexed matrix P, entries in row-major order"""
    n = P.shape[0]
    idx = torch.tril_indices(n, n, device="cuda")
    val = P[idx[0], idx[1]].contiguous()
    crow = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    crow[1:] = torch.cumsum(torch.arange(1, n + 1, device="cuda"), 0)
    return crow.int(), idx[1].int().contiguous(), val, (n, n)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def run(A, csr, n, k, trans, repeats, out_path):
    g = torch.Generator("cuda").manual_seed(100 + k)
    B = 1.0 + torch.rand(n, k, dtype=torch.float64, device="cuda", generator=g)
    X, V, W = torch.empty_like(B), torch.empty_like(B), torch.empty_like(B)
    Bs = B if trans == "N" else B.flip(0).contiguous()     # the block as the lower CSR system takes it
    lda, ldx = A.stride(1), V.stride(0)

    def block():
        X.copy_(B)
        ex.extrsm_dev(A, X, "L", trans, "N", 8, True)

    def loop():
        V.copy_(B)
        for j in range(k):
            ex.extrsv_dev("L", trans, "N", n, A, lda, V[:, j], 8, True, incx=ldx)

    def sparse():
        W.copy_(Bs)
        ex.exsptrsm_dev(csr, W, "L", "N", 8, True)

    ex.set_trsm_path(0)
    ex.set_sptrsm_path(0)
    block()                                # warm round: sizes the workspace of each; then the bits, before any timing
    info = ex.last_trsm_info()
    loop()
    sparse()
    ex.last_sptrsm_info()                  # (raises if the watchdog of the last call was raised)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(X).all()), "the solution is not finite"
    assert bool((X.view(torch.int64) == V.view(torch.int64)).all()), "extrsm_dev differs from the loop of extrsv_dev"
    Ws = W if trans == "N" else W.flip(0)
    assert bool((X.view(torch.int64) == Ws.contiguous().view(torch.int64)).all()), "extrsm_dev differs from exsptrsm_dev"
    t = {"extrsm": [], "loop": [], "sparse": []}
    for i in range(repeats):               # interleaved: one of each per repetition
        t["extrsm"].append(timed(block))
        t["loop"].append(timed(loop))
        t["sparse"].append(timed(sparse))
        print(f"# n={n} k={k} {trans} {i + 1}/{repeats}: extrsm {t['extrsm'][-1]:.0f} us, loop {t['loop'][-1]:.0f} us, "
              f"exsptrsm {t['sparse'][-1]:.0f} us", file=sys.stderr, flush=True)
    out = {"n": n, "k": k, "uplo": "L", "trans": trans, "repeats": repeats, "info": info, "bits_equal": True,
           "extrsm_us": summary(t["extrsm"]), "loop_extrsv_us": summary(t["loop"]), "exsptrsm_us": summary(t["sparse"])}
    spread = lambda s: s["max"] - s["min"]  # noqa: E731
    out["speedup_vs_loop"] = out["loop_extrsv_us"]["median"] / out["extrsm_us"]["median"]
    out["speedup_vs_exsptrsm"] = out["exsptrsm_us"]["median"] / out["extrsm_us"]["median"]
    out["gap_us"] = out["loop_extrsv_us"]["median"] - out["extrsm_us"]["median"]
    out["spread_us"] = spread(out["loop_extrsv_us"]) + spread(out["extrsm_us"])
    out["faster_beyond_spread"] = out["gap_us"] > out["spread_us"]
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ns", default="2048,8192")
    ap.add_argument("--ks", default="4,16,64")
    ap.add_argument("--trans", default="N,T")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trsm_bench.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "the median is over at least 10 repetitions"
    ex.load_library().exblas_hip_init(-1)
    rows = []
    for n in (int(v) for v in a.ns.split(",")):
        A = triangle(n)
        for trans in a.trans.split(","):
            csr = csr_of_lower(A if trans == "N" else A.t().flip(0, 1))
            for k in (int(v) for v in a.ks.split(",")):
                rows.append(run(A, csr, n, k, trans, a.repeats, a.out))
            del csr
        del A
    fmt = lambda s: f"{s['median'] / 1e3:.2f} ({s['min'] / 1e3:.2f}-{s['max'] / 1e3:.2f})"  # noqa: E731
    print("| n | k | op | ExTRSM ms | loop of k ExTRSV ms | ExSpTRSM (dense CSR) ms | vs loop | vs ExSpTRSM |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['k']} | L,{r['trans']} | {fmt(r['extrsm_us'])} | {fmt(r['loop_extrsv_us'])} | "
              f"{fmt(r['exsptrsm_us'])} | {r['speedup_vs_loop']:.2f}x | {r['speedup_vs_exsptrsm']:.2f}x |")
    for r in rows:
        if r["n"] == 8192 and r["k"] == 16:
            print(f"speed condition, n = 8192, k = 16, L,{r['trans']}: gap {r['gap_us'] / 1e3:.2f} ms, spread "
                  f"{r['spread_us'] / 1e3:.2f} ms: {'MET' if r['faster_beyond_spread'] else 'NOT MET'}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
