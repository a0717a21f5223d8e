"""ExBGEMM benchmark: the block update Y = alpha X C + beta Y on row-major blocks, X n x p, C p x q, Y n x q, at n = 2^21
and 2^16 with (p, q) = (4, 4), (16, 16) and (64, 64), each as the update of a Krylov iteration (alpha = -1, beta = 1) and
as a plain product (alpha = 1, beta = 0), up to three ways on the same blocks:
  exbgemm_us   one exbgemm_dev call
  exspmm_us    exspmm_dev on X stored as a dense CSR matrix (int32 indices; row_ptr and col_idx are built once, outside
               the timing): the same bits by contract, and what a caller without ExBGEMM has
  exgemm_us    exgemm_dev ('N', 'N', row-major), only where its contract gives the same value: alpha = 1, beta = 0
Before anything is timed the results are asserted to be bit-identical.  The routines are then timed interleaved (one of
each per repetition, device events around each call; Y is restored before the events), --repeats (10) repetitions
after the warm round, and reported as median with the spread (min, max) and, for ExBGEMM, the fraction of 8 TB/s that
the bytes of X, Y in (beta != 0) and Y out amount to.  An ExGEMM call that takes longer than a second is timed three
times only.  Per configuration one JSON line is printed and appended to --out, then the table, and the verdict on
n = 2^21, p = q = 16: ExBGEMM must beat the ExSpMM form by more than the sum of the two (max - min) spreads.

    python tools/bench_bgemm.py [--ns 2097152,65536] [--pq 4x4,16x16,64x64] [--repeats 10] [--out profiles/bgemm_bench.jsonl]
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

HBM_BYTES_PER_US = 8e12 / 1e6


def dense_csr(n, p):
    """int32 (row_ptr, col_idx) of the n x p CSR matrix that stores every entry of a dense block"""
    crow = (torch.arange(n + 1, dtype=torch.int64, device="cuda") * p).int()
    col = torch.arange(p, dtype=torch.int32, device="cuda").repeat(n)
    return crow, col


def timed(prep, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prep()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "count": len(ts)}


def run(n, p, q, alpha, beta, repeats, out_path):
    g = torch.Generator("cuda").manual_seed(100 + p + q)
    rand = lambda *shape: 2.0 * torch.rand(*shape, dtype=torch.float64, device="cuda", generator=g) - 1.0  # noqa: E731
    X, C, Y0 = rand(n, p), rand(p, q), rand(n, q)
    Y, V, W = torch.empty_like(Y0), torch.empty_like(Y0), torch.empty_like(Y0)
    crow, col = dense_csr(n, p)
    A = (crow, col, X.view(-1), (n, p))
    with_gemm = alpha == 1.0 and beta == 0.0

    def block():
        ex.exbgemm_dev(X, C, alpha, beta, Y, 8, True)

    def sparse():
        ex.exspmm_dev(A, C, alpha, beta, V, 8, True)

    def gemm():
        ex.exgemm_dev("N", "N", n, q, p, alpha, X, p, C, q, beta, W, q, 8, True)

    ex.set_bgemm_path(0)
    ex.set_spmm_path(0)
    restore = {"exbgemm": lambda: Y.copy_(Y0), "exspmm": lambda: V.copy_(Y0), "exgemm": lambda: W.copy_(Y0)}
    calls = {"exbgemm": block, "exspmm": sparse}
    if with_gemm:
        calls["exgemm"] = gemm
    warm, info = {}, None
    for name, fn in calls.items():          # the warm round sizes the workspaces; then the bits, before any timing
        warm[name] = timed(restore[name], fn)
        if name == "exbgemm":               # (the next routine reuses the workspace that holds the counters)
            info = ex.last_bgemm_info()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(Y).all()), "the result is not finite"
    assert bool((Y.view(torch.int64) == V.view(torch.int64)).all()), "exbgemm_dev differs from exspmm_dev on the dense CSR"
    if with_gemm:
        assert bool((Y.view(torch.int64) == W.view(torch.int64)).all()), "exbgemm_dev differs from exgemm_dev"
    reps = {name: repeats for name in calls}
    if with_gemm and warm["exgemm"] > 1e6:
        reps["exgemm"] = 3
    t = {name: [] for name in calls}
    for i in range(repeats):                # interleaved: one of each per repetition
        for name, fn in calls.items():
            if i < reps[name]:
                t[name].append(timed(restore[name], fn))
        print(f"# n={n} p={p} q={q} alpha={alpha} beta={beta} {i + 1}/{repeats}: "
              + ", ".join(f"{name} {ts[-1]:.0f} us" for name, ts in t.items()), file=sys.stderr, flush=True)
    nbytes = 8 * (n * p + n * q * (2 if beta != 0.0 else 1))
    out = {"n": n, "p": p, "q": q, "alpha": alpha, "beta": beta, "repeats": repeats, "info": info, "bits_equal": True,
           "bytes": nbytes}
    for name, ts in t.items():
        out[f"{name}_us"] = summary(ts)
    spread = lambda s: s["max"] - s["min"]  # noqa: E731
    out["hbm_fraction"] = nbytes / out["exbgemm_us"]["median"] / HBM_BYTES_PER_US
    out["speedup_vs_exspmm"] = out["exspmm_us"]["median"] / out["exbgemm_us"]["median"]
    if with_gemm:
        out["speedup_vs_exgemm"] = out["exgemm_us"]["median"] / out["exbgemm_us"]["median"]
    out["gap_us"] = out["exspmm_us"]["median"] - out["exbgemm_us"]["median"]
    out["spread_us"] = spread(out["exspmm_us"]) + spread(out["exbgemm_us"])
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
    ap.add_argument("--ns", default=f"{1 << 21},{1 << 16}")
    ap.add_argument("--pq", default="4x4,16x16,64x64")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bgemm_bench.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "the median is over at least 10 repetitions"
    ex.load_library().exblas_hip_init(-1)
    rows = []
    for n in (int(v) for v in a.ns.split(",")):
        for p, q in (tuple(int(v) for v in s.split("x")) for s in a.pq.split(",")):
            for alpha, beta in ((-1.0, 1.0), (1.0, 0.0)):
                rows.append(run(n, p, q, alpha, beta, a.repeats, a.out))
                torch.cuda.empty_cache()
    fmt = lambda s: f"{s['median'] / 1e3:.3f} ({s['min'] / 1e3:.3f}-{s['max'] / 1e3:.3f})" if s else "-"  # noqa: E731
    print("| n | p | q | alpha, beta | ExBGEMM ms | of 8 TB/s | ExSpMM (dense CSR) ms | ExGEMM ms | vs ExSpMM |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['p']} | {r['q']} | {r['alpha']:g}, {r['beta']:g} | {fmt(r['exbgemm_us'])} | "
              f"{100 * r['hbm_fraction']:.1f} % | {fmt(r['exspmm_us'])} | {fmt(r.get('exgemm_us'))} | "
              f"{r['speedup_vs_exspmm']:.2f}x |")
    for r in rows:
        if r["n"] == 1 << 21 and r["p"] == 16 and r["q"] == 16:
            print(f"speed condition, n = 2^21, p = q = 16, alpha = {r['alpha']:g}, beta = {r['beta']:g}: gap "
                  f"{r['gap_us'] / 1e3:.3f} ms, spread {r['spread_us'] / 1e3:.3f} ms: "
                  f"{'MET' if r['faster_beyond_spread'] else 'NOT MET'}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
