"""ExBTRSM benchmark: the solve from the right X op(T) = B on a tall row-major block, X n x p, T p x p, at n = 2^21 and
2^16 with p = 4, 16 and 64, for ('U', 'N') and ('L', 'T') (both run forward), alpha = 1, fpe = 8, three ways on the same
data:
  exbtrsm_us     one exbtrsm_dev call
  transposed_us  what a caller without ExBTRSM has: X.t().contiguous(), extrsm_dev with the other trans on the p x n
                 block, and the transpose back -- all three inside the timed span.  The same bits by contract.
  exbgemm_us     exbgemm_dev with q = p, beta = 0 on the same X against the triangle as a full p x p block: for
                 orientation only (twice the products, no chain, no division)
Before anything is timed ExBTRSM and the transposed form are asserted to be bit-identical.  The routines are then timed
interleaved (one of each per repetition, device events around each call; X is restored before the events), --repeats
(10) repetitions after the warm round, and reported as median with the spread (min, max), with the share of outputs that
ExBTRSM rounded in registers.  Per configuration one JSON line is printed and appended to --out, then the table, and the
verdict on n = 2^21, p = 16: ExBTRSM must beat the transposed form by more than the sum of the two (max - min) spreads,
in both orientations.

    python tools/bench_btrsm.py [--ns 2097152,65536] [--ps 4,16,64] [--repeats 10] [--out profiles/btrsm_bench.jsonl]
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
FLIP = {"N": "T", "T": "N"}


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


def run(n, p, uplo, trans, repeats, out_path):
    g = torch.Generator("cuda").manual_seed(200 + p)
    rand = lambda *shape: 2.0 * torch.rand(*shape, dtype=torch.float64, device="cuda", generator=g) - 1.0  # noqa: E731
    # op(T) = M, upper, off-diagonal entries below 1 / p against a diagonal in [1, 2): the solution stays near B
    M = torch.triu(rand(p, p), 1) / p + torch.diag(1.5 + 0.5 * rand(p))
    stored = M if trans == "N" else M.t()                     # T[i, j] as indexed
    T = stored.t().contiguous().t()                           # column-major: strides (1, p)
    C = stored.contiguous()                                   # for ExBGEMM: a full row-major block
    X0 = rand(n, p)
    X, Xa, Y = torch.empty_like(X0), torch.empty_like(X0), torch.empty_like(X0)
    back = [None]

    def right():
        ex.exbtrsm_dev(T, X, uplo, trans, "N", 1.0, 8, True)

    def transposed():
        xt = Xa.t().contiguous()
        ex.extrsm_dev(T, xt, uplo, FLIP[trans], "N", 8, True)
        back[0] = xt.t().contiguous()

    def gemm():
        ex.exbgemm_dev(X0, C, 1.0, 0.0, Y, 8, True)

    ex.set_btrsm_path(0)
    ex.set_trsm_path(0)
    ex.set_bgemm_path(0)
    restore = {"exbtrsm": lambda: X.copy_(X0), "transposed": lambda: Xa.copy_(X0), "exbgemm": lambda: None}
    calls = {"exbtrsm": right, "transposed": transposed, "exbgemm": gemm}
    warm, info = {}, None
    for name, fn in calls.items():          # the warm round sizes the workspaces; then the bits, before any timing
        warm[name] = timed(restore[name], fn)
        if name == "exbtrsm":               # (the next routine reuses the workspace that holds the counters)
            info = ex.last_btrsm_info()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(X).all()), "the result is not finite"
    assert bool((X.view(torch.int64) == back[0].view(torch.int64)).all()), "exbtrsm_dev differs from the transposed extrsm_dev"
    assert info[0] + info[1] == n * p
    t = {name: [] for name in calls}
    for i in range(repeats):                # interleaved: one of each per repetition
        for name, fn in calls.items():
            t[name].append(timed(restore[name], fn))
        print(f"# n={n} p={p} {uplo}{trans} {i + 1}/{repeats}: "
              + ", ".join(f"{name} {ts[-1]:.0f} us" for name, ts in t.items()), file=sys.stderr, flush=True)
    nbytes = 8 * 2 * n * p
    out = {"n": n, "p": p, "uplo": uplo, "trans": trans, "alpha": 1.0, "fpe": 8, "repeats": repeats, "info": info,
           "in_registers": info[0] / (n * p), "bits_equal": True, "bytes": nbytes}
    for name, ts in t.items():
        out[f"{name}_us"] = summary(ts)
    spread = lambda s: s["max"] - s["min"]  # noqa: E731
    out["hbm_fraction"] = nbytes / out["exbtrsm_us"]["median"] / HBM_BYTES_PER_US
    out["speedup_vs_transposed"] = out["transposed_us"]["median"] / out["exbtrsm_us"]["median"]
    out["ratio_to_exbgemm"] = out["exbtrsm_us"]["median"] / out["exbgemm_us"]["median"]
    out["gap_us"] = out["transposed_us"]["median"] - out["exbtrsm_us"]["median"]
    out["spread_us"] = spread(out["transposed_us"]) + spread(out["exbtrsm_us"])
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
    ap.add_argument("--ps", default="4,16,64")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "btrsm_bench.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "the median is over at least 10 repetitions"
    ex.load_library().exblas_hip_init(-1)
    rows = []
    for n in (int(v) for v in a.ns.split(",")):
        for p in (int(v) for v in a.ps.split(",")):
            for uplo, trans in (("U", "N"), ("L", "T")):
                rows.append(run(n, p, uplo, trans, a.repeats, a.out))
                torch.cuda.empty_cache()
    fmt = lambda s: f"{s['median'] / 1e3:.3f} ({s['min'] / 1e3:.3f}-{s['max'] / 1e3:.3f})"  # noqa: E731
    print("| n | p | uplo, trans | ExBTRSM ms | of 8 TB/s | in registers | transpose + ExTRSM + transpose ms | ExBGEMM ms | "
          "vs transposed |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['n']} | {r['p']} | {r['uplo']}, {r['trans']} | {fmt(r['exbtrsm_us'])} | "
              f"{100 * r['hbm_fraction']:.1f} % | {100 * r['in_registers']:.2f} % | {fmt(r['transposed_us'])} | "
              f"{fmt(r['exbgemm_us'])} | {r['speedup_vs_transposed']:.2f}x |")
    for r in rows:
        if r["n"] == 1 << 21 and r["p"] == 16:
            print(f"speed condition, n = 2^21, p = 16, {r['uplo']}, {r['trans']}: gap {r['gap_us'] / 1e3:.3f} ms, spread "
                  f"{r['spread_us'] / 1e3:.3f} ms: {'MET' if r['faster_beyond_spread'] else 'NOT MET'}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
