"""Block-Jacobi benchmark with general blocks on one device: the batched ExGETRF (factor) and the batched ExGETRS (apply)
beside the batched Cholesky pair of the same build on the same shapes, and beside torch.linalg.lu_factor / lu_solve on the
same blocks.

Shapes: n = 2^20 rows in blocks of p = 4, 16, 64 (batch = n / p diagonally dominant random NONSYMMETRIC blocks with their
rows rotated by one, so that every step interchanges; the Cholesky pair runs on SPD blocks of the same size), k = 4
right-hand sides, fpe = 8.  Forms:
  getrf_us / getrs_us     one exgetrf_batched_dev / exgetrs_batched_dev call
  potrf_us / potrs_us     one expotrf_batched_dev / expotrs_batched_dev call (both sweeps)
  torch_lu_us / torch_solve_us   torch.linalg.lu_factor on the [batch, p, p] blocks / torch.linalg.lu_solve on [batch, p, k]
Before anything is timed: info == 0 everywhere, the counters equal batch p^2 and 2 n k, and the exact solution is compared
with torch's (the largest relative difference is reported; torch's bits depend on its library, nothing is asserted on them
beyond 1e-9).  Device events; the data is restored before each repetition (outside the events); the forms are timed
interleaved, --repeats (10) repetitions after a warm round, and reported as median (min-max).  No threshold: the expectation
is roughly twice the Cholesky sums for the factor.

    python tools/bench_bjacobi_lu.py [--n 1048576] [--ps 4,16,64] [--k 4] [--repeats 10] [--out profiles/bjacobi_lu_bench.jsonl]
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


def general_blocks(p, batch, seed):
    """diagonally dominant nonsymmetric blocks with full-mantissa entries, rows rotated by one: [batch, p, p] row-major"""
    g = torch.Generator("cuda").manual_seed(seed)
    B = torch.rand(batch, p, p, dtype=torch.float64, device="cuda", generator=g) - 0.5
    B = B + (p + 1.0) * torch.eye(p, dtype=torch.float64, device="cuda")
    return torch.roll(B, 1, dims=1).contiguous()


def spd_blocks(p, batch, seed):
    g = torch.Generator("cuda").manual_seed(seed)
    B = torch.rand(batch, p, p, dtype=torch.float64, device="cuda", generator=g) - 0.5
    return B + B.transpose(1, 2) + (p + 1.0) * torch.eye(p, dtype=torch.float64, device="cuda")


def run(n, p, k, repeats, out_path):
    batch = n // p
    assert batch * p == n
    A0, S0 = general_blocks(p, batch, 700 + p), spd_blocks(p, batch, 500 + p)
    A, S = torch.empty_like(A0), torch.empty_like(S0)
    ipiv = torch.zeros((batch, p), dtype=torch.int32, device="cuda")
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    g = torch.Generator("cuda").manual_seed(600 + p + k)
    X0 = torch.rand(n, k, dtype=torch.float64, device="cuda", generator=g) - 0.5
    X = torch.empty_like(X0)
    keep = {}

    def restore():
        A.copy_(A0)
        S.copy_(S0)
        X.copy_(X0)

    def getrf():
        ex.exgetrf_batched_dev(A, ipiv, info, 8, True)

    def potrf():
        ex.expotrf_batched_dev(S, "U", info, 8, True)

    def torch_lu():
        keep["lu"] = torch.linalg.lu_factor(A0)

    # ---- checks, before anything is timed ----
    timed(restore, getrf)
    cnt = ex.last_getrf_batched_info()
    assert int(info.abs().max().item()) == 0 and cnt[0] + cnt[1] == batch * p * p
    interchanges = int((ipiv != torch.arange(1, p + 1, dtype=torch.int32, device="cuda")).sum().item())
    LU, PV = A.clone(), ipiv.clone()
    timed(restore, potrf)
    assert int(info.abs().max().item()) == 0
    R = S.clone()
    timed(restore, torch_lu)
    tlu, tpiv = keep["lu"]

    def getrs():
        ex.exgetrs_batched_dev(LU, PV, X, 8, True)

    def potrs():
        ex.expotrs_batched_dev(R, X, "U", "B", 8, True)

    def torch_solve():
        keep["x"] = torch.linalg.lu_solve(tlu, tpiv, X0.view(batch, p, k))

    timed(restore, getrs)
    scnt = ex.last_getrs_batched_info()
    assert scnt[0] + scnt[1] == 2 * n * k
    mine = X.clone()                                          # (the next restore puts X0 back)
    timed(restore, torch_solve)
    ref = keep["x"].reshape(n, k)
    diff = float(((mine - ref).abs().max() / ref.abs().max()).item())
    del mine
    assert diff < 1e-9, diff
    t = {name: [] for name in ("getrf", "potrf", "torch_lu", "getrs", "potrs", "torch_solve")}
    fns = {"getrf": getrf, "potrf": potrf, "torch_lu": torch_lu, "getrs": getrs, "potrs": potrs, "torch_solve": torch_solve}
    for name, fn in fns.items():                              # the warm round
        timed(restore, fn)
    for _ in range(repeats):                                  # interleaved
        for name, fn in fns.items():
            t[name].append(timed(restore, fn))
    out = {"n": n, "p": p, "k": k, "batch": batch, "fpe": 8, "repeats": repeats, "interchanges": interchanges,
           "factor_in_registers": cnt[0] / (cnt[0] + cnt[1]), "apply_in_registers": scnt[0] / (scnt[0] + scnt[1]),
           "max_rel_diff_to_torch": diff}
    for name in fns:
        out[name + "_us"] = summary(t[name])
    out["getrf_over_potrf"] = out["getrf_us"]["median"] / out["potrf_us"]["median"]
    out["getrs_over_potrs"] = out["getrs_us"]["median"] / out["potrs_us"]["median"]
    out["getrf_over_torch"] = out["getrf_us"]["median"] / out["torch_lu_us"]["median"]
    out["getrs_over_torch"] = out["getrs_us"]["median"] / out["torch_solve_us"]["median"]
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")
    del A, A0, S, S0, X, X0, LU, R, keep
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--ps", default="4,16,64")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bjacobi_lu_bench.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "the median is over at least 10 repetitions"
    ex.load_library().exblas_hip_init(-1)
    for r in ("getrf", "getrs", "potrf", "potrs"):
        getattr(ex, f"set_{r}_batched_path")(0)
    rows = [run(a.n, p, a.k, a.repeats, a.out) for p in (int(v) for v in a.ps.split(",") if v)]
    fmt = lambda s: f"{s['median']:.1f} ({s['min']:.1f}-{s['max']:.1f})"  # noqa: E731
    print("| p | batch | ExGETRF us | ExPOTRF us | ratio | torch lu_factor us | ExGETRS us | ExPOTRS us | ratio |"
          " torch lu_solve us | in registers (factor / apply) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['p']} | {r['batch']} | {fmt(r['getrf_us'])} | {fmt(r['potrf_us'])} | {r['getrf_over_potrf']:.2f} | "
              f"{fmt(r['torch_lu_us'])} | {fmt(r['getrs_us'])} | {fmt(r['potrs_us'])} | {r['getrs_over_potrs']:.2f} | "
              f"{fmt(r['torch_solve_us'])} | {100 * r['factor_in_registers']:.1f} % / {100 * r['apply_in_registers']:.1f} % |")
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
