"""ExSpTRSM benchmark: the workloads S1 (lower triangle of the 27-point stencil on 128^3) and S2 (a bidiagonal chain of
2^20 rows: pure hand-off latency) of bench_sptrsv.py with k = 1, 4, 16, 64 right-hand sides.

Per workload and k one JSON line is printed and appended to --out.  Everything is timed with device events, one event
pair per repeat, --repeats (5) repeats after one warm call, and reported as median with the spread (min, max):
  exsptrsm_us        one ExSpTRSM call, including the copy of B into X
  loop_exsptrsv_us   in the same run, the loop of k exsptrsv_dev calls on k contiguous vectors, each with its copy of b
  plain_fpe1_us      the plain fp64 ExSpTRSM (fpe = 1)
and the counters of the ExSpTRSM call, the speed-up, whether the gap exceeds the spread of the loop, and the check that
every column of X has the bits of the ExSpTRSV result (with the CRC of both).

    python tools/bench_sptrsm.py [--only S1,S2] [--ks 1,4,16,64] [--scale 1.0] [--repeats 5] [--out profiles/sptrsm_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exblas_amd as ex  # noqa: E402
from bench_spmv import crc  # noqa: E402
from bench_sptrsv import chain, stencil_lower, values  # noqa: E402


def repeated(fn, repeats, what=""):
    """microseconds of each of `repeats` runs of fn (device events around each one); a progress line per run on stderr"""
    out = []
    for i in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
        print(f"# {what} {i + 1}/{repeats}: {out[-1]:.0f} us", file=sys.stderr, flush=True)
    return out


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}


def run(name, crow, col, m, k, repeats, out_path):
    val, b = values(crow, col, m, 11)
    A = (crow, col, val, (m, m))
    g = torch.Generator("cuda").manual_seed(100 + k)
    B = 1.0 + torch.rand(m, k, dtype=torch.float64, device="cuda", generator=g)
    B[:, 0] = b
    Bt = B.t().contiguous()            # the k right-hand sides as contiguous vectors
    X = torch.empty_like(B)
    V = torch.empty_like(Bt)

    def block(fpe=8):
        X.copy_(B)
        ex.exsptrsm_dev(A, X, "L", "N", fpe, True)

    def loop():
        for j in range(k):
            V[j].copy_(Bt[j])
            ex.exsptrsv_dev(A, V[j], "L", "N", 8, True)

    out = {"workload": name, "m": m, "k": k, "nnz": col.numel(), "repeats": repeats}
    ex.set_sptrsm_path(0)
    ex.set_sptrsv_path(0)
    block()                            # warm: sizes the workspace
    out["info"] = ex.last_sptrsm_info()
    t_block = repeated(block, repeats, f"{name} k={k} exsptrsm")
    V[0].copy_(Bt[0])
    ex.exsptrsv_dev(A, V[0], "L", "N", 8, True)
    t_loop = repeated(loop, repeats, f"{name} k={k} loop of exsptrsv")
    ex.last_sptrsv_info()              # (raises if the watchdog of the last call was raised)
    same = bool((X.t().contiguous().view(torch.int64) == V.view(torch.int64)).all())
    out["columns_equal_exsptrsv"] = same
    out["crc"] = {"exsptrsm": crc(X.t().contiguous()), "exsptrsv_loop": crc(V)}
    out["finite"] = bool(torch.isfinite(X).all())
    block(1)
    t_plain = repeated(lambda: block(1), repeats, f"{name} k={k} plain")
    out["exsptrsm_us"], out["loop_exsptrsv_us"], out["plain_fpe1_us"] = summary(t_block), summary(t_loop), summary(t_plain)
    out["speedup_vs_loop"] = out["loop_exsptrsv_us"]["median"] / out["exsptrsm_us"]["median"]
    out["loop_spread_us"] = out["loop_exsptrsv_us"]["max"] - out["loop_exsptrsv_us"]["min"]
    out["gap_us"] = out["loop_exsptrsv_us"]["median"] - out["exsptrsm_us"]["median"]
    out["faster_beyond_spread"] = out["gap_us"] > out["loop_spread_us"]
    out["us_per_row"] = out["exsptrsm_us"]["median"] / m
    out["vs_plain"] = out["exsptrsm_us"]["median"] / out["plain_fpe1_us"]["median"]
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="S1,S2")
    ap.add_argument("--ks", default="1,4,16,64")
    ap.add_argument("--scale", type=float, default=1.0, help="S2 size factor (S1 is fixed)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sptrsm_bench.jsonl"))
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    todo, ks = a.only.split(","), [int(v) for v in a.ks.split(",")]
    if "S1" in todo:
        crow, col = stencil_lower(128)
        for k in ks:
            run("S1_stencil27_lower_128^3", crow, col, 128 ** 3, k, a.repeats, a.out)
        del crow, col
    if "S2" in todo:
        m = int((1 << 20) * a.scale)
        crow, col = chain(m)
        for k in ks:
            run("S2_bidiagonal_chain", crow, col, m, k, a.repeats, a.out)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
