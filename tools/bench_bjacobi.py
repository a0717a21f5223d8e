"""Block-Jacobi benchmark on one device: the batched ExPOTRF (factor) and the batched ExPOTRS (apply) against the single
routines looped over the blocks, which is what a caller had before them.

Shapes: n = 2^20 rows in blocks of p = 4, 8, 16, 32, 64 (batch = n / p diagonally dominant random SPD blocks), k = 1, 4, 16
right-hand sides, fpe = 8.  Forms:
  factor_us        one expotrf_batched_dev call on all blocks
  factor_loop_us   expotrf_dev per block, on a SAMPLE of --sample (256) blocks, extrapolated linearly to the batch (marked
                   "extrapolated": the loop is a chain of launches, its time is proportional to their number)
  apply_us         one expotrs_batched_dev call (both sweeps) on the n x k block
  apply_loop_us    extrsm_dev twice per block ('T' then 'N'), on the same sample, extrapolated in the same way
Before anything is timed the batched outputs are asserted bit-equal to the loop's on the sample.  Device events; the data
is restored before each repetition (outside the events); the forms are timed interleaved, --repeats (10) repetitions after
a warm round, and reported as median (min-max).  Derived figures:
  apply_bytes      16 n k + 8 batch p (p + 1) / 2, what the apply must move; apply_frac_hbm: that over the time, as a
                   fraction of the HBM peak (8 TB/s)
  per_pivot_us     the factor's time over the pivots ONE wave walks one after the other (its matrices, in turn, times p):
                   comparable to ExPOTRF's 3.1 to 3.5 us per pivot
The condition: the batched forms beat the loop at every shape.

    python tools/bench_bjacobi.py [--n 1048576] [--ps 4,8,16,32,64] [--ks 1,4,16] [--sample 256] [--repeats 10]
                                  [--out profiles/bjacobi_bench.jsonl]
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

HBM_PEAK = 8.0e12                         # bytes / s


def timed(prep, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prep()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def summary(ts, scale=1.0):
    return {"median": statistics.median(ts) * scale, "min": min(ts) * scale, "max": max(ts) * scale, "count": len(ts)}


def emit(out, out_path):
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")
    return out


def pivots_per_wave(p, batch):
    """how many pivots are walked in turn on one wave slot of the device by the batched factor: the rounds in which the
    grid becomes resident (the staged triangles limit the workgroups per CU), the items of a workgroup, times p"""
    pw = 1 << max(p - 1, 0).bit_length()
    g = max(64 // pw, 1)
    nitems = -(-batch // (4 * g))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = -(-nitems // min(cus * 8, nitems))
    grid = -(-nitems // per)
    lds = 4 * g * p * (p | 1) * 8 + 3328                    # the triangles of four waves, accumulators, counters, stops
    resident = cus * max(1, min(8, (160 * 1024) // lds))
    return -(-grid // resident) * per * p


def blocks(p, batch, seed):
    """diagonally dominant SPD blocks with full-mantissa entries, [batch, p, p] row-major"""
    g = torch.Generator("cuda").manual_seed(seed)
    B = torch.rand(batch, p, p, dtype=torch.float64, device="cuda", generator=g) - 0.5
    return B + B.transpose(1, 2) + (p + 1.0) * torch.eye(p, dtype=torch.float64, device="cuda")


def run(n, p, ks, sample, repeats, out_path):
    batch = n // p
    assert batch * p == n and sample <= batch
    D0 = blocks(p, batch, 500 + p)
    D = torch.empty_like(D0)
    info = torch.zeros(batch, dtype=torch.int32, device="cuda")
    one = torch.zeros(1, dtype=torch.int32, device="cuda")

    def factor():
        ex.expotrf_batched_dev(D, "U", info, 8, True)

    def factor_loop():
        for b in range(sample):
            ex.expotrf_dev(D[b], "U", one, 8, True)

    restore = lambda: D.copy_(D0)  # noqa: E731
    # ---- bit-equality on the sample, before anything is timed ----
    timed(restore, factor_loop)
    loop_r = D[:sample].clone()
    timed(restore, factor)
    cnt = ex.last_potrf_batched_info()
    assert int(info.abs().max().item()) == 0 and cnt[0] + cnt[1] == batch * p * (p + 1) // 2
    assert torch.equal(D[:sample].view(torch.int64), loop_r.view(torch.int64)), "batched factor != looped expotrf_dev"
    R = D.clone()                                            # the factors the applies use
    tf, tl = [], []
    for _ in range(repeats):                                 # interleaved
        tf.append(timed(restore, factor))
        tl.append(timed(restore, factor_loop))
    ppw = pivots_per_wave(p, batch)
    out = {"part": "factor", "n": n, "p": p, "batch": batch, "fpe": 8, "repeats": repeats, "sample": sample,
           "in_registers": cnt[0] / (cnt[0] + cnt[1]), "factor_us": summary(tf),
           "factor_loop_us": dict(summary(tl, batch / sample), extrapolated=True, sample_us=statistics.median(tl)),
           "pivots_per_wave": ppw}
    out["per_pivot_us"] = out["factor_us"]["median"] / ppw
    out["per_matrix_ns"] = 1e3 * out["factor_us"]["median"] / batch
    out["speedup"] = out["factor_loop_us"]["median"] / out["factor_us"]["median"]
    out["beats_loop"] = out["factor_us"]["max"] < out["factor_loop_us"]["min"]
    rows = [emit(out, out_path)]
    del D, D0
    for k in ks:
        g = torch.Generator("cuda").manual_seed(600 + p + k)
        X0 = torch.rand(n, k, dtype=torch.float64, device="cuda", generator=g) - 0.5
        X = torch.empty_like(X0)

        def apply():
            ex.expotrs_batched_dev(R, X, "U", "B", 8, True)

        def apply_loop():
            for b in range(sample):
                ex.extrsm_dev(R[b], X[b * p:(b + 1) * p], "U", "T", "N", 8, True)
                ex.extrsm_dev(R[b], X[b * p:(b + 1) * p], "U", "N", "N", 8, True)

        restore_x = lambda: X.copy_(X0)  # noqa: E731
        timed(restore_x, apply_loop)
        loop_x = X[:sample * p].clone()
        timed(restore_x, apply)
        cnt = ex.last_potrs_batched_info()
        assert cnt[0] + cnt[1] == 2 * n * k
        assert torch.equal(X[:sample * p].view(torch.int64), loop_x.view(torch.int64)), "batched apply != looped extrsm_dev"
        ta, tl = [], []
        for _ in range(repeats):
            ta.append(timed(restore_x, apply))
            tl.append(timed(restore_x, apply_loop))
        nbytes = 16 * n * k + 8 * batch * p * (p + 1) // 2
        out = {"part": "apply", "n": n, "p": p, "k": k, "batch": batch, "fpe": 8, "repeats": repeats, "sample": sample,
               "in_registers": cnt[0] / (cnt[0] + cnt[1]), "apply_us": summary(ta),
               "apply_loop_us": dict(summary(tl, batch / sample), extrapolated=True, sample_us=statistics.median(tl)),
               "apply_bytes": nbytes}
        out["apply_bytes_per_s"] = nbytes / (out["apply_us"]["median"] * 1e-6)
        out["apply_frac_hbm"] = out["apply_bytes_per_s"] / HBM_PEAK
        out["speedup"] = out["apply_loop_us"]["median"] / out["apply_us"]["median"]
        out["beats_loop"] = out["apply_us"]["max"] < out["apply_loop_us"]["min"]
        rows.append(emit(out, out_path))
        del X, X0
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--ps", default="4,8,16,32,64")
    ap.add_argument("--ks", default="1,4,16")
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bjacobi_bench.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "the median is over at least 10 repetitions"
    ex.load_library().exblas_hip_init(-1)
    ex.set_potrf_batched_path(0)
    ex.set_potrs_batched_path(0)
    rows = []
    for p in (int(v) for v in a.ps.split(",") if v):
        rows += run(a.n, p, [int(v) for v in a.ks.split(",") if v], a.sample, a.repeats, a.out)
    fmt = lambda s: f"{s['median']:.1f} ({s['min']:.1f}-{s['max']:.1f})"  # noqa: E731
    print("| p | batch | batched factor us | looped expotrf_dev us (extrapolated) | speed-up | per pivot us | per matrix ns |"
          " in registers |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        if r["part"] == "factor":
            print(f"| {r['p']} | {r['batch']} | {fmt(r['factor_us'])} | {fmt(r['factor_loop_us'])} | {r['speedup']:.0f}x | "
                  f"{r['per_pivot_us']:.2f} | {r['per_matrix_ns']:.1f} | {100 * r['in_registers']:.1f} % |")
    print("| p | k | batched apply us | looped extrsm_dev x 2 us (extrapolated) | speed-up | GB moved | GB/s | of HBM peak |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        if r["part"] == "apply":
            print(f"| {r['p']} | {r['k']} | {fmt(r['apply_us'])} | {fmt(r['apply_loop_us'])} | {r['speedup']:.0f}x | "
                  f"{r['apply_bytes'] / 1e9:.3f} | {r['apply_bytes_per_s'] / 1e9:.0f} | {100 * r['apply_frac_hbm']:.1f} % |")
    ok = all(r["beats_loop"] for r in rows)
    print(f"condition, the batched forms beat the loop at every shape: {'MET' if ok else 'NOT MET'}")
    torch.cuda.synchronize()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
