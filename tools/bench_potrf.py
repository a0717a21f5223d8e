"""ExPOTRF benchmark, two parts, on one device.

(a) The routine at p = 4, 16, 32, 64, 128, 512 on G = X^T X of a random 4p x p block, fpe = 8, against the two routes a
caller has without it:
  expotrf_us   one expotrf_dev call (device events; G restored before the events)
  host_us      G.cpu() -> numpy.linalg.cholesky -> .cuda(), wall clock with the synchronisation it implies
  torch_us     torch.linalg.cholesky on the device (device events)
Both are asserted close to ExPOTRF (not bit-identical: they sum in plain fp64) before anything is timed.  The time per
pivot is printed beside ExTRSV's measured chain step (13.4 ms / 32768 rows) for orientation.

(b) The CholQR chain Q = X R^-1, R = chol(X^T X), at n = 2^16 and 2^21, p = 16 and 64, in three forms, wall clock from a
synchronised start to a synchronised end, X restored before the start:
  host_chain_us      exbdot_dev, the host factorisation (D2H, numpy, H2D), exbtrsm_dev
  device_chain_us    excholqr_dev, eager: three launches, no synchronisation inside
  graph_chain_us     the same, captured once and replayed

The routines of a part are timed interleaved (one of each per repetition), --repeats (10) repetitions after the warm
round, and reported as median with the spread (min, max).  Per configuration one JSON line is printed and appended to
--out, then the tables, and the verdict on n = 2^16, p = 16: the all-device eager chain must beat the chain with the host
factorisation by more than the sum of the two (max - min) spreads.

    python tools/bench_potrf.py [--ps 4,16,32,64,128,512] [--ns 65536,2097152] [--chain-ps 16,64] [--repeats 10]
                                [--out profiles/potrf_bench.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import exblas_amd as ex  # noqa: E402

TRSV_STEP_US = 13.4e3 / 32768            # ExTRSV's measured time per row of its chain


def timed(prep, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    prep()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def walled(prep, fn):
    prep()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def summary(ts):
    return {"median": statistics.median(ts), "min": min(ts), "max": max(ts), "count": len(ts)}


def spread(s):
    return s["max"] - s["min"]


def emit(out, out_path):
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")
    return out


def host_factor(G):
    """the upper factor by the host route: D2H, numpy, H2D"""
    return torch.from_numpy(np.ascontiguousarray(np.linalg.cholesky(G.cpu().numpy()).T)).cuda()


def run_routine(p, repeats, out_path):
    g = torch.Generator("cuda").manual_seed(300 + p)
    Xm = torch.randn(4 * p, p, dtype=torch.float64, device="cuda", generator=g)
    G0 = ex.exbdot_dev(Xm)
    G = torch.empty_like(G0)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    keep = [None, None]
    calls = {"expotrf": (timed, lambda: G.copy_(G0), lambda: ex.expotrf_dev(G, "U", info, 8, True)),
             "host": (walled, lambda: None, lambda: keep.__setitem__(0, host_factor(G0))),
             "torch": (timed, lambda: None, lambda: keep.__setitem__(1, torch.linalg.cholesky(G0, upper=True)))}
    ex.set_potrf_path(0)
    counters = None
    for name, (clock, prep, fn) in calls.items():          # the warm round; then the comparison, before any timing
        clock(prep, fn)
        if name == "expotrf":
            counters = ex.last_potrf_info()
    assert int(info.item()) == 0 and counters[0] + counters[1] == p * (p + 1) // 2
    R = torch.triu(G)
    for other in keep:
        assert torch.allclose(R, torch.triu(other), rtol=1e-9, atol=1e-12), "the factors are not close"
    t = {name: [] for name in calls}
    for _ in range(repeats):                                # interleaved: one of each per repetition
        for name, (clock, prep, fn) in calls.items():
            t[name].append(clock(prep, fn))
    out = {"part": "routine", "p": p, "fpe": 8, "repeats": repeats, "info": counters,
           "in_registers": counters[0] / (p * (p + 1) // 2)}
    for name, ts in t.items():
        out[f"{name}_us"] = summary(ts)
    out["per_pivot_us"] = out["expotrf_us"]["median"] / p
    out["trsv_step_us"] = TRSV_STEP_US
    return emit(out, out_path)


def run_chain(n, p, repeats, out_path):
    g = torch.Generator("cuda").manual_seed(400 + p)
    X0 = torch.randn(n, p, dtype=torch.float64, device="cuda", generator=g)
    X = torch.empty_like(X0)
    res = {}

    def host_chain():
        G = ex.exbdot_dev(X)
        R = host_factor(G)
        ex.exbtrsm_dev(R, X, "U", "N")
        res["host"] = R

    def device_chain():
        _, R, inf = ex.excholqr_dev(X)
        res["device"], res["info"] = R, inf

    restore = lambda: X.copy_(X0)  # noqa: E731
    walled(restore, host_chain)
    Qh = X.clone()
    walled(restore, device_chain)
    assert int(res["info"].item()) == 0
    assert torch.allclose(torch.triu(res["device"]), torch.triu(res["host"]), rtol=1e-9, atol=1e-12)
    assert torch.allclose(X, Qh, rtol=1e-7, atol=1e-9)
    torch.cuda.synchronize()
    s, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            ex.excholqr_dev(X)
    calls = {"host_chain": host_chain, "device_chain": device_chain, "graph_chain": graph.replay}
    for fn in calls.values():
        walled(restore, fn)
    t = {name: [] for name in calls}
    for _ in range(repeats):
        for name, fn in calls.items():
            t[name].append(walled(restore, fn))
    out = {"part": "chain", "n": n, "p": p, "fpe": 8, "repeats": repeats}
    for name, ts in t.items():
        out[f"{name}_us"] = summary(ts)
    out["gap_us"] = out["host_chain_us"]["median"] - out["device_chain_us"]["median"]
    out["spread_us"] = spread(out["host_chain_us"]) + spread(out["device_chain_us"])
    out["faster_beyond_spread"] = out["gap_us"] > out["spread_us"]
    del graph
    return emit(out, out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ps", default="4,16,32,64,128,512")
    ap.add_argument("--ns", default=f"{1 << 16},{1 << 21}")
    ap.add_argument("--chain-ps", default="16,64")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "potrf_bench.jsonl"))
    a = ap.parse_args()
    assert a.repeats >= 10, "the median is over at least 10 repetitions"
    ex.load_library().exblas_hip_init(-1)
    rows = [run_routine(int(p), a.repeats, a.out) for p in a.ps.split(",") if p]
    chains = []
    for n in (int(v) for v in a.ns.split(",") if v):
        for p in (int(v) for v in a.chain_ps.split(",") if v):
            chains.append(run_chain(n, p, a.repeats, a.out))
            torch.cuda.empty_cache()
    fmt = lambda s: f"{s['median']:.1f} ({s['min']:.1f}-{s['max']:.1f})"  # noqa: E731
    print("| p | ExPOTRF us | per pivot us | ExTRSV step us | in registers | host route us (wall) | torch.linalg.cholesky us |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['p']} | {fmt(r['expotrf_us'])} | {r['per_pivot_us']:.2f} | {r['trsv_step_us']:.2f} | "
              f"{100 * r['in_registers']:.1f} % | {fmt(r['host_us'])} | {fmt(r['torch_us'])} |")
    print("| n | p | chain, host factorisation us | chain, all device, eager us | chain, captured us | gap us | spreads us |")
    print("|---|---|---|---|---|---|---|")
    for r in chains:
        print(f"| {r['n']} | {r['p']} | {fmt(r['host_chain_us'])} | {fmt(r['device_chain_us'])} | {fmt(r['graph_chain_us'])} | "
              f"{r['gap_us']:.1f} | {r['spread_us']:.1f} |")
    for r in chains:
        if r["n"] == 1 << 16 and r["p"] == 16:
            print(f"speed condition, n = 2^16, p = 16: gap {r['gap_us']:.1f} us, spreads {r['spread_us']:.1f} us: "
                  f"{'MET' if r['faster_beyond_spread'] else 'NOT MET'}")
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
