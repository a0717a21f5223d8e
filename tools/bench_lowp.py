#!/usr/bin/env python3
"""bench_lowp.py -- narrow-input ExSUM / ExDOT (float32, float16, bfloat16) on one MI355X at n = 2^log2n elements.

    python tools/bench_lowp.py [--log2n 28] [--steps 40] [--warmup 10] [--out profiles/lowp_bench.jsonl]
    python tools/bench_lowp.py --sweep 1,2,3,4,6,8,16,32,48     # kernel time against workgroups per CU

Inputs are resident in HBM and the steps rotate over 4 distinct buffers, as bench.py does (no step is served by the
Infinity Cache from the one before); 400 ms of untimed load first.  Per dtype and op, in ONE process:
  kernel_ms   the streaming kernel's own dispatch duration (events attached to the dispatch packet,
              exblas_set_launch_events), mean and median over the steps
  call_ms     the whole call exsum_lp_dev / exdot_lp_dev (streaming kernel + finalize), K calls between two events
beside two yardsticks:
  fp64        exsum_dev / exdot_dev on 2^log2n doubles: the fp64 kernels, which this tool does not touch
  widen       the only route there was before: x.double() followed by exsum_dev, the conversion included
and the plain-read probe (stream_read_dev on the fp64 buffers) that says what the box streams today.  Each result line
carries Gelem/s, TB/s of the narrow data and the fraction of the probe's TB/s.  One JSON object per line, appended to
--out and printed.  --sweep sets every workgroups-per-CU knob through exblas_set_tuning (fp64 kernels included, so run it
in a process of its own) and reports the narrow kernels' kernel_ms only."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NARROW = ("float32", "float16", "bfloat16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotate", type=int, default=4)
    ap.add_argument("--fpe", type=int, default=8)
    ap.add_argument("--sweep", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lowp_bench.jsonl"))
    args = ap.parse_args()

    import torch
    import exblas_amd as ex
    lib = ex.load_library()
    lib.exblas_hip_init(-1)
    n = 1 << args.log2n
    gen = torch.Generator(device="cuda").manual_seed(1)

    def buffers(dtype, count):
        out = []
        for _ in range(count):
            t = torch.empty(n, dtype=dtype, device="cuda")
            for lo in range(0, n, 1 << 26):                      # in slices: the float32 source stays small
                t[lo:lo + (1 << 26)] = torch.randn(min(1 << 26, n - lo), device="cuda", generator=gen)
            out.append(t)
        return out

    def prewarm(fn, ms=400.0):
        t0 = time.perf_counter()
        while (time.perf_counter() - t0) * 1e3 < ms:
            for i in range(10):
                fn(i)
            torch.cuda.synchronize()

    def kernel_ms(accumulate):
        """accumulate(i) launches the streaming kernel of step i; the finalize follows it as in a real call"""
        rec = ex.new_record_buffer()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in ev:
            a.record()
            b.record()
        for i in range(args.warmup):
            accumulate(i)
            ex.finish_dev(out=rec)
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(ev):
            ex.set_launch_events(a, b)
            accumulate(args.warmup + i)
            ex.finish_dev(out=rec)
        torch.cuda.synchronize()
        s = sorted(a.elapsed_time(b) for a, b in ev)
        return sum(s) / len(s), s[len(s) // 2]

    def call_ms(call):
        for i in range(args.warmup):
            call(i)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for i in range(args.steps):
            call(args.warmup + i)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    lines = []

    def emit(d):
        d = dict({"tool": "bench_lowp", "log2n": args.log2n, "steps": args.steps, "rotate": args.rotate, "fpe": args.fpe}, **d)
        lines.append(d)
        print(json.dumps(d), flush=True)

    R = args.rotate
    if args.sweep:
        for name in NARROW:
            xs, ys = buffers(getattr(torch, name), R), buffers(getattr(torch, name), R)
            prewarm(lambda i: ex.exsum_lp_accumulate_dev(xs[i % R], args.fpe) or ex.finish_dev())
            for bpc in [int(v) for v in args.sweep.split(",")]:
                assert lib.exblas_set_tuning(bpc, -1, -1) == 0
                for fpe in sorted({0, args.fpe}):
                    ms, med = kernel_ms(lambda i: ex.exsum_lp_accumulate_dev(xs[i % R], fpe))
                    gs = ex.last_blas1_info()[1]
                    md, medd = kernel_ms(lambda i: ex.exdot_lp_accumulate_dev(xs[i % R], ys[i % R], fpe))
                    emit({"sweep": True, "dtype": name, "bpc": bpc, "fpe": fpe, "exsum_kernel_ms": ms, "exsum_kernel_ms_median": med,
                          "exsum_grid": gs, "exdot_kernel_ms": md, "exdot_kernel_ms_median": medd,
                          "exdot_grid": ex.last_blas1_info()[1]})
            del xs, ys
            torch.cuda.empty_cache()
    else:
        # the yardsticks first: the fp64 kernels on 2^log2n doubles, and the plain-read probe
        xd, yd = buffers(torch.float64, R), buffers(torch.float64, R)
        prewarm(lambda i: ex.exsum_accumulate_dev(xd[i % R], args.fpe) or ex.finish_dev())
        sink = torch.zeros(1, dtype=torch.float64, device="cuda")
        pm = call_ms(lambda i: ex.stream_read_dev(xd[i % R], sink))
        probe_tbs = n * 8 / (pm * 1e-3) / 1e12
        emit({"what": "probe", "op": "stream_read_dev", "dtype": "float64", "call_ms": pm, "TBs": probe_tbs})
        base = {}
        for op in ("exsum", "exdot"):
            if op == "exsum":
                km, kmed = kernel_ms(lambda i: ex.exsum_accumulate_dev(xd[i % R], args.fpe))
                cm = call_ms(lambda i: ex.exsum_dev(xd[i % R], args.fpe))
            else:
                km, kmed = kernel_ms(lambda i: ex.exdot_accumulate_dev(xd[i % R], yd[i % R], args.fpe))
                cm = call_ms(lambda i: ex.exdot_dev(xd[i % R], yd[i % R], args.fpe))
            bpe = 8 if op == "exsum" else 16
            base[op] = (km, cm)
            emit({"what": "fp64", "op": op, "dtype": "float64", "kernel_ms": km, "kernel_ms_median": kmed, "call_ms": cm,
                  "Gelems_kernel": n / km / 1e6, "Gelems_call": n / cm / 1e6, "TBs": n * bpe / (km * 1e-3) / 1e12,
                  "frac_of_probe": n * bpe / (km * 1e-3) / 1e12 / probe_tbs, "grid": ex.last_blas1_info()[1]})
        del xd, yd
        torch.cuda.empty_cache()
        for name in NARROW:
            dt = getattr(torch, name)
            xs, ys = buffers(dt, R), buffers(dt, R)
            es = xs[0].element_size()
            prewarm(lambda i: ex.exsum_lp_accumulate_dev(xs[i % R], args.fpe) or ex.finish_dev(), 200.0)
            for op in ("exsum", "exdot"):
                if op == "exsum":
                    km, kmed = kernel_ms(lambda i: ex.exsum_lp_accumulate_dev(xs[i % R], args.fpe))
                    grid = ex.last_blas1_info()[1]
                    cm = call_ms(lambda i: ex.exsum_lp_dev(xs[i % R], args.fpe))
                    wm = call_ms(lambda i: ex.exsum_dev(xs[i % R].double(), args.fpe))
                    k0, _ = kernel_ms(lambda i: ex.exsum_lp_accumulate_dev(xs[i % R], 0))
                else:
                    km, kmed = kernel_ms(lambda i: ex.exdot_lp_accumulate_dev(xs[i % R], ys[i % R], args.fpe))
                    grid = ex.last_blas1_info()[1]
                    cm = call_ms(lambda i: ex.exdot_lp_dev(xs[i % R], ys[i % R], args.fpe))
                    wm = call_ms(lambda i: ex.exdot_dev(xs[i % R].double(), ys[i % R].double(), args.fpe))
                    k0, _ = kernel_ms(lambda i: ex.exdot_lp_accumulate_dev(xs[i % R], ys[i % R], 0))
                bpe = es * (1 if op == "exsum" else 2)
                tbs = n * bpe / (km * 1e-3) / 1e12
                emit({"what": "narrow", "op": op, "dtype": name, "kernel_ms": km, "kernel_ms_median": kmed, "call_ms": cm,
                      "kernel_ms_fpe0": k0, "widen_then_fp64_call_ms": wm, "fp64_kernel_ms": base[op][0],
                      "fp64_call_ms": base[op][1], "Gelems_kernel": n / km / 1e6, "Gelems_call": n / cm / 1e6,
                      "Gelems_widen_route": n / wm / 1e6, "TBs": tbs, "frac_of_probe": tbs / probe_tbs,
                      "speedup_vs_widen_route": wm / cm, "elem_rate_vs_fp64_kernel": base[op][0] / km, "grid": grid})
            del xs, ys
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            for d in lines:
                fh.write(json.dumps(d) + "\n")


if __name__ == "__main__":
    main()
