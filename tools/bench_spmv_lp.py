"""Narrow ExSpMV / ExSpMM benchmark: W1 of tools/bench_spmv.py (27-point stencil on 128^3, int32 indices) as ExSpMV and
as ExSpMM at k = 4 and 16, for every accepted type pair (values float32 / float16 / bfloat16, vectors float64 or the
values' type), the data cast from ONE seeded fp64 set.

Each case is timed against the fp64 entry on the widened operands twice: with the .double() conversion of the matrix
inside the timed region (what a caller who holds narrow data pays today) and with it outside (the fp64 kernels alone).
The three versions alternate in one process, `--rounds` times; the time reported is the median of the rounds and the
spread their (max - min) / median.  One JSON line per case with the byte floor from the shapes (row pointers, column
indices, values, the x gather counted once, y), the times, floor bytes over time, and a CRC of the result bits: for the
pairs with float64 vectors it must equal the fp64 entry's.

    python tools/bench_spmv_lp.py [--k 1,4,16] [--rounds 3] [--grid 128] [--min-s 0.15]
"""
import argparse
import json
import os
import statistics
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exblas_amd as ex  # noqa: E402
from bench_spmv import stencil, timed  # noqa: E402

PAIRS = [(v, x) for v in ("float32", "float16", "bfloat16") for x in ("float64", v)]


def crc(t):
    return zlib.crc32(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())


def floor_bytes(m, n, nnz, k, index_bytes, vbytes, xbytes):
    """what the product must move at the least: the index arrays and the values once, X once (the gather counted once), Y"""
    return (m + 1) * index_bytes + nnz * (index_bytes + vbytes) + n * k * xbytes + m * k * xbytes


def run(crow, col, val64, x64, m, n, k, vt, xt, rounds, min_s):
    tv, tx = getattr(torch, vt), getattr(torch, xt)
    val = val64.to(tv)
    wide = val.double()                                  # the widened operands: what the fp64 entry is given
    if k == 1:
        x = x64[:n].to(tx)
        xw = x.double()
        y, yw = torch.zeros(m, dtype=tx, device="cuda"), torch.zeros(m, dtype=torch.float64, device="cuda")
        lp = lambda: ex.exspmv_lp_dev((crow, col, val, (m, n)), x, 1.0, 0.0, y)                       # noqa: E731
        f_in = lambda: ex.exspmv_dev((crow, col, val.double(), (m, n)), xw, 1.0, 0.0, yw)             # noqa: E731
        f_out = lambda: ex.exspmv_dev((crow, col, wide, (m, n)), xw, 1.0, 0.0, yw)                    # noqa: E731
    else:
        x = x64[:n * k].view(n, k).to(tx)
        xw = x.double()
        y, yw = torch.zeros((m, k), dtype=tx, device="cuda"), torch.zeros((m, k), dtype=torch.float64, device="cuda")
        lp = lambda: ex.exspmm_lp_dev((crow, col, val, (m, n)), x, 1.0, 0.0, y)                       # noqa: E731
        f_in = lambda: ex.exspmm_dev((crow, col, val.double(), (m, n)), xw, 1.0, 0.0, yw)             # noqa: E731
        f_out = lambda: ex.exspmm_dev((crow, col, wide, (m, n)), xw, 1.0, 0.0, yw)                    # noqa: E731
    times = {"lp": [], "fp64_convert_inside": [], "fp64_widened": []}
    for _ in range(rounds):
        for name, fn in (("lp", lp), ("fp64_convert_inside", f_in), ("fp64_widened", f_out)):
            times[name].append(timed(fn, min_s))
    info = None
    lp()
    info = ex.last_spmv_info() if k == 1 else ex.last_spmm_info()
    f_out()
    torch.cuda.synchronize()
    nnz = col.numel()
    ib = crow.element_size()
    out = {"routine": "exspmv_lp" if k == 1 else "exspmm_lp", "workload": "W1_stencil27", "m": m, "n": n, "nnz": nnz, "k": k,
           "val": vt, "vec": xt, "index_bits": 8 * ib, "rounds": rounds, "info": info}
    fl = {"lp": floor_bytes(m, n, nnz, k, ib, val.element_size(), x.element_size()),
          "fp64_convert_inside": floor_bytes(m, n, nnz, k, ib, 8, 8), "fp64_widened": floor_bytes(m, n, nnz, k, ib, 8, 8)}
    for name, ts in times.items():
        med = statistics.median(ts)
        out[name] = {"us": med * 1e6, "spread": (max(ts) - min(ts)) / med, "floor_bytes": fl[name],
                     "floor_GBps": fl[name] / med * 1e-9}
    out["lp_over_fp64_widened"] = out["lp"]["us"] / out["fp64_widened"]["us"]
    out["lp_over_fp64_convert_inside"] = out["lp"]["us"] / out["fp64_convert_inside"]["us"]
    out["crc_lp"], out["crc_fp64"] = crc(y), crc(yw)
    if xt == "float64":
        out["crc_agree"] = out["crc_lp"] == out["crc_fp64"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="1,4,16", help="1: ExSpMV; above: ExSpMM with that many columns")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--min-s", type=float, default=0.15)
    ap.add_argument("--pairs", default=",".join(f"{v}:{x}" for v, x in PAIRS))
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    crow, col = stencil(a.grid)
    m = n = a.grid ** 3
    ks = [int(v) for v in a.k.split(",")]
    val64 = ex.gen_dev("fpuniform", col.numel(), 11, 10, 0)
    x64 = ex.gen_dev("fpuniform", n * max(ks), 12, 10, 0)
    for k in ks:
        for pair in a.pairs.split(","):
            vt, xt = pair.split(":")
            run(crow, col, val64, x64, m, n, k, vt, xt, a.rounds, a.min_s)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
