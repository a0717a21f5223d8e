"""ExSpILU0 benchmark: the factor and its apply on the 7-point and the 27-point stencil of 128^3 (int32 indices).

Each workload prints one JSON line and appends it to --out: the time of one exspilu0_dev call (device events around enough
calls to last >= 0.5 s; eager, i.e. with the one-word read of row_ptr[m] that sizes the mailbox, and as a captured graph,
which reads nothing back), the same under path 1 (every rounding through the accumulator), path 2 (the
several-entries-per-lane form) and fpe = 1 (the plain form), the apply (both sweeps) on a vector and on a block of 4
columns, and beside them ONE ExSpTRSV sweep ('L', 'U') on the same matrix: the yardstick, a kernel with the same
dependency chain that existed before this one.  The counters, both info words and a CRC of the factor's bits on every
exact path (they must agree) go with them.

    python tools/bench_spilu0.py [--only S7,S27] [--k 128] [--out profiles/spilu0_bench.jsonl]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exblas_amd as ex  # noqa: E402
from bench_spmv import crc, timed  # noqa: E402


def stencil(k, points):
    """the 7- or 27-point stencil on k^3, columns ascending in every row"""
    i = torch.arange(k ** 3, device="cuda")
    z, y, x = i // (k * k), (i // k) % k, i % k
    cols = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if points == 7 and abs(dz) + abs(dy) + abs(dx) > 1:
                    continue
                ok = (z + dz >= 0) & (z + dz < k) & (y + dy >= 0) & (y + dy < k) & (x + dx >= 0) & (x + dx < k)
                cols.append(torch.where(ok, i + (dz * k + dy) * k + dx, torch.full_like(i, -1)))
    c = torch.stack(cols, 1)
    mask = c >= 0
    crow = torch.zeros(k ** 3 + 1, dtype=torch.int64, device="cuda")
    crow[1:] = torch.cumsum(mask.sum(1), 0)
    return crow.int(), c[mask].int().contiguous()


def values(crow, col, m, seed):
    """off the diagonal -[1, 2) / row length, the diagonal in [2, 3): nonsymmetric values, diagonally dominant"""
    g = torch.Generator("cuda").manual_seed(seed)
    lens = (crow[1:] - crow[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), lens)
    v = 1.0 + torch.rand(col.numel(), dtype=torch.float64, device="cuda", generator=g)
    return torch.where(col.long() == rows, v + 1.0, -v / lens[rows].double())


def graph_timed(fn):
    """fn captured once (after a warm call) and replayed"""
    fn()
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            fn()
    return timed(g.replay)


def run(name, crow, col, m, out_path):
    val = values(crow, col, m, 11)
    A = (crow, col, val, (m, m))
    lu, info = torch.empty_like(val), torch.zeros(2, dtype=torch.int64, device="cuda")
    out = {"workload": name, "m": m, "nnz": col.numel(), "index_bits": 8 * crow.element_size(),
           "max_row": int((crow[1:] - crow[:-1]).max())}

    def factor(fpe=8):
        return ex.exspilu0_dev(A, out=lu, info=info, fpe=fpe)

    crcs = {}
    for key, path in (("exspilu0", 0), ("accumulator_path", 1), ("wide_path", 2)):
        ex.set_spilu0_path(path)
        out[key + "_us"] = graph_timed(factor) * 1e6
        factor()
        crcs[key] = crc(lu)
        if path == 0:
            out["exspilu0_eager_us"] = timed(factor) * 1e6
            factor()
            out["counters"] = ex.last_spilu0_info()
            out["info"] = info.cpu().tolist()
            out["finite"] = bool(torch.isfinite(lu).all())
    ex.set_spilu0_path(0)
    out["plain_fpe1_us"] = graph_timed(lambda: factor(1)) * 1e6
    LU, _ = factor()
    b = 1.0 + torch.rand(m, 4, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    b1 = b[:, 0].contiguous()
    x1, x4 = torch.empty_like(b1), torch.empty_like(b)

    def apply1():
        x1.copy_(b1)
        ex.exspilu0_apply_dev(LU, x1)

    def apply4():
        x4.copy_(b)
        ex.exspilu0_apply_dev(LU, x4)

    def sweep():
        x1.copy_(b1)
        ex.exsptrsv_dev(LU, x1, "L", "U")

    out["apply_k1_us"] = timed(apply1) * 1e6
    out["apply_k4_us"] = timed(apply4) * 1e6
    out["exsptrsv_sweep_us"] = timed(sweep) * 1e6
    out["factor_vs_exsptrsv_sweep"] = out["exspilu0_us"] / out["exsptrsv_sweep_us"]
    out["us_per_row"] = out["exspilu0_us"] / m
    out["crc"] = crcs
    out["crc_agree"] = len(set(crcs.values())) == 1
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="S7,S27")
    ap.add_argument("--k", type=int, default=128, help="the grid is k^3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spilu0_bench.jsonl"))
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    for key, points in (("S7", 7), ("S27", 27)):
        if key in a.only.split(","):
            crow, col = stencil(a.k, points)
            run(f"{key}_stencil{points}_{a.k}^3", crow, col, a.k ** 3, a.out)
            del crow, col
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
