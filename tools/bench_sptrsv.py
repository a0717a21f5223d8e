"""ExSpTRSV benchmark: S1 the lower triangle (with diagonal) of the 27-point stencil on 128^3 (int32), S2 a bidiagonal
chain of 2^20 rows (the latency per dependent row), S3 the lower triangle of the power-law matrix W2 of bench_spmv.py
(its longest row last, so that it depends on every other row).

Each workload prints one JSON line and appends it to --out: the time of one ExSpTRSV call chain (device events around
enough calls to last >= 0.5 s; every call is preceded by the copy of b into x, which is part of the figure), the same
under path 1 (every row from its accumulator), path 2 (one row per wave) and fpe = 1 (the plain solve), ExSpMV on the
same triangle (the throughput a solve cannot beat), for the chain also dense ExTRSV's microseconds per row, the
counters, and a CRC of the result bits of every exact path (they must agree).

    python tools/bench_sptrsv.py [--only S1,S2,S3] [--scale 1.0] [--out profiles/sptrsv_bench.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exblas_amd as ex  # noqa: E402
from bench_spmv import crc, stencil, timed  # noqa: E402


def values(crow, col, m, seed):
    """diagonal entries in [1, 2), the others +-[1, 2) / (4 * row length): every row contracts, the solution stays finite"""
    g = torch.Generator("cuda").manual_seed(seed)
    nnz = col.numel()
    lens = (crow[1:] - crow[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), lens)
    v = 1.0 + torch.rand(nnz, dtype=torch.float64, device="cuda", generator=g)
    sign = torch.randint(0, 2, (nnz,), device="cuda", generator=g).double() * 2.0 - 1.0
    off = v * sign / (4.0 * lens[rows].double())
    val = torch.where(col.long() == rows, v, off)
    b = (1.0 + torch.rand(m, dtype=torch.float64, device="cuda", generator=g))
    return val, b


def stencil_lower(k):
    crow, col = stencil(k)
    m = k ** 3
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), (crow[1:] - crow[:-1]).long())
    keep = col.long() <= rows
    lens = torch.zeros(m, dtype=torch.int64, device="cuda").index_add_(0, rows[keep], torch.ones_like(rows[keep]))
    ncrow = torch.zeros(m + 1, dtype=torch.int64, device="cuda")
    ncrow[1:] = torch.cumsum(lens, 0)
    return ncrow.int(), col[keep].contiguous()


def chain(m):
    crow = torch.arange(m + 1, device="cuda", dtype=torch.int64) * 2 - 1
    crow[0] = 0
    col = torch.stack([torch.arange(m, device="cuda") - 1, torch.arange(m, device="cuda")], 1).reshape(-1)[1:]
    return crow.int(), col.int().contiguous()


def power_law_lower(m, nnz_target, longest, seed=1):
    """bench_spmv.power_law's row lengths, reversed (the longest row is the last); every column is folded into the lower
    triangle (col mod (row + 1): duplicates occur and count) and the first entry of a row is its diagonal"""
    rng = np.random.default_rng(seed)
    lens = np.floor(rng.pareto(1.2, size=m) * 8 + 1).astype(np.int64)
    lens[0] = longest
    lens = np.minimum(lens, longest)
    scale = (nnz_target - longest) / max(1, lens[1:].sum())
    lens[1:] = np.maximum(1, np.floor(lens[1:] * scale)).astype(np.int64)
    lens = lens[::-1].copy()
    crow = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).cuda()
    nnz = int(crow[-1])
    col = torch.randint(0, m, (nnz,), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), torch.from_numpy(lens).cuda())
    col = col % (rows + 1)
    col[crow[:-1]] = torch.arange(m, device="cuda")
    return crow.int(), col.int().contiguous()


def run(name, crow, col, m, out_path, dense_n=0):
    nnz = col.numel()
    isz = crow.element_size()
    val, b = values(crow, col, m, 11)
    x = torch.empty_like(b)
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    A = (crow, col, val, (m, m))
    out = {"workload": name, "m": m, "nnz": nnz, "index_bits": 8 * isz, "max_row": int((crow[1:] - crow[:-1]).max())}

    def solve(fpe=8):
        x.copy_(b)
        ex.exsptrsv_dev(A, x, "L", "N", fpe, True)

    crcs = {}
    for key, path in (("exsptrsv_us", 0), ("accumulator_path_us", 1), ("row_per_wave_path_us", 2)):
        ex.set_sptrsv_path(path)
        out[key] = timed(solve) * 1e6
        solve()
        crcs[key[:-3]] = crc(x)
        if path == 0:
            out["info"] = ex.last_sptrsv_info()
            out["finite"] = bool(torch.isfinite(x).all())
    ex.set_sptrsv_path(0)
    out["plain_fpe1_us"] = timed(lambda: solve(1)) * 1e6
    out["copy_b_us"] = timed(lambda: x.copy_(b)) * 1e6
    out["exspmv_same_triangle_us"] = timed(lambda: ex.exspmv_dev(A, b, 1.0, 0.0, y)) * 1e6
    out["us_per_row"] = out["exsptrsv_us"] / m
    if dense_n:
        n = dense_n
        g = torch.Generator("cuda").manual_seed(5)
        a = torch.rand(n * n, dtype=torch.float64, device="cuda", generator=g) / n
        a.view(n, n).diagonal().add_(1.0)
        bd = 1.0 + torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
        xd = torch.empty_like(bd)

        def dense():
            xd.copy_(bd)
            ex.extrsv_dev("L", "N", "N", n, a, n, xd, 8, True)

        out["dense_extrsv_n"] = n
        out["dense_extrsv_us_per_row"] = timed(dense) * 1e6 / n
    out["crc"] = crcs
    out["crc_agree"] = len(set(crcs.values())) == 1
    out["vs_plain"] = out["exsptrsv_us"] / out["plain_fpe1_us"]
    out["vs_exspmv"] = out["exsptrsv_us"] / out["exspmv_same_triangle_us"]
    line = json.dumps(out)
    print(line, flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="S1,S2,S3")
    ap.add_argument("--scale", type=float, default=1.0, help="S2 / S3 size factor (S1 is fixed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sptrsv_bench.jsonl"))
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    todo = a.only.split(",")
    if "S1" in todo:
        crow, col = stencil_lower(128)
        run("S1_stencil27_lower_128^3", crow, col, 128 ** 3, a.out)
        del crow, col
    if "S2" in todo:
        m = int((1 << 20) * a.scale)
        crow, col = chain(m)
        run("S2_bidiagonal_chain", crow, col, m, a.out, dense_n=8192)
        del crow, col
    if "S3" in todo:
        m = int((1 << 20) * a.scale)
        crow, col = power_law_lower(m, int((1 << 26) * a.scale), max(1 << 20, m) if a.scale >= 1 else m)
        run("S3_powerlaw_lower", crow, col, m, a.out)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
