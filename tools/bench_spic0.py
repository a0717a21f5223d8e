"""ExSpIC0 benchmark: the IC(0) factor and its apply on the 7-point and the 27-point stencil of 128^3 (int32 indices).

Values: a symmetric diagonally dominant M-matrix (off the diagonal -1, the diagonal the row's count plus 1), so IC(0)
exists and info must be [0, 0].  Each workload prints one JSON line and appends it to --out: the time of one exspic0_dev
call (device events around enough calls to last >= 0.5 s; eager, i.e. with the one-word read of row_ptr[m] that sizes
the mailbox, and as a captured graph, which reads nothing back), the same under path 1 (every rounding through the
accumulator), path 2 (the several-entries-per-lane form) and fpe = 1 (the plain form), the apply (both sweeps) on a
vector and on a block of 4 columns, and beside them ExSpILU0's factor of the same matrix in the same run (captured): the
yardstick, a routine with the same row chain that does a superset of the products.  The counters of both, both info
words and a CRC of the factor's bits on every exact path (they must agree) go with them.

    python tools/bench_spic0.py [--only S7,S27] [--k 128] [--out profiles/spic0_bench.jsonl]
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
from bench_spilu0 import graph_timed, stencil  # noqa: E402
from bench_spmv import crc, timed  # noqa: E402


def values(crow, col, m):
    """the symmetric M-matrix: -1 off the diagonal, the row's count plus 1 on it"""
    lens = (crow[1:] - crow[:-1]).long()
    rows = torch.repeat_interleave(torch.arange(m, device="cuda"), lens)
    return torch.where(col.long() == rows, (lens[rows] + 1).double(), torch.full_like(rows, -1).double())


def run(name, crow, col, m, out_path):
    val = values(crow, col, m)
    A = (crow, col, val, (m, m))
    ll, info = torch.empty_like(val), torch.zeros(2, dtype=torch.int64, device="cuda")
    lens = crow[1:] - crow[:-1]
    out = {"workload": name, "m": m, "nnz": col.numel(), "index_bits": 8 * crow.element_size(),
           "max_row": int(lens.max()), "owned": (col.numel() + m) // 2}

    def factor(fpe=8):
        return ex.exspic0_dev(A, out=ll, info=info, fpe=fpe)

    crcs = {}
    for key, path in (("exspic0", 0), ("accumulator_path", 1), ("wide_path", 2)):
        ex.set_spic0_path(path)
        out[key + "_us"] = graph_timed(factor) * 1e6
        factor()
        crcs[key] = crc(ll)
        if path == 0:
            out["exspic0_eager_us"] = timed(factor) * 1e6
            factor()
            out["counters"] = ex.last_spic0_info()
            out["info"] = info.cpu().tolist()
            out["finite"] = bool(torch.isfinite(ll).all())
    ex.set_spic0_path(0)
    out["plain_fpe1_us"] = graph_timed(lambda: factor(1)) * 1e6
    LL, _ = factor()
    b = 1.0 + torch.rand(m, 4, dtype=torch.float64, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    b1 = b[:, 0].contiguous()
    x1, x4 = torch.empty_like(b1), torch.empty_like(b)

    def apply1():
        x1.copy_(b1)
        ex.exspic0_apply_dev(LL, x1)

    def apply4():
        x4.copy_(b)
        ex.exspic0_apply_dev(LL, x4)

    out["apply_k1_us"] = timed(apply1) * 1e6
    out["apply_k4_us"] = timed(apply4) * 1e6
    # the yardstick: ExSpILU0 on the same matrix, same run
    lu, info_lu = torch.empty_like(val), torch.zeros(2, dtype=torch.int64, device="cuda")
    out["exspilu0_us"] = graph_timed(lambda: ex.exspilu0_dev(A, out=lu, info=info_lu)) * 1e6
    ex.exspilu0_dev(A, out=lu, info=info_lu)
    out["exspilu0_counters"] = ex.last_spilu0_info()
    out["exspilu0_info"] = info_lu.cpu().tolist()
    out["ic0_vs_ilu0"] = out["exspic0_us"] / out["exspilu0_us"]
    out["us_per_row"] = out["exspic0_us"] / m
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spic0_bench.jsonl"))
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
