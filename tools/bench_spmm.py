"""ExSpMM benchmark: the workloads of tools/bench_spmv.py (W1 27-point stencil on 128^3, int32; W2 power-law row
lengths; W3 a dense stripe as CSR) against a dense block of k = 4, 16, 64 columns.

One JSON line per (workload, k): the kernel-chain time of ExSpMM (device events around enough calls to last >= 0.5 s),
the yardstick -- k calls of ExSpMV, each on its own contiguous column (X is stored transposed for this leg, so the loop
pays no copy) --, ExSpMM under fpe = 1 (the plain kernel), the accumulator-only path (exblas_set_spmm_path(1)), torch's
CSR product A @ X, and a CRC of the result bits of every exact path and of the column loop (they must agree).  W1 runs
once more with lognormal(0, 50) data at k = 16, where most outputs are deferred to the accumulator kernel.

    python tools/bench_spmm.py [--only W1,W2,W3,W1wide] [--k 4,16,64] [--scale 1.0]
"""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exblas_amd as ex  # noqa: E402
from bench_spmv import power_law, stencil, timed  # noqa: E402


def crc(t):
    return zlib.crc32(t.contiguous().cpu().numpy().view(np.uint8).tobytes())


def run(name, crow, col, m, n, k, kind=("fpuniform", 10, 0)):
    nnz = col.numel()
    val = ex.gen_dev(kind[0], nnz, 11, kind[1], kind[2])
    Xt = ex.gen_dev(kind[0], n * k, 12, kind[1], kind[2]).view(k, n)   # column j of X, contiguous
    X = Xt.t().contiguous()                                            # row-major n x k
    Y = torch.zeros((m, k), dtype=torch.float64, device="cuda")
    Yt = torch.zeros((k, m), dtype=torch.float64, device="cuda")
    A = (crow, col, val, (m, n))
    out = {"workload": name, "data": kind[0], "m": m, "n": n, "nnz": nnz, "k": k, "index_bits": 8 * crow.element_size()}
    crcs = {}
    ex.set_spmm_path(0)
    out["exspmm_us"] = timed(lambda: ex.exspmm_dev(A, X, 1.0, 0.0, Y)) * 1e6
    crcs["auto"] = crc(Y)
    out["info"] = ex.last_spmm_info()

    def loop():
        for j in range(k):
            ex.exspmv_dev(A, Xt[j], 1.0, 0.0, Yt[j])
    out["column_loop_us"] = timed(loop) * 1e6
    crcs["column_loop"] = crc(Yt.t())
    ex.set_spmm_path(1)
    out["accumulator_path_us"] = timed(lambda: ex.exspmm_dev(A, X, 1.0, 0.0, Y)) * 1e6
    crcs["accumulator"] = crc(Y)
    ex.set_spmm_path(0)
    out["plain_fpe1_us"] = timed(lambda: ex.exspmm_dev(A, X, 1.0, 0.0, Y, fpe=1)) * 1e6
    try:
        At = torch.sparse_csr_tensor(crow.long(), col.long(), val, size=(m, n))
        out["torch_csr_mm_us"] = timed(lambda: At @ X) * 1e6
    except Exception as exc:  # noqa: BLE001
        out["torch_csr_mm_us"] = None
        out["torch_csr_mm_error"] = str(exc)[:120]
    out["crc"] = crcs
    out["crc_agree"] = len(set(crcs.values())) == 1
    out["loop_over_exspmm"] = out["column_loop_us"] / out["exspmm_us"]
    out["vs_plain"] = out["exspmm_us"] / out["plain_fpe1_us"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="W1,W2,W3,W1wide")
    ap.add_argument("--k", default="4,16,64")
    ap.add_argument("--scale", type=float, default=1.0, help="W2 / W3 size factor (W1 is fixed)")
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    todo = a.only.split(",")
    ks = [int(v) for v in a.k.split(",")]
    if "W1" in todo or "W1wide" in todo:
        crow, col = stencil(128)
        if "W1" in todo:
            for k in ks:
                run("W1_stencil27_128^3", crow, col, 128 ** 3, 128 ** 3, k)
        if "W1wide" in todo:
            run("W1_stencil27_128^3", crow, col, 128 ** 3, 128 ** 3, 16, kind=("lognormal", 0.0, 50.0))
        del crow, col
    if "W2" in todo:
        m = int((1 << 20) * a.scale)
        crow, col = power_law(m, int((1 << 26) * a.scale), max(1 << 20, m))
        for k in ks:
            run("W2_powerlaw", crow, col, m, m, k)
        del crow, col
    if "W3" in todo:
        m, n = int(32768 * a.scale), 4096
        crow = (torch.arange(m + 1, device="cuda", dtype=torch.int64) * n).int()
        col = torch.arange(n, device="cuda", dtype=torch.int32).repeat(m)
        for k in ks:
            run("W3_dense_stripe", crow, col, m, n, k)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
