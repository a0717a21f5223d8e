"""Row-sharded ExBDOT benchmark: what the export / round split and the all-reduce form cost over exbdot_dev on one GPU.

n = 2^21 rows (the 128^3 grid of the sparse benchmarks), row-major blocks, ld == k, fpuniform data: 'D' at k = 16 and 'G'
at p = q = 8.  Per case the kernel-chain time (device events around enough calls to last >= 0.3 s) of
  exbdot_dev                          memset, accumulate, finalize
  exbdot_export_dev + exbdot_round_dev  memset, accumulate, export (72 int64 per output written), round (read again)
  exbdot_allreduce                    on a one-rank host communicator without callbacks: the export in place, no
                                      collective, the round -- the fixed cost of the form without any transport
and a CRC of the output bits of each, which must agree.  One JSON line per case, printed and appended to --out.

    python tools/bench_bdot_sharded.py [--rows 2097152] [--out profiles/bdot_sharded_bench.jsonl]
"""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exblas_amd as ex  # noqa: E402
from bench_spmv import timed  # noqa: E402


def crc(t):
    return zlib.crc32(t.contiguous().cpu().numpy().view(np.uint8).tobytes())


def run(comm, mode, n, p, q, out_path):
    X = ex.gen_dev("fpuniform", n * p, 12, 10, 0).view(n, p)
    Y = ex.gen_dev("fpuniform", n * q, 13, 10, 0).view(n, q)
    outputs = p if mode == "D" else p * q
    shape = (p,) if mode == "D" else (p, q)
    out = torch.zeros(shape, dtype=torch.float64, device="cuda")
    sets = torch.zeros((outputs, ex.SET_WORDS), dtype=torch.int64, device="cuda")
    res = {"mode": mode, "data": "fpuniform", "n": n, "p": p, "q": q, "outputs": outputs, "bytes": 8 * n * (p + q),
           "set_bytes": 8 * ex.SET_WORDS * outputs}
    crcs = {}
    res["exbdot_us"] = timed(lambda: ex.exbdot_dev(X, Y, mode, out), 0.3) * 1e6
    crcs["exbdot_dev"] = crc(out)

    def split():
        ex.exbdot_export_dev(X, Y, mode, sets)
        ex.exbdot_round_dev(sets, mode, p, q, out)
    out.zero_()
    res["export_round_us"] = timed(split, 0.3) * 1e6
    crcs["export_round"] = crc(out)
    res["export_us"] = timed(lambda: ex.exbdot_export_dev(X, Y, mode, sets), 0.3) * 1e6
    res["round_us"] = timed(lambda: ex.exbdot_round_dev(sets, mode, p, q, out), 0.3) * 1e6
    out.zero_()
    res["allreduce_one_rank_us"] = timed(lambda: ex.exbdot_allreduce(comm, X, Y, mode, out), 0.3) * 1e6
    crcs["allreduce_one_rank"] = crc(out)
    # two halves of the rows exported apart and rounded together: the same bits again
    h = (n // 2) & ~1
    two = torch.stack([ex.exbdot_export_dev(X[:h], Y[:h], mode), ex.exbdot_export_dev(X[h:], Y[h:], mode)])
    crcs["two_shards"] = crc(ex.exbdot_round_dev(two, mode, p, q))
    res["crc"] = crcs
    res["crc_agree"] = len(set(crcs.values())) == 1
    res["export_round_extra_us"] = res["export_round_us"] - res["exbdot_us"]
    res["allreduce_extra_us"] = res["allreduce_one_rank_us"] - res["exbdot_us"]
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "a") as fh:
        fh.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bdot_sharded_bench.jsonl"))
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    comm = ex.Comm.host(0, 1, None, None, None)
    try:
        run(comm, "D", a.rows, 16, 16, a.out)
        run(comm, "G", a.rows, 8, 8, a.out)
        torch.cuda.synchronize()
    finally:
        comm.destroy()


if __name__ == "__main__":
    main()
