"""ExBDOT benchmark: n = 2^21 rows (the 128^3 grid of the sparse benchmarks), row-major blocks, ld == k.

One JSON line per case.  'D' at k = 4, 16, 64 and 'G' at p = q = 4, 8, 16 on fpuniform data, and one run of each mode on
lognormal(0, 50) data.  Per case: the kernel-chain time of ExBDOT (device events around enough calls to last >= 0.3 s),
the yardstick -- the loop of exdot_dev(X[:, i], Y[:, j], incx=ldx, incy=ldy) calls, k of them for 'D' and p * q for 'G'
--, ExBDOT under fpe = 1, for 'D' the plain two-stream read probe over the same bytes, for 'G' at 4 x 4 one
exgemm_dev('T', 'N', ...) call, and a CRC of the result bits of every exact path (automatic, the two test paths, fpe = 0,
the loop), which must agree.

    python tools/bench_bdot.py [--only D,G,wide] [--rows 2097152]
"""
import argparse
import ctypes as C
import json
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exblas_amd as ex  # noqa: E402
from bench_spmv import timed  # noqa: E402


def crc(t):
    return zlib.crc32(t.contiguous().cpu().numpy().view(np.uint8).tobytes())


def once(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def run(mode, n, p, q, kind=("fpuniform", 10, 0)):
    X = ex.gen_dev(kind[0], n * p, 12, kind[1], kind[2]).view(n, p)
    Y = ex.gen_dev(kind[0], n * q, 13, kind[1], kind[2]).view(n, q)
    pairs = [(j, j) for j in range(p)] if mode == "D" else [(i, j) for i in range(p) for j in range(q)]
    shape = (p,) if mode == "D" else (p, q)
    out = torch.zeros(shape, dtype=torch.float64, device="cuda")
    recs = [ex.new_record_buffer() for _ in pairs]
    res = {"mode": mode, "data": kind[0], "n": n, "p": p, "q": q, "outputs": len(pairs), "bytes": 8 * n * (p + q)}
    crcs = {}
    ex.set_bdot_path(0)
    res["exbdot_us"] = timed(lambda: ex.exbdot_dev(X, Y, mode, out), 0.3) * 1e6
    crcs["auto"] = crc(out)

    def loop():
        for (i, j), rec in zip(pairs, recs):
            ex.exdot_dev(X[:, i], Y[:, j], incx=p, incy=q, n=n, out=rec)
    res["exdot_loop_us"] = timed(loop, 0.3) * 1e6
    words = torch.stack([r[ex.OUT_EXACT] for r in recs]).view(torch.float64).view(shape)
    crcs["exdot_loop"] = crc(words)
    res["loop_product_flags"] = int(torch.stack([r[ex.OUT_FLAGS] for r in recs]).bitwise_and(0x78).max())
    for path in (1, 2):
        ex.set_bdot_path(path)
        out.zero_()
        res[f"path{path}_us"] = once(lambda: ex.exbdot_dev(X, Y, mode, out)) * 1e6
        crcs[f"path{path}"] = crc(out)
    ex.set_bdot_path(0)
    out.zero_()
    res["fpe0_us"] = once(lambda: ex.exbdot_dev(X, Y, mode, out, fpe=0, early_exit=False)) * 1e6
    crcs["fpe0"] = crc(out)
    res["plain_fpe1_us"] = timed(lambda: ex.exbdot_dev(X, Y, mode, out, fpe=1), 0.3) * 1e6
    lib = ex.load_library()
    if mode == "D":
        sink = torch.zeros(1, dtype=torch.float64, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        res["read2_probe_us"] = timed(lambda: lib.exblas_stream_read2_dev(
            C.c_void_p(X.data_ptr()), C.c_void_p(Y.data_ptr()), n * p, 0, st, C.c_void_p(sink.data_ptr())), 0.3) * 1e6
        res["exbdot_GBps"] = res["bytes"] / res["exbdot_us"] * 1e-3
        res["read2_probe_GBps"] = res["bytes"] / res["read2_probe_us"] * 1e-3
    elif p == 4:
        cm = torch.zeros((p, q), dtype=torch.float64, device="cuda")
        res["exgemm_TN_us"] = once(lambda: ex.exgemm_dev("T", "N", p, q, n, 1.0, X, p, Y, q, 0.0, cm, q)) * 1e6
        res["exgemm_crc_agrees"] = crc(cm) == crcs["auto"]
    res["crc"] = crcs
    res["crc_agree"] = len(set(crcs.values())) == 1
    res["loop_over_exbdot"] = res["exdot_loop_us"] / res["exbdot_us"]
    res["vs_plain"] = res["exbdot_us"] / res["plain_fpe1_us"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="D,G,wide")
    ap.add_argument("--rows", type=int, default=1 << 21)
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    todo = a.only.split(",")
    if "D" in todo:
        for k in (4, 16, 64):
            run("D", a.rows, k, k)
    if "G" in todo:
        for k in (4, 8, 16):
            run("G", a.rows, k, k)
    if "wide" in todo:
        run("D", a.rows, 16, 16, kind=("lognormal", 0.0, 50.0))
        run("G", a.rows, 8, 8, kind=("lognormal", 0.0, 50.0))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
