"""ExSpMV benchmark: W1 27-point stencil on 128^3 (int32), W2 power-law row lengths, W3 a dense stripe as CSR.

Each workload prints one JSON line: the kernel-chain time of ExSpMV (device events around enough calls to last
>= 0.5 s), the fraction of 8 TB/s from the algorithmic bytes, the same workload under fpe = 1 (the plain kernel),
torch's CSR product, the accumulator-only path (exblas_set_spmv_path(1)), W3 also under ExGEMV 'N', and a CRC of the
result bits of every ExSpMV path (they must agree).

    python tools/bench_spmv.py [--only W1,W2,W3] [--scale 1.0]
"""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import exblas_amd as ex  # noqa: E402

PEAK = 8.0e12


def timed(fn, min_s=0.5):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    one = max(e0.elapsed_time(e1) * 1e-3, 1e-6)
    reps = max(3, int(min_s / one))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def stencil(k):
    dev = "cuda"
    i = torch.arange(k ** 3, device=dev)
    z, y, x = i // (k * k), (i // k) % k, i % k
    cols = []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                ok = (z + dz >= 0) & (z + dz < k) & (y + dy >= 0) & (y + dy < k) & (x + dx >= 0) & (x + dx < k)
                cols.append(torch.where(ok, i + (dz * k + dy) * k + dx, torch.full_like(i, -1)))
    c = torch.stack(cols, 1)
    mask = c >= 0
    crow = torch.zeros(k ** 3 + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(mask.sum(1), 0)
    return crow.int(), c[mask].int()


def power_law(m, nnz_target, longest, seed=1):
    rng = np.random.default_rng(seed)
    lens = np.floor(rng.pareto(1.2, size=m) * 8 + 1).astype(np.int64)
    lens[0] = longest
    lens = np.minimum(lens, longest)
    scale = (nnz_target - longest) / max(1, lens[1:].sum())
    lens[1:] = np.maximum(1, np.floor(lens[1:] * scale)).astype(np.int64)
    crow = np.concatenate([[0], np.cumsum(lens)])
    nnz = int(crow[-1])
    col = torch.randint(0, m, (nnz,), device="cuda", generator=torch.Generator("cuda").manual_seed(seed))
    return torch.from_numpy(crow).cuda().int(), col.int()


def crc(t):
    return zlib.crc32(t.cpu().numpy().view(np.uint8).tobytes())


def run(name, crow, col, m, n, dense=None):
    nnz = col.numel()
    isz = crow.element_size()
    val = ex.gen_dev("fpuniform", nnz, 11, 10, 0)
    x = ex.gen_dev("fpuniform", n, 12, 10, 0)
    y = torch.zeros(m, dtype=torch.float64, device="cuda")
    A = (crow, col, val, (m, n))
    bytes_ = nnz * (8 + isz) + (m + 1) * isz + 8 * n + 8 * m
    out = {"workload": name, "m": m, "n": n, "nnz": nnz, "index_bits": 8 * isz, "alg_bytes": bytes_}
    crcs = {}
    ex.set_spmv_path(0)
    t = timed(lambda: ex.exspmv_dev(A, x, 1.0, 0.0, y))
    crcs["auto"] = crc(y)
    out["exspmv_us"] = t * 1e6
    out["frac_of_8TBs"] = bytes_ / t / PEAK
    out["info"] = ex.last_spmv_info()
    ex.set_spmv_path(1)
    out["accumulator_path_us"] = timed(lambda: ex.exspmv_dev(A, x, 1.0, 0.0, y)) * 1e6
    crcs["accumulator"] = crc(y)
    ex.set_spmv_path(0)
    out["plain_fpe1_us"] = timed(lambda: ex.exspmv_dev(A, x, 1.0, 0.0, y, fpe=1)) * 1e6
    try:
        At = torch.sparse_csr_tensor(crow.long(), col.long(), val, size=(m, n))
        xv = x.view(-1, 1)
        out["torch_csr_us"] = timed(lambda: At @ xv) * 1e6
    except Exception as exc:  # noqa: BLE001
        out["torch_csr_us"] = None
        out["torch_csr_error"] = str(exc)[:120]
    if dense is not None:
        Ad = dense(val)
        out["exgemv_N_us"] = timed(lambda: ex.exgemv_dev("N", m, n, 1.0, Ad, m, x, 0.0, y, 8, True)) * 1e6
        crcs["exgemv"] = crc(y)
    out["crc"] = crcs
    out["crc_agree"] = len(set(crcs.values())) == 1
    out["vs_plain"] = out["exspmv_us"] / out["plain_fpe1_us"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="W1,W2,W3")
    ap.add_argument("--scale", type=float, default=1.0, help="W2 / W3 size factor (W1 is fixed)")
    a = ap.parse_args()
    ex.load_library().exblas_hip_init(-1)
    todo = a.only.split(",")
    if "W1" in todo:
        crow, col = stencil(128)
        run("W1_stencil27_128^3", crow, col, 128 ** 3, 128 ** 3)
        del crow, col
    if "W2" in todo:
        m = int((1 << 20) * a.scale)
        crow, col = power_law(m, int((1 << 26) * a.scale), max(1 << 20, m))
        run("W2_powerlaw", crow, col, m, m)
        del crow, col
    if "W3" in todo:
        m, n = int(32768 * a.scale), 4096
        crow = (torch.arange(m + 1, device="cuda", dtype=torch.int64) * n).int()
        col = torch.arange(n, device="cuda", dtype=torch.int32).repeat(m)
        # the same matrix column-major for ExGEMV 'N': A(i, j) = val[i * n + j]
        run("W3_dense_stripe", crow, col, m, n, dense=lambda v: v.view(m, n).t().contiguous().view(-1))
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
