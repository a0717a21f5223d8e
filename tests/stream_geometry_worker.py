"""Runs one geometry's plan of tests/stream_geometry_cases.py in this process, whose environment carries the geometry knobs
(EXBLAS_BPC_*, EXBLAS_BLOCKS_PER_CU, EXBLAS_GRID_ADJ, EXBLAS_NGROUPS: read once, when the library creates its context).

Started by tests/test_gpu_stream_geometry.py in a fresh process.  Usage: stream_geometry_worker.py INPUT.npz OUTPUT.npz.
This script holds no expectations: it reads operands and a plan, runs them and writes what came out.

Input: "plan", a JSON list of entries (stream_geometry_cases.build_plan), and the buffers narrow_x, narrow_y, wide_x, wide_y
(x: ExSUM's operand and ExDOT's second one, y: ExDOT's first).  The wide_then_narrow family is the wide buffer below the
entry's index "wtn" and the narrow one from there on.  Entry kinds:
  plain  exsum_dev / exdot_dev on the slice [off, off + n * inc) of the family's buffers
  acc    three exsum / exdot_accumulate_dev calls on consecutive slices of n elements, then finish_dev
  lone   operands built on the device by stream_geometry_cases.lone_build: a background that cancels inside every
         double2, 2^(12 j) (ExDOT: that times 1) at the entry's j-th seam position
Optional "tuning" = [blocks per CU, group accumulators, n]: after the plan, exblas_set_tuning with these and one ExSUM of
the first n narrow elements (tuning_rec, tuning_info).
Output: rec [entries, 128] (the records) and info [entries, 4] (last_blas1_info after each entry's last launch)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(inp, outp):
    import torch
    import exblas_amd as ex
    import stream_geometry_cases as G
    assert torch.cuda.is_available(), "the worker needs a HIP device"
    ex.load_library().exblas_hip_init(-1)
    z = np.load(inp, allow_pickle=False)
    plan = json.loads(str(z["plan"]))
    buf = {(fam, w): torch.from_numpy(z[f"{name}_{w}"]).cuda() for fam, name in ((G.NARROW, "narrow"), (G.WIDE, "wide"))
           for w in "xy"}
    wtn_cache = {}

    def operand(e, which):
        if e["family"] != G.WTN:
            return buf[e["family"], which]
        key = (e["wtn"], which)
        if key not in wtn_cache:
            wtn_cache.clear() if len(wtn_cache) >= 4 else None
            wtn_cache[key] = torch.cat([buf[G.WIDE, which][:e["wtn"]], buf[G.NARROW, which][e["wtn"]:]])
        return wtn_cache[key]

    def placed(dense, off, inc):
        """dense values at off, off + inc, ... of a fresh 16-byte-aligned buffer; returns the view that starts at off"""
        n = dense.numel()
        out = torch.zeros(off + n * inc + 2, dtype=torch.float64, device="cuda")
        assert out.data_ptr() % 16 == 0
        out[off:off + n * inc:inc] = dense
        return out[off:]

    rec = torch.zeros(len(plan), ex.OUT_WORDS, dtype=torch.int64, device="cuda")
    info = np.zeros((len(plan), 4), dtype=np.int64)
    for i, e in enumerate(plan):
        n, fpe, ee, dot = e["n"], e["fpe"], bool(e["ee"]), e["routine"] == G.DOT
        x, y = operand(e, "x"), operand(e, "y")
        assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0
        if e["kind"] == "lone":
            pos, head = [p for _, p in e["pos"]], G.lone_head(e)
            vals = G.lone_values(len(pos))
            if dot:     # a = y carries the seam values and the sign that cancels, b = x carries 1
                a = placed(G.lone_build(torch, y, n, head, pos, vals, True), e["offa"], e["inca"])
                b = placed(G.lone_build(torch, x, n, head, pos, [1.0] * len(pos), False), e["offb"], e["incb"])
                ex.exdot_dev(a, b, fpe, ee, incx=e["inca"], incy=e["incb"], n=n, out=rec[i])
            else:
                a = placed(G.lone_build(torch, x, n, head, pos, vals, True), e["offa"], e["inca"])
                ex.exsum_dev(a, fpe, ee, inca=e["inca"], n=n, out=rec[i])
        elif e["kind"] == "acc":
            for part in range(3):
                lo = e["offa"] + part * n
                if dot:
                    ex.exdot_accumulate_dev(y[lo:lo + n], x[lo:lo + n], fpe, ee, n=n)
                else:
                    ex.exsum_accumulate_dev(x[lo:lo + n], fpe, ee, n=n)
            ex.finish_dev(out=rec[i])
        elif dot:
            ex.exdot_dev(y[e["offa"]:], x[e["offb"]:], fpe, ee, incx=e["inca"], incy=e["incb"], n=n, out=rec[i])
        else:
            ex.exsum_dev(x[e["offa"]:], fpe, ee, inca=e["inca"], n=n, out=rec[i])
        info[i] = ex.last_blas1_info()
    out = {}
    if "tuning" in z.files:     # [blocks per CU, group accumulators, n]: exblas_set_tuning reports through last_blas1_info
        bpc, ngroups, n = (int(v) for v in z["tuning"])
        assert ex.load_library().exblas_set_tuning(bpc, ngroups, -1) == 0
        out["tuning_rec"] = ex.exsum_dev(buf[G.NARROW, "x"][:n], 8, True).cpu().numpy()
        out["tuning_info"] = np.array(ex.last_blas1_info(), dtype=np.int64)
    torch.cuda.synchronize()
    np.savez(outp, rec=rec.cpu().numpy(), info=info, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
