"""Plays the R ranks of exbdot_allreduce one after another in this one process, over the library's host-callback
transport (Comm.host) -- the block counterpart of tests/rank_worker.py.

Started by tests/test_gpu_bdot_allreduce.py in a fresh process: a communicator of more than one rank sets a process-wide
latch in the library.  Usage: bdot_rank_worker.py INPUT.npz OUTPUT.npz.  This script holds no expectations: it reads
operands, runs them and writes what came out.

Input: "plan", a JSON list of [name, pool, R, mode, p, q, fpe, early exit], and
  {pool}_x, {pool}_y   row pools (n x p and n x q) that the shards of several jobs draw from
  {name}_rows, {name}_off   the pool rows of every rank, concatenated, and where rank r's begin ([R + 1])
Rank r runs on path r % 3; with fpe < 0 it takes the variant (r + job) % 6 of {0, 3, 8} x early exit, so that the ranks
of a job differ.  fpe == 1 goes to the C entry point directly (the Python wrapper refuses it) and its return code is kept.
Two passes per job.  Pass 1: every rank runs; the all-reduce callback records a copy of each buffer it is given and
leaves it unchanged; the results of this pass are discarded.  Pass 2: the callback requires the same buffer again (the
export is reproducible) and overwrites it with the int64 sum over all ranks; run on every rank for R <= 8, else on the
first and the last.  The broadcast and all-gather callbacks raise.
Output per name: {name}_c [ranks run, the whole C buffer: p x (q + 2) or p + 2, a sentinel in the padding], {name}_ranks,
{name}_calls [R, calls] (the length of every all-reduce call of pass 1), {name}_contrib [R, words] (what the rank gave,
call after call), {name}_rc [2, R] (return codes of both passes; 0 where the wrapper returned)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SENTINEL = -12345.678
VARIANTS = [(fpe, ee) for fpe in (0, 3, 8) for ee in (False, True)]


class Transport:
    def __init__(self):
        self.record, self.rank, self.call, self.contrib, self.sums = True, 0, 0, [], []

    def begin(self, record, rank):
        self.record, self.rank, self.call = record, rank, 0

    def reset(self, R):
        self.contrib, self.sums = [[] for _ in range(R)], []

    def allreduce(self, buf):
        if self.record:
            self.contrib[self.rank].append(buf.copy())
        else:
            mine = self.contrib[self.rank][self.call]
            if buf.shape != mine.shape or not (buf == mine).all():
                raise RuntimeError(f"rank {self.rank} call {self.call}: the exported sets differ from the first pass")
            buf[:] = self.sums[self.call]
        self.call += 1

    def close_pass_one(self):
        lens = [[len(b) for b in c] for c in self.contrib]
        assert all(l == lens[0] for l in lens), f"the ranks made different all-reduce calls: {lens}"
        self.sums = [np.sum(np.stack([c[k] for c in self.contrib]), axis=0, dtype=np.int64) for k in range(len(lens[0]))]

    @staticmethod
    def refuse(*_):
        raise RuntimeError("exbdot_allreduce called a broadcast or an all-gather")


def main(inp, outp):
    import torch
    import exblas_amd as ex
    assert torch.cuda.is_available(), "the worker needs a HIP device"
    lib = ex.load_library()
    lib.exblas_hip_init(-1)
    z = np.load(inp, allow_pickle=False)
    plan = json.loads(str(z["plan"]))
    tr = Transport()
    comms, pools, out = {}, {}, {}
    for job, (name, pool, R, mode, p, q, fpe, ee) in enumerate(plan):
        if R not in comms:
            comms[R] = [ex.Comm.host(r, R, tr.allreduce, tr.refuse, tr.refuse) for r in range(R)]
        if pool not in pools:
            pools[pool] = (torch.from_numpy(z[pool + "_x"]).cuda(), torch.from_numpy(z[pool + "_y"]).cuda())
        cm, (PX, PY) = comms[R], pools[pool]
        rows, off = torch.from_numpy(z[name + "_rows"]).cuda(), z[name + "_off"]
        shards = [(PX[rows[off[r]:off[r + 1]]].contiguous(), PY[rows[off[r]:off[r + 1]]].contiguous()) for r in range(R)]
        ranks = list(range(R)) if R <= 8 else [0, R - 1]
        shape = (p, q + 2) if mode == "G" else (p + 2,)
        rc = np.zeros((2, R), dtype=np.int64)

        def run(r, pas):
            cbuf = torch.full(shape, SENTINEL, dtype=torch.float64, device="cuda")
            view = cbuf[:, :q] if mode == "G" else cbuf[:p]
            X, Y = shards[r]
            ex.set_bdot_path(r % 3)
            f, e = VARIANTS[(r + job) % len(VARIANTS)] if fpe < 0 else (fpe, bool(ee))
            if f == 1:
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                rc[pas, r] = lib.exblas_exbdot_allreduce_dev(cm[r].handle, mode.encode(), X.shape[0], p, q,
                                                             C.c_void_p(X.data_ptr()), max(p, 1), C.c_void_p(Y.data_ptr()),
                                                             max(q, 1), C.c_void_p(view.data_ptr()), shape[-1] if mode == "G" else 1,
                                                             f, int(e), st)
            else:
                got = ex.exbdot_allreduce(cm[r], X, Y, mode, view, f, e)
                assert got.data_ptr() == cbuf.data_ptr()
            return cbuf

        tr.reset(R)
        for r in range(R):
            tr.begin(True, r)
            run(r, 0)
        tr.close_pass_one()
        res = []
        for r in ranks:
            tr.begin(False, r)
            res.append(run(r, 1))
            assert tr.call == len(tr.sums), "the second pass made other calls than the first"
        torch.cuda.synchronize()
        out[name + "_c"] = np.stack([c.cpu().numpy().ravel() for c in res])
        out[name + "_ranks"] = np.array(ranks)
        out[name + "_calls"] = np.array([[len(b) for b in c] for c in tr.contrib], dtype=np.int64).reshape(R, -1)
        out[name + "_contrib"] = np.stack([np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in tr.contrib])
        out[name + "_rc"] = rc
    ex.set_bdot_path(0)
    for cs in comms.values():
        for c in cs:
            c.destroy()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
