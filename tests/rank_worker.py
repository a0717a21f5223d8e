"""Plays R ranks of the multi-rank ExSUM / ExDOT entry points one after another in this one process, over the library's
host-callback transport (Comm.host: the C path of gloo and RCCL -- finalize_groups export, callback, finalize_sets fold).

Started by tests/test_gpu_rank_rounding_edges.py in a fresh process: a communicator of more than one rank sets a
process-wide latch in the library.  Usage: rank_worker.py INPUT.npz OUTPUT.npz.  This script holds no expectations: it
reads operands, runs them and writes what came out.

Input: "plan", a JSON list of [name, R, mode] (mode: allreduce, finish or pipelined), and per name
  {name}_a, {name}_b   the operands of every job and rank, concatenated (b is unused by an ExSUM job)
  {name}_off           [jobs, R + 1] where rank r's shard of a job starts; {name}_meta [jobs, 3]: fpe, early exit, is ExDOT
Two passes per job.  Pass 1: every rank runs; the all-reduce callback records a copy of each buffer it is given (two per
reduction: 72 words, then 144) and leaves it unchanged; the records of this pass are discarded.  Pass 2: the callback
requires the same buffer again (the export is reproducible) and overwrites it with the int64 sum over all ranks; run on
every rank for R <= 8, else on the first and the last.  The broadcast and all-gather callbacks raise.
Output per name: {name}_rec [jobs, ranks run, 128], {name}_ranks, {name}_main [jobs, R, 72], {name}_ext [jobs, R, 144]."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


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
                raise RuntimeError(f"rank {self.rank} call {self.call}: the exported set differs from the first pass")
            buf[:] = self.sums[self.call]
        self.call += 1

    def close_pass_one(self):
        ncall = len(self.contrib[0])
        assert all(len(c) == ncall for c in self.contrib), "the ranks made different numbers of all-reduce calls"
        self.sums = [np.sum(np.stack([c[k] for c in self.contrib]), axis=0, dtype=np.int64) for k in range(ncall)]

    @staticmethod
    def refuse(*_):
        raise RuntimeError("a blas1 reduction called a broadcast or an all-gather")


def main(inp, outp):
    import torch
    import exblas_amd as ex
    assert torch.cuda.is_available(), "the worker needs a HIP device"
    ex.load_library().exblas_hip_init(-1)
    z = np.load(inp, allow_pickle=False)
    plan = json.loads(str(z["plan"]))
    tr = Transport()
    comms, out = {}, {}
    for name, R, mode in plan:
        if R not in comms:
            comms[R] = [ex.Comm.host(r, R, tr.allreduce, tr.refuse, tr.refuse) for r in range(R)]
        cm = comms[R]
        A, Bv = torch.from_numpy(z[name + "_a"]).cuda(), torch.from_numpy(z[name + "_b"]).cuda()
        off, meta = z[name + "_off"], z[name + "_meta"]
        n = off.shape[0]
        ranks = list(range(R)) if R <= 8 else [0, R - 1]
        rec = torch.zeros(n, len(ranks), ex.OUT_WORDS, dtype=torch.int64, device="cuda")
        scratch = ex.new_record_buffer()
        main_w = np.zeros((n, R, ex.SET_WORDS), dtype=np.int64)
        ext_w = np.zeros((n, R, 2 * ex.SET_WORDS), dtype=np.int64)

        def reduce(j, r, dst):
            o0, o1 = int(off[j, r]), int(off[j, r + 1])
            fpe, ee, dot = int(meta[j, 0]), bool(meta[j, 1]), bool(meta[j, 2])
            a, b = A[o0:o1], Bv[o0:o1]
            if mode == "allreduce":
                ex.exdot_allreduce(cm[r], a, b, fpe, ee, out=dst) if dot else ex.exsum_allreduce(cm[r], a, fpe, ee, out=dst)
            elif mode == "finish":
                h = (o1 - o0) // 2
                for lo, hi in ((0, h), (h, o1 - o0)):
                    ex.exdot_accumulate_dev(a[lo:hi], b[lo:hi], fpe, ee, n=hi - lo) if dot else ex.exsum_accumulate_dev(a[lo:hi], fpe, ee, n=hi - lo)
                ex.allreduce_finish(cm[r], out=dst)
            elif dot:
                ex.exdot_allreduce_pipelined(cm[r], a, b, fpe, ee, out=dst)
            else:
                ex.exsum_allreduce_pipelined(cm[r], a, fpe, ee, out=dst)

        # a pipelined rank issues the whole sequence and then drains; the other modes take one job at a time
        groups = [list(range(n))] if mode == "pipelined" else [[j] for j in range(n)]
        for group in groups:
            tr.reset(R)
            for r in range(R):
                tr.begin(True, r)
                for j in group:
                    reduce(j, r, scratch)
                if mode == "pipelined":
                    ex.pipeline_drain(cm[r])
            tr.close_pass_one()
            assert len(tr.sums) == 2 * len(group), "not two all-reduce calls per reduction"
            for k, j in enumerate(group):
                for r in range(R):
                    main_w[j, r], ext_w[j, r] = tr.contrib[r][2 * k], tr.contrib[r][2 * k + 1]
            for i, r in enumerate(ranks):
                tr.begin(False, r)
                for j in group:
                    reduce(j, r, rec[j, i])
                if mode == "pipelined":
                    ex.pipeline_drain(cm[r])
        torch.cuda.synchronize()
        out[name + "_rec"], out[name + "_ranks"] = rec.cpu().numpy(), np.array(ranks)
        out[name + "_main"], out[name + "_ext"] = main_w, ext_w
    for cs in comms.values():
        for c in cs:
            c.destroy()
    np.savez(outp, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
