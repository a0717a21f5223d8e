"""The multi-rank and multi-device merge of ExSUM / ExDOT on constructed totals dealt adversarially (tests/rank_cases.py),
bit for bit.

A blas1 result is the same bits for any rank count and any device list only if the merge is exact: every rank (every
part of a host-pointer call) normalises its accumulators to a 72-word digit set, ExDOT also exports a LOW and a HIGH
digit set (k_finalize with ext_out), the sets are added as int64 words, and a second k_finalize (ext_in) propagates the
carries, folds the LOW and HIGH sums back in and rounds once.  Here the deciding half or sticky unit sits on another rank
than the mantissa, ranks hold negative partial totals (a signed top digit over a borrow run of 0xffffffff digits) or
partial totals beyond 2^1024 under a finite total, the LOW / HIGH sets are non-zero on some ranks and cancel in the sum,
and a rank's stale exported set has to be overwritten with zeros.

Ranks: tests/rank_worker.py plays R = 2, 3, 8 and 64 ranks one after another in one fresh child process through
exblas_exsum_allreduce_dev, exblas_exdot_allreduce_dev, exblas_allreduce_finish_dev and the two pipelined calls over the
host-callback transport, and writes records and every rank's exported sets to a file; the tests here compare that file
with expectations made of Python integers alone (blas1_cases, helpers.expected_fields).  Devices: the same cases through
exsum_record / exdot_record with exblas_set_host_devices([0] * nv).  No tolerance.  Each test prints what it ran."""
import json
import math
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import blas1_cases as B
import rank_cases as RC
from helpers import bits, exact_int_from_digits, expected_fields, same_bits

pytestmark = pytest.mark.gpu

WORKER_TIMEOUT = 240
PLAIN_TWIN = "pipe_r2_plain"          # the pipelined sequence once more through the plain calls
EXT_SCALE = 1 << (32 * 38)            # superacc.hip.h: EXT_SHIFT_DIGITS -- the LOW unit is 2^-1216 units, the HIGH unit 2^1216


def _mode(name):
    return "finish" if name.startswith("finish") else ("pipelined" if name.startswith("pipe") and name != PLAIN_TWIN else "allreduce")


def _pack(jobs):
    R = jobs[0].shards.R
    off = np.zeros((len(jobs), R + 1), dtype=np.int64)
    meta = np.zeros((len(jobs), 3), dtype=np.int64)
    a, b, pos = [], [], 0
    for j, job in enumerate(jobs):
        sh = job.shards
        assert sh.R == R
        meta[j] = (job.fpe, int(job.ee), int(sh.is_dot))
        for r in range(R):
            off[j, r] = pos
            a.append(sh.a[r])
            b.append(sh.b[r] if sh.is_dot else np.zeros(len(sh.a[r])))
            pos += len(sh.a[r])
        off[j, R] = pos
    return np.concatenate(a), np.concatenate(b), off, meta


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    """the worker's output: (batches, arrays).  One child process, one timeout; a crash or a timeout fails the fixture
    and with it every test that needs it -- nothing more is started"""
    import time
    t0 = time.perf_counter()
    batches = dict(RC.batches())
    batches[PLAIN_TWIN] = batches["pipe_r2"]
    tmp = tmp_path_factory.mktemp("ranks")
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    arrays = {"plan": np.array(json.dumps([[name, jobs[0].shards.R, _mode(name)] for name, jobs in batches.items()]))}
    for name, jobs in batches.items():
        arrays[name + "_a"], arrays[name + "_b"], arrays[name + "_off"], arrays[name + "_meta"] = _pack(jobs)
    np.savez(inp, **arrays)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "rank_worker.py")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [worker, inp, outp]
    t1 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    reductions = sum(len(jobs) * (R + (R if R <= 8 else 2)) for jobs in batches.values() for R in [jobs[0].shards.R])   # two passes
    print(f"rank worker: {time.perf_counter() - t1:.2f} s for {reductions} reductions of one rank each "
          f"({t1 - t0:.2f} s to build and write the cases)")
    z = np.load(outp, allow_pickle=False)
    return batches, {k: z[k] for k in z.files}


def _fail(what, name, jobs, bad, got=None, want=None):
    idx = np.nonzero(bad)[0]
    def show(i):
        extra = () if got is None else (hex(int(got[i])), hex(int(want[i])))
        return (int(i), repr(jobs[i].shards), jobs[i].fpe, jobs[i].ee) + extra
    assert not len(idx), (what, name, len(idx), [show(i) for i in idx[:5]])


def _set_value(words):
    assert not words[B.NDIG:].any(), "words 68 .. 71 of an extension set are not zero"
    return exact_int_from_digits(words[:B.NDIG])


def _check_records(name, jobs, rec):
    """every record that was produced, field by field; rec: [jobs, k, 128] (all k must be identical)"""
    import exblas_amd as ex
    n = len(jobs)
    for i in range(1, rec.shape[1]):
        _fail(f"the record of run {i} differs from that of run 0", name, jobs, (rec[:, i] != rec[:, 0]).any(axis=1))
    out = rec[:, 0]
    want = bits([j.shards.want for j in jobs])
    flags = np.array([j.shards.flags for j in jobs], dtype=np.int64)
    _fail("exact", name, jobs, ~same_bits(out[:, ex.OUT_EXACT], want), out[:, ex.OUT_EXACT], want)
    _fail("flags", name, jobs, out[:, ex.OUT_FLAGS] != flags, out[:, ex.OUT_FLAGS], flags)
    # refmode, canon and digits where the total is an integer number of units (ExSUM), masked like the single-GPU tests
    si = [i for i, j in enumerate(jobs) if not j.shards.is_dot and j.shards.case is not None]
    if si:
        sj = [jobs[i] for i in si]
        _, ref, canon, digits, fits = expected_fields([j.shards.case for j in sj])
        o = out[si]
        _fail("refmode", name, sj, fits & ~same_bits(o[:, ex.OUT_REFMODE], ref), o[:, ex.OUT_REFMODE], ref)
        _fail("canon", name, sj, fits & (o[:, ex.OUT_CANON:ex.OUT_CANON + 41] != canon).any(axis=1))
        _fail("digits", name, sj, (o[:, ex.OUT_DIGITS:ex.OUT_DIGITS + 68] != digits).any(axis=1))
    return n


def _check_exports(name, jobs, main, ext):
    """what every rank handed to the all-reduce: main [jobs, R, 72], ext [jobs, R, 144]"""
    S = B.NDIG
    for j, job in enumerate(jobs):
        sh = job.shards
        if sh.T_r is None and sh.low_r is None:
            continue                                                  # (non-finite operands: no exact partial totals)
        for r in range(sh.R):
            what = (name, j, repr(sh), "rank", r)
            low, high = ext[j, r, :RC_SET], ext[j, r, RC_SET:]
            for which, words, part in (("LOW", low, sh.low_r[r]), ("HIGH", high, sh.high_r[r])):
                assert ((words[:S - 1] >= 0) & (words[:S - 1] < 1 << 32)).all(), what + (which, "a digit outside [0, 2^32)")
                if part is None:
                    assert not words.any(), what + (which, "set not zero on a rank without such a product")
            if sh.T_r is None:
                continue
            if not sh.is_dot:
                assert (main[j, r, :S] == B.digits_matrix([sh.T_r[r]])[0]).all(), what + ("main digits",)
                assert not main[j, r, S:].any(), what + ("main words 68 .. 71",)
            else:
                # ExDOT: each exported set holds exactly its share of the rank's products
                lo_v, hi_v = sh.low_r[r] or Fraction(0), sh.high_r[r] or Fraction(0)
                assert Fraction(_set_value(low), EXT_SCALE) == lo_v, what + ("LOW value",)
                assert _set_value(high) * EXT_SCALE == hi_v, what + ("HIGH value",)
                assert exact_int_from_digits(main[j, r, :S]) == sh.T_r[r] - lo_v - hi_v, what + ("main value",)
                assert ((main[j, r, :S - 1] >= 0) & (main[j, r, :S - 1] < 1 << 32)).all(), what + ("main digit range",)
                assert main[j, r, S:S + 3].tolist() == [0, 0, 0], what + ("non-finite indicators",)
                assert main[j, r, S + 3] == (sh.low_r[r] is not None) + 65536 * (sh.high_r[r] is not None), what + ("word 71",)


RC_SET = 72


def _run(played, name):
    batches, z = played
    jobs = batches[name]
    n = _check_records(name, jobs, z[name + "_rec"])
    _check_exports(name, jobs, z[name + "_main"], z[name + "_ext"])
    R = jobs[0].shards.R
    used = sorted({(j.shards.partition, str(j.shards.ballast)) for j in jobs})
    print(f"{name}: {n} cases at R = {R}, records of ranks {z[name + '_ranks'].tolist()}, "
          f"{len({p for p, _ in used})} partitions x {len({b for _, b in used})} ballast settings")
    return jobs, z


@pytest.mark.parametrize("R", [2, 3, 8])
def test_exsum_ranks(played, R):
    """A - D over R simulated ranks through exblas_exsum_allreduce_dev: the record's fields, and every rank's exported
    digit set against digits_from_int of its partial total (negative ones and ones beyond 2^1024 included)"""
    jobs, _ = _run(played, f"sum_r{R}")
    kinds = {(c.family, c.kind) for c in B.sum_cases()}
    assert {(j.shards.case.family, j.shards.case.kind) for j in jobs} == kinds
    assert any(t < 0 < j.shards.T for j in jobs for t in j.shards.T_r)
    assert any(abs(t) > B.DBL_MAX_UNITS >= abs(j.shards.T) for j in jobs for t in j.shards.T_r)


@pytest.mark.parametrize("R", [2, 3, 8])
def test_exdot_ranks(played, R):
    """F over R simulated ranks through exblas_exdot_allreduce_dev with main, LOW and HIGH ballast: the double, the flag
    word, and the exact value of every exported main, LOW and HIGH set"""
    jobs, _ = _run(played, f"dot_r{R}")
    assert {j.shards.ballast for j in jobs} == set(RC.DOT_BALLAST)
    assert {c.kind for c in B.family_f_high()} <= {j.shards.case.kind for j in jobs}


def test_allreduce_finish_after_two_accumulate_calls(played):
    """exblas_allreduce_finish_dev after two *_accumulate_dev calls per rank (the rank's shard cut in two)"""
    jobs, _ = _run(played, "finish_r3")
    assert len(jobs) == 50 and any(j.shards.is_dot for j in jobs) and any(not j.shards.is_dot for j in jobs)


def test_pipelined_slots(played):
    """16 reductions per rank through the pipelined calls and pipeline_drain: each accumulator slot (and its exported
    extension sets) sees a case with HIGH products, then one with none, then one with LOW only, then a plain ExSUM; every
    record equals the expectation and the record of the plain call"""
    jobs, z = _run(played, "pipe_r2")
    _run(played, PLAIN_TWIN)
    assert (z["pipe_r2_rec"] == z[PLAIN_TWIN + "_rec"]).all()
    assert (z["pipe_r2_main"] == z[PLAIN_TWIN + "_main"]).all() and (z["pipe_r2_ext"] == z[PLAIN_TWIN + "_ext"]).all()
    for slot in range(2):
        seen = [j.shards.flags if j.shards.is_dot else -1 for j in jobs[slot::2]]
        assert seen[:4] == [16 | 64, 0, 8 | 32, -1], seen


def test_flag_counters_over_64_ranks(played):
    """40 ranks with a product below 2^-968, 3 with a finite overflowing product that cancels: word 71 of the summed set"""
    jobs, z = _run(played, "counters_r64")
    summed = z["counters_r64_main"][0].sum(axis=0)
    assert summed[71] == RC.COUNTER_UNDER + RC.COUNTER_OVER * 65536, hex(int(summed[71]))
    assert jobs[0].shards.flags == 8 | 16 | 32 | 64 and z["counters_r64_ranks"].tolist() == [0, 63]


def test_non_finite_table(played):
    """Inf / NaN on single ranks at R = 3: flags are the OR, NaN if a NaN or both infinities were seen, else the infinity"""
    jobs, z = played[0]["nonfinite_r3"], played[1]
    rec = z["nonfinite_r3_rec"]
    for i, job in enumerate(jobs):
        sh = job.shards
        for k in range(rec.shape[1]):
            got = float(rec[i, k, 0:1].view(np.float64)[0])
            same = (math.isnan(got) and math.isnan(sh.want)) or got == sh.want
            assert same and rec[i, k, 2] == sh.flags, (repr(sh), k, got, sh.want, int(rec[i, k, 2]), sh.flags)
    print(f"non-finite table: {len(jobs)} rows at R = 3")


# ---------------------------------------------------------------------------------------------
# the host-pointer merge over several virtual devices (host_reduce, nv > 1): no communicator
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    exblas_amd.load_library().exblas_hip_init(-1)
    return exblas_amd


def _host_layout(sh, nv, inc, offset):
    """one host array per operand: part v covers [n v / nv, n (v + 1) / nv) and holds shard v, zero-padded (a 0 * 0 product
    raises no flag); between strided elements and in front of the offset: NaN, which must not be read"""
    slot = max(2, max(len(x) for x in sh.a))
    n = nv * slot
    assert all((n * v) // nv == v * slot for v in range(nv + 1))
    out = []
    for parts in ((sh.a, sh.b) if sh.is_dot else (sh.a,)):
        dense = np.zeros(n)
        for v in range(nv):
            dense[v * slot:v * slot + len(parts[v])] = parts[v]
        buf = np.full(offset + (n - 1) * inc + 1, np.nan)
        buf[offset::inc] = dense
        out.append(buf)
    return n, out


@pytest.mark.parametrize("nv", [2, 3, 8])
def test_host_merge_over_virtual_devices(ex, nv):
    """about 300 ExSUM and 300 ExDOT cases per device list through exsum_record / exdot_record, every third one strided
    and offset (inca = 3, offset 5)"""
    import ctypes as C
    lib = ex.load_library()
    sums, dots = RC.host_batches(nv)
    devs = (C.c_int * nv)(*([0] * nv))
    assert lib.exblas_set_host_devices(nv, devs) == 0
    try:
        recs = []
        for k, job in enumerate(sums + dots):
            sh = job.shards
            inc, offset = (3, 5) if k % 3 == 0 else (1, 0)
            n, arrs = _host_layout(sh, nv, inc, offset)
            if sh.is_dot:
                r = ex.exdot_record(n, arrs[0], inc, offset, arrs[1], inc, offset, job.fpe, job.ee)
            else:
                r = ex.exsum_record(n, arrs[0], inc, offset, job.fpe, job.ee)
            recs.append(r.words)
    finally:
        assert lib.exblas_set_host_devices(0, None) == 0
    rec = np.stack(recs)[:, None, :]
    _check_records(f"host sums nv={nv}", sums, rec[:len(sums)])
    _check_records(f"host dots nv={nv}", dots, rec[len(sums):])
    assert len(sums) >= 100 and len(dots) >= 100
    assert {j.shards.partition for j in sums + dots} == set(RC.PARTITIONS)
    assert {j.shards.ballast for j in dots} == set(RC.DOT_BALLAST)
    print(f"host merge over {nv} virtual devices: {len(sums)} sums, {len(dots)} dots")
