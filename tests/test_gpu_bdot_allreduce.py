"""GPU tests of exbdot_allreduce: R = 2, 3, 8 and 64 ranks played in one fresh child process over the host-callback
transport (tests/bdot_rank_worker.py), held to Python integers here: the doubles on every rank, what every rank gave to
the all-reduce, and how many all-reduce calls of which length were made.  And one rank over RCCL, against exbdot_dev."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bdot_rank_cases as S
import blas1_cases as B

pytestmark = pytest.mark.gpu

WORKER_TIMEOUT = 240
SENTINEL = -12345.678
W = 72
BALLAST_ROWS = max(S.BALLAST_K)
INVALID = 1   # hipErrorInvalidValue


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _pool(con):
    """the construction's rows, then 3 rows of +g and 3 rows of -g (with y_row): what a shard's row indices point into"""
    yb = np.tile(S.ballast_y(con.q), (BALLAST_ROWS, 1))
    g = np.full((BALLAST_ROWS, con.p), S.BALLAST_G)
    return np.concatenate([con.X, g, -g]), np.concatenate([con.Y, yb, yb])


def _rows(sh):
    """per rank the pool rows of its shard, in the shard's order"""
    n, out = sh.con.n, []
    for r, part in enumerate(sh.rows):
        front = list(range(n, n + sh.k)) if (sh.k and r == sh.ra) else []
        back = list(range(n + BALLAST_ROWS, n + BALLAST_ROWS + sh.k)) if (sh.k and r == sh.rb) else []
        out.append(np.array(front + list(part) + back, dtype=np.int64))
    return out


class Batch:
    """an integer block pair beyond one batch of outputs, cut into three shards (the middle one empty)"""

    def __init__(self, name, mode, n, p, q):
        rng = np.random.default_rng(p + q)
        self.name, self.mode, self.n, self.p, self.q = name, mode, n, p, q
        self.X = rng.integers(-(1 << 20), 1 << 20, size=(n, p)).astype(np.float64)
        self.Y = rng.integers(-(1 << 20), 1 << 20, size=(n, q)).astype(np.float64)
        self.cut = [0, 3, 3, n]
        self.outputs = p if mode == "D" else p * q

    def exact(self, a, b):
        X, Y = self.X[a:b].astype(np.int64), self.Y[a:b].astype(np.int64)
        return ((X * Y).sum(axis=0) if self.mode == "D" else X.T @ Y).ravel()


BATCHES = (Batch("batch_g", "G", 8, 65, 2), Batch("batch_d", "D", 8, 4097, 4097))
BATCH_CALLS = {"batch_g": [64 * 2 * W, 1 * 2 * W], "batch_d": [4096 * W, 1 * W]}


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    """(jobs by name, the worker's arrays).  One child process, one timeout; a crash or a timeout fails the fixture and
    with it every test that needs it -- nothing more is started"""
    tmp = tmp_path_factory.mktemp("bdot_ranks")
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    arrays, plan, jobs = {}, [], {}
    for ci, con in enumerate(S.constructions()):
        arrays[f"pool{ci}_x"], arrays[f"pool{ci}_y"] = _pool(con)

    def add(name, sh, fpe=-1, ee=0):
        ci = S.constructions().index(sh.con)
        rows = _rows(sh)
        for r in (0, sh.R - 1):
            assert (arrays[f"pool{ci}_x"][rows[r]] == sh.X[r]).all() and (arrays[f"pool{ci}_y"][rows[r]] == sh.Y[r]).all()
        arrays[name + "_rows"] = np.concatenate(rows)
        arrays[name + "_off"] = np.cumsum([0] + [len(x) for x in rows]).astype(np.int64)
        plan.append([name, f"pool{ci}", sh.R, sh.con.mode, sh.con.p, sh.con.q, fpe, ee])
        jobs[name] = sh

    for R in S.RANKS:
        for sh in S.jobs(R):
            add(f"r{R}_{sh.index}", sh)
    ints = S.constructions()[3]
    add("r64_ints", S.Shards(ints, 5, 64, "round_robin", 3))
    add("silent_r2", S.Shards(ints, 0, 2, "contiguous", 0), fpe=9, ee=1)
    add("plain_r2", S.Shards(ints, 0, 2, "contiguous", 0), fpe=1, ee=0)
    for b in BATCHES:
        arrays[b.name + "_pool_x"], arrays[b.name + "_pool_y"] = b.X, b.Y
        arrays[b.name + "_rows"] = np.arange(b.n, dtype=np.int64)
        arrays[b.name + "_off"] = np.array(b.cut, dtype=np.int64)
        plan.append([b.name, b.name + "_pool", 3, b.mode, b.p, b.q, -1, 0])
    arrays["plan"] = np.array(json.dumps(plan))
    np.savez(inp, **arrays)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bdot_rank_worker.py")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [worker, inp, outp]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(outp, allow_pickle=False)
    return jobs, {k: z[k] for k in z.files}


def _c_of(z, name, mode, p, q):
    """(C on every rank that ran [ranks, outputs], its padding)"""
    c = z[name + "_c"]
    if mode == "D":
        return c[:, :p], c[:, p:]
    c = c.reshape(len(c), p, q + 2)
    return c[:, :, :q].reshape(len(c), p * q), c[:, :, q:].reshape(len(c), -1)


def test_planted_cases_on_every_rank(played):
    jobs, z = played
    names = [n for n in jobs if n not in ("silent_r2", "plain_r2")]
    assert {jobs[n].R for n in names} == {2, 3, 8, 64}
    for name in names:
        sh = jobs[name]
        con, R = sh.con, sh.R
        ranks = z[name + "_ranks"].tolist()
        assert ranks == (list(range(R)) if R <= 8 else [0, R - 1])
        assert (z[name + "_rc"] == 0).all()
        c, pad = _c_of(z, name, con.mode, con.p, con.q)
        assert (_bits(pad) == _bits(np.array([SENTINEL]))[0]).all(), (sh, "the padding of C was written")
        for i in range(len(ranks)):
            bad = np.argwhere((_bits(c[i]) != _bits(con.want)) & con.keep)
            assert bad.size == 0, (sh, "rank", ranks[i], bad[:5].tolist())
            assert (_bits(c[i]) == _bits(c[0])).all(), (sh, "C differs between the ranks", ranks[i])
        # one call over all outputs; every rank, one without rows included, gave its own digit sets
        assert (z[name + "_calls"] == con.outputs * W).all() and z[name + "_calls"].shape == (R, 1), (sh, z[name + "_calls"])
        contrib = z[name + "_contrib"].reshape(R, con.outputs, W)
        for r in range(R):
            bad = np.argwhere((contrib[r, :, :B.NDIG] != sh.digits_r(r)).any(axis=1) & con.keep)
            assert bad.size == 0, (sh, "rank", r, "digits", bad[:5].tolist())
            assert (contrib[r, :, B.NDIG:][con.keep] == 0).all(), (sh, r)
            if len(sh.X[r]) == 0:
                assert (contrib[r] == 0).all(), (sh, r, "a rank without rows gives zero sets")


def test_corners_were_played(played):
    jobs, _ = played
    for R in S.RANKS:
        reached = set()
        for name, sh in jobs.items():
            if sh.R == R and name.startswith(f"r{R}_"):
                reached |= S.corners(sh)
        assert reached >= {"negative under positive", "beyond 2^1024 under finite", "deciding unit alone", "empty shard"}, (R, reached)


def test_batches_make_one_call_each(played):
    _, z = played
    for b in BATCHES:
        assert (z[b.name + "_rc"] == 0).all()
        calls = z[b.name + "_calls"]
        assert calls.tolist() == [BATCH_CALLS[b.name]] * 3, (b.name, calls.tolist())     # the empty rank makes the same calls
        contrib = z[b.name + "_contrib"].reshape(3, b.outputs, W)
        for r, (lo, hi) in enumerate(zip(b.cut, b.cut[1:])):
            want = B.digits_matrix([int(v) << B.U for v in b.exact(lo, hi)])
            bad = np.argwhere((contrib[r, :, :B.NDIG] != want).any(axis=1))
            assert bad.size == 0, (b.name, r, bad[:5].tolist())
            assert (contrib[r, :, B.NDIG:] == 0).all()
        c, pad = _c_of(z, b.name, b.mode, b.p, b.q)
        assert (_bits(pad) == _bits(np.array([SENTINEL]))[0]).all()
        for i in range(3):
            assert (_bits(c[i]) == _bits(b.exact(0, b.n).astype(np.float64))).all(), (b.name, i)


def test_silent_return_and_plain_sums_make_no_call(played):
    jobs, z = played
    for name, rc in (("silent_r2", 0), ("plain_r2", INVALID)):
        assert z[name + "_calls"].size == 0 and z[name + "_contrib"].size == 0, name
        assert (z[name + "_rc"] == rc).all(), (name, z[name + "_rc"])     # on every rank, in both passes
        assert (_bits(z[name + "_c"]) == _bits(np.array([SENTINEL]))[0]).all(), (name, "C was written")


def test_rccl_transport_one_rank_gives_the_exbdot_dev_bits():
    import torch
    import exblas_amd as ex
    assert torch.cuda.is_available()
    comm = ex.Comm.rccl(ex.Comm.unique_id(), 0, 1)
    try:
        for con in S.constructions()[2:]:
            X, Y = torch.from_numpy(con.X).cuda(), torch.from_numpy(con.Y).cuda()
            for fpe, ee in ((8, True), (0, False)):
                want = ex.exbdot_dev(X, Y, con.mode, None, fpe, ee)
                got = ex.exbdot_allreduce(comm, X, Y, con.mode, None, fpe, ee)
                torch.cuda.synchronize()
                assert torch.equal(want.view(torch.int64), got.view(torch.int64)), (con, fpe, ee)
                assert ((_bits(got.cpu().numpy().ravel()) == _bits(con.want)) | ~con.keep).all(), con
        b = BATCHES[0]
        X, Y = torch.from_numpy(b.X).cuda(), torch.from_numpy(b.Y).cuda()
        got = ex.exbdot_allreduce(comm, X, Y, b.mode)
        assert torch.equal(got.view(torch.int64), ex.exbdot_dev(X, Y, b.mode).view(torch.int64))
    finally:
        comm.destroy()
