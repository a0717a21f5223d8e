"""Every positional seam of the streaming ExSUM / ExDOT kernels in every launch geometry, bit for bit.

k_blas1_stream and k_blas1_strided (fp64 front ends SumF64 and DotF64) are positional bookkeeping: a scalar head, tiles dealt round-robin to the
workgroups, two register sets with two exits, re-fetched last tiles, a grid-strided remainder, a scalar tail, a bypass
counter, group accumulators chosen by blockIdx.x % ngroups.  Which of these a size exercises is decided by the launch
geometry, and the geometry knobs (EXBLAS_BPC_*, EXBLAS_BLOCKS_PER_CU, EXBLAS_GRID_ADJ, EXBLAS_NGROUPS) are read once, when
the library creates its context.  So each geometry of tests/stream_geometry_cases.py runs in a fresh child process
(tests/stream_geometry_worker.py), one at a time, and this module compares what the child wrote with totals made of Python
integers alone: the reported kernel, grid and group count against the model (so that the sizes provably reach the seams
they were chosen for), then digits, the correctly rounded double and the flag word of every record.  The lone-element
cases decode a mismatch into the names of the seams that were dropped or counted twice.  No tolerance anywhere.

If a child ends by a signal, a timeout or any error exit, the remaining geometries fail without starting another child."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import stream_geometry_cases as G
from helpers import exact_int_from_digits

pytestmark = pytest.mark.gpu

# the child: python + torch + library start-up, the operands to the device, about 1700 launches well below a millisecond
# each and twice that many small host calls: 2.1 to 2.5 s on an MI355X.  The parent allows about ten times that.
WORKER_TIMEOUT = 25
GEOMETRY_KNOBS = ("EXBLAS_BPC_SUM", "EXBLAS_BPC_DOT", "EXBLAS_BPC_SA", "EXBLAS_BPC_HEAVY", "EXBLAS_BLOCKS_PER_CU",
                  "EXBLAS_GRID_ADJ", "EXBLAS_NGROUPS")
_broken = []          # set when a child died: what happened


@pytest.fixture(scope="module")
def num_cu():
    import torch
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)


@pytest.fixture(scope="module")
def data_cache():
    return {}


def _run_child(tmp, env_extra, arrays):
    inp, outp = str(tmp / "in.npz"), str(tmp / "out.npz")
    np.savez(inp, **arrays)
    env = {k: v for k, v in os.environ.items() if k not in GEOMETRY_KNOBS}
    env.update(env_extra)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_geometry_worker.py")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [worker, inp, outp]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=WORKER_TIMEOUT, env=env)
    except subprocess.TimeoutExpired as exc:
        _broken.append(f"the child of {env_extra} did not finish within {WORKER_TIMEOUT} s")
        raise AssertionError(_broken[-1]) from exc
    if r.returncode != 0:      # a signal, or an error exit (a HIP fault surfaces as one): nothing more is started on the card
        how = f"ended by signal {-r.returncode}" if r.returncode < 0 else f"exited with status {r.returncode}"
        _broken.append(f"the child of {env_extra} {how}")
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    z = np.load(outp, allow_pickle=False)
    return {k: z[k] for k in z.files}


def _describe(e):
    return (f"{'exdot' if e['routine'] else 'exsum'} {e['kind']} {G.FAMILIES[e['family']]} fpe={e['fpe']} ee={e['ee']} n={e['n']} "
            f"inc=({e['inca']},{e['incb']}) off=({e['offa']},{e['offb']})")


@pytest.mark.parametrize("geometry", G.GEOMETRY_NAMES)
def test_stream_seams(geometry, num_cu, data_cache, tmp_path):
    assert not _broken, f"not started: {_broken[0]}"
    import exblas_amd as ex
    t0 = time.perf_counter()
    env = G.geometries(num_cu)[geometry]
    entries, _ = G.build_plan(num_cu, geometry)
    length = G.plan_length(entries)
    if "data" not in data_cache or data_cache["data"].length < length:
        data_cache["data"] = G.Data(max(length, data_cache["data"].length if "data" in data_cache else 0))
    data = data_cache["data"]
    arrays = {"plan": np.array(G.plan_json(entries))}
    for fam, name in ((G.NARROW, "narrow"), (G.WIDE, "wide")):
        arrays[name + "_x"], arrays[name + "_y"] = data.fam[fam].x[:length], data.fam[fam].y[:length]
    tuning = (1, 5, (num_cu + 3) * G.TILE + 5) if geometry == "default" else None
    if tuning:
        arrays["tuning"] = np.array(tuning, dtype=np.int64)
    t1 = time.perf_counter()
    got = _run_child(tmp_path, env, arrays)
    rec, info, tuned_rec, tuned_info = got["rec"], got["info"], got.get("tuning_rec"), got.get("tuning_info")
    t2 = time.perf_counter()
    assert rec.shape == (len(entries), ex.OUT_WORDS) and info.shape == (len(entries), 4)

    # 1. the launches are the ones the sizes were chosen for
    wrong = []
    for i, e in enumerate(entries):
        want = G.entry_launch(num_cu, env, e) + (G.env_ngroups(env), num_cu)
        if tuple(int(v) for v in info[i]) != want:
            wrong.append((_describe(e), "reported", tuple(int(v) for v in info[i]), "model", want))
    assert not wrong, ("the library's launch geometry is not stream_geometry_cases.launch_model's: update the model", len(wrong),
                       wrong[:5])

    # 2. every record, bit for bit
    memo, bad, named = {}, [], []
    for i, e in enumerate(entries):
        want = G.expected_total(data, e, memo)
        got = exact_int_from_digits(rec[i, ex.OUT_DIGITS:ex.OUT_DIGITS + ex.NDIGITS])
        exact = float(rec[i, ex.OUT_EXACT:ex.OUT_EXACT + 1].view(np.float64)[0])
        flags = int(rec[i, ex.OUT_FLAGS])
        if got == want and exact == G.exact_double(want) and flags == 0:
            continue
        if e["kind"] == "lone":
            named.append(f"{_describe(e)} grid {int(info[i, 1])}: {G.lone_decode(got, [nm for nm, _ in e['pos']])[1]} (flags {flags:#x})")
            continue
        if info[i, 0] in (G.K_EXSUM, G.K_EXDOT):
            s = G.seams(e["n"], e["offa"] & 1 if e["routine"] == G.SUM else 0, int(info[i, 1]))
            where = f"tiles {s['ntiles']} {sorted(s['tile_counts'])} each, remainder {s['rem']} in {s['rem_strides']} strides, " \
                    f"head {s['head']}, tail {s['tail']}"
        else:
            where = str(G.seams_strided(e["n"], int(info[i, 1])))
        bad.append(f"{_describe(e)} grid {int(info[i, 1])}: {where}; exact {exact!r}, want {G.exact_double(want)!r}, "
                   f"digits {'equal' if got == want else 'differ'}, flags {flags:#x}")
    t3 = time.perf_counter()
    print(f"{geometry}: {len(entries)} entries, num_cu {num_cu}; build {t1 - t0:.2f} s, child {t2 - t1:.2f} s, check {t3 - t2:.2f} s")
    report = "\n".join([f"{geometry}: {len(named)} lone-element cases and {len(bad)} other records are wrong"] + named[:12] + bad[:12])
    assert not named and not bad, report

    if tuning:      # exblas_set_tuning (exercised once, not relied on) reports through the same words
        tuned = dict(EXBLAS_BPC_SUM=str(tuning[0]), EXBLAS_NGROUPS=str(tuning[1]))
        want = G.launch_model(num_cu, tuned, G.SUM, tuning[2]) + (tuning[1], num_cu)
        assert tuple(int(v) for v in tuned_info) == want, (tuned_info, want)
        digits = exact_int_from_digits(tuned_rec[ex.OUT_DIGITS:ex.OUT_DIGITS + ex.NDIGITS])
        assert digits == data.total(G.SUM, G.NARROW, 0, tuning[2]), "the ExSUM after exblas_set_tuning is not the exact total"
