"""Context handles (exblas_ctx_create / *_ctx): private accumulators, flags and workspace per handle.

The reference's GPU launchers keep kernels and buffers in file-static globals (src/gpu/blas/blas1/ExSUM.Launcher.cpp:16-36)
-- one call at a time per process.  The *_dev layer shares one accumulator set and one workspace per device (work must be
ordered on the device); handles remove that constraint.  Parity is unchanged: every result here is compared bit for bit
with the default-context call, which tests/test_gpu_blas1.py and test_gpu_blas23.py pin to the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ex():
    import exblas_amd
    return exblas_amd


def _bits(t):
    return t.cpu().numpy().view(np.int64)


def test_interleaved_accumulations_merge_on_the_default_context_and_not_on_handles(ex):
    """The documented behaviour of the shared accumulators, and its cure: accumulate(x1), accumulate(y), accumulate(x2),
    finish on the default context is ONE exact sum over x1, y, x2 (several arrays folded into one reduction -- by
    design); on two handles the same interleaving yields sum(x1, x2) and sum(y), each equal to its stand-alone call."""
    import torch
    n = (1 << 20) + 5
    x1 = ex.gen_dev("ill_cond", n, 1, 1e32)
    x2 = ex.gen_dev("lognormal", n, 2, 0.0, 2.0)
    y = ex.gen_dev("fpuniform_signed", n, 3, 40, 20)
    # default context: everything between two finishes is one reduction
    ex.exsum_accumulate_dev(x1)
    ex.exsum_accumulate_dev(y)
    ex.exsum_accumulate_dev(x2)
    merged = ex.read_record(ex.finish_dev())
    whole = ex.read_record(ex.exsum_dev(torch.cat([x1, y, x2])))
    assert merged.exact == whole.exact and (merged.canon == whole.canon).all()
    # handles: independent
    ca, cb = ex.Context(), ex.Context()
    ca.exsum_accumulate(x1)
    cb.exsum_accumulate(y)
    ca.exsum_accumulate(x2)
    ra, rb = ex.read_record(ca.finish()), ex.read_record(cb.finish())
    wa = ex.read_record(ex.exsum_dev(torch.cat([x1, x2])))
    wb = ex.read_record(ex.exsum_dev(y))
    assert ra.exact == wa.exact and (ra.canon == wa.canon).all()
    assert rb.exact == wb.exact and (rb.canon == wb.canon).all()
    # the handles left the default context's accumulators untouched (still zero between calls)
    again = ex.read_record(ex.exsum_dev(y))
    assert again.exact == wb.exact and (again.canon == wb.canon).all()
    ca.destroy()
    cb.destroy()


def test_two_streams_two_handles_run_concurrently(ex):
    """ExSUM / ExDOT on one stream and ExGEMM / ExGEMV / ExTRSV on another, each through its own handle, enqueued
    back to back with no ordering between the streams: every result equals the serial default-context result."""
    import torch
    lib = ex.load_library()
    nsum = (1 << 24) + 7
    xs = [ex.gen_dev("ill_cond", nsum, 11 + i, 1e32) for i in range(3)]
    ys = [ex.gen_dev("lognormal", nsum, 21 + i, 0.0, 2.0) for i in range(3)]
    m, n, k = 1000, 700, 900
    A = ex.gen_dev("fpuniform_signed", m * k, 31, 12, 6)
    B = ex.gen_dev("fpuniform_signed", k * n, 32, 12, 6)
    C0 = ex.gen_dev("fpuniform_signed", m * n, 33, 10, 5)
    gm, gn = 3000, 2000
    GA = ex.gen_dev("fpuniform_signed", gm * gn, 34, 20, 10)
    gx = ex.gen_dev("fpuniform_signed", gn, 35, 20, 10)
    gy0 = ex.gen_dev("fpuniform_signed", gm, 36, 20, 10)
    tn = 700
    TA = ex.gen_dev("fpuniform", tn * tn, 37, 1.0, 0.0)
    TA.view(tn, tn).diagonal().copy_(ex.gen_dev("fpuniform", tn, 38, 1.0, 12.0))
    tb = ex.gen_dev("fpuniform_signed", tn, 39, 10, 0)
    # serial reference results on the default context
    want_sum = [ex.read_record(ex.exsum_dev(x)) for x in xs]
    want_dot = [ex.read_record(ex.exdot_dev(x, y)) for x, y in zip(xs, ys)]
    want_c = C0.clone()
    ex.exgemm_dev("N", "N", m, n, k, 1.0, A, k, B, n, 1.0, want_c, n, 8, True)
    want_y = gy0.clone()
    ex.exgemv_dev("N", gm, gn, 1.0, GA, gm, gx, 1.0, want_y, 8, True)
    want_t = tb.clone()
    ex.extrsv_dev("L", "N", "N", tn, TA, tn, want_t, 8, True)
    torch.cuda.synchronize()

    c1, c2 = ex.Context(), ex.Context()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    rounds = 6
    recs_sum = [[ex.new_record_buffer() for _ in xs] for _ in range(rounds)]
    recs_dot = [[ex.new_record_buffer() for _ in xs] for _ in range(rounds)]
    outs_c = [C0.clone() for _ in range(rounds)]
    outs_y = [gy0.clone() for _ in range(rounds)]
    outs_t = [tb.clone() for _ in range(rounds)]
    torch.cuda.synchronize()
    for r in range(rounds):
        with torch.cuda.stream(s1):
            for i, (x, y) in enumerate(zip(xs, ys)):
                c1.exsum(x, 8, True, out=recs_sum[r][i])
                c1.exdot(x, y, 8, True, out=recs_dot[r][i])
        with torch.cuda.stream(s2):
            c2.exgemm("N", "N", m, n, k, 1.0, A, k, B, n, 1.0, outs_c[r], n, 8, True)
            c2.exgemv("N", gm, gn, 1.0, GA, gm, gx, 1.0, outs_y[r], 8, True)
            c2.extrsv("L", "N", "N", tn, TA, tn, outs_t[r], 8, True)
    torch.cuda.synchronize()
    for r in range(rounds):
        for i in range(len(xs)):
            for got, want in ((ex.read_record(recs_sum[r][i]), want_sum[i]), (ex.read_record(recs_dot[r][i]), want_dot[i])):
                assert got.exact == want.exact and got.refmode == want.refmode and (got.canon == want.canon).all(), (r, i)
        assert (_bits(outs_c[r]) == _bits(want_c)).all(), r
        assert (_bits(outs_y[r]) == _bits(want_y)).all(), r
        assert (_bits(outs_t[r]) == _bits(want_t)).all(), r
    # each handle grew its OWN workspace; the default context's is what the serial calls left
    assert c2.workspace_bytes() > 0 and c1.workspace_bytes() == 0
    import ctypes as C
    info = (C.c_int * 8)()
    c2.exgemm("N", "N", m, n, k, 1.0, A, k, B, n, 1.0, outs_c[0], n, 8, True)   # (the info block lives in the workspace: valid
    assert lib.exblas_last_gemm_info_ctx(c2.handle, info) == 0 and info[0] == 4  #  until the handle's next gemv / trsv)
    c1.destroy()
    c2.destroy()


def test_handle_lifecycle(ex):
    """create / use / destroy repeatedly; NULL handle = the default context; knobs are inherited at creation"""
    import ctypes as C
    import torch
    lib = ex.load_library()
    x = ex.gen_dev("ill_cond", 100003, 5, 1e32)
    want = ex.read_record(ex.exsum_dev(x, 4, False))
    for _ in range(5):
        c = ex.Context()
        got = ex.read_record(c.exsum(x, 4, False))
        assert got.exact == want.exact and (got.canon == want.canon).all()
        c.destroy()
        c.destroy()                                    # idempotent
    rec = ex.new_record_buffer()
    rc = lib.exblas_exsum_ctx(None, C.c_void_p(x.data_ptr()), x.numel(), 1, 4, 0,
                              C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(rec.data_ptr()))
    assert rc == 0
    got = ex.read_record(rec)
    assert got.exact == want.exact and (got.canon == want.canon).all()
    # gemm path knob set before creation is what the handle uses
    m = n = k = 96
    A, B = ex.gen_dev("fpuniform", m * k, 6, 10, 0), ex.gen_dev("fpuniform", k * n, 7, 10, 0)
    try:
        lib.exblas_set_gemm_path(1)                    # scalar kernel only
        c = ex.Context()
        Cm = torch.zeros(m * n, dtype=torch.float64, device="cuda")
        c.exgemm("N", "N", m, n, k, 1.0, A, k, B, n, 0.0, Cm, n, 8, True)
        info = (C.c_int * 8)()
        assert lib.exblas_last_gemm_info_ctx(c.handle, info) == 0 and info[0] == 0
        c.destroy()
    finally:
        lib.exblas_set_gemm_path(0)


def test_launch_events_bracket_the_streaming_kernel(ex):
    """exblas_set_launch_events: the next accumulate call attaches the events to its kernel's dispatch packet -- they
    complete with the kernel, measure a plausible duration, are consumed by ONE launch, and the result is unchanged."""
    import torch
    n = (1 << 24) + 3
    x = ex.gen_dev("ill_cond", n, 3, 1e32)
    y = ex.gen_dev("lognormal", n, 4, 0.0, 2.0)
    want_s = ex.read_record(ex.exsum_dev(x, 8, True))
    want_d = ex.read_record(ex.exdot_dev(x, y, 8, True))
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); e1.record()                       # (a torch event gets its handle at its first record())
    torch.cuda.synchronize()
    for op in ("sum", "dot"):
        ex.set_launch_events(e0, e1)
        if op == "sum":
            ex.exsum_accumulate_dev(x, 8, True)
        else:
            ex.exdot_accumulate_dev(x, y, 8, True)
        got = ex.read_record(ex.finish_dev())
        torch.cuda.synchronize()
        want = want_s if op == "sum" else want_d
        assert got.exact == want.exact and (got.canon == want.canon).all()
        ms = e0.elapsed_time(e1)
        bytes_ = n * (8 if op == "sum" else 16)
        assert 0.0 < ms < 5.0 and bytes_ / (ms * 1e-3) < 8.5e12, (op, ms)      # a kernel time, below the HBM peak
        # consumed: a second launch without events does not move them
        t_before = e0.elapsed_time(e1)
        ex.exsum_accumulate_dev(x, 8, True)
        ex.finish_dev()
        torch.cuda.synchronize()
        assert e0.elapsed_time(e1) == t_before


def _words(ex, rec):
    return ex.read_record(rec).words


def test_handle_equals_default_on_strides_counts_and_accumulate(ex):
    """The arguments the handle methods lacked before they became the one implementation: a stride, both strides with an
    explicit count, and exdot_accumulate.  A handle and the default context give the same record, all 128 words."""
    import torch
    n = 100003
    x = ex.gen_dev("ill_cond", 3 * n, 41, 1e32)
    y = ex.gen_dev("fpuniform_signed", 3 * n, 42, 40, 20)
    c = ex.Context()
    try:
        assert (_words(ex, c.exsum(x, 4, False, inca=3)) == _words(ex, ex.exsum_dev(x, 4, False, inca=3))).all()
        got = _words(ex, c.exdot(x, y, 8, True, incx=2, incy=3, n=n))
        assert (got == _words(ex, ex.exdot_dev(x, y, 8, True, incx=2, incy=3, n=n))).all()
        x1, x2, y1, y2 = x[:n], x[n:2 * n + 1], y[:n], y[n:2 * n + 1]
        c.exdot_accumulate(x1, y1)
        c.exdot_accumulate(x2, y2)
        got = _words(ex, c.finish())
        assert (got == _words(ex, ex.exdot_dev(torch.cat([x1, x2]), torch.cat([y1, y2])))).all()
    finally:
        c.destroy()


def _bidiagonal(m):
    """lower bidiagonal, dominant diagonal, as (row_ptr, col_idx, val, (m, m)) numpy arrays"""
    crow = np.concatenate([[0], 2 * np.arange(1, m + 1) - 1]).astype(np.int32)
    col = np.concatenate([[0]] + [[i - 1, i] for i in range(1, m)]).astype(np.int32)
    val = np.concatenate([[4.0]] + [[0.5 + i / 256.0, 4.0 + i / 64.0] for i in range(1, m)])
    return crow, col, val, (m, m)


_KNOBS_CHILD = """
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
import exblas_amd as ex
lib = ex.load_library()
ex.set_spmv_path(1); ex.set_spmm_path(1); ex.set_sptrsv_path(1); ex.set_sptrsm_path(1)
lib.exblas_set_gemm_path(1)
m, k = 70, 3
A = _bidiagonal(m)
b = 1.0 + np.arange(m) / 128.0
B = np.stack([b, -b, 3.0 * b], axis=1)
out = {}
ex.exspmv(A, b); out["spmv"] = ex.last_spmv_info()
ex.exspmm(A, B); out["spmm"] = ex.last_spmm_info()
ex.exsptrsv(A, b); out["sptrsv"] = ex.last_sptrsv_info()
ex.exsptrsm(A, B); out["sptrsm"] = ex.last_sptrsm_info()
c = ex.Context()
n = 96
P, Q = ex.gen_dev("fpuniform", n * n, 6, 10, 0), ex.gen_dev("fpuniform", n * n, 7, 10, 0)
R = torch.zeros(n * n, dtype=torch.float64, device="cuda")
c.exgemm("N", "N", n, n, n, 1.0, P, n, Q, n, 0.0, R, n, 8, True)
info = (C.c_int * 8)()
out["gemm_rc"] = lib.exblas_last_gemm_info_ctx(c.handle, info)
out["gemm"] = list(info)
c.destroy()
print("RESULT " + json.dumps(out))
"""


def test_knobs_set_before_a_layer_exists_reach_it():
    """The path knobs are set when only the default context exists; the host-array calls then create the host layer's
    context and a handle is created after that.  Both must take the knobs: every row / output rounded from its
    accumulator, the scalar ExGEMM kernel.  A fresh process, so that the layers do not exist yet."""
    import inspect
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", inspect.getsource(_bidiagonal) + _KNOBS_CHILD, root], capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.split("RESULT ", 1)[1])
    m, k = 70, 3
    for name, units in (("spmv", m), ("spmm", m * k), ("sptrsv", m), ("sptrsm", m * k)):
        assert out[name][0] == 0 and out[name][1] == units, (name, out)
    assert out["gemm_rc"] == 0 and out["gemm"][0] == 0, out


def test_release_workspace_forgets_every_pointer_into_it(ex):
    """After exblas_release_workspace no last_*_info query may follow a pointer into the freed block: ExSpMV / ExSpMM
    answer "no call", the solves and ExGEMM answer zeros; the next call works as before."""
    import ctypes as C
    import torch
    lib = ex.load_library()
    m, k = 70, 3
    crow, col, val, shape = _bidiagonal(m)
    A = (torch.from_numpy(crow).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(val).cuda(), shape)
    b = torch.from_numpy(1.0 + np.arange(m) / 128.0).cuda()
    B = torch.stack([b, -b, 3.0 * b], dim=1).contiguous()
    before = _bits(ex.exspmv_dev(A, b))
    ex.exspmm_dev(A, B)
    ex.exsptrsv_dev(A, b.clone())
    ex.exsptrsm_dev(A, B.clone())
    gm, gk, gn = 130, 200, 75           # the int8-path shape of smoke(): its info block lives in the workspace
    P, Q = ex.gen_dev("fpuniform", gm * gk, 3, 10, 0), ex.gen_dev("fpuniform", gk * gn, 4, 10, 0)
    ex.exgemm_dev("N", "N", gm, gn, gk, 1.0, P, gk, Q, gn, 0.0, torch.zeros(gm * gn, dtype=torch.float64, device="cuda"),
                  gn, 8, True)
    assert lib.exblas_release_workspace() == 0
    out4 = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.exblas_last_spmv_info(out4) == -1
    assert lib.exblas_last_spmm_info(out4) == -1
    for query in (lib.exblas_last_sptrsv_info, lib.exblas_last_sptrsm_info):
        out4 = (C.c_int64 * 4)(7, 7, 7, 7)
        assert query(out4) == 0 and list(out4) == [0, 0, 0, 0]
    info = (C.c_int * 8)(7, 7, 7, 7, 7, 7, 7, 7)
    assert lib.exblas_last_gemm_info(info) == 0 and info[0] == 0
    assert (_bits(ex.exspmv_dev(A, b)) == before).all()


def test_release_workspace_forgets_the_block_routines_counter_slots(ex):
    """The same for the routines whose last_*_info follows a pointer AND a count into the workspace (ExBGEMM, ExBTRSM,
    ExPOTRF: a pair of counters per workgroup) and for ExTRSM's header: after exblas_release_workspace each query writes
    zeros and returns 0, and the next call of each routine gives the bits it gave before."""
    import ctypes as C
    import torch
    lib = ex.load_library()
    n, p = 70, 3
    r = np.arange(n, dtype=np.float64)
    X0 = torch.from_numpy(1.0 + np.outer(r, [1.0, -2.0, 3.0]) / 128.0 + np.outer(r % 7, [0.5, 0.25, -0.125])).cuda()
    A = torch.from_numpy(np.tril(1.0 / (1.0 + np.abs(r[:, None] - r[None, :]))) + 2.0 * np.eye(n)).cuda()
    Cm = torch.tensor([[1.0, 0.5, -0.25], [0.0, 2.0, 0.75], [3.0, -1.0, 1.5]], dtype=torch.float64, device="cuda")
    M = np.array([[2.0, 0.5, -0.25], [0.0, 1.5, 0.75], [0.0, 0.0, 1.25]])
    G0 = torch.from_numpy(M.T @ M).cuda()               # well conditioned: the Gram matrix of a 3 x 3 triangle
    T = torch.from_numpy(M).cuda()

    def calls():
        G, info = ex.expotrf_dev(G0.clone(), "U")
        return [_bits(ex.extrsm_dev(A, X0.clone(), "L", "N", "N")), _bits(ex.exbgemm_dev(X0, Cm, 0.5, 2.0, X0.clone())),
                _bits(ex.exbtrsm_dev(T, X0.clone(), "U", "N", "N")), _bits(G), info.cpu().numpy()]

    before = calls()
    assert before[4][0] == 0
    assert lib.exblas_release_workspace() == 0
    for query in (lib.exblas_last_trsm_info, lib.exblas_last_bgemm_info, lib.exblas_last_btrsm_info,
                  lib.exblas_last_potrf_info):
        out4 = (C.c_int64 * 4)(7, 7, 7, 7)
        assert query(out4) == 0 and list(out4) == [0, 0, 0, 0]
    for was, now in zip(before, calls()):
        assert (was == now).all()
