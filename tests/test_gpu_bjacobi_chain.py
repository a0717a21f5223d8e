"""GPU suite for the block-Jacobi chain: csr_diag_blocks_dev, the batched ExPOTRF, the batched ExPOTRS on a small SPD CSR
matrix (the 2-D five-point Laplacian on 24 x 24 with a full-mantissa perturbation of the diagonal), against the chain of
the Fraction models; identical across paths and contexts; captured into one graph on one stream and replayed on new data."""
import functools

import numpy as np
import pytest

import bjacobi_cases as J

pytestmark = pytest.mark.gpu

M, K = 24, 3
PS = (8, 7)                                      # 576 = 72 * 8 = 82 * 7 + 2


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_potrf_batched_path(0)
    exblas_amd.set_potrs_batched_path(0)


@functools.lru_cache(maxsize=None)
def _system(seed, p):
    """(A dense, X0, the model's R and X) of one data set"""
    A = J.laplacian(M, seed)
    X0 = (np.random.default_rng([seed, 80]).random((M * M, K)) - 0.5) * 8
    R, X = J.chain_model(A, p, X0)
    return A, X0, R, X


def _csr(A, itype):
    import torch
    sp = torch.from_numpy(A).to_sparse_csr()
    return (sp.crow_indices().to(itype).cuda(), sp.col_indices().to(itype).cuda(), sp.values().cuda(), tuple(A.shape))


def _same(got, want, mask, what):
    J.same_bits(np.asarray(got), want, mask, what)


@pytest.mark.parametrize("p", PS)
def test_chain_equals_the_model_chain_on_every_path_and_context(ex, p):
    import torch
    A, X0, R, X = _system(0, p)
    n = A.shape[0]
    up = J.tri_mask(p, "U")
    ctx = ex.Context()
    try:
        for path in (0, 1, 2, 3):
            ex.set_potrf_batched_path(path)
            ex.set_potrs_batched_path(path)
            for who, factor, apply in (("default", ex.expotrf_batched_dev, ex.expotrs_batched_dev),
                                       ("private", ctx.expotrf_batched, ctx.expotrs_batched)):
                D = ex.csr_diag_blocks_dev(_csr(A, torch.int32 if path % 2 else torch.int64), p)
                assert D.is_cuda and tuple(D.shape) == (-(-n // p), p, p)
                assert (D.cpu().numpy() == J.diag_blocks(A, p)).all()
                Rd, info = factor(D, "U")
                assert Rd is D and int(info.abs().max().item()) == 0
                _same(D.cpu().numpy(), R, up, ("factor", p, path, who))
                assert (D.cpu().numpy()[:, ~up] == J.diag_blocks(A, p)[:, ~up]).all()
                Xd = torch.from_numpy(X0).cuda()
                assert apply(D, Xd) is Xd
                _same(Xd.cpu().numpy(), X, np.ones_like(X, dtype=bool), ("apply", p, path, who))
        assert np.allclose(X, np.linalg.solve(_blockdiag(A, p), X0), rtol=1e-10)
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
        ex.set_potrf_batched_path(0)
        ex.set_potrs_batched_path(0)


def _blockdiag(A, p):
    n = A.shape[0]
    Mb = np.zeros_like(A)
    for b in range(-(-n // p)):
        s = slice(b * p, min(n, (b + 1) * p))
        Mb[s, s] = A[s, s]
    return Mb


def test_each_call_is_one_kernel_node_and_no_memset_node(ex):
    """the census of DESIGN 5c-2, with the counting helpers of test_gpu_graph_replay"""
    import torch
    from test_gpu_graph_replay import _count_nodes, _hip_runtime
    hip = _hip_runtime()
    A, X0, _, _ = _system(0, 8)
    D0 = torch.from_numpy(J.diag_blocks(A, 8)).cuda()
    D, Xd = D0.clone(), torch.from_numpy(X0).cuda()
    info = torch.zeros(D.shape[0], dtype=torch.int32, device="cuda")
    ex.expotrf_batched_dev(D0, "U", info)
    calls = {"expotrf_batched_dev": lambda: ex.expotrf_batched_dev(D, "U", info),
             "expotrs_batched_dev": lambda: ex.expotrs_batched_dev(D0, Xd),
             "expotrs_batched_dev, one sweep": lambda: ex.expotrs_batched_dev(D0, Xd, "U", "1")}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        for name, fn in calls.items():
            fn()                                   # the warm call: the workspace and the dynamic-LDS limit
            s.synchronize()
            assert _count_nodes(hip, s, fn) == {"kernel": 1}, name
            s.synchronize()
    torch.cuda.synchronize()


@pytest.mark.parametrize("p", PS)
def test_factor_and_apply_captured_into_one_graph_replay_on_new_data(ex, p):
    """one stream, no parallel branches: restore the blocks and X, factor, apply; two replays on data sets the capture
    never saw, info words and bits read after each"""
    import torch
    A, X0, R, X = _system(0, p)
    nb = R.shape[0]
    dsrc = torch.from_numpy(J.diag_blocks(A, p)).cuda()
    xsrc = torch.from_numpy(X0).cuda()
    D, Xd = torch.empty_like(dsrc), torch.empty_like(xsrc)
    info = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    D.copy_(dsrc)
    Xd.copy_(xsrc)
    ex.expotrf_batched_dev(D, "U", info)                            # one warm call each
    ex.expotrs_batched_dev(D, Xd)
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            D.copy_(dsrc)
            Xd.copy_(xsrc)
            ex.expotrf_batched_dev(D, "U", info)
            ex.expotrs_batched_dev(D, Xd)
    up = J.tri_mask(p, "U")
    for seed in (1, 2):
        A2, X2, R2, W2 = _system(seed, p)
        dsrc.copy_(torch.from_numpy(J.diag_blocks(A2, p)))
        xsrc.copy_(torch.from_numpy(X2))
        info.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(info.abs().max().item()) == 0
        _same(D.cpu().numpy(), R2, up, ("replayed factor", p, seed))
        _same(Xd.cpu().numpy(), W2, np.ones_like(W2, dtype=bool), ("replayed apply", p, seed))
        assert (R2[:, up].view(np.int64) != R[:, up].view(np.int64)).any()
        scnt = ex.last_potrs_batched_info()                         # the last call of the graph: its slots are the live ones
        assert scnt[0] + scnt[1] == 2 * A.shape[0] * K
    del g
