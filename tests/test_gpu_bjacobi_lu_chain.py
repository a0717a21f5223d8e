"""GPU suite for the block-Jacobi chain with general blocks: csr_diag_blocks_dev, the batched ExGETRF, the batched ExGETRS
on a small nonsymmetric CSR matrix (the five-point upwind convection-diffusion operator with full-mantissa coefficients),
against the chain of the exact models; identical across paths and contexts; captured into one graph on one stream and
replayed on new data."""
import functools

import numpy as np
import pytest

import bjacobi_cases as J
import getrf_cases as G

pytestmark = pytest.mark.gpu

M, K = 31, 3                                     # 961 = 240 * 4 + 1 = 137 * 7 + 2 = 60 * 16 + 1: a short last block each
MG = 15                                          # the replayed graphs: 225 = 56 * 4 + 1 = 32 * 7 + 1 = 14 * 16 + 1
PS = (4, 7, 16)


@pytest.fixture(scope="module")
def ex():
    import torch
    import exblas_amd
    assert torch.cuda.is_available()
    exblas_amd.load_library().exblas_hip_init(-1)
    yield exblas_amd
    exblas_amd.set_getrf_batched_path(0)
    exblas_amd.set_getrs_batched_path(0)


@functools.lru_cache(maxsize=None)
def _system(m, seed, p):
    """(A dense, X0, the model's W, ipiv and X) of one data set"""
    A = G.convection_diffusion(m, seed)
    X0 = (np.random.default_rng([seed, 96]).random((m * m, K)) - 0.5) * 8
    W, ipiv, X = G.chain_model(A, p, X0)
    return A, X0, W, ipiv, X


def _csr(A, itype):
    import torch
    sp = torch.from_numpy(A).to_sparse_csr()
    return (sp.crow_indices().to(itype).cuda(), sp.col_indices().to(itype).cuda(), sp.values().cuda(), tuple(A.shape))


def _same(got, want, what):
    J.same_bits(np.asarray(got), want, np.ones_like(want, dtype=bool), what)


def _blockdiag(A, p):
    n = A.shape[0]
    Mb = np.zeros_like(A)
    for b in range(-(-n // p)):
        s = slice(b * p, min(n, (b + 1) * p))
        Mb[s, s] = A[s, s]
    return Mb


@pytest.mark.parametrize("p", PS)
def test_chain_equals_the_model_chain_on_every_path_and_context(ex, p):
    import torch
    A, X0, W, ipiv, X = _system(M, 0, p)
    n = A.shape[0]
    assert (A != A.T).any() and n % p != 0
    ctx = ex.Context()
    try:
        for path in (0, 1, 2, 3):
            ex.set_getrf_batched_path(path)
            ex.set_getrs_batched_path(path)
            for who, factor, apply in (("default", ex.exgetrf_batched_dev, ex.exgetrs_batched_dev),
                                       ("private", ctx.exgetrf_batched, ctx.exgetrs_batched)):
                D = ex.csr_diag_blocks_dev(_csr(A, torch.int32 if path % 2 else torch.int64), p)
                assert D.is_cuda and tuple(D.shape) == (-(-n // p), p, p)
                assert (D.cpu().numpy() == J.diag_blocks(A, p)).all()
                LU, piv, info = factor(D)
                assert LU is D and int(info.abs().max().item()) == 0
                _same(D.cpu().numpy(), W, ("factor", p, path, who))
                assert (piv.cpu().numpy() == ipiv).all()
                Xd = torch.from_numpy(X0).cuda()
                assert apply(D, piv, Xd) is Xd
                _same(Xd.cpu().numpy(), X, ("apply", p, path, who))
        assert np.allclose(X, np.linalg.solve(_blockdiag(A, p), X0), rtol=1e-9)
    finally:
        torch.cuda.synchronize()
        ctx.destroy()
        ex.set_getrf_batched_path(0)
        ex.set_getrs_batched_path(0)


def test_each_call_is_one_kernel_node_and_no_memset_node(ex):
    """the census of DESIGN 5c-2, with the counting helpers of test_gpu_graph_replay"""
    import torch
    from test_gpu_graph_replay import _count_nodes, _hip_runtime
    hip = _hip_runtime()
    A, X0, _, _, _ = _system(MG, 0, 7)
    D0 = torch.from_numpy(J.diag_blocks(A, 7)).cuda()
    D, Xd = D0.clone(), torch.from_numpy(X0).cuda()
    info = torch.zeros(D.shape[0], dtype=torch.int32, device="cuda")
    piv = torch.zeros((D.shape[0], 7), dtype=torch.int32, device="cuda")
    piv2 = torch.zeros_like(piv)
    ex.exgetrf_batched_dev(D0, piv, info)
    calls = {"exgetrf_batched_dev": lambda: ex.exgetrf_batched_dev(D, piv2, info),
             "exgetrs_batched_dev": lambda: ex.exgetrs_batched_dev(D0, piv, Xd)}
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
    never saw, pivots, info words and bits read after each"""
    import torch
    A, X0, W, ipiv, X = _system(MG, 0, p)
    nb = W.shape[0]
    dsrc = torch.from_numpy(J.diag_blocks(A, p)).cuda()
    xsrc = torch.from_numpy(X0).cuda()
    D, Xd = torch.empty_like(dsrc), torch.empty_like(xsrc)
    info = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    piv = torch.full((nb, p), -1, dtype=torch.int32, device="cuda")
    D.copy_(dsrc)
    Xd.copy_(xsrc)
    ex.exgetrf_batched_dev(D, piv, info)                            # one warm call each
    ex.exgetrs_batched_dev(D, piv, Xd)
    torch.cuda.synchronize()
    s, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            D.copy_(dsrc)
            Xd.copy_(xsrc)
            ex.exgetrf_batched_dev(D, piv, info)
            ex.exgetrs_batched_dev(D, piv, Xd)
    for seed in (1, 2):
        A2, X2, W2, ipiv2, Z2 = _system(MG, seed, p)
        dsrc.copy_(torch.from_numpy(J.diag_blocks(A2, p)))
        xsrc.copy_(torch.from_numpy(X2))
        info.fill_(-1)
        piv.fill_(-1)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert int(info.abs().max().item()) == 0 and (piv.cpu().numpy() == ipiv2).all()
        _same(D.cpu().numpy(), W2, ("replayed factor", p, seed))
        _same(Xd.cpu().numpy(), Z2, ("replayed apply", p, seed))
        assert (W2.view(np.int64) != W.view(np.int64)).any()
        scnt = ex.last_getrs_batched_info()                         # the last call of the graph: its slots are the live ones
        assert scnt[0] + scnt[1] == 2 * A.shape[0] * K
    del g
