"""Child process of tests/test_gpu_lowp.py::test_tuning_does_not_change_the_record: the narrow ExSUM / ExDOT of one input
under two exblas_set_tuning block counts.  The knob is process-wide, so it is turned in a process of its own."""
import sys

sys.path.insert(0, sys.argv[1])

import torch  # noqa: E402

import exblas_amd as ex  # noqa: E402

lib = ex.load_library()
lib.exblas_hip_init(-1)
same, grids = True, set()
for name, t in (("float32", 4096), ("float16", 8192), ("bfloat16", 8192)):
    g = torch.Generator(device="cuda").manual_seed(3)
    n = 4096 * t + 5
    x = (torch.randn(n, device="cuda", generator=g) * torch.exp2(torch.randint(-12, 12, (n,), device="cuda", generator=g).float())
         ).to(getattr(torch, name))
    y = torch.randn(n, device="cuda", generator=g).to(getattr(torch, name))
    recs = []
    for bpc in (2, 7):
        assert lib.exblas_set_tuning(bpc, -1, -1) == 0
        s = ex.exsum_lp_dev(x[1:])
        grids.add((name, "sum", bpc, ex.last_blas1_info()[1]))
        d = ex.exdot_lp_dev(x[1:], y[1:])
        grids.add((name, "dot", bpc, ex.last_blas1_info()[1]))
        recs.append((s.cpu(), d.cpu()))
    same = same and torch.equal(recs[0][0], recs[1][0]) and torch.equal(recs[0][1], recs[1][1])
    same = same and torch.equal(recs[0][0], ex.exsum_dev(x[1:].double()).cpu())
by = {}
for name, op, bpc, grid in grids:
    by.setdefault((name, op), set()).add(grid)
print("grids", sorted(grids))
print("same records:", same)
print("grids differ:", all(len(v) == 2 for v in by.values()))
