"""CPU suite: the C-ABI library builds for gfx950, loads, and exports every symbol the headers declare."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import exblas_amd
    return exblas_amd.load_library()


def _declared_c_symbols():
    txt = open(os.path.join(ROOT, "include", "exblas_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(exblas_[a-z0-9_]+)\s*\(", txt)))


def test_c_abi_symbols_exported(lib):
    import exblas_amd
    declared = _declared_c_symbols()
    assert len(declared) >= 18
    assert sorted(exblas_amd.C_ABI_SYMBOLS) == declared
    for name in declared:
        assert hasattr(lib, name), name


def test_last_blas1_info_is_declared_exported_and_wrapped(lib):
    """exblas_last_blas1_info (the launch report the stream-geometry tests rest on): in the header, in the symbol list, in
    the library with its argument type, behind a Python wrapper; a NULL pointer is refused before any device is touched."""
    import exblas_amd
    assert "exblas_last_blas1_info" in _declared_c_symbols() and "exblas_last_blas1_info" in exblas_amd.C_ABI_SYMBOLS
    assert lib.exblas_last_blas1_info.argtypes == [ctypes.POINTER(ctypes.c_int)]
    assert callable(exblas_amd.last_blas1_info)
    assert lib.exblas_last_blas1_info(None) == 1       # hipErrorInvalidValue


def test_cxx_api_symbols_exported():
    """exsum/exdot/exgemv/extrsv/exgemm with the reference's C++ signatures (blas1.hpp:48,74; blas2.hpp:57,95; blas3.hpp:56)."""
    import exblas_amd
    out = subprocess.run(["nm", "-D", "--defined-only", "-C", exblas_amd.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for sig in ("exsum(int, double*, int, int, int, bool, bool)",
                "exdot(int, double*, int, int, double*, int, int, int, bool)",
                "exgemv(char, int, int, double, double*, int, int, double*, int, int, double, double*, int, int, int, bool)",
                "extrsv(char, char, char, int, double*, int, int, double*, int, int, int, bool)",
                "exgemm(char, char, int, int, int, double, double*, int, double*, int, double, double*, int, int, bool)",
                "init_ill_cond(int, double*, double)", "init_naive(int, double*)",
                "init_fpuniform(int, double*, int, int)", "init_lognormal(int, double*, double, double)"):
        assert sig in out, sig


def test_library_contains_gfx950_code_object():
    import exblas_amd
    data = open(exblas_amd.LIB_PATH, "rb").read()
    assert b"gfx950" in data


def test_no_gpu_means_loud_failure(lib):
    """Without a HIP device the product refuses to compute (no CPU fallback)."""
    import torch
    import exblas_amd
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert lib.exblas_hip_device_count() == 0
    with pytest.raises(RuntimeError):
        exblas_amd.exsum(4, [1.0, 2.0, 3.0, 4.0], 1, 0, 0)


def test_set_tuning_refuses_a_kernel_variant():
    """The library builds one kernel per configuration: exblas_set_tuning's third argument accepts only -1 and 0, and any
    other value is refused with hipErrorInvalidValue before the device is touched.  A fresh child process: without a
    device, any path that reaches the context ends the process."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import exblas_amd; "
            "print('ret', exblas_amd.load_library().exblas_set_tuning(-1, -1, 5))")
    r = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("ret 1"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_dev_functions_are_the_default_contexts_methods():
    """Every routine with a handle form has one Python body, a Context method; the module's *_dev function is that method
    bound to the context without a handle (the device's default context).  Importing and looking creates no context."""
    import inspect
    import exblas_amd
    names = ["exsum", "exdot", "exsum_accumulate", "exdot_accumulate", "finish", "exgemv", "extrsv", "exgemm", "exspmv",
             "exspmm", "exsptrsv", "exsptrsm", "exbdot", "exbdot_export", "exbdot_round"]
    owners = set()
    for name in names:
        f = getattr(exblas_amd, name + "_dev")
        assert inspect.ismethod(f) and f.__func__ is getattr(exblas_amd.Context, name), name
        assert isinstance(f.__self__, exblas_amd.Context) and f.__self__.handle is None, name
        params = list(inspect.signature(getattr(exblas_amd.Context, name)).parameters.values())
        assert params[0].name == "self" and inspect.signature(f) == inspect.Signature(params[1:]), name
        owners.add(id(f.__self__))
    assert len(owners) == 1
    f.__self__.destroy()            # nothing to destroy
    assert f.__self__.handle is None


def test_product_does_not_import_oracle():
    """The shipped package may mention the oracle in comments, but never import, include, link or dlopen it."""
    bad = re.compile(r"^\s*(from|import)\s+.*oracle|#\s*include\s*[\"<].*oracle|CDLL\(.*oracle|dlopen\(.*oracle", re.M)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "exblas_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, f), errors="ignore").read()
                assert not bad.search(txt), (f, "uses oracle code")


def test_residue_gemm_tables_selftest(lib):
    """The residue ExGEMM path (blas3_crt.hip) reconstructs an integer from its residues modulo up to 39 coprime 8-bit
    moduli with constant tables generated on the host.  exblas_crt_selftest runs a host mirror of the device
    arithmetic (Garner inside groups of three, classical CRT across the 24-bit super-moduli, fp64 fraction sum for the
    multiple of M) over those tables: 200 random integers |S| < M_L / 4 per modulus count L = 1..39, no GPU involved.
    The GPU parity tests (tests/test_gpu_blas23.py::test_exgemm_residue_path_*) check the kernels end to end."""
    assert lib.exblas_crt_selftest(200, 1) == 0
    assert lib.exblas_crt_selftest(50, 12345) == 0


def test_reference_test_programs_link_against_the_drop_in():
    """INTEGRATION.md's claim "no source change": the reference's own GPU test programs
    (/root/reference/tests/test.ex{sum,dot,gemv,gemm,trsv}.gpu.cpp), compiled where they lie against THIS repository's
    include/ and linked against libexblas.so by the committed recipe (oracle/Makefile: reftests).  Every public entry
    point they call must resolve to a C++ symbol our library exports.  Where the reference is absent, the symbols those
    programs import are checked from the list recorded off the compiled programs (tests/golden/reftest_symbols.json,
    make_golden.py --ref-core); the GPU box runs the prebuilt binaries (tests/test_gpu_reference_tests.py)."""
    import json
    import subprocess
    import exblas_amd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    want = {"exsum": "_Z5exsumiPdiiibb", "exdot": "_Z5exdotiPdiiS_iiib", "exgemv": "_Z6exgemvciidPdiiS_iidS_iiib",
            "exgemm": "_Z6exgemmcciiidPdiS_idS_iib", "extrsv": "_Z6extrsvccciPdiiS_iiib"}
    exported = subprocess.run(["nm", "-D", "--defined-only", exblas_amd.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in exported.splitlines() if ln.strip()}
    with open(os.path.join(root, "tests", "golden", "reftest_symbols.json")) as fh:
        recorded = json.load(fh)
    assert sorted(recorded) == sorted(want)
    for op, sym in want.items():
        assert sym in recorded[op] and any("init_" in s for s in recorded[op]), (op, recorded[op])
        missing = set(recorded[op]) - exported
        assert not missing, (op, missing)
    if not os.path.isdir("/root/reference/tests"):
        return
    exblas_amd.load_library()
    r = subprocess.run(["make", "-C", os.path.join(root, "oracle"), "reftests"], capture_output=True, text=True)
    assert r.returncode == 0 and "built _ref/reftest_" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    for op, sym in want.items():
        exe = os.path.join(root, "oracle", "_ref", f"reftest_{op}")
        assert os.path.exists(exe), exe
        und = subprocess.run(["nm", "-D", "--undefined-only", exe], capture_output=True, text=True).stdout
        und = {ln.split()[-1] for ln in und.splitlines() if ln.strip()}
        assert sym in und, (op, sorted(s for s in und if s.startswith("_Z")))
        missing = {s for s in und if s.startswith("_Z") and ("init_" in s or s == sym)} - exported
        assert not missing, (op, missing)
