"""CPU: the C ABI and the binding carry hipsdp_sparsecuts / hipsdp_sparsecuts_stats with the documented signatures, the unit entry of
the large TPower kernel stays in the test library, the new HIP source is part of the build, and the numpy restatement reproduces
rows of the table of tests/harness/sparsecuts_large_cases.py, so the fixture of the GPU tests is checked where no device is needed."""
import ctypes as C
import os
import re
import importlib.util
import pytest
from conftest import ROOT
import sparsecuts_large_cases as L


def _hdr(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_sparsecuts_is_declared_and_bound():
    hdr = _hdr("hipsdp.h")
    d = r"\s*,\s*double\s*\*\s*"
    i = r"\s*,\s*int\s*\*\s*"
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+block\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*int\s+size\s*,\s*const\s+hipsdp_sparsecut_opts\s*\*\s*opts" + i + "ncuts" + d + "lmin" + d + "eigvals" + d
                     + "coefs" + d + "lhs" + d + "vecs" + i + "iters" + i + r"flags\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert re.search(r"#define\s+HIPSDP_SPARSECUTS_MAXN\s+512\b", hdr)
    units = _hdr("hipsdp_units.h")
    assert not re.search(r"hipsdp_sparsecuts(_stats)?\s*\(", units)             # product symbols: declared in hipsdp.h alone
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_large_unit\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*Z\s*,"
                     r"\s*const\s+double\s*\*\s*v0\s*,\s*double\s+maxeig\s*,\s*int\s+size\s*,\s*const\s+hipsdp_sparsecut_opts\s*\*\s*opts"
                     + i + "ncuts" + d + "eigvals" + d + "vecs" + i + "iters" + i + r"flags\s*\)", units)
    assert "hipsdp_sparsecuts_large_unit" not in hdr
    spec = importlib.util.spec_from_file_location("hipsdp_binding_scone", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.Solver.sparsecuts) and callable(mod.sparsecuts_stats) and callable(mod.Solver.sparsecuts_stats)
    assert callable(mod.sparsecuts_large_unit)
    assert C.sizeof(mod.SparsecutOpts) == 32


def test_libraries_export_what_they_should(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_sparsecuts") and hasattr(lib, "hipsdp_sparsecuts_stats")
    assert hasattr(hb.ulib(), "hipsdp_sparsecuts_large_unit") and not hasattr(lib, "hipsdp_sparsecuts_large_unit")
    assert hasattr(hb.ulib(), "hipsdp_sparsecuts") and hasattr(hb.ulib(), "hipsdp_sparsecuts_stats")
    # no device work: the totals are readable before any call, and NULL outputs are allowed
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_sparsecuts_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_sparsecuts_stats(None, None, None) == 0
    assert lib.hipsdp_sparsecuts(None, 0, None, 4, None, None, None, None, None, None, None, None, None) == 3
    opts = hb.SparsecutOpts(1e-6, 1e-6, 0.0, 5, 0)
    assert lib.hipsdp_sparsecuts(None, 0, None, 4, C.byref(opts), None, None, None, None, None, None, None, None) == 3


def test_the_large_kernels_are_built_from_their_own_source():
    with open(os.path.join(ROOT, "scip-sdp_amd", "Makefile")) as f:
        assert "csrc/sparsecuts_large.hip" in f.read()
    with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", "sparsecuts_large.hip")) as f:
        src = f.read()
    assert "__global__" in src and "k_sc_tpower_large" in src and "k_sc_coefs_large" in src and "atomicAdd" not in src
    # one workgroup: the launch of the TPower kernel has a grid of one
    assert re.search(r"hipLaunchKernelGGL\(\s*k_sc_tpower_large\s*,\s*dim3\(1\)\s*,\s*dim3\(SCL_NT\)", src)
    assert re.search(r"#define\s+SCL_NT\s+512\b", src)


@pytest.mark.parametrize("row", [1, 5])
def test_the_restatement_reproduces_rows_of_the_table(row):
    """family 4, block 1 (150 rows) at size 10 and the block of 129 rows at size 48: the cut and iteration totals the GPU tests pin"""
    name, spec, size, cuts, its = L.TABLE[row]
    r = L.reference(spec, size)                 # (asserts the margins)
    mg = r[9]
    assert (r[0], r[7], r[8]) == (cuts, its, 0)
    assert mg.select >= 3.8e-5 and mg.conv >= 2.4e-10 and mg.feas >= 1.0e-6
    A, ys, y, b = L.block(spec)
    assert A.shape[1] > 128 and r[1] < -L.TOL
    for c in range(r[0]):
        assert len(r[6][c]) == size and r[3][c] @ ys - r[4][c] >= -1e-9
