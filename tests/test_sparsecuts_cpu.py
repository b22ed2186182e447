"""CPU: the C ABI and the binding carry hipsdp_sparsecuts_all / hipsdp_sparsecuts_all_stats with the documented signatures, the unit
entry point of the TPower kernel stays in the test library, the new HIP source is part of the build, and the numpy restatement
(tests/harness/sparsecuts_ref.py) returns the hand result on a 3 x 3 example."""
import ctypes as C
import os
import re
import importlib.util
import numpy as np
from conftest import ROOT
import sparsecuts_ref as R


def _hdr(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_sparsecuts_all_is_declared_and_bound():
    hdr = _hdr("hipsdp.h")
    d = r"\s*,\s*double\s*\*\s*"
    i = r"\s*,\s*int\s*\*\s*"
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_all\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*const\s+int\s*\*\s*sizes\s*,\s*const\s+hipsdp_sparsecut_opts\s*\*\s*opts" + i + "ncuts" + d + "lmin" + d
                     + "eigvals" + d + "coefs" + d + "lhs" + d + "vecs" + i + "iters" + i + r"flags\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_all_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert re.search(r"#define\s+HIPSDP_SPARSECUTS_MAXIT\s+10000\b", hdr)
    assert re.search(r"typedef\s+struct\s+hipsdp_sparsecut_opts\s*\{[^}]*double\s+tol\s*;[^}]*double\s+feastol\s*;[^}]*double\s+convtol\s*;"
                     r"[^}]*int\s+maxcuts\s*;[^}]*int\s+maxit\s*;[^}]*\}\s*hipsdp_sparsecut_opts\s*;", hdr)
    units = _hdr("hipsdp_units.h")
    assert not re.search(r"hipsdp_sparsecuts_all(_stats)?\s*\(", units)         # product symbols: declared in hipsdp.h alone
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_unit\s*\(", units) and "hipsdp_sparsecuts_unit" not in hdr
    spec = importlib.util.spec_from_file_location("hipsdp_binding_scall", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.Solver.sparsecuts_all) and callable(mod.sparsecuts_all_stats) and callable(mod.Solver.sparsecuts_all_stats)
    assert callable(mod.sparsecuts_unit)
    assert [f[0] for f in mod.SparsecutOpts._fields_] == ["tol", "feastol", "convtol", "maxcuts", "maxit"]
    assert C.sizeof(mod.SparsecutOpts) == 32


def test_library_exports_the_new_symbols(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_sparsecuts_all") and hasattr(lib, "hipsdp_sparsecuts_all_stats")
    assert hasattr(hb.ulib(), "hipsdp_sparsecuts_unit") and not hasattr(lib, "hipsdp_sparsecuts_unit")
    # no device work: the totals are readable before any call, and NULL outputs are allowed
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_sparsecuts_all_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_sparsecuts_all_stats(None, None, None) == 0
    assert lib.hipsdp_sparsecuts_all(None, None, None, None, None, None, None, None, None, None, None, None) == 3
    opts = hb.SparsecutOpts(1e-6, 1e-6, 0.0, 5, 0)
    assert lib.hipsdp_sparsecuts_all(None, None, None, C.byref(opts), None, None, None, None, None, None, None, None) == 3


def test_the_kernels_are_built_from_their_own_source():
    with open(os.path.join(ROOT, "scip-sdp_amd", "Makefile")) as f:
        assert "csrc/sparsecuts.hip" in f.read()
    with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", "sparsecuts.hip")) as f:
        src = f.read()
    assert "__global__" in src and "k_sc_tpower" in src and "k_sc_coefs" in src and "atomicAdd" not in src


def test_the_restatement_returns_the_hand_result_on_a_3_by_3_example():
    """Z = [[-2, 0, 0], [0, 1, 0], [0, 0, -1]], v0 = (3, 2, 1) / sqrt(14), maxeig = 1, size 1.  M = diag(3, 0, 2).
    Run 1: w = M v0 ~ (9, 0, 2): entry 0 stays, x = e_0, value 3, again e_0 and 3 - the run stops after 2 iterations; scalar = 1 - 3
    = -2: cut (-2, e_0); Z becomes diag(0, 1, -1), maxeig 3, M = diag(3, 2, 4).
    Run 2: w ~ (9, 4, 4): entry 0, value 3, 2 iterations; scalar = 3 - 3 = 0: not negative, the loop ends.  1 cut, 4 iterations."""
    Z = np.diag([-2.0, 1.0, -1.0])
    v0 = np.array([3.0, 2.0, 1.0]) / np.sqrt(14.0)
    vals, vecs, sups, iters, flags, mg = R.sparse_cuts_matrix(Z, v0, 1.0, 1, 1e-6, 5)
    assert list(vals) == [-2.0]
    assert np.array_equal(vecs, np.array([[1.0, 0.0, 0.0]]))
    assert [list(s) for s in sups] == [[0]]
    assert iters == 4 and flags == 0
    assert mg.longest == 2 and abs(mg.feas - 1e-6) <= 1e-18 and mg.select > 0.5
    # size 2 from the same start: run 1 keeps entries 0 and 2 (|w| ~ 9, 0, 2) and converges to e_0 within the pair
    vals2, vecs2, sups2, iters2, flags2, _ = R.sparse_cuts_matrix(Z, v0, 1.0, 2, 1e-6, 1)
    assert len(vals2) == 1 and list(sups2[0]) == [0, 2] and flags2 == 0
    assert abs(vals2[0] + 2.0) <= 1e-5 and abs(abs(vecs2[0][0]) - 1.0) <= 1e-2 and vecs2[0][1] == 0.0
    # ties: of equal absolute values the smaller index stays
    x, sup, val, it, fl = R.tpower(np.ones((4, 4)), np.array([1.0, -1.0, 1.0, 1.0]), 2)
    assert list(sup) == [0, 1] and fl == 0 and abs(val - 2.0) <= 1e-12
    # the cap and the zero iterate
    assert R.tpower(np.diag([3.0, 2.9, 1.0]), np.ones(3), 3, maxit=2)[3:] == (2, 1)
    assert R.tpower(np.zeros((3, 3)), np.ones(3), 2)[3:] == (0, 2)
    # the block-level entry: lmin >= -tol, an oversized target and maxcuts = 0 give no cut
    A = np.array([np.diag([2.0, -1.0, 1.0]), np.zeros((3, 3))])
    assert R.sparse_cuts_dense(A, np.zeros(1), 1, 1e-6, 1e-6, 5)[0] == 1              # Z = -A0 = diag(-2, 1, -1)
    assert R.sparse_cuts_dense(A, np.zeros(1), 4, 1e-6, 1e-6, 5)[:2] == (0, -2.0)
    assert R.sparse_cuts_dense(A, np.zeros(1), 1, 1e-6, 1e-6, 0)[:2] == (0, -2.0)
    assert R.sparse_cuts_dense(-A, np.zeros(1), 1, 1e-6, 1e-6, 5)[:2] == (1, -1.0)
    assert R.sparse_cuts_dense(np.array([-np.eye(3), np.zeros((3, 3))]), np.zeros(1), 1, 1e-6, 1e-6, 5)[:2] == (0, 1.0)
