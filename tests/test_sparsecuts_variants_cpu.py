"""CPU: the restatement of the sparse-cut loop with the reference's three switches (tests/harness/sparsecuts_variants_ref.py) and the
interface of hipsdp_sparsecuts_all_ex / hipsdp_sparsecuts_ex.  With variant 0 the restatement is sparsecuts_ref's loop; a hand example
shows what recomputesparseev changes; and every case the GPU tests compare (tests/harness/sparsecuts_variants_cases.py) is shown to
be STABLE first: none of the restatement's decisions is close, the eigenvectors it takes are well defined, and perturbing every
eigenpair it takes by 1e-9 relative - the residual bound of the eigen contract - moves no cut count, support or iteration number."""
import ctypes as C
import os
import re
import importlib.util
import numpy as np
import pytest
from conftest import ROOT
import host_check
import sparsecuts_ref as R
import sparsecuts_variants_ref as V
import sparsecuts_variants_cases as K


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.mark.parametrize("name,size", [("f0", 4), ("b12", 4), ("b40", 10)])
def test_variant_0_is_the_default_restatement(name, size):
    blocks, ys, y, b = K.family(name)
    for A in blocks:
        r0 = R.sparse_cuts_dense(A, y, size, K.TOL, K.FEASTOL, K.MAXCUTS)
        r1 = V.sparse_cuts_dense_ex(A, y, size, K.TOL, K.FEASTOL, K.MAXCUTS, 0)
        assert r1[0] == r0[0] and r1[1] == r0[1] and r1[7:9] == r0[7:9]
        assert all(np.array_equal(a, b_) for a, b_ in zip(r1[2:6], r0[2:6]))
        assert [list(s) for s in r1[6]] == [list(s) for s in r0[6]]
        assert (r1[9].select, r1[9].conv, r1[9].feas, r1[9].longest) == (r0[9].select, r0[9].conv, r0[9].feas, r0[9].longest)
        assert sum(r1[10]) == r0[7] and len(r1[10]) == (r0[0] + 1 if r0[7] else 0)


def test_hand_example_recomputesparseev_cuts_with_the_submatrix_eigenvalue():
    Z = K.HAND_Z
    lam, W = np.linalg.eigh(Z)
    out = {}
    for variant in (0, 1):
        out[variant] = V.sparse_cuts_matrix_ex(Z, W[:, 0], float(lam[-1]), K.HAND_SIZE, K.TOL, K.FEASTOL, 1, variant, convtol=K.HAND_CONVTOL)
    (v0, x0, s0, it0, f0, _, runs0), (v1, x1, s1, it1, f1, _, runs1) = out[0], out[1]
    assert len(v0) == len(v1) == 1 and runs0[0] == runs1[0] == 2          # TPower stopped early, both loops cut once
    assert list(s0[0]) == list(s1[0]) and len(s1[0]) == 2
    S = np.ix_(s1[0], s1[0])
    sub = np.linalg.eigvalsh(Z[S])
    assert abs(v1[0] - sub[0]) <= 1e-12 * abs(sub[0])
    assert abs(v0[0] - x0[0] @ Z @ x0[0]) <= 1e-12
    assert abs(sub[0] - (-1.95 - np.sqrt(0.0125))) <= 1e-14
    assert v1[0] < v0[0] - 0.1, (v1[0], v0[0])                            # strictly, and visibly, below the default's value
    assert abs(np.linalg.norm(x1[0]) - 1.0) <= 1e-14 and np.count_nonzero(x1[0]) == 2
    # the same through the dense entry: the block whose Z(y) is the hand matrix
    A, y = K.hand_block()
    r = V.sparse_cuts_dense_ex(A, y, K.HAND_SIZE, K.TOL, K.FEASTOL, 1, 1, convtol=K.HAND_CONVTOL)
    assert r[0] == 1 and abs(r[2][0] - sub[0]) <= 1e-12 * abs(sub[0])


def test_the_tol_rule_ends_the_loop_and_sets_bit_2():
    """tol above |lambda|: the submatrix eigenvalue is not below -tol, the loop ends with no cut from that run"""
    Z = K.HAND_Z
    lam, W = np.linalg.eigh(Z)
    vals, vecs, sups, iters, flags, mg, runs = V.sparse_cuts_matrix_ex(Z, W[:, 0], float(lam[-1]), 2, 10.0, K.FEASTOL, 3, 1)
    assert len(vals) == 0 and flags == 4 and len(runs) == 1 and iters == runs[0] > 0


def test_interface_is_declared_bound_and_built():
    hdr = _read("include", "hipsdp.h")
    d = r"\s*,\s*double\s*\*\s*"
    i = r"\s*,\s*int\s*\*\s*"
    tail = r"\s*,\s*unsigned\s+variant" + i + "ncuts" + d + "lmin" + d + "eigvals" + d + "coefs" + d + "lhs" + d + "vecs" + i + "iters" + i \
        + r"flags\s*\)"
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_all_ex\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*const\s+int\s*\*\s*sizes\s*,\s*const\s+hipsdp_sparsecut_opts\s*\*\s*opts" + tail, hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_ex\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+block\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*int\s+size\s*,\s*const\s+hipsdp_sparsecut_opts\s*\*\s*opts" + tail, hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_ex_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    for name, bit in (("RECOMPUTE_SPARSEEV", 1), ("RECOMPUTE_INITIAL", 2), ("EXACTTRANS", 4)):
        assert re.search(r"#define\s+HIPSDP_SC_%s\s+%d\b" % (name, bit), hdr)
    assert not re.search(r"hipsdp_sparsecuts(_all)?_ex(_stats)?\s*\(", _read("include", "hipsdp_units.h"))
    spec = importlib.util.spec_from_file_location("hipsdp_binding_scvar", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.Solver.sparsecuts_all_ex) and callable(mod.Solver.sparsecuts_ex)
    assert callable(mod.sparsecuts_ex_stats) and callable(mod.Solver.sparsecuts_ex_stats)
    assert (mod.SC_RECOMPUTE_SPARSEEV, mod.SC_RECOMPUTE_INITIAL, mod.SC_EXACTTRANS) == (V.SPARSEEV, V.INITIAL, V.EXACTTRANS) == (1, 2, 4)
    assert C.sizeof(mod.SparsecutOpts) == 32                             # the switches travel beside the options, not inside them
    assert "csrc/sparsecuts_rounds.hip" in _read("scip-sdp_amd", "Makefile")
    src = _read("scip-sdp_amd", "csrc", "sparsecuts_rounds.hip")
    assert "__global__" in src and "k_scr_tpower" in src and "k_scr_cut" in src
    assert "atomic" not in src.replace("no atomic", "")                  # the stream's order is the only synchronisation
    # ONE TPower run for both loops: the rounds and k_sc_tpower call the same device function, 128 threads, a thread per row
    run = _read("scip-sdp_amd", "csrc", "hs_sc_tpower.h")
    assert re.search(r"#define\s+SC_NT\s+128\b", run) and "sc_tpower_run(" in run
    assert "sc_tpower_run(" in src and "sc_tpower_run(" in _read("scip-sdp_amd", "csrc", "sparsecuts.hip")
    assert "csrc/hs_sc_tpower.h" in _read("scip-sdp_amd", "Makefile")
    # the documents no longer call the switches unserved
    assert "NOT served - with any of them set" not in _read("INTEGRATION.md")
    assert "hipsdp_sparsecuts_all_ex" in _read("INTEGRATION.md") and "hipsdp_sparsecuts_all_ex" in _read("DESIGN.md")


def test_the_layout_of_the_rounds_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/cut_plan_rounds_check.cpp + csrc/hs_cut_plan.cpp, host compiler,
    -fsanitize=address,undefined: a program of its own with the runtimes linked in (nothing is loaded into python, nothing is
    preloaded)"""
    host_check.run_clean(tmp_path, "cut_plan_rounds_check.cpp", ["hs_cut_plan.cpp"], "cut plan rounds check: ok")
    assert "hs_scr_layout_make" in _read("scip-sdp_amd", "csrc", "cut_calls.hip") and "hs_scr_block_make" in _read("scip-sdp_amd", "csrc", "cut_calls.hip")


def test_libraries_export_the_calls_and_check_their_arguments(hb):
    lib = hb.lib()
    for name in ("hipsdp_sparsecuts_all_ex", "hipsdp_sparsecuts_ex", "hipsdp_sparsecuts_ex_stats"):
        assert hasattr(lib, name) and hasattr(hb.ulib(), name), name
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_sparsecuts_ex_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_sparsecuts_ex_stats(None, None, None) == 0
    opts = hb.SparsecutOpts(1e-6, 1e-6, 0.0, 5, 0)
    ERR_ARG = 3
    for variant in (0, 1, 7, 8, 1 << 20):
        u = C.c_uint(variant)
        assert lib.hipsdp_sparsecuts_all_ex(None, None, None, C.byref(opts), u, None, None, None, None, None, None, None, None) == ERR_ARG
        assert lib.hipsdp_sparsecuts_ex(None, 0, None, 4, C.byref(opts), u, None, None, None, None, None, None, None, None) == ERR_ARG
    after = (C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1))
    assert lib.hipsdp_sparsecuts_ex_stats(*[C.byref(a) for a in after]) == 0
    assert [a.value for a in after] == [c.value, l.value, r.value]       # nothing counted


@pytest.mark.parametrize("name,size,variant", K.CASES)
def test_every_named_case_is_stable(name, size, variant):
    worst = K.check_margins(name, size, variant)
    print("%s size %d variant %d: worst margins select %.2e conv %.2e feas %.2e submatrix gap %.2e deflated gap %.2e tol %.2e"
          % ((name, size, variant) + tuple(worst)))
