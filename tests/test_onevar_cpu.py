"""CPU: the numpy restatement that the GPU tests of hipsdp_onevar_bounds compare against is itself set against the oracle's
solve_one_var_sdp (the reference's formulation mu A_i - C_i with C_i built as cons_sdp.c:2072-2099 builds it) and against the five
known answers of the reference's unit test; the instance family keeps its share of undecidable jobs and its status mix; the C ABI,
the libraries and the binding carry the call.  What needs a shaped solver (every single argument error, count == 0) is checked in
tests/test_gpu_onevar.py: a solver cannot be created without a device."""
import ctypes as C
import json
import os
import re
import importlib.util
import numpy as np
import pytest
from conftest import ROOT, GOLDEN
import sdpi_driver
import onevar_cases as K


def _entries(M):
    n = M.shape[0]
    return [(r, c, float(M[r, c])) for r in range(n) for c in range(r + 1) if M[r, c] != 0.0]


def _const_matrix(A, ub, i):
    """C_i of tightenBounds (cons_sdp.c:2072-2099): a fresh copy of the constant matrix, minus ub_k A_k for every other variable k,
    in index order"""
    Cm = A[0].copy()
    for k in range(len(ub)):
        if k != i and ub[k] != 0.0:
            Cm -= A[k + 1] * ub[k]
    return Cm


def _oracle(A, lb, ub, i, feastol):
    """(status, optval, evals) of the oracle on the reference's formulation"""
    calls = [0]

    def lmin(M):
        calls[0] += 1
        return sdpi_driver.lmin_numpy(M)

    n = A.shape[1]
    objval, optval, cert = sdpi_driver.solve_one_var_sdp(1.0, lb[i], ub[i], n, _entries(_const_matrix(A, ub, i)), _entries(A[i + 1]),
                                                         feastol, lmin=lmin)
    if objval is None:
        return K.DECLINED, None, 0
    if objval >= sdpi_driver.INF:
        return K.INFEASIBLE, optval, calls[0]
    if optval == lb[i] and cert == 0.0:
        return K.LB, optval, calls[0]
    return K.INNER, optval, calls[0]


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "n%d" % s[0])
def test_restatement_agrees_with_the_oracle_on_the_family(size):
    """the device formulation Z(u) + (mu - u_i) A_i against the reference's mu A_i - C_i: the two matrices differ by rounding alone,
    so on decidable jobs status and evaluations are equal, an INNER answer lies within the concavity bound, a bound is returned
    exactly"""
    worst = 0.0
    for fl, sd, A, lb, ub, refs in K.instances(size):
        Z = K.z_of(A, ub)
        for i, r in enumerate(refs):
            st, ov, ne = _oracle(A, lb, ub, i, K.FEASTOL)
            if not K.decidable(K.NEWTON, r[5]):
                continue
            assert (st, ne) == (r[0], r[4]), (fl, sd, i)
            if st == K.INNER:
                bound, g = K.inner_bound(Z, A[i + 1], ub[i], ov, r[1], K.FEASTOL)
                worst = max(worst, abs(ov - r[1]) * g / K.FEASTOL)
                assert abs(ov - r[1]) <= bound, (fl, sd, i)
            elif st == K.LB or len(r[5]) <= 2:
                assert ov == r[1], (fl, sd, i)
            else:
                bound, g = K.inner_bound(Z, A[i + 1], ub[i], ov, r[1], K.FEASTOL)
                assert abs(ov - r[1]) <= bound, (fl, sd, i)             # (INFEASIBLE at a mu: held to the same bound)
    print("n = %d: worst |optval - oracle| g / feastol = %.3g" % (size[0], worst))


def test_known_answers_of_the_reference_unit_test():
    with open(os.path.join(GOLDEN, "onevar_cases.json")) as f:
        G = json.load(f)
    assert len(G["cases"]) == 5
    for c in G["cases"]:
        n = c["n"]
        A0, A1 = sdpi_driver._dense(n, c["const"]), sdpi_driver._dense(n, c["var"])
        st, ov, f, g, ne, log = K.onevar_ref(-A0, A1, 0.0, K.NEWTON, c["lb"], c["ub"], G["eps"], infinity=G["infinity"])
        if c["infeasible"]:
            assert st == K.INFEASIBLE, c["name"]
        else:
            assert st in (K.LB, K.INNER) and abs(ov - c["optval"]) <= G["eps"], (c["name"], ov)
    assert [c["optval"] for c in G["cases"]] == [1.0, 1.0, None, None, 1.541381]


def test_undecidable_cap_and_status_mix():
    total = und = 0
    mix = {0: set(), 1: set()}
    for size in K.SIZES:
        jobs = bad = 0
        here = set()
        for fl, sd, A, lb, ub, refs in K.instances(size):
            for r in refs:
                jobs += 1
                bad += 0 if K.decidable(K.NEWTON, r[5]) else 1
                here.add(r[0])
                assert r[4] <= 13
        assert bad <= K.UNDECIDABLE_CAP * jobs, (size, bad, jobs)
        assert here == {K.LB, K.INNER, K.INFEASIBLE}, (size, here)
        mix[K.size_class(size[0])] |= here
        total += jobs
        und += bad
    assert und <= K.UNDECIDABLE_CAP * total, (und, total)
    assert mix[0] == mix[1] == {K.LB, K.INNER, K.INFEASIBLE}
    print("%d of %d jobs undecidable" % (und, total))


def test_twopoint_and_limits_of_the_restatement():
    """the three outcomes of TWOPOINT, DECLINED and GAVEUP on a 1 x 1 block by hand: M(mu) = mu - 0.5"""
    Z, A = np.array([[-0.5]]), np.array([[1.0]])
    assert K.onevar_ref(Z, A, 0.0, K.TWOPOINT, 0.6, 1.0, 1e-6)[:2] == (K.LB, 0.6)
    assert K.onevar_ref(Z, A, 0.0, K.TWOPOINT, 0.0, 1.0, 1e-6)[:2] == (K.UBONLY, 1.0)
    assert K.onevar_ref(Z, A, 0.0, K.TWOPOINT, 0.0, 0.25, 1e-6)[:2] == (K.INFEASIBLE, 0.25)
    assert K.onevar_ref(Z, A, 0.0, K.NEWTON, 0.0, 1e20, 1e-6)[0] == K.DECLINED
    assert K.onevar_ref(Z, A, 0.0, K.NEWTON, -1e20, 1.0, 1e-6)[0] == K.DECLINED
    st, ov, f, g, ne, log = K.onevar_ref(Z, A, 0.0, K.NEWTON, 0.0, 1.0, 1e-6)
    assert (st, ne) == (K.INNER, 3) and abs(ov - (0.5 - 0.5e-6)) <= 1e-15 and g == 1.0
    assert K.onevar_ref(Z, A, 0.0, K.NEWTON, 0.0, 1.0, 1e-6, maxevals=2)[:2] == (K.GAVEUP, 0.0)
    assert K.onevar_ref(Z, A, 0.0, K.NEWTON, 0.0, 0.25, 1e-6)[:2] == (K.INFEASIBLE, 0.25)


def _hdr(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_onevar_bounds_is_declared_and_bound():
    hdr = _hdr("hipsdp.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_bounds\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+block\s*,\s*const\s+double\s*\*\s*u\s*,"
                     r"\s*int\s+count\s*,\s*const\s+int\s*\*\s*vars\s*,\s*const\s+int\s*\*\s*kind\s*,\s*const\s+double\s*\*\s*lb\s*,"
                     r"\s*const\s+double\s*\*\s*ub\s*,\s*const\s+hipsdp_onevar_opts\s*\*\s*opts\s*,\s*int\s*\*\s*status\s*,"
                     r"\s*double\s*\*\s*optval\s*,\s*double\s*\*\s*lmin\s*,\s*double\s*\*\s*grad\s*,\s*int\s*\*\s*evals\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_bounds_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    for name, val in (("MAXN", 128), ("NEWTON", 0), ("TWOPOINT", 1), ("LB", 0), ("INNER", 1), ("INFEASIBLE", 2), ("UBONLY", 3),
                      ("DECLINED", 4), ("GAVEUP", 5)):
        assert re.search(r"#define\s+HIPSDP_ONEVAR_%s\s+%d\b" % (name, val), hdr), name
    units = _hdr("hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_unit\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*int\s+count\s*,", units)
    assert "hipsdp_onevar_unit" not in hdr and not re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_bounds", units)
    spec = importlib.util.spec_from_file_location("hipsdp_binding_onevar", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    import inspect
    assert list(inspect.signature(mod.Solver.onevar_bounds).parameters) == ["self", "block", "u", "lb", "ub", "feastol", "vars", "kind",
                                                                            "infinity", "maxevals"]
    p = inspect.signature(mod.Solver.onevar_bounds).parameters
    assert (p["vars"].default, p["kind"].default, p["infinity"].default, p["maxevals"].default) == (None, None, 1e20, 0)
    assert callable(mod.onevar_bounds_stats) and callable(mod.Solver.onevar_bounds_stats) and callable(mod.onevar_unit)
    assert C.sizeof(mod.OnevarOpts) == 24
    assert (mod.ONEVAR_NEWTON, mod.ONEVAR_TWOPOINT) == (K.NEWTON, K.TWOPOINT)
    assert (mod.ONEVAR_LB, mod.ONEVAR_INNER, mod.ONEVAR_INFEASIBLE, mod.ONEVAR_UBONLY, mod.ONEVAR_DECLINED, mod.ONEVAR_GAVEUP) == \
        (K.LB, K.INNER, K.INFEASIBLE, K.UBONLY, K.DECLINED, K.GAVEUP)


def test_libraries_export_the_calls_and_refuse_a_missing_solver(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_onevar_bounds") and hasattr(lib, "hipsdp_onevar_bounds_stats")
    assert hasattr(hb.ulib(), "hipsdp_onevar_unit") and not hasattr(lib, "hipsdp_onevar_unit")
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_onevar_bounds_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_onevar_bounds_stats(None, None, None) == 0
    # no device is looked at: without a solver every call is an argument error, whatever else it carries
    opts = hb.OnevarOpts(1e-6, 1e20, 0)
    one = (C.c_double * 1)(0.0)
    st = (C.c_int * 1)(7)
    assert lib.hipsdp_onevar_bounds(None, 0, None, 1, None, None, None, None, None, None, None, None, None, None) == 3
    assert lib.hipsdp_onevar_bounds(None, 0, one, 1, None, None, one, one, C.byref(opts), st, one, None, None, None) == 3
    assert lib.hipsdp_onevar_bounds(None, 0, one, 0, None, None, one, one, C.byref(opts), st, one, None, None, None) == 3
    assert st[0] == 7
    c2, l2, r2 = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_onevar_bounds_stats(C.byref(c2), C.byref(l2), C.byref(r2)) == 0
    assert (c2.value, l2.value, r2.value) == (c.value, l.value, r.value)


def test_the_kernel_and_the_host_side_are_where_the_build_expects_them():
    with open(os.path.join(ROOT, "scip-sdp_amd", "Makefile")) as f:
        assert "csrc/onevar.hip" in f.read()
    with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", "eigi.hip")) as f:
        src = f.read()
    assert "k_onevar_small" in src and "k_onevar_mid" in src and "int hs_onevar_newton(" in src
    assert re.search(r"d_syevi_small<false>\(n, 1, wantvec, sm, eo, 0ULL, NULL\)", src)       # full accuracy: mtol at its default
    with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", "onevar.hip")) as f:
        host = f.read()
    assert "__global__" not in host and "hs_ec_form_z(" in host and "hs_onevar_newton(" in host and "atomicAdd" not in src
