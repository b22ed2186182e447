"""CPU: hipsdp_rounding_frame / hipsdp_rounding_recombine / hipsdp_rounding_stats are declared, bound and exported, the unit entry lives in
the units library alone, the numpy restatement (tests/harness/roundprob_ref.py) is what the reference's loops compute - exactly on
integer data, against np.longdouble on random data, and through the two identities that do not depend on the basis -, the header's
launch formulas are the host functions, the host-side planning (csrc/hs_round_plan.cpp) runs clean in a stand-alone program under
AddressSanitizer + UBSan, and the sources keep the shape the design asks for."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess

import numpy as np

from conftest import ROOT
import host_check
import roundprob_ref as ref

PKG = os.path.join(ROOT, "scip-sdp_amd")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _sym(rng, n):
    R = rng.standard_normal((n, n))
    return (R + R.T) / 2.0


def test_calls_are_declared_and_bound():
    hdr, uhdr = _read("include", "hipsdp.h"), _read("include", "hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rounding_frame\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+int\s*\*\s*xnnz\s*,"
                     r"\s*const\s+int\s*\*\s*const\s*\*\s*xrow\s*,\s*const\s+int\s*\*\s*const\s*\*\s*xcol\s*,"
                     r"\s*const\s+double\s*\*\s*const\s*\*\s*xval\s*,", hdr)
    assert re.search(r"typedef\s+struct\s+hipsdp_rounding_out\s*\{\s*int\s+cap;\s*int\s+nnz_out;\s*int\s*\*\s*rowout\s*,\s*\*\s*colout;"
                     r"\s*double\s*\*\s*valout;\s*\}\s*hipsdp_rounding_out;", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rounding_recombine\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*lambda[^;]*"
                     r"double\s+epsilon\s*,\s*int\s+mode\s*,\s*hipsdp_rounding_out\s*\*\s*out", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rounding_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert not re.search(r"HIPSDP_API[^;]*\bhipsdp_rounding_(frame|recombine|stats)\s*\(", uhdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rounding_coefs_unit\s*\(", uhdr) and "hipsdp_rounding_coefs_unit" not in hdr
    spec = importlib.util.spec_from_file_location("hipsdp_binding_rounding", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert list(inspect.signature(mod.Solver.rounding_frame).parameters)[:2] == ["self", "X"]
    assert list(inspect.signature(mod.Solver.rounding_recombine).parameters)[:4] == ["self", "lam", "epsilon", "mode"]
    assert callable(mod.rounding_stats) and callable(mod.rounding_coefs_unit)
    assert [f[0] for f in mod.RoundingOut._fields_] == ["cap", "nnz_out", "rowout", "colout", "valout"]


def test_libraries_export_accordingly_and_null_solvers_are_refused_without_a_device(hb):
    lib, ulib = hb.lib(), hb.ulib()
    for name in ("hipsdp_rounding_frame", "hipsdp_rounding_recombine", "hipsdp_rounding_stats"):
        assert hasattr(lib, name), name
    assert hasattr(ulib, "hipsdp_rounding_coefs_unit") and not hasattr(lib, "hipsdp_rounding_coefs_unit")
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_rounding_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_rounding_stats(None, None, None) == 0 and lib.hipsdp_rounding_stats(None, C.byref(l), None) == 0
    assert hb.rounding_stats() == (c.value, l.value, r.value)
    cnt = np.zeros(1, dtype=np.int32)
    x = np.zeros(4)
    dp = x.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.hipsdp_rounding_frame(None, cnt.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, dp, dp, dp, None, None) == 3
    tab = (hb.RoundingOut * 1)()
    assert lib.hipsdp_rounding_recombine(None, dp, C.c_double(1e-9), 0, tab) == 3
    assert hb.rounding_stats() == (c.value, l.value, r.value)


def test_restatement_is_exact_on_integer_data_with_a_signed_permutation():
    rng = np.random.default_rng(1)
    for n, m in ((1, 1), (3, 2), (17, 5), (65, 3)):
        A = rng.integers(-3, 4, (m + 1, n, n)).astype(np.float64)
        A = np.tril(A) + np.transpose(np.tril(A, -1), (0, 2, 1))
        pi = rng.permutation(n)
        V = np.zeros((n, n))
        V[np.arange(n), pi] = rng.choice([-1.0, 1.0], n)
        want = np.stack([np.diag(A[i])[pi] for i in range(m + 1)], axis=1)
        assert np.array_equal(ref.coefficients(V, A), want)
        assert np.array_equal(np.asarray(ref.coefficients_einsum(V, A), dtype=np.float64), want)
        lam = rng.integers(-4, 5, n).astype(np.float64)
        # V^T diag(lam) V with a signed permutation: lam_k at (pi_k, pi_k) in mode 1, P diag(lam) P^T entry (i, j) = sum_c V_ic lam_c V_jc in mode 0
        R1 = np.zeros((n, n)); R1[pi, pi] = lam
        inv = np.argsort(pi)
        R0 = np.zeros((n, n)); R0[np.arange(n), np.arange(n)] = lam[pi]
        assert np.array_equal(ref.recombine(V, lam, 1), R1) and np.array_equal(ref.recombine(V, lam, 0), R0)
        assert inv.shape == (n,)


def test_restatement_matches_longdouble_and_the_two_basis_free_identities():
    rng = np.random.default_rng(2)
    for n, m in ((3, 1), (17, 5), (64, 3), (65, 2), (130, 1)):
        A = np.stack([_sym(rng, n) / np.sqrt(n) for _ in range(m + 1)])
        X = _sym(rng, n) / np.sqrt(n)
        lam, V = ref.decompose(X)
        tab = ref.coefficients(V, A)
        want = ref.coefficients_einsum(V, A)
        b = ref.coefficient_bound(V, A, n * (n + 1) // 2)
        assert np.all(np.abs(np.asarray(tab, dtype=np.longdouble) - want) <= b), (n, m)
        fro = np.array([np.linalg.norm(A[i]) for i in range(m + 1)])
        top = float(np.max(np.abs(lam)))
        tr = np.array([np.trace(A[i]) for i in range(m + 1)])
        inner = np.array([np.sum(A[i] * X) for i in range(m + 1)])
        assert np.all(np.abs(tab.sum(axis=0) - tr) <= 2 * n * 1e-11 * fro + b.sum(axis=0))
        assert np.all(np.abs(lam @ tab - inner) <= 2 * (np.sqrt(n) * 1e-9 + n * 1e-11) * top * fro + np.abs(lam) @ b)
        for mode in (0, 1):
            R = ref.recombine(V, lam, mode)
            Rl = ref.recombine(V, lam, mode, dtype=np.longdouble)
            assert np.all(np.abs(np.asarray(R, dtype=np.longdouble) - Rl) <= ref.recombine_bound(V, lam, mode)), (n, mode)
        assert np.linalg.norm(ref.recombine(V, lam, 1) - X) <= 2 * (np.sqrt(n) * 1e-9 + n * 1e-11) * top
        r, c, v = ref.kept(ref.recombine(V, lam, 1), 1e-9)
        assert np.all(r <= c) and np.all(np.abs(v) > 1e-9) and np.all(np.diff(r * n + c) > 0)
    M = ref.expand(3, [0, 1, 2], [0, 0, 1], [1.0, 2.0, 3.0])
    assert np.array_equal(M, np.array([[1.0, 2.0, 0.0], [2.0, 0.0, 3.0], [0.0, 3.0, 0.0]]))


def test_header_formulas_are_the_host_functions(tmp_path):
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"\[1 \.\. 128 rows\] 4 \+ \[129 \.\. 512 rows\] \(nmax \+ 6 \+ 6 ceil\(nmax / 32\)\) \+ 4", hdr)
    assert re.search(r"\[1 \.\. 128 rows\] 2 \+ \[129 \.\. 512 rows\] 2", hdr)
    src = tmp_path / "launches.cpp"
    src.write_text('#include <stdio.h>\n#include "hs_round_plan.h"\nint main(void) { const int ns[] = {0, 129, 130, 200, 512};\n'
                   'for (int s = 0; s < 2; ++s) for (int k = 0; k < 5; ++k) printf("%lld %lld ", hs_rf_launches(s, ns[k]), '
                   'hs_rf2_launches(s, ns[k] > 0)); return 0; }\n')
    exe = str(tmp_path / "launches")
    r = subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    want = []
    for s in (0, 1):
        for n in (0, 129, 130, 200, 512):
            one = (4 * s + (n + 6 + 6 * -(-n // 32) if n else 0) + 4) if (s or n) else 0
            want += [one, 2 * s + (2 if n else 0)]
    assert out == want


def test_host_planning_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/round_plan_check.cpp + csrc/hs_round_plan.cpp, host compiler, -fsanitize=address,undefined:
    a program of its own with the runtimes linked in (nothing is loaded into python, nothing is preloaded)"""
    host_check.run_clean(tmp_path, "round_plan_check.cpp", ["hs_round_plan.cpp"], "round plan check: ok")


def test_sources_keep_their_shape():
    mk = _read("scip-sdp_amd", "Makefile")
    assert "csrc/rounding.hip" in mk and "csrc/hs_round_plan.cpp" in mk and "csrc/hs_round_plan.h" in mk
    plan = _read("scip-sdp_amd", "csrc", "hs_round_plan.cpp") + _read("scip-sdp_amd", "csrc", "hs_round_plan.h")
    assert "hip_runtime" not in plan and "hs_kernels.h" not in plan and "hs_rf_decode" in plan and "hs_rf_slice_rule" in plan
    rf = _read("scip-sdp_amd", "csrc", "rounding.hip")
    for k in ("k_rf_gather", "k_rf_coefs_scalar", "k_rf_coefs_mc", "k_rf_store"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, rf), k
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in rf and "hs_rf_decode(" in rf and "hs_rf_weight(" in rf
    assert not re.search(r"atomic\w*\s*\(", rf) and "cooperative" not in rf and "grid.sync" not in rf
    assert "hs_rf_weight(" in _read("scip-sdp_amd", "csrc", "hs_ec_sweep.h")             # the weighting is kept in one place
    cc = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    body = cc[cc.index("int rf_chunk("):]
    assert 'hs_chunk_env("HIPSDP_ROUNDING_CHUNK")' in body and "getenv" not in body
    # stage 2 shares the recombine and write launches: the kernels exist once, in the files of the projections
    for k, f in (("k_pp_recombine", "psd_many.hip"), ("k_pp_write", "psd_many.hip"), ("k_ppl_recombine", "psd_large.hip"),
                 ("k_ppl_write", "psd_large.hip")):
        assert len(re.findall(r"__global__[^;{]*\b%s\s*\(" % k, _read("scip-sdp_amd", "csrc", f))) == 1
        assert not re.search(r"__global__[^;{]*\b%s\s*\(" % k, rf + cc)
    for f in ("hs_pp_recombine(", "hs_pp_write(", "hs_ppl_recombine(", "hs_ppl_write("):
        assert f in body, f
    assert "HIPSDP_ROUNDING_CHUNK" in _read("INTEGRATION.md")
