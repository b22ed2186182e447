"""CPU: hipsdp_onevar_bounds_all - the C ABI, the libraries and the binding carry the call; every argument error is refused before
a device is looked at; the workspace layout (hs_ova_layout, csrc/hs_cut_plan.cpp) runs clean in a stand-alone program under
AddressSanitizer + UBSan; the multi-block family of tests/test_gpu_onevar_all.py keeps its share of undecidable jobs and its status
mix against the numpy restatement; EXTREMES restated with numpy.  What needs a shaped solver is checked in
tests/test_gpu_onevar_all.py: a solver cannot be created without a device."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import numpy as np
from conftest import ROOT
import host_check
import onevar_cases as K
import onevar_all_cases as KA

PKG = os.path.join(ROOT, "scip-sdp_amd")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_call_is_declared_and_bound():
    hdr, units = _read("include", "hipsdp.h"), _read("include", "hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_bounds_all\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*u\s*,"
                     r"\s*int\s+count\s*,\s*const\s+int\s*\*\s*blocks\s*,\s*const\s+int\s*\*\s*vars\s*,\s*const\s+int\s*\*\s*kind\s*,"
                     r"\s*const\s+double\s*\*\s*lb\s*,\s*const\s+double\s*\*\s*ub\s*,\s*const\s+hipsdp_onevar_opts\s*\*\s*opts\s*,"
                     r"\s*int\s*\*\s*status\s*,\s*double\s*\*\s*optval\s*,\s*double\s*\*\s*lmin\s*,\s*double\s*\*\s*grad\s*,"
                     r"\s*int\s*\*\s*evals\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_bounds_all_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert re.search(r"#define\s+HIPSDP_ONEVAR_EXTREMES\s+2\b", hdr) and re.search(r"#define\s+HIPSDP_ONEVAR_DONE\s+6\b", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_all_unit\s*\(\s*int\s+device\s*,\s*int\s+count\s*,\s*const\s+int\s*\*\s*n\s*,", units)
    assert "hipsdp_onevar_all_unit" not in hdr and not re.search(r"HIPSDP_API\s+int\s+hipsdp_onevar_bounds_all", units)
    spec = importlib.util.spec_from_file_location("hipsdp_binding_onevar_all", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = inspect.signature(mod.Solver.onevar_bounds_all).parameters
    assert list(p) == ["self", "u", "lb", "ub", "feastol", "blocks", "vars", "kind", "infinity", "maxevals"]
    assert [p[k].default for k in ("blocks", "vars", "kind", "infinity", "maxevals")] == [None, None, None, 1e20, 0]
    assert callable(mod.onevar_bounds_all_stats) and callable(mod.Solver.onevar_bounds_all_stats) and callable(mod.onevar_all_unit)
    assert (mod.ONEVAR_EXTREMES, mod.ONEVAR_DONE) == (KA.EXTREMES, KA.DONE) == (2, 6)


def test_libraries_export_the_calls(hb):
    lib, ulib = hb.lib(), hb.ulib()
    assert hasattr(lib, "hipsdp_onevar_bounds_all") and hasattr(lib, "hipsdp_onevar_bounds_all_stats")
    assert hasattr(ulib, "hipsdp_onevar_all_unit") and not hasattr(lib, "hipsdp_onevar_all_unit")


def test_argument_errors_and_the_totals_without_a_device(hb):
    """no device is looked at: every error of the list returns HIPSDP_ERR_ARG (3), status stays, the totals stay.  Without a device
    there is no shaped solver, so `solver NULL` stands in front of every other error here; with a solver each one is checked alone in
    tests/test_gpu_onevar_all.py"""
    lib = hb.lib()
    f = lib.hipsdp_onevar_bounds_all
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_onevar_bounds_all_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_onevar_bounds_all_stats(None, None, None) == 0
    opts, neg = hb.OnevarOpts(1e-6, 1e20, 0), hb.OnevarOpts(-1.0, 1e20, 0)
    o = C.byref(opts)
    two = (C.c_double * 2)(0.0, 0.0)
    st = (C.c_int * 2)(7, 7)
    idx, bad, kbad = (C.c_int * 2)(0, 0), (C.c_int * 2)(0, -1), (C.c_int * 2)(0, 3)
    calls = [
        (None, None, 2, None, None, None, None, None, None, None, None),          # everything missing
        (None, two, 2, idx, idx, idx, two, two, o, st, two),                      # the solver alone
        (None, None, 2, idx, idx, idx, two, two, o, st, two),                     # u
        (None, two, 2, idx, idx, idx, None, two, o, st, two),                     # lb
        (None, two, 2, idx, idx, idx, two, None, o, st, two),                     # ub
        (None, two, 2, idx, idx, idx, two, two, None, st, two),                   # opts
        (None, two, 2, idx, idx, idx, two, two, o, None, two),                    # status
        (None, two, 2, idx, idx, idx, two, two, o, st, None),                     # optval
        (None, two, -1, idx, idx, idx, two, two, o, st, two),                     # count < 0
        (None, two, 2, bad, idx, idx, two, two, o, st, two),                      # a block index
        (None, two, 2, idx, bad, idx, two, two, o, st, two),                      # a variable index
        (None, two, 2, idx, idx, kbad, two, two, o, st, two),                     # a kind
        (None, two, 2, idx, idx, idx, two, two, C.byref(neg), st, two),           # feastol < 0
        (None, two, 2, idx, None, idx, two, two, o, st, two),                     # one of blocks / vars without the other
        (None, two, 2, None, idx, idx, two, two, o, st, two),
        (None, two, 2, None, None, None, two, two, o, st, two),                   # both NULL
        (None, two, 0, idx, idx, idx, two, two, o, st, two),                      # count == 0 does not get past a missing solver
    ]
    for a in calls:
        assert f(*a, None, None, None) == 3, a
    assert list(st) == [7, 7]
    c2, l2, r2 = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_onevar_bounds_all_stats(C.byref(c2), C.byref(l2), C.byref(r2)) == 0
    assert (c2.value, l2.value, r2.value) == (c.value, l.value, r.value)
    # the order in the source: the argument checks stand in front of the first look at the device
    src = _read("scip-sdp_amd", "csrc", "onevar.hip")
    body = src[src.index('extern "C" int hipsdp_onevar_bounds_all('):]
    assert body.index("return HIPSDP_ERR_ARG") < body.index("hs_solver_cut_enter(") < body.index("hs_onevar_all(")
    assert body.count("return HIPSDP_ERR_ARG") == 3 and body.index("if ( count == 0 )") < body.index("hs_solver_cut_enter(")


def test_layout_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/onevar_plan_check.cpp + csrc/hs_cut_plan.cpp, host compiler,
    -fsanitize=address,undefined: a program of its own with the runtimes linked in (nothing is loaded into python, nothing is
    preloaded)"""
    host_check.run_clean(tmp_path, "onevar_plan_check.cpp", ["hs_cut_plan.cpp"], "onevar plan check: ok")


def test_the_layout_stays_host_only_and_the_kernels_share_their_bodies():
    assert "hip_runtime" not in _read("scip-sdp_amd", "csrc", "hs_cut_plan.cpp")
    hdr = _read("scip-sdp_amd", "csrc", "hs_cut_plan.h")
    assert "hip_runtime" not in hdr and "hs_kernels.h" not in hdr and "hs_common.h" not in hdr and "hs_ova_layout_make" in hdr
    host = _read("scip-sdp_amd", "csrc", "onevar.hip")
    assert "__global__" not in host and "hs_ova_layout_make(" in host and "hs_solver_cut_blocks(" in host and "hs_device_cus()" in host
    src = _read("scip-sdp_amd", "csrc", "eigi.hip")
    for name in ("k_onevar_all_small", "k_onevar_all_mid", "int hs_onevar_all("):
        assert name in src, name
    # one definition of every shared body, called from the per-block kernels and from the new ones
    for name in ("ov_stage_a", "ov_begin", "ov_decide", "ov_store", "ov_run_small", "ov_run_mid"):
        assert len(re.findall(r"__device__\s+__forceinline__\s+void\s+%s\s*\(" % name, src)) == 1, name
    assert src.count("ov_run_small<false>(") == 1 and src.count("ov_run_small<true>(") == 1
    assert src.count("ov_run_mid<false>(") == 1 and src.count("ov_run_mid<true>(") == 1
    assert src.count("ov_decide(P, &S,") == 2                       # the two evaluation loops, written once each


def test_multi_block_family_undecidable_cap_and_status_mix():
    """five blocks that share six variables, 9 flavours x 2 seeds: 540 jobs against the restatement"""
    assert KA.MULTI_BLOCKS == [(3, 1), (17, 3), (64, 6), (65, 6), (128, 12)] and KA.MULTI_M == 6
    total = und = 0
    mix = [set() for _ in KA.MULTI_BLOCKS]
    for fl, sd, blocks, lb, ub, refs in KA.multi_instances():
        assert [A.shape for A in blocks] == [(7, n, n) for n, _ in KA.MULTI_BLOCKS] and len(lb) == len(ub) == 6
        # the bounds are shared and drawn once; the variables' matrices are those of the one-block family
        rng = np.random.default_rng([6, sd, 77])
        assert np.array_equal(ub, rng.uniform(0.5, 2.0, 6))
        for b, (n, rank) in enumerate(KA.MULTI_BLOCKS):
            ref_a = K.family(n, 6, rank, sd, 0.0, 0.0, fl[2])[0]
            assert np.array_equal(blocks[b][1:], ref_a[1:])
            E = np.random.default_rng([n, 6, sd, 5]).standard_normal((n, n))
            A0 = fl[0] * np.tensordot(ub, ref_a[1:], axes=1) + fl[1] * 0.5 * (E + E.T)
            assert np.allclose(blocks[b][0], 0.5 * (A0 + A0.T), rtol=0.0, atol=1e-13)
            for r in refs[b]:
                total += 1
                und += 0 if K.decidable(K.NEWTON, r[5]) else 1
                mix[b].add(r[0])
                assert r[4] <= 13
    assert total == 540
    assert und <= K.UNDECIDABLE_CAP * total, (und, total)
    for b in range(len(mix)):
        assert mix[b] == {K.LB, K.INNER, K.INFEASIBLE}, (b, mix[b])
    print("%d of %d jobs undecidable" % (und, total))


def test_extremes_restated():
    """lambda_min and lambda_max of A_i alone by numpy.linalg.eigvalsh: the family's A_i are positive definite (allmatricespsd holds)
    except the last variable of the indefinite flavour; a zero matrix has both at 0; one row is the entry itself"""
    blocks, lb, ub, refs = KA.multi_instance(K.FLAVOURS[1], 1)
    for A in blocks:
        for i in range(KA.MULTI_M):
            lo, hi = KA.extremes_ref(A[i + 1])
            w = np.linalg.eigvalsh(A[i + 1])
            assert lo == w[0] and hi == w[-1] and 0.02 <= lo <= hi
    blocks, lb, ub, refs = KA.multi_instance(K.FLAVOURS[6], 2)
    for A in blocks:
        assert KA.extremes_ref(A[KA.MULTI_M])[0] < 0.0 < KA.extremes_ref(A[KA.MULTI_M])[1]
        assert all(KA.extremes_ref(A[i + 1])[0] > 0.0 for i in range(KA.MULTI_M - 1))
    assert KA.extremes_ref(np.zeros((17, 17))) == (0.0, 0.0)
    assert KA.extremes_ref(np.array([[-0.25]])) == (-0.25, -0.25)
    assert KA.extremes_ref(np.diag([3.0, -1.0, 2.0])) == (-1.0, 3.0)
