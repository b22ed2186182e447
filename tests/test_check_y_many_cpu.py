"""CPU: hipsdp_check_y_many - the C ABI, the product library and the binding carry the call and its stats, the two unit entries live in
the units library alone, every argument error is refused before a device is looked at, the launch formula of the header is the host
function hs_cm_launches, and the rounding harness (tests/harness/rounding.py) follows the rule of heur_sdprand.c:335-359 on a
hand-written case.  What needs a shaped solver is checked in tests/test_gpu_check_y_many.py."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess
import numpy as np
from conftest import ROOT
import rounding

PKG = os.path.join(ROOT, "scip-sdp_amd")
ERR_ARG = 3


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_header_declares_both_signatures():
    hdr, units = _read("include", "hipsdp.h"), _read("include", "hipsdp_units.h")
    hdr_nc = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_check_y_many\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+count\s*,\s*const\s+double\s*\*\s*Y\s*,"
                     r"\s*double\s*\*\s*lmin\s*,\s*double\s*\*\s*lpviol\s*,\s*int\s*\*\s*served\s*\)", hdr_nc)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_check_y_many_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr_nc)
    assert not re.search(r"HIPSDP_API[^;]*\bhipsdp_check_y_many(_stats)?\s*\(", units)             # the product call is not a unit entry
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_form_z_many_unit\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+count\s*,\s*const\s+double\s*\*\s*Y\s*,"
                     r"\s*double\s*\*\s*Z\s*,\s*int\s*\*\s*served\s*,\s*int\s*\*\s*launches\s*\)", units)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_check_many_group\s*\(\s*void\s*\)", units)
    assert "hipsdp_form_z_many_unit" not in hdr and "hipsdp_check_many_group" not in hdr


def test_the_product_library_exports_the_call_and_the_units_library_the_unit_entries(hb):
    lib, ulib = hb.lib(), hb.ulib()
    assert hasattr(lib, "hipsdp_check_y_many") and hasattr(lib, "hipsdp_check_y_many_stats")
    for name in ("hipsdp_form_z_many_unit", "hipsdp_check_many_group"):
        assert hasattr(ulib, name) and not hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libhipsdp.so")], stdout=subprocess.PIPE, text=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert {"hipsdp_check_y_many", "hipsdp_check_y_many_stats"} <= names
    assert not {"hipsdp_form_z_many_unit", "hipsdp_check_many_group"} & names
    # the group is a compile-time constant the tests stand on: small enough for the register budget, more than one candidate per pass
    G = hb.check_many_group()
    assert 2 <= G <= 32 and re.search(r"#define\s+HS_CM_G\s+%d\b" % G, _read("scip-sdp_amd", "csrc", "hs_kernels.h"))


def test_the_binding_has_the_wrappers():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_check_y_many", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert list(inspect.signature(mod.Solver.check_y_many).parameters)[:2] == ["self", "Y"]
    assert list(inspect.signature(mod.Solver.form_z_many_unit).parameters) == ["self", "Y"]
    assert callable(mod.Solver.check_y_many_stats) and callable(mod.check_y_many_stats) and callable(mod.check_many_group)


def test_argument_errors_and_the_totals_without_a_device(hb):
    """no device is looked at: with a NULL solver every call of the list returns HIPSDP_ERR_ARG and writes nothing, _stats takes NULL
    pointers and works before any call, and the totals stay (with a solver the errors are checked in tests/test_gpu_check_y_many.py)"""
    lib = hb.lib()
    f = lib.hipsdp_check_y_many
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_check_y_many_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_check_y_many_stats(None, None, None) == 0
    assert lib.hipsdp_check_y_many_stats(None, C.byref(l), None) == 0
    assert hb.check_y_many_stats() == (c.value, l.value, r.value)
    Y = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    lm = (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    lp = (C.c_double * 2)(7.0, 7.0)
    sv = (C.c_int * 2)(77, 77)
    for a in [(None, 2, Y, lm, lp, sv), (None, -1, Y, lm, lp, sv), (None, 2, None, lm, lp, sv), (None, 2, Y, None, lp, sv),
              (None, 0, None, None, None, None), (None, 1, Y, lm, None, None)]:
        assert f(*a) == ERR_ARG, a
    assert list(lm) == [7.0] * 4 and list(lp) == [7.0] * 2 and list(sv) == [77, 77]
    assert hb.check_y_many_stats() == (c.value, l.value, r.value)
    # the order in the source: the argument checks stand in front of the first look at the device
    src = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    body = src[src.index("int check_y_many_impl("):src.index("int hs_check_many_form_z(")]
    assert body.count("return HIPSDP_ERR_ARG") == 1
    assert body.index("return HIPSDP_ERR_ARG") < body.index("cm_enter(") < body.index("cm_chunk(")
    # ... and the shared entry of the calls over candidate points looks at the device, in this order, and refuses nothing
    entry = src[src.index("int cm_enter("):src.index("long long cm_candidate_len(")]
    assert entry.index("hs_solver_lp_rows(") < entry.index("cm_served(")
    assert "return HIPSDP_ERR_ARG" not in entry and "getenv" not in entry
    assert 'hs_chunk_env("HIPSDP_CHECK_MANY_CHUNK")' in body and "hs_chunks_run(" in body


def test_the_launch_formula_of_the_header_is_the_host_function(tmp_path):
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"\[any block\] \+ \[1 \.\. 64 rows\] \+ \[65 \.\. 128 rows\] \+ \[129 \.\. 512 rows\] \(nmax \+ 3\) \+ 1", hdr)
    prog = tmp_path / "launches.cpp"
    prog.write_text('#include "hs_cut_plan.h"\n#include <stdio.h>\nint main(void)\n{\n'
                    '   for (int s = 0; s < 2; ++s) for (int m = 0; m < 2; ++m) for (int n = 0; n <= 512; n += (n == 0 ? 129 : 383))\n'
                    '      printf("%d %d %d %lld\\n", s, m, n, hs_cm_launches(s || m || n, s, m, n));\n'
                    '   return 0;\n}\n')
    exe = str(tmp_path / "launches")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(prog), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    seen = 0
    for line in subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split("\n"):
        if not line:
            continue
        s, m, n, got = (int(t) for t in line.split())
        assert got == (1 if s or m or n else 0) + s + m + (n + 3 if n else 0) + 1, line
        seen += 1
    assert seen == 12


def test_the_kernel_file_is_built_and_keeps_the_hazard_rule():
    mk = _read("scip-sdp_amd", "Makefile")
    assert "csrc/check_many.hip" in mk
    text = _read("scip-sdp_amd", "csrc", "check_many.hip")
    for name in ("k_cm_form_z", "k_cm_result"):
        assert re.search(r"__global__\s+void\s+__launch_bounds__\(\w+\)\s+%s\s*\(" % name, text), name
    assert "cooperative" not in text.lower() and "grid.sync" not in text and not re.search(r"atomic\w*\s*\(", text)
    # the values-only many-matrix instances are new wrappers of the shared bodies in eigi.hip
    eigi = _read("scip-sdp_amd", "csrc", "eigi.hip")
    for name, body in (("k_lmin_many_small", "d_syevi_small<false>("), ("k_lmin_many_mid", "d_syevi_mid(")):
        at = eigi.index(name + "(")
        assert body in eigi[at:eigi.index("\n}\n", at)], name


def test_the_rounding_rule_on_a_hand_written_case():
    """heur_sdprand.c:335-359 by hand: fraction 0 and 1 (within SCIP's 1e-6) never move the wrong way, a bound that leaves one direction
    decides, a domain without an integer drops the candidate, continuous variables keep their value, and frac <= r rounds down"""
    R = rounding.round_one
    assert R(0.0, 0, 1, 0.0) == 0.0 and R(1.0, 0, 1, 0.999999) == 1.0 and R(3.0, 0, 9, 0.0) == 3.0
    assert R(1e-7, 0, 1, 0.0) == 0.0 and R(1 - 1e-7, 0, 1, 0.999) == 1.0 and R(2 + 1e-7, 0, 9, 0.0) == 2.0
    assert R(0.3, 0, 1, 0.3) == 0.0 and R(0.3, 0, 1, 0.31) == 0.0 and R(0.3, 0, 1, 0.29) == 1.0          # frac <= r: down
    assert R(2.75, 0, 9, 0.5) == 3.0 and R(2.75, 0, 9, 0.8) == 2.0 and R(-1.25, -5, 5, 0.5) == -1.0 and R(-1.25, -5, 5, 0.9) == -2.0
    assert R(0.4, 1, 1, 0.99) == 1.0 and R(0.6, 0, 0, 0.0) == 0.0                                         # one direction left
    assert R(0.4, 2, 3, 0.5) is None and R(5.5, 0, 4, 0.5) is None                                        # none left
    y = np.array([0.25, 0.0, 1.0, 0.5, 0.999, 7.3])
    isint = [True, True, True, True, True, False]
    lb, ub = [0, 0, 0, 0, 0, -10], [1, 1, 1, 1, 1, 10]
    Y, keep = rounding.roundings(y, isint, lb, ub, 200, seed=5)
    assert Y.shape == (200, 6) and keep.all()
    assert np.all(Y[:, 1] == 0.0) and np.all(Y[:, 2] == 1.0) and np.all(Y[:, 5] == 7.3)
    assert np.all((Y[:, :5] == 0.0) | (Y[:, :5] == 1.0)) and np.all(Y[:, :5] >= 0) and np.all(Y[:, :5] <= 1)
    # a fixed seed: the same draws, candidate j whatever the count; the draws behind the rule, recomputed
    Y2, _ = rounding.roundings(y, isint, lb, ub, 7, seed=5)
    assert np.array_equal(Y[:7], Y2)
    d = np.random.default_rng(5).random((200, 6))
    assert np.array_equal(Y[:, 0], np.where(0.25 <= d[:, 0], 0.0, 1.0)) and np.array_equal(Y[:, 3], np.where(0.5 <= d[:, 3], 0.0, 1.0))
    ups = Y[:, [0, 3, 4]].mean(axis=0)
    assert abs(ups[0] - 0.25) < 0.1 and abs(ups[1] - 0.5) < 0.12 and ups[2] > 0.95
    # a continuous variable the relaxation left a hair outside its bounds is moved onto the bound
    Y5, _ = rounding.roundings(np.array([0.1 + 3e-7, -2e-8]), [False, False], [-1e20, 0.0], [0.1, 1.0], 2, seed=1)
    assert np.all(Y5[:, 0] == 0.1) and np.all(Y5[:, 1] == 0.0)
    # bounds decide, and an empty integer domain drops the row
    Y3, keep3 = rounding.roundings(np.array([0.5, 0.5]), [True, True], [1, 0], [1, 0], 5, seed=1)
    assert keep3.all() and np.all(Y3[:, 0] == 1.0) and np.all(Y3[:, 1] == 0.0)
    _, keep4 = rounding.roundings(np.array([0.5]), [True], [2], [3], 3, seed=1)
    assert not keep4.any()


def test_check_roundings_orders_the_feasible_rows_by_objective():
    class Fake:
        def check_y_many(self, Y):
            lmin = np.array([[0.1, 0.0], [-1e-7, 0.2], [-1e-3, 0.2], [0.3, 0.3]])
            return lmin, np.array([0.0, 1e-7, 0.0, 1e-3]), np.zeros(2, dtype=np.int32)
    Y = np.array([[3.0], [1.0], [0.0], [2.0]])
    order, lmin, lpviol = rounding.check_roundings(Fake(), Y, [1.0])
    assert order == [1, 0] and lmin.shape == (4, 2) and lpviol.shape == (4,)
    order, _, _ = rounding.check_roundings(Fake(), Y, [-1.0])
    assert order == [0, 1]
