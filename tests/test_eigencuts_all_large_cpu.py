"""CPU: hipsdp_eigencuts_all_large - the C ABI, the library and the binding carry the call, its stats and (units library only) the unit
entry of the batched selection; every argument error is refused before a device is looked at; the cases of tests/harness/
eigencuts_all_large_cases.py keep the margins that make counts and vectors comparable; the launch formula of the header is the host
function hs_ecl_launches; the chunk layout (hs_ecl_layout_make, hs_ecl_block_make) and the chunks of hs_chunk_end run clean in a
stand-alone program under AddressSanitizer + UBSan.  What needs a shaped solver is checked in tests/test_gpu_eigencuts_all_large.py."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess
import numpy as np
import pytest
from conftest import ROOT
import host_check
import eigencuts_all_large_cases as E

PKG = os.path.join(ROOT, "scip-sdp_amd")
ERR_ARG = 3


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_call_is_declared_and_bound():
    hdr, units = _read("include", "hipsdp.h"), _read("include", "hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_eigencuts_all_large\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*double\s+tol\s*,\s*int\s+maxcuts\s*,\s*int\s*\*\s*ncuts\s*,\s*double\s*\*\s*lmin\s*,\s*double\s*\*\s*eigvals\s*,"
                     r"\s*double\s*\*\s*coefs\s*,\s*double\s*\*\s*lhs\s*,\s*double\s*\*\s*vecs\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_eigencuts_all_large_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert re.search(r"#define\s+HIPSDP_EIGENCUTS_LARGE_MAXN\s+512\b", hdr) and re.search(r"#define\s+HIPSDP_EIGENCUTS_LARGE_MAXCUTS\s+32\b", hdr)
    assert not re.search(r"HIPSDP_API[^;]*\bhipsdp_eigencuts_all_large(_stats)?\s*\(", units)          # the product call is not a unit entry
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_syevx_many_below_unit\s*\(\s*int\s+device\s*,\s*int\s+count\s*,\s*const\s+int\s*\*\s*n\s*,"
                     r"\s*const\s+double\s*\*\s*A\s*,\s*double\s+bound\s*,\s*int\s+maxk\s*,\s*int\s+cap\s*,\s*int\s*\*\s*cnt\s*,"
                     r"\s*double\s*\*\s*lam\s*,\s*double\s*\*\s*V\s*\)", units)
    assert "hipsdp_syevx_many_below_unit" not in hdr
    spec = importlib.util.spec_from_file_location("hipsdp_binding_eigencuts_all_large", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert list(inspect.signature(mod.Solver.eigencuts_all_large).parameters) == ["self", "y", "tol", "maxcuts"]
    assert callable(mod.eigencuts_all_large_stats) and callable(mod.Solver.eigencuts_all_large_stats)
    assert list(inspect.signature(mod.syevx_many_below_unit).parameters) == ["mats", "bound", "maxk", "cap", "device"]


def test_the_libraries_export_the_calls(hb):
    lib, ulib = hb.lib(), hb.ulib()
    assert hasattr(lib, "hipsdp_eigencuts_all_large") and hasattr(lib, "hipsdp_eigencuts_all_large_stats")
    # the unit entry is in the units library alone
    assert hasattr(ulib, "hipsdp_syevx_many_below_unit") and not hasattr(lib, "hipsdp_syevx_many_below_unit")


def test_argument_errors_and_the_totals_without_a_device(hb):
    """no device is looked at: every error of the list returns HIPSDP_ERR_ARG, ncuts stays, the totals stay (without a device `solver
    NULL` stands in front of every other error; with a solver they are checked in tests/test_gpu_eigencuts_all_large.py)"""
    lib = hb.lib()
    f = lib.hipsdp_eigencuts_all_large
    assert hb.eigencuts_all_large_stats() == hb.Solver.eigencuts_all_large_stats()
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_eigencuts_all_large_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_eigencuts_all_large_stats(None, None, None) == 0
    y = (C.c_double * 2)(0.0, 0.0)
    buf = (C.c_double * 64)()
    k = (C.c_int * 2)(77, 77)
    tol = C.c_double(1e-6)
    calls = [
        (None, None, 5, None, None, None, None, None, None),
        (None, None, 5, k, None, buf, buf, buf, None),                   # y
        (None, y, 5, None, None, buf, buf, buf, None),                   # ncuts
        (None, y, -1, k, None, buf, buf, buf, None),                     # maxcuts < 0
        (None, y, 33, k, None, buf, buf, buf, None),                     # maxcuts > 32
        (None, y, 5, k, None, None, buf, buf, None),                     # maxcuts > 0, eigvals
        (None, y, 5, k, None, buf, None, buf, None),                     # coefs
        (None, y, 5, k, None, buf, buf, None, None),                     # lhs
        (None, y, 0, k, None, None, None, None, None),                   # (no solver)
        (None, y, 5, k, buf, buf, buf, buf, buf),
    ]
    for a in calls:
        assert f(a[0], a[1], tol, a[2], *a[3:]) == ERR_ARG, a
    assert list(k) == [77, 77]
    assert hb.eigencuts_all_large_stats() == (c.value, l.value, r.value)
    # the order in the source: the argument checks stand in front of the first look at the device
    src = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    body = src[src.index("int eigencuts_all_large_impl("):src.index('extern "C" int hipsdp_eigencuts_all_stats(')]
    assert body.count("return HIPSDP_ERR_ARG") == 2 and "HIPSDP_EIGENCUTS_LARGE_MAXCUTS" in body
    # large_served is the first function that touches the device (hs_solver_cut_enter_large)
    served = src[src.index("int large_served("):src.index("struct LargeRun")]
    assert "hs_solver_cut_enter_large(" in served and body.count("hs_solver_cut_") == 0
    assert body.rindex("return HIPSDP_ERR_ARG") < body.index("d.ncuts[b] = -1") < body.index("large_served(") < body.index("ecl_chunk(")


@pytest.mark.parametrize("name,k,rows", E.ROWS)
def test_every_compared_block_keeps_its_margins(name, k, rows):
    """recomputed from the oracle, so that the cases cannot drift: more than 32 eigenvalues <= -tol (maxcuts 5 and 32 return exactly
    maxcuts cuts), relative gaps >= 1e-3 among the selected values and the next one (vectors defined up to sign), no eigenvalue
    within 1e-3 of -tol (counts immune to rounding), and nothing to cut at ys"""
    blocks, ys, y, b = E.family(name)
    assert blocks[k].shape == (E.M + 1, rows, rows) and k in E.large_blocks(name)
    for mc in (E.MAXCUTS, E.WIDE):
        below, gap, dist = E.margins(name, k, mc)
        print("%s block %d (%d rows) maxcuts %d: %d eigenvalues <= -tol, smallest relative gap %.2g, nearest eigenvalue to -tol %.2g"
              % (name, k, rows, mc, below, gap, dist))
        assert below > E.WIDE and gap >= E.MIN_GAP and dist >= E.MIN_TOL_DIST
        lmin, ev, co, lh, ve = E.reference(name, k, mc)
        assert len(ev) == mc and ev[0] == lmin and co.shape == (mc, E.M) and ve.shape == (mc, rows)
    ws = np.linalg.eigvalsh(E.zmat(name, k, at_ys=True))
    assert -1e-12 <= ws[0] and len(E.reference(name, k, E.MAXCUTS)[1]) == E.MAXCUTS


def test_no_block_is_left_out_and_the_multiple_case_is_multiple():
    assert E.large_blocks("f3") == [1, 3] and [A.shape[1] for A in E.family("f3")[0]] == [16, 150, 48, 200, 10]
    assert set((f, k) for f, k, n in E.ROWS) == {(f, k) for f in E.FAMILIES for k in E.large_blocks(f)}
    blocks, y, b, W, ev = E.multiple_case()
    assert blocks[0].shape == (2, 129, 129) and len(y) == 1 and y[0] == 0.0
    assert np.array_equal(np.tensordot(y, blocks[0][1:], axes=(0, 0)) - blocks[0][0], W)
    assert np.sum(np.abs(ev + 0.01) <= 1e-12) == 129 - 12 and ev[117] > 0.0


def test_the_family_of_the_chunk_tests_has_three_large_blocks_with_five_cuts_each():
    """f4: rows 130, 12, 129, 131; every large block has at least maxcuts = 5 eigenvalues <= -tol (the oracle returns 5 cuts), so every
    chunk of the chunk test copies out full lists"""
    blocks, ys, y, b = E.family(E.CHUNKED)
    assert [A.shape[1] for A in blocks] == [130, 12, 129, 131] and E.large_blocks(E.CHUNKED) == [0, 2, 3]
    for k in E.large_blocks(E.CHUNKED):
        below = int(np.sum(E.spectrum(E.CHUNKED, k) <= -E.TOL))
        lmin, ev, co, lh, ve = E.reference(E.CHUNKED, k, E.MAXCUTS)
        print("f4 block %d: %d eigenvalues <= -tol, %d cuts" % (k, below, len(ev)))
        assert below >= E.MAXCUTS == 5 and len(ev) == E.MAXCUTS and np.all(ev <= -E.TOL)


def test_the_launch_formula_of_the_header_is_the_host_function(tmp_path):
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"2 \+ \(nmax - 1\) \+ 1 \+ 2 \[maxcuts > 0\] \+ 1\s+=\s+nmax \+ 3 \+ 2 \[maxcuts > 0\]", hdr)
    prog = tmp_path / "launches.cpp"
    prog.write_text('#include "hs_cut_plan.h"\n#include <stdio.h>\nint main(void)\n{\n'
                    '   for (int mc = 0; mc <= 32; ++mc) for (int n = 129; n <= 512; ++n)\n'
                    '      if ( n == 129 || n == 200 || n == 512 ) printf("%d %d %lld\\n", mc, n, hs_ecl_launches(mc, n));\n'
                    '   return 0;\n}\n')
    exe = str(tmp_path / "launches")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(prog), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split("\n")
    seen = 0
    for line in out:
        if not line:
            continue
        mc, n, got = (int(t) for t in line.split())
        assert got == 2 + (n - 1) + 1 + (2 if mc > 0 else 0) + 1 <= n + 6, line
        seen += 1
    assert seen == 33 * 3


def test_layout_and_chunks_run_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/cut_plan_ecl_check.cpp + csrc/hs_cut_plan.cpp, host compiler,
    -fsanitize=address,undefined: a program of its own with the runtimes linked in (nothing is loaded into python, nothing is
    preloaded)"""
    host_check.run_clean(tmp_path, "cut_plan_ecl_check.cpp", ["hs_cut_plan.cpp"], "cut plan ecl check: ok")


def test_the_sources_are_where_the_build_expects_them_and_share_the_sweep():
    mk = _read("scip-sdp_amd", "Makefile")
    assert "csrc/eigcuts_large.hip" in mk and "csrc/hs_ec_sweep.h" in mk
    sweep = _read("scip-sdp_amd", "csrc", "hs_ec_sweep.h")
    # one body of the sweep and of its reduction; the kernel of the small blocks and the kernel of the large ones call it
    for name in ("ec_sweep", "ec_sweep_store"):
        assert len(re.findall(r"__device__\s+__forceinline__\s+void\s+%s\s*\(" % name, sweep)) == 1, name
    small, large = _read("scip-sdp_amd", "csrc", "eigcuts.hip"), _read("scip-sdp_amd", "csrc", "eigcuts_large.hip")
    for text in (small, large):
        assert '#include "hs_ec_sweep.h"' in text and "ec_sweep_store(" in text and "ec_sweep<" not in text
    for name in ("k_ecl_clear", "k_ecl_cuts"):
        assert re.search(r"__global__\s+void\s+__launch_bounds__\(\w+\)\s+%s\s*\(" % name, large), name
    # the hazard rule: the kernel boundary is the only synchronisation between workgroups; no floating-point atomics
    for text in (sweep, large):
        assert "cooperative" not in text.lower() and "grid.sync" not in text and not re.search(r"atomic\w*\s*\(", text)
    # the batched selection wraps the device bodies of the single matrix
    sx = _read("scip-sdp_amd", "csrc", "syevx.hip")
    assert '#include "hs_syevx_below_many.h"' in sx and "csrc/hs_syevx_below_many.h" in mk
    wr = _read("scip-sdp_amd", "csrc", "hs_syevx_below_many.h")
    for name, body in (("k_syevx_values_below_many", "d_syevx_values("), ("k_syevx_tvec_below_many", "d_syevx_tvec("),
                       ("k_syevx_back_below_many", "d_syevx_back(")):
        at = wr.index(name + "(")
        assert "__global__ void __launch_bounds__" in wr[wr.rindex("\n", 0, at):at] and body in wr[at:wr.index("\n}\n", at)], name
    for name in ("d_syevx_values", "d_syevx_tvec", "d_syevx_back"):
        assert len(re.findall(r"__device__\s+__forceinline__\s+void\s+%s\s*\(" % name, sx)) == 1, name
    host = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    assert 'hs_chunk_env("HIPSDP_EIGENCUTS_LARGE_CHUNK")' in host and "hs_ecl_layout_make(" in host and "hs_chunks_run(" in host
    chunks = _read("scip-sdp_amd", "csrc", "hs_chunks.h")
    assert "int hs_chunk_end(" in chunks and "hs_chunk_end(" in chunks[chunks.index("hs_chunks_run("):]
    plan = _read("scip-sdp_amd", "csrc", "hs_cut_plan.h")
    assert "hs_ecl_layout_make" in plan and "hs_ecl_block_make" in plan and "hs_ecl_launches" in plan
