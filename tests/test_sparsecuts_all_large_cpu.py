"""CPU: hipsdp_sparsecuts_all_large - the C ABI, the library and the binding carry the call and its stats; every argument error is
refused before a device is looked at; the cases of tests/harness/sparsecuts_all_large_cases.py are stable in the numpy restatement
(so that the GPU tests may compare counts, supports and iteration numbers); the launch formula of the header is the host function
hs_sclr_launches; the chunk layout (hs_sclr_layout_make, hs_sclr_block_make) and the chunks of hs_chunk_end run clean in a
stand-alone program under AddressSanitizer + UBSan.  What needs a shaped solver is checked in tests/test_gpu_sparsecuts_all_large.py."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import subprocess
import pytest
from conftest import ROOT
import host_check
import sparsecuts_all_large_cases as L

PKG = os.path.join(ROOT, "scip-sdp_amd")
ERR_ARG = 3


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_call_is_declared_and_bound():
    hdr, units = _read("include", "hipsdp.h"), _read("include", "hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_all_large\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*const\s+int\s*\*\s*sizes\s*,\s*const\s+hipsdp_sparsecut_opts\s*\*\s*opts\s*,\s*unsigned\s+variant\s*,"
                     r"\s*int\s*\*\s*ncuts\s*,\s*double\s*\*\s*lmin\s*,\s*double\s*\*\s*eigvals\s*,\s*double\s*\*\s*coefs\s*,"
                     r"\s*double\s*\*\s*lhs\s*,\s*double\s*\*\s*vecs\s*,\s*int\s*\*\s*iters\s*,\s*int\s*\*\s*flags\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparsecuts_all_large_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert "hipsdp_sparsecuts_all_large" not in units
    # the limit is stated where the caller reads it, and the _ex call points here
    assert re.search(r"sizes\[b\] exceeds 128 while HIPSDP_SC_RECOMPUTE_SPARSEEV is set", hdr)
    assert "keep the host loop for such a" not in hdr and hdr.count("hipsdp_sparsecuts_all_large") >= 4
    spec = importlib.util.spec_from_file_location("hipsdp_binding_sparsecuts_all_large", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = inspect.signature(mod.Solver.sparsecuts_all_large).parameters
    assert list(p) == ["self", "y", "sizes", "tol", "feastol", "maxcuts", "variant", "convtol", "maxit"]
    assert [p[k].default for k in ("convtol", "maxit")] == [0, 0]
    assert callable(mod.sparsecuts_all_large_stats) and callable(mod.Solver.sparsecuts_all_large_stats)


def test_the_library_exports_the_calls(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_sparsecuts_all_large") and hasattr(lib, "hipsdp_sparsecuts_all_large_stats")


def test_argument_errors_and_the_totals_without_a_device(hb):
    """no device is looked at: every error of the list returns HIPSDP_ERR_ARG, ncuts stays, the totals stay (without a device `solver
    NULL` stands in front of every other error; with a solver they are checked in tests/test_gpu_sparsecuts_all_large.py)"""
    lib = hb.lib()
    f = lib.hipsdp_sparsecuts_all_large
    assert hb.sparsecuts_all_large_stats() == hb.Solver.sparsecuts_all_large_stats()
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_sparsecuts_all_large_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_sparsecuts_all_large_stats(None, None, None) == 0
    opts, neg, zero = hb.SparsecutOpts(1e-6, 1e-6, 0.0, 5, 0), hb.SparsecutOpts(1e-6, 1e-6, 0.0, -1, 0), hb.SparsecutOpts(1e-6, 1e-6, 0.0, 0, 0)
    o = C.byref(opts)
    y = (C.c_double * 2)(0.0, 0.0)
    buf = (C.c_double * 64)()
    sizes = (C.c_int * 2)(4, 4)
    k = (C.c_int * 2)(77, 77)
    calls = [
        (None, None, None, None, 0, None, None, None, None, None, None, None, None),
        (None, None, sizes, o, 0, k, None, buf, buf, buf, None, None, None),                    # y
        (None, y, None, o, 0, k, None, buf, buf, buf, None, None, None),                       # sizes
        (None, y, sizes, None, 0, k, None, buf, buf, buf, None, None, None),                   # opts
        (None, y, sizes, o, 0, None, None, buf, buf, buf, None, None, None),                   # ncuts
        (None, y, sizes, C.byref(neg), 0, k, None, buf, buf, buf, None, None, None),           # maxcuts < 0
        (None, y, sizes, o, 0, k, None, None, buf, buf, None, None, None),                     # maxcuts > 0, eigvals
        (None, y, sizes, o, 0, k, None, buf, None, buf, None, None, None),                     # coefs
        (None, y, sizes, o, 0, k, None, buf, buf, None, None, None, None),                     # lhs
        (None, y, sizes, o, 8, k, None, buf, buf, buf, None, None, None),                      # variant 8
        (None, y, sizes, C.byref(zero), 9, k, None, None, None, None, None, None, None),
        (None, y, sizes, o, 7, k, None, buf, buf, buf, None, None, None),                      # (a solver without a shape)
    ]
    for a in calls:
        assert f(a[0], a[1], a[2], a[3], C.c_uint(a[4]), *a[5:]) == ERR_ARG, a
    assert list(k) == [77, 77]
    assert hb.sparsecuts_all_large_stats() == (c.value, l.value, r.value)
    # the order in the source: the argument checks stand in front of the first look at the device
    src = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    entry = src[src.index('extern "C" int hipsdp_sparsecuts_all_large('):]
    assert entry.index("variant_ok(variant)") < entry.index("sparsecuts_all_large_impl(")
    body = src[src.index("int sparsecuts_all_large_impl("):src.index("/* hipsdp_sparsecuts (variant = 0, booked under g_sc1)")]
    # the three argument errors are those of sc_all_args, which writes nothing and looks at no device ...
    args = src[src.index("int sc_all_args("):src.index("/* hipsdp_sparsecuts_all (variant = 0)")]
    assert args.count("return HIPSDP_ERR_ARG") == 3 and "ncuts[" not in args and "hs_solver_cut_" not in args and "HS_HIP" not in args
    # ... large_served is the first function that touches the device (hs_solver_cut_enter_large), and behind it nothing is an argument error
    served = src[src.index("int large_served("):src.index("struct LargeRun")]
    assert "hs_solver_cut_enter_large(" in served and body.count("hs_solver_cut_") == 0
    assert body.index("sc_all_args(") < body.index("d.ncuts[b] = -1") < body.index("large_served(") < body.index("sclr_chunk(")
    assert "return HIPSDP_ERR_ARG" not in body
    # the partner for the blocks of at most 128 rows checks its arguments through the same function, in the same place
    small = src[src.index("int sparsecuts_all_impl("):src.index("/* a block of at most 128 rows")]
    assert small.index("sc_all_args(") < small.index("d.ncuts[b] = -1") < small.index("hs_solver_cut_enter(") and "return HIPSDP_ERR_ARG" not in small


@pytest.mark.parametrize("name,k,size,variant", L.CASES + L.CASES0)
def test_every_compared_case_is_stable_in_the_restatement(name, k, size, variant):
    got = L.check_margins(name, k, size, variant)
    r = L.reference(name, k, size, variant)
    print("%s block %d size %d variant %d: %d cuts, %d iterations; margins select %.3g conv %.3g feas %.3g sub_gap %.3g defl_gap %.3g tol %.3g"
          % ((name, k, size, variant, r[0], r[7]) + got))
    assert r[8] == 0 and r[1] < -L.TOL
    assert 128 < L.family(name)[0][k].shape[1] <= 512


def test_no_block_is_left_out_and_the_quiet_block_is_quiet():
    assert L.large_blocks("f3") == [1, 3] and [A.shape[1] for A in L.family("f3")[0]] == [16, 150, 48, 200, 10]
    for name, (n, seed) in L.SINGLES.items():
        blocks, ys, y, b = L.family(name)
        assert len(blocks) == 1 and blocks[0].shape == (L.M + 1, n, n) and L.large_blocks(name) == [0]
    rows = set((f, k) for f, k, sz in L.ROWS)
    assert rows == {("f3", 1), ("f3", 3), ("n129", 0), ("n257", 0), ("n512", 0)}
    for f, k, sz in L.ROWS:
        for v in L.SWITCHED:
            assert (f, k, sz, v) in L.CASES
    assert sorted(c[3] for c in L.CASES if c[:3] == ("n129", 0, 4)) == [1, 2, 3, 4, 5, 6, 7]
    # the 200-row block at size 4: the loop ends at once under every mask, after the same run
    for v in (0, 1, 2, 4, 7):
        r = L.reference(*L.QUIET, v)
        assert (r[0], r[7], r[8]) == (0, 73, 0)
    # every compared row cuts under every mask (nothing is compared on empty lists alone)
    for c in L.CASES + L.CASES0:
        assert L.reference(*c)[0] >= 1, c


def test_the_family_of_the_chunk_tests_has_three_large_blocks_that_all_cut():
    """f4: rows 130, 12, 129, 131, so the served order 3, 0, 2 is not the index order; every large block gives at least one cut at the
    size and the masks of the chunk test (the restatement), so that no chunk copies out empty lists alone"""
    blocks, ys, y, b = L.family(L.CHUNKED)
    assert [A.shape[1] for A in blocks] == [130, 12, 129, 131] and len(y) == L.M and L.large_blocks(L.CHUNKED) == [0, 2, 3]
    assert (L.CHUNKED_SIZE, L.CHUNKED_MASKS) == (4, (0, 7))
    for k in L.large_blocks(L.CHUNKED):
        for v in L.CHUNKED_MASKS:
            r = L.reference(L.CHUNKED, k, L.CHUNKED_SIZE, v)
            print("f4 block %d variant %d: %d cuts, %d iterations" % (k, v, r[0], r[7]))
            assert r[0] >= 1, (k, v)


def test_the_launch_formula_of_the_header_is_the_host_function(tmp_path):
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"1 \+ \(nmax \+ 3\) \+ r \(1 \+ 4 s \+ d \(nmax \+ 3\)\) \+ 1 \+ \[maxcuts > 0\],\s+r = maxcuts with variant != 0, r = 0 with variant == 0", hdr)
    prog = tmp_path / "launches.cpp"
    prog.write_text('#include "hs_cut_plan.h"\n#include <stdio.h>\nint main(void)\n{\n'
                    '   for (unsigned v = 0; v < 8; ++v) for (int mc = 0; mc <= 5; ++mc) for (int n = 129; n <= 512; ++n)\n'
                    '      if ( n == 129 || n == 200 || n == 512 ) printf("%u %d %d %lld\\n", v, mc, n, hs_sclr_launches(v, mc, n));\n'
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
        v, mc, n, got = (int(t) for t in line.split())
        s, d = int(bool(v & 1)), int(bool(v & 6))
        rounds = mc if v != 0 else 0
        assert got == 1 + (n + 3) + rounds * (1 + 4 * s + d * (n + 3)) + 1 + (1 if mc > 0 else 0), line
        seen += 1
    assert seen == 8 * 6 * 3


def test_layout_and_chunks_run_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/cut_plan_large_check.cpp + csrc/hs_cut_plan.cpp, host compiler,
    -fsanitize=address,undefined: a program of its own with the runtimes linked in (nothing is loaded into python, nothing is
    preloaded)"""
    host_check.run_clean(tmp_path, "cut_plan_large_check.cpp", ["hs_cut_plan.cpp"], "cut plan large check: ok")


def test_the_sources_are_where_the_build_expects_them_and_share_their_bodies():
    mk = _read("scip-sdp_amd", "Makefile")
    assert "csrc/sparsecuts_large_rounds.hip" in mk and "csrc/hs_scl_tpower.h" in mk
    body = _read("scip-sdp_amd", "csrc", "hs_scl_tpower.h")
    # one body of the TPower run, of the loop and of the coefficients; the one-block kernels and the many-block kernels call them
    for name in ("scl_tpower_run", "scl_tpower_loop", "scl_coefs_block"):
        assert len(re.findall(r"__device__\s+__forceinline__\s+\w+\s+%s\s*\(" % name, body)) == 1, name
    one, many = _read("scip-sdp_amd", "csrc", "sparsecuts_large.hip"), _read("scip-sdp_amd", "csrc", "sparsecuts_large_rounds.hip")
    assert "scl_tpower_loop(" in one and "scl_coefs_block(" in one
    assert "scl_tpower_loop(" in many and "scl_tpower_run(" in many and "scl_coefs_block(" in many
    for name in ("k_sclr_stage", "k_sclr_tpower_all", "k_sclr_tpower", "k_sclr_cut", "k_sclr_coefs"):
        assert re.search(r"__global__\s+void\s+__launch_bounds__\(\w+\)\s+%s\s*\(" % name, many), name
    # the hazard rule: the kernel boundary is the only synchronisation between workgroups
    for text in (body, many):
        assert "cooperative" not in text.lower() and "grid.sync" not in text and not re.search(r"atomic\w*\s*\(", text)
    host = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    assert 'hs_chunk_env("HIPSDP_SPARSECUTS_LARGE_CHUNK")' in host and "hs_sclr_layout_make(" in host and "hs_chunks_run(" in host
    chunks = _read("scip-sdp_amd", "csrc", "hs_chunks.h")
    assert "int hs_chunk_end(" in chunks and "hs_chunk_end(" in chunks[chunks.index("hs_chunks_run("):] and "#include <hip" not in chunks and "hip_runtime" not in chunks
    # one tail: neither chunk function reads back on its own
    for name, end in (("int sclr_chunk(", "int sparsecuts_all_large_impl("), ("int ecl_chunk(", "int eigencuts_all_large_impl(")):
        fn = host[host.index(name):host.index(end)]
        assert "DeviceToHost" not in fn and "large_begin(" in fn and "large_end(" in fn, name
    assert "getenv" not in host
    plan = _read("scip-sdp_amd", "csrc", "hs_cut_plan.h")
    assert "hs_sclr_layout_make" in plan and "hs_sclr_block_make" in plan and "hs_sclr_launches" in plan
