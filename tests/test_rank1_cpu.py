"""CPU: hipsdp_rank1_check_many - the C ABI, the product library and the binding carry the call and its stats, the two unit entries live
in the units library alone, every argument error is refused before a device is looked at, the launch formula of the header is the host
function hs_r1_launches, and the numpy restatement of the two scans (tests/harness/rank1_cases.py) reproduces hand-written 3 x 3 cases,
ties included.  What needs a device is checked in tests/test_gpu_rank1.py."""
import ctypes as C
import importlib.util
import inspect
import itertools
import os
import re
import subprocess
import numpy as np
from conftest import ROOT
import rank1_cases as r1

PKG = os.path.join(ROOT, "scip-sdp_amd")
ERR_ARG = 3
PRODUCT = ("hipsdp_rank1_check_many", "hipsdp_rank1_check_many_stats", "hipsdp_rank1_approx", "hipsdp_rank1_approx_stats")
UNITS = ("hipsdp_rank1_minors_unit", "hipsdp_lsel_many_unit")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_headers_declare_the_signatures():
    hdr, units = _read("include", "hipsdp.h"), _read("include", "hipsdp_units.h")
    hdr_nc = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    units_nc = re.sub(r"/\*.*?\*/", " ", units, flags=re.S)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rank1_check_many\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+count\s*,\s*const\s+double\s*\*\s*Y\s*,"
                     r"\s*double\s+feastol\s*,\s*double\s*\*\s*lam\s*,\s*double\s*\*\s*minorev\s*,\s*int\s*\*\s*minorind\s*,"
                     r"\s*double\s*\*\s*minordet\s*,\s*int\s*\*\s*detind\s*,\s*int\s*\*\s*served\s*\)", hdr_nc)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rank1_check_many_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr_nc)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rank1_minors_unit\s*\(\s*int\s+device\s*,\s*int\s+count\s*,\s*const\s+int\s*\*\s*n\s*,"
                     r"\s*const\s+double\s*\*\s*Z\s*,\s*double\s+feastol\s*,\s*double\s*\*\s*minorev\s*,\s*int\s*\*\s*minorind\s*,"
                     r"\s*double\s*\*\s*minordet\s*,\s*int\s*\*\s*detind\s*\)", units_nc)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_lsel_many_unit\s*\(\s*int\s+device\s*,\s*int\s+count\s*,\s*const\s+int\s*\*\s*n\s*,"
                     r"\s*const\s+double\s*\*\s*Z\s*,\s*double\s*\*\s*lam\s*\)", units_nc)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rank1_approx\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*const\s+int\s*\*\s*want\s*,\s*double\s*\*\s*lmax\s*,\s*double\s*\*\s*vec\s*,\s*double\s*\*\s*rhs\s*,"
                     r"\s*int\s*\*\s*served\s*\)", hdr_nc)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_rank1_approx_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr_nc)
    for name in PRODUCT:
        assert not re.search(r"HIPSDP_API[^;]*\b%s\s*\(" % name, units_nc), name
    for name in UNITS:
        assert name not in hdr, name
    # the contract the header has to state: the closed form, the asserted-away case, the switch
    assert "h - sqrt(g g + b b)" in hdr and "asserts that case away" in hdr and "HIPSDP_RANK1_CHUNK" in hdr


def test_each_library_exports_its_own_set(hb):
    lib, ulib = hb.lib(), hb.ulib()
    for name in PRODUCT:
        assert hasattr(lib, name) and hasattr(ulib, name), name          # (the units library contains the engine)
    for name in UNITS:
        assert hasattr(ulib, name) and not hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(PKG, "lib", "libhipsdp.so")], stdout=subprocess.PIPE, text=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert set(PRODUCT) <= names and not set(UNITS) & names


def test_the_binding_has_the_wrappers():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_rank1", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert list(inspect.signature(mod.Solver.rank1_check_many).parameters)[:3] == ["self", "Y", "feastol"]
    assert callable(mod.Solver.rank1_check_many_stats) and callable(mod.rank1_check_many_stats)
    assert list(inspect.signature(mod.Solver.rank1_approx).parameters)[:3] == ["self", "y", "want"]
    assert inspect.signature(mod.Solver.rank1_approx).parameters["want"].default is None
    assert callable(mod.Solver.rank1_approx_stats) and callable(mod.rank1_approx_stats)
    assert list(inspect.signature(mod.rank1_minors_unit).parameters)[:2] == ["mats", "feastol"]
    assert list(inspect.signature(mod.lsel_many_unit).parameters)[:1] == ["mats"]


def test_argument_errors_and_the_totals_without_a_device(hb):
    """no device is looked at: with a NULL solver every call of the list returns HIPSDP_ERR_ARG and writes nothing, _stats takes NULL
    pointers and works before any call, and the totals stay"""
    lib = hb.lib()
    f = lib.hipsdp_rank1_check_many
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_rank1_check_many_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_rank1_check_many_stats(None, None, None) == 0
    assert lib.hipsdp_rank1_check_many_stats(None, C.byref(l), None) == 0
    assert hb.rank1_check_many_stats() == (c.value, l.value, r.value)
    Y = (C.c_double * 4)(0.0, 0.0, 0.0, 0.0)
    lam = (C.c_double * 12)(*([7.0] * 12))
    me, md = (C.c_double * 4)(*([7.0] * 4)), (C.c_double * 4)(*([7.0] * 4))
    mi, di = (C.c_int * 8)(*([77] * 8)), (C.c_int * 8)(*([77] * 8))
    sv = (C.c_int * 2)(77, 77)
    tol = C.c_double(1e-6)
    for a in [(None, 2, Y, tol, lam, me, mi, md, di, sv), (None, -1, Y, tol, lam, me, mi, md, di, sv),
              (None, 2, None, tol, lam, me, mi, md, di, sv), (None, 2, Y, tol, None, me, mi, md, di, sv),
              (None, 2, Y, C.c_double(-1.0), lam, me, mi, md, di, sv), (None, 2, Y, C.c_double(float("nan")), lam, me, mi, md, di, sv),
              (None, 2, Y, tol, lam, me, None, md, di, sv), (None, 2, Y, tol, lam, me, mi, None, di, sv),
              (None, 0, None, tol, None, None, None, None, None, None), (None, 1, Y, tol, lam, None, None, None, None, None)]:
        assert f(*a) == ERR_ARG, a
    assert list(lam) == [7.0] * 12 and list(me) == [7.0] * 4 and list(md) == [7.0] * 4
    assert list(mi) == [77] * 8 and list(di) == [77] * 8 and list(sv) == [77, 77]
    assert hb.rank1_check_many_stats() == (c.value, l.value, r.value)
    # the order in the source: the argument checks stand in front of the first look at the device
    src = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    body = src[src.index("int rank1_check_many_impl("):src.index('extern "C" int hipsdp_rank1_check_many(')]
    assert body.count("return HIPSDP_ERR_ARG") == 1
    assert body.index("return HIPSDP_ERR_ARG") < body.index("cm_enter(") < body.index("r1_chunk(")
    # ... and the shared entry of the calls over candidate points looks at the device, in this order, and refuses nothing
    entry = src[src.index("int cm_enter("):src.index("long long cm_candidate_len(")]
    assert entry.index("hs_solver_lp_rows(") < entry.index("cm_served(")
    assert "return HIPSDP_ERR_ARG" not in entry and "getenv" not in entry
    assert 'hs_chunk_env("HIPSDP_RANK1_CHUNK")' in body and "hs_chunks_run(" in body
    # hipsdp_rank1_approx
    g = lib.hipsdp_rank1_approx
    a0 = hb.rank1_approx_stats()
    assert lib.hipsdp_rank1_approx_stats(None, None, None) == 0
    wt = (C.c_int * 2)(1, 1)
    for a in [(None, Y, wt, me, lam, md, sv), (None, None, wt, me, lam, md, sv), (None, Y, None, None, lam, md, sv),
              (None, Y, None, me, None, md, sv), (None, Y, None, me, lam, None, None)]:
        assert g(*a) == ERR_ARG, a
    assert list(lam) == [7.0] * 12 and list(me) == [7.0] * 4 and list(md) == [7.0] * 4 and list(sv) == [77, 77]
    assert hb.rank1_approx_stats() == a0
    body = src[src.index("int rank1_approx_impl("):src.index('extern "C" int hipsdp_rank1_approx(')]
    assert body.count("return HIPSDP_ERR_ARG") == 1
    assert body.index("return HIPSDP_ERR_ARG") < body.index("hs_solver_cut_enter_large(") < body.index("r1a_chunk(")
    assert 'hs_chunk_env("HIPSDP_RANK1_APPROX_CHUNK")' in body and "hs_chunks_run(" in body
    # the unit entries refuse their arguments in front of the device too
    ulib = hb.ulib()
    n1 = (C.c_int * 1)(2)
    n0 = (C.c_int * 1)(513)
    assert ulib.hipsdp_rank1_minors_unit(0, 0, n1, Y, tol, me, mi, md, di) == ERR_ARG
    assert ulib.hipsdp_rank1_minors_unit(0, 1, n0, Y, tol, me, mi, md, di) == ERR_ARG
    assert ulib.hipsdp_rank1_minors_unit(0, 1, n1, Y, C.c_double(-1.0), me, mi, md, di) == ERR_ARG
    assert ulib.hipsdp_rank1_minors_unit(0, 1, n1, None, tol, me, mi, md, di) == ERR_ARG
    assert ulib.hipsdp_lsel_many_unit(0, 0, n1, Y, lam) == ERR_ARG
    assert ulib.hipsdp_lsel_many_unit(0, 1, n0, Y, lam) == ERR_ARG
    assert ulib.hipsdp_lsel_many_unit(0, 1, n1, Y, None) == ERR_ARG
    assert list(me) == [7.0] * 4 and list(lam) == [7.0] * 12


def test_the_launch_formula_of_the_header_is_the_host_function(tmp_path):
    """every subset of the four size classes (1 .. 64, 65 .. 128, 129 .. 512 rows present or not; no block at all) and nmax in
    {129, 130, 512}"""
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"3 \[any block\] \+ \[1 \.\. 64 rows\] \+ \[65 \.\. 128 rows\] \+ \[129 \.\. 512 rows\] \(nmax \+ 1\)", hdr)
    prog = tmp_path / "launches.cpp"
    prog.write_text('#include "hs_cut_plan.h"\n#include <stdio.h>\nint main(void)\n{\n'
                    '   const int nm[4] = {0, 129, 130, 512};\n'
                    '   for (int s = 0; s < 2; ++s) for (int m = 0; m < 2; ++m) for (int k = 0; k < 4; ++k)\n'
                    '      printf("%d %d %d %lld %lld\\n", s, m, nm[k], hs_r1_launches(s || m || nm[k], s, m, nm[k]),\n'
                    '         hs_cm_launches(s || m || nm[k], s, m, nm[k]));\n'
                    '   return 0;\n}\n')
    exe = str(tmp_path / "launches")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(prog), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    seen = 0
    for line in subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split("\n"):
        if not line:
            continue
        s, m, n, got, cm = (int(t) for t in line.split())
        anyb = 1 if s or m or n else 0
        assert got == 3 * anyb + s + m + (n + 1 if n else 0), line
        # the shape of hipsdp_check_y_many with the two vector launches of the large class gone, plus the minors launch
        assert got == cm + anyb - (2 if n else 0) - (1 - anyb), line
        seen += 1
    assert seen == 16


def test_the_launch_formula_of_the_approximation_call(tmp_path):
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"2 \+ 3 \[1 \.\. 128 rows\] \+ \[129 \.\. 512 rows\] \(nmax \+ 3\)", hdr)
    prog = tmp_path / "launches.cpp"
    prog.write_text('#include "hs_cut_plan.h"\n#include <stdio.h>\nint main(void)\n{\n'
                    '   const int nm[4] = {0, 129, 130, 512};\n'
                    '   for (int s = 0; s < 2; ++s) for (int k = 0; k < 4; ++k)\n'
                    '      printf("%d %d %lld\\n", s, nm[k], hs_r1a_launches(s, nm[k]));\n'
                    '   return 0;\n}\n')
    exe = str(tmp_path / "launches")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(prog), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    lines = [l for l in subprocess.run([exe], stdout=subprocess.PIPE, text=True).stdout.split("\n") if l]
    assert len(lines) == 8
    for line in lines:
        s, n, got = (int(t) for t in line.split())
        assert got == 2 + 3 * s + (n + 3 if n else 0), line


def test_the_kernel_file_is_built_and_keeps_the_reduction_rule():
    mk = _read("scip-sdp_amd", "Makefile")
    assert "csrc/rank1.hip" in mk
    text = _read("scip-sdp_amd", "csrc", "rank1.hip")
    for name in ("k_r1_minors", "k_r1_result", "k_r1_negate", "k_r1_rhs"):
        assert re.search(r"__global__\s+void\s+__launch_bounds__\(\w+\)\s+%s\s*\(" % name, text), name
    assert "cooperative" not in text.lower() and "grid.sync" not in text and not re.search(r"atomic\w*\s*\(", text)
    # the three-index many-kernels are wrappers of the shared bodies, which take the further indices
    eigi = _read("scip-sdp_amd", "csrc", "eigi.hip")
    for name, body in (("k_lsel_many_small", "d_syevi_small<false>("), ("k_lsel_many_mid", "d_syevi_mid(")):
        at = eigi.index(name + "(")
        assert body in eigi[at:eigi.index("\n}\n", at)], name
    sx, ix = _read("scip-sdp_amd", "csrc", "syevx.hip"), _read("scip-sdp_amd", "csrc", "hs_syevx_index_many.h")
    assert '#include "hs_syevx_index_many.h"' in sx
    at = ix.index("k_syevx_values_index_many(")
    assert ix[at:ix.index("\n}\n", at)].count("d_syevx_values(") == 2
    assert "dim3(count, 2)" in sx[sx.index("int hs_syevx_many_index("):]


# ---- the numpy restatement on hand-written cases --------------------------------------------------------------------------------------------

def test_the_pair_order_is_the_references():
    i, k = r1.pairs(4)
    assert list(zip(i.tolist(), k.tolist())) == [(1, 0), (2, 0), (2, 1), (3, 0), (3, 1), (3, 2)]
    assert len(r1.pairs(1)[0]) == 0


def test_the_eigenvalue_scan_by_hand():
    # diag (4, 1, 4), off-diagonals 0: the minors' smaller eigenvalues are 1 (1,0), 4 (2,0), 1 (2,1)
    assert r1.scan_ev(np.diag([4.0, 1.0, 4.0])) == (4.0, (2, 0))
    # a tie: diag (3, 3, 3) with zeros gives 3 three times, the FIRST pair wins
    assert r1.scan_ev(np.diag([3.0, 3.0, 3.0])) == (3.0, (1, 0))
    # a tie behind a smaller first value: (1,0) gives 1, (2,0) and (2,1) ... diag (1, 5, 5): 1, 1, 5
    assert r1.scan_ev(np.diag([1.0, 5.0, 5.0])) == (5.0, (2, 1))
    # [[2, 1], [1, 2]] has eigenvalues 1 and 3; with a third row that lowers every other minor
    Z = np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.5]])
    assert r1.scan_ev(Z) == (1.0, (1, 0))
    # nothing positive: exactly singular minors (rank one), negative definite, and one row
    u = np.array([1.0, -1.0, 1.0])
    assert r1.scan_ev(5.0 * np.outer(u, u)) == (0.0, (-1, -1))
    assert r1.scan_ev(-np.eye(3)) == (0.0, (-1, -1))
    assert r1.scan_ev(np.array([[9.0]])) == (0.0, (-1, -1))
    # the closed form against numpy's eigvalsh on these
    ref, i, k = r1.ev_reference(Z)
    assert np.allclose(ref, r1.minor_ev(Z[i, i], Z[i, k], Z[k, k]), rtol=0, atol=1e-15)


def test_the_determinant_scan_by_hand():
    # minors in order (1,0), (2,0), (2,1): 2*3 - 1 = 5, 2*4 - 4 = 4, 3*4 - 9 = 3
    Z = np.array([[2.0, 1.0, 2.0], [1.0, 3.0, 3.0], [2.0, 3.0, 4.0]])
    assert np.array_equal(r1.minors(Z), [5.0, 4.0, 3.0])
    assert r1.scan_det(Z, 1e-6) == (5.0, (1, 0))
    assert r1.scan_det(Z, 4.0) == (5.0, (1, 0))          # 4 and 3 are within the tolerance, 5 is not
    assert r1.scan_det(Z, 5.0) == (5.0, (-1, -1))        # a minor EQUAL to feastol is no violation
    # the first violating pair is not the largest one: minors 0, -2, 1
    Z = np.array([[1.0, 1.0, 2.0], [1.0, 1.0, 1.0], [2.0, 1.0, 2.0]])
    assert np.array_equal(r1.minors(Z), [0.0, -2.0, 1.0])
    assert r1.scan_det(Z, 1.5) == (2.0, (2, 0))
    assert r1.scan_det(Z, 2.0) == (2.0, (-1, -1))
    assert r1.scan_det(Z, 0.5) == (2.0, (2, 0))
    # ties: all minors equal, the first violating pair is (1, 0)
    assert r1.scan_det(r1.constant(3), 1.0) == (3.0, (1, 0))
    assert r1.scan_det(np.array([[4.0]]), 0.0) == (0.0, (-1, -1))


def test_the_right_hand_side_by_hand():
    A0 = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 5.0], [3.0, 5.0, 6.0]])
    v = np.array([1.0, 2.0, -1.0])
    got = r1.rhs(A0, 2.0, v)
    # rows (0,0) | (1,0) (1,1) | (2,0) (2,1) (2,2)
    assert np.array_equal(got, [1 + 2, 2 + 4, 4 + 8, 3 - 2, 5 - 4, 6 + 2])


def test_the_families_have_their_planted_answer():
    for n, p, q in [(3, 0, 2), (65, 64, 0), (129, 63, 64)]:
        Z, want = r1.planted_pair(n, p, q)
        ev, pair = r1.scan_ev(Z)
        assert pair == want and ev > 9.0
        ref, i, k = r1.ev_reference(Z)
        order = np.argsort(ref)
        assert ref[order[-1]] - ref[order[-2]] > 8.0 and (i[order[-1]], k[order[-1]]) == want
    assert r1.scan_ev(r1.constant(5)) == (1.0, (1, 0))
    assert r1.scan_ev(r1.negative_definite(17)) == (0.0, (-1, -1))
    blocks, Y, cs = r1.rank_one_blocks([3, 17], 4, 3)
    for A, c in zip(blocks, cs):
        for y in Y:
            Z = r1.zmat(A, y)
            assert np.all(np.abs(Z) == np.abs(Z[0, 0])) and Z[0, 0] > 0
            assert r1.scan_ev(Z) == (0.0, (-1, -1)) and r1.scan_det(Z, 1e-9) == (0.0, (-1, -1))


def test_the_conscheck_loop_over_outputs_is_the_loop_point_by_point():
    """on the host alone: the outputs are made by numpy, so both restatements must agree"""
    blocks, Y = r1.family([3, 3], 4, "negative", 5, seed=2)
    lam = np.zeros((5, 2, 3))
    mev = np.zeros((5, 2))
    mind = np.zeros((5, 2, 2), dtype=np.int32)
    for j, b in itertools.product(range(5), range(2)):
        Z = r1.zmat(blocks[b], Y[j])
        w = np.linalg.eigvalsh(Z)
        lam[j, b] = [w[0], w[1], w[2]]
        mev[j, b], mind[j, b] = r1.scan_ev(Z)
    a = r1.conscheck_from_call(lam, mev, mind, 1e-6)
    b = r1.conscheck_numpy(blocks, Y, 1e-6)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert not a[0].all()
