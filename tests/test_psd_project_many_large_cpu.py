"""CPU: hipsdp_psd_project_many_large / hipsdp_psd_project_many_large_stats are declared, bound and exported as documented, the unit
entry of the batched decomposition lives in the units library alone, the argument checks answer without a device, the inputs of
the GPU tests (tests/harness/psd_large_cases.py) meet the two preconditions under which kept / dropped entries and raised / kept
eigenvalues are decided by far more than rounding, the launch formula of the header is the host function, the host-side planning
(csrc/hs_psd_large_plan.cpp) runs clean in a stand-alone program under AddressSanitizer + UBSan, and the sources keep the shape
the design asks for (one body per stage in syevr.hip, no atomics, no grid barrier)."""
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
import psd_project_ref as ref
import psd_large_cases as cases

PKG = os.path.join(ROOT, "scip-sdp_amd")
EPS = cases.EPSILON


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_pplarge", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_calls_are_declared_and_bound():
    hdr, uhdr = _read("include", "hipsdp.h"), _read("include", "hipsdp_units.h")
    assert re.search(r"#define\s+HIPSDP_PSD_LARGE_MINN\s+129\b", hdr) and re.search(r"#define\s+HIPSDP_PSD_LARGE_MAXN\s+512\b", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_psd_project_many_large\s*\(\s*int\s+device\s*,\s*int\s+count\s*,\s*hipsdp_psd_job\s*\*\s*jobs\s*,"
                     r"\s*double\s+epsilon\s*,\s*int\s+mode\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_psd_project_many_large_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert not re.search(r"hipsdp_psd_project_many_large(_stats)?\s*\(", uhdr)          # product symbols: declared in hipsdp.h alone
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_syevr_many_unit\s*\(\s*int\s+device\s*,\s*int\s+count\s*,\s*const\s+int\s*\*\s*n\s*,"
                     r"\s*const\s+double\s*\*\s*A\s*,\s*int\s+cap\s*,\s*double\s*\*\s*lam\s*,\s*double\s*\*\s*V\s*\)", uhdr)
    assert "hipsdp_syevr_many_unit" not in hdr
    assert "hipsdp_syevr" in hdr and "block Jacobi" in hdr.split("hipsdp_psd_project_many_stats")[-1]      # mode 0: the header says whose vectors
    mod = _binding()
    assert list(inspect.signature(mod.psd_project_many_large).parameters) == ["jobs", "epsilon", "mode", "device"]
    assert list(inspect.signature(mod.psd_project_many_large_stats).parameters) == []
    assert list(inspect.signature(mod.syevr_many_unit).parameters) == ["mats", "cap", "device"]


def test_libraries_export_accordingly_and_arguments_are_checked_without_a_device(hb):
    lib, ulib = hb.lib(), hb.ulib()
    assert hasattr(lib, "hipsdp_psd_project_many_large") and hasattr(lib, "hipsdp_psd_project_many_large_stats")
    assert hasattr(ulib, "hipsdp_syevr_many_unit") and not hasattr(lib, "hipsdp_syevr_many_unit")
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_psd_project_many_large_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_psd_project_many_large_stats(None, None, None) == 0
    eps = C.c_double(EPS)
    call = lib.hipsdp_psd_project_many_large
    assert call(0, 0, None, eps, 0) == 0                                                # nothing to do
    assert call(0, 1, None, eps, 0) == 3 and call(0, -1, None, eps, 0) == 3
    tab = (hb.PsdJob * 1)()
    assert call(0, 1025, tab, eps, 0) == 3
    n = 130
    row = np.array([0, 1, 129], np.int32)
    col = np.array([0, 0, 2], np.int32)
    val = np.array([1.0, 2.0, 3.0])
    ro, co, vo = np.zeros(6, np.int32), np.zeros(6, np.int32), np.zeros(6)
    PI, PD = C.POINTER(C.c_int), C.POINTER(C.c_double)

    def fill():
        tab[0].n, tab[0].nnz, tab[0].minev, tab[0].cap, tab[0].nnz_out = n, 3, 1e-4, 6, -5
        tab[0].row, tab[0].col, tab[0].val = row.ctypes.data_as(PI), col.ctypes.data_as(PI), val.ctypes.data_as(PD)
        tab[0].rowout, tab[0].colout, tab[0].valout = ro.ctypes.data_as(PI), co.ctypes.data_as(PI), vo.ctypes.data_as(PD)

    fill()
    assert call(0, 1, tab, eps, 2) == 3 and call(0, 1, tab, eps, -1) == 3 and call(-1, 1, tab, eps, 0) == 3
    for field, bad in (("n", 0), ("nnz", -1), ("cap", -1), ("n", 129)):                 # (129 rows: the triplet (129, 2) lies outside)
        fill()
        setattr(tab[0], field, bad)
        assert call(0, 1, tab, eps, 0) == 3, (field, bad)
    for null in ("row", "col", "val", "rowout", "colout", "valout"):
        fill()
        setattr(tab[0], null, None)
        assert call(0, 1, tab, eps, 0) == 3, null
    fill()
    col[1] = -1
    assert call(0, 1, tab, eps, 0) == 3
    col[1] = 0
    assert tab[0].nnz_out == -5                                                         # nothing was touched
    c2, l2, r2 = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_psd_project_many_large_stats(C.byref(c2), C.byref(l2), C.byref(r2)) == 0
    assert (c2.value, l2.value, r2.value) == (c.value, l.value, r.value)


@pytest.fixture(scope="module")
def all_cases():
    return cases.all_jobs()


def test_no_case_is_left_out(all_cases):
    names = [j.name for j in all_cases]
    assert len(set(names)) == len(names)
    assert sorted(set(j.n for j in all_cases)) == [129, 160, 200, 257, 512]
    assert sum(j.name.startswith("random_") for j in all_cases) == 4 * 2 * 2 + 1 and sum(j.n == 512 for j in all_cases) == 1
    assert [(j.n, j.name) for j in all_cases if j.name.startswith("low_rank")] == [
        (129, "low_rank_n129_r12_s0"), (200, "low_rank_n200_r20_s0.25"), (257, "low_rank_n257_r30_s-0.01")]
    assert [j.name for j in all_cases if j.name.startswith("blocks")] == ["blocks_150_107", "blocks_100_29"]
    assert [j.name for j in all_cases if j.name.startswith("edge")] == ["edge_empty", "edge_diag", "edge_psd"]
    mixed = cases.mixed_jobs()
    assert sorted(j.name for j in mixed) == sorted(j.name for j in all_cases if j.n <= 257 and not j.name.startswith("edge"))
    assert [j.name for j in mixed] != sorted(j.name for j in mixed)                     # shuffled, and always the same way
    assert [j.name for j in mixed] == [j.name for j in cases.mixed_jobs()]
    assert [M.shape[0] for M in cases.decomposition_table()] == [129, 160, 200, 257, 129]


def test_every_case_meets_both_preconditions(all_cases):
    """the band (1e-10, 1e-8) is empty on the spectral form, and no eigenvalue lies within 1e-6 scale of minev - epsilon"""
    worst = None
    for job in all_cases:
        M = ref.expand_sparse(job.n, job.row, job.col, job.val).reshape(job.n, job.n)
        assert np.array_equal(M, job.M), job.name
        S = ref.spectral(job.n, job.row, job.col, job.val, job.minev)
        assert cases.band_is_empty(S), job.name
        lam = np.linalg.eigvalsh(M)
        dist = np.min(np.abs(lam - (job.minev - EPS)))
        if worst is None or dist / job.scale < worst[0]:
            worst = (dist / job.scale, dist, job.name)
        assert dist > 1e-6 * job.scale, (job.name, dist)
    print("smallest distance of an eigenvalue to minev - epsilon: %.3e (%s)" % (worst[1], worst[2]))
    low = [j for j in all_cases if j.name.startswith("low_rank")]
    for job, (n, r, shift) in zip(low, cases.LOW_RANK):
        lam = np.linalg.eigvalsh(job.M)
        assert np.sum(np.abs(lam - shift) < 1e-12) == n - r, job.name                   # one cluster of n - r equal eigenvalues
    psd = [j for j in all_cases if j.name == "edge_psd"][0]
    assert np.linalg.eigvalsh(psd.M).min() >= 0.5 - 1e-12


def test_header_formula_is_the_host_function(tmp_path):
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"nmax\s*\+\s*8\s*\+\s*6\s*ceil\(\s*nmax\s*/\s*32\s*\)", hdr)
    src = tmp_path / "launches.cpp"
    src.write_text('#include <stdio.h>\n#include "hs_psd_large_plan.h"\nint main(void) { const int ns[] = {129, 160, 200, 257, 512};\n'
                   'for (int k = 0; k < 5; ++k) printf("%d ", hs_ppl_launches(ns[k])); return 0; }\n')
    exe = str(tmp_path / "launches")
    r = subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(PKG, "csrc"), str(src), os.path.join(PKG, "csrc", "hs_psd_large_plan.cpp"),
                        "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    assert out == [n + 8 + 6 * -(-n // 32) for n in (129, 160, 200, 257, 512)] == [167, 198, 250, 319, 616]


def test_host_planning_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/psd_large_plan_check.cpp + csrc/hs_psd_large_plan.cpp, host compiler,
    -fsanitize=address,undefined: a program of its own with the runtimes linked in (nothing is loaded into python, nothing is
    preloaded)"""
    host_check.run_clean(tmp_path, "psd_large_plan_check.cpp", ["hs_psd_large_plan.cpp"], "psd large plan check: ok")


def test_sources_keep_their_shape():
    mk = _read("scip-sdp_amd", "Makefile")
    assert "csrc/psd_large.hip" in mk and "csrc/hs_psd_large_plan.cpp" in mk and "csrc/hs_psd_large_plan.h" in mk
    assert "hip_runtime" not in _read("scip-sdp_amd", "csrc", "hs_psd_large_plan.cpp") + _read("scip-sdp_amd", "csrc", "hs_psd_large_plan.h")
    sr = _read("scip-sdp_amd", "csrc", "syevr.hip")
    for stage in ("values", "order", "step", "ortho_prev", "ortho_panel", "back"):
        assert len(re.findall(r"__device__\s+__forceinline__\s+void\s+d_syevr_%s\s*\(" % stage, sr)) == 1, stage
        # the kernel of one matrix and the kernel of many matrices both call the one body
        assert len(re.findall(r"__global__[^;{]*\bk_syevr_%s(_many)?\s*\(" % stage, sr)) == 2, stage
        assert len(re.findall(r"\bd_syevr_%s\s*\(" % stage, sr)) == 3, stage
    assert len(re.findall(r"__device__\s+__forceinline__", sr)) == 6
    assert not re.search(r"atomic\w*\s*\(", sr)
    pl = _read("scip-sdp_amd", "csrc", "psd_large.hip")
    for k in ("k_ppl_expand", "k_ppl_recombine", "k_ppl_write"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, pl), k
    assert not re.search(r"atomic\w*\s*\(", pl) and "cooperative" not in pl and "grid.sync" not in pl
    assert "hs_syevx_many_cols" in pl and "hs_syevr_many_tvec" in pl and "hs_syevr_many_back" in pl
    assert "__builtin_amdgcn_mfma_f64_16x16x4f64" in pl and "hs_ppl_launches" in _read("scip-sdp_amd", "csrc", "hs_psd_large_plan.h")
    # the chunk rule, the chunk variable and the totals are the shared ones (hs_chunks.h, hs_cut_stats.h)
    assert 'hs_chunk_env("HIPSDP_PSD_LARGE_CHUNK")' in pl and "getenv" not in pl and "CutStats" in pl and "hs_syevx_many_cap(" in pl
    plan = _read("scip-sdp_amd", "csrc", "hs_psd_large_plan.cpp")
    assert '#include "hs_chunks.h"' in plan and "hs_chunk_end(" in plan and "hs_cut_plan" not in plan
