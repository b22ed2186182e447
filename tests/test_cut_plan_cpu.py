"""CPU: the workspace layouts of the cut calls (hipsdp_eigencuts_all, hipsdp_sparsecuts_all, hipsdp_sparsecuts: csrc/hs_cut_plan.cpp)
run clean in a stand-alone program under AddressSanitizer + UBSan - segments in the documented order, disjoint and aligned, the read-back
window around the result arrays alone, the views written through on heap blocks of exactly the stated lengths, and literal offsets
for a few shapes per call form - and the file is host-only and part of the build."""
import os
import subprocess
from conftest import ROOT

PKG = os.path.join(ROOT, "scip-sdp_amd")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_layouts_run_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/cut_plan_check.cpp + csrc/hs_cut_plan.cpp, host compiler, -fsanitize=address,undefined:
    a program of its own with the runtimes linked in (nothing is loaded into python, nothing is preloaded)"""
    exe = str(tmp_path / "cut_plan_check")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "harness", "cut_plan_check.cpp"),
           os.path.join(PKG, "csrc", "hs_cut_plan.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "cut plan check: ok" in r.stdout, r.stdout[-4000:]
    assert "AddressSanitizer" not in r.stdout and "runtime error:" not in r.stdout, r.stdout[-4000:]


def test_the_layouts_are_host_only_and_built_into_the_library():
    assert "csrc/hs_cut_plan.cpp" in _read("scip-sdp_amd", "Makefile")
    assert "hip_runtime" not in _read("scip-sdp_amd", "csrc", "hs_cut_plan.cpp")
    hdr = _read("scip-sdp_amd", "csrc", "hs_cut_plan.h")
    assert "hip_runtime" not in hdr and "hs_kernels.h" not in hdr and "hs_common.h" not in hdr
    src = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    for name in ("hs_ec_layout_make", "hs_sc_layout_make", "hs_scl_layout_make", "hs_cut_view"):
        assert name in src, name
