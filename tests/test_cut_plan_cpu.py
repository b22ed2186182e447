"""CPU: the workspace layouts of the cut calls (hipsdp_eigencuts_all, hipsdp_sparsecuts_all, hipsdp_sparsecuts: csrc/hs_cut_plan.cpp)
run clean in a stand-alone program under AddressSanitizer + UBSan - segments in the documented order, disjoint and aligned, the read-back
window around the result arrays alone, the views written through on heap blocks of exactly the stated lengths, and literal offsets
for a few shapes per call form - and the file is host-only and part of the build."""
import os
from conftest import ROOT
import host_check


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_layouts_run_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/cut_plan_check.cpp + csrc/hs_cut_plan.cpp, host compiler, -fsanitize=address,undefined:
    a program of its own with the runtimes linked in (nothing is loaded into python, nothing is preloaded)"""
    host_check.run_clean(tmp_path, "cut_plan_check.cpp", ["hs_cut_plan.cpp"], "cut plan check: ok")


def test_the_layouts_are_host_only_and_built_into_the_library():
    assert "csrc/hs_cut_plan.cpp" in _read("scip-sdp_amd", "Makefile")
    assert "hip_runtime" not in _read("scip-sdp_amd", "csrc", "hs_cut_plan.cpp")
    hdr = _read("scip-sdp_amd", "csrc", "hs_cut_plan.h")
    assert "hip_runtime" not in hdr and "hs_kernels.h" not in hdr and "hs_common.h" not in hdr
    src = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    for name in ("hs_ec_layout_make", "hs_sc_layout_make", "hs_scl_layout_make", "hs_cut_view"):
        assert name in src, name
