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


def test_the_tail_of_a_chunk_stands_once():
    """one tail for every call and chunk, chunk_readback: the copy of the result range, the synchronise and the two counters stand once
    in the file, cut_readback adds the view of a cut layout to it, and a chunk without a cut layout passes no dummy layout to get it"""
    src = _read("scip-sdp_amd", "csrc", "cut_calls.hip")
    assert src.count("stats->readbacks += 1") == 1 and src.count("stats->launches += launches") == 1
    tail = src[src.index("int chunk_readback("):src.index("int cut_readback(")]
    assert tail.index("hipMemcpyDeviceToHost") < tail.index("hipStreamSynchronize(") < tail.index("stats->launches += launches") \
        < tail.index("stats->readbacks += 1")
    assert tail.count("hipMemcpyAsync(") == 1 and tail.count("hipStreamSynchronize(") == 1 and "len.res_off" in tail and "len.res_len" in tail
    view = src[src.index("int cut_readback("):src.index("int sxm_job(")]
    assert view.index("chunk_readback(") < view.index("hs_cut_view(") and "hipStreamSynchronize" not in view
    # the dummy layout (a zeroed hs_cut_res with ints = sup = -1) that five chunks once built for the tail's sake is gone
    assert src.count("none.ints = none.sup") == 0 and "hs_cut_res none" not in src
    assert src.count("chunk_readback(") >= 7
