"""CPU: the C ABI and the binding carry hipsdp_psd_project_many / hipsdp_psd_project_many_stats with the documented signatures, the
ctypes structure of the binding is the header's hipsdp_psd_job field for field (checked against what the host compiler lays out), and
the host-side planning of the call (argument checks, class sort, slab offsets: csrc/hs_psd_plan.cpp) runs clean in a stand-alone
program under AddressSanitizer + UBSan."""
import ctypes as C
import os
import re
import subprocess
import importlib.util
from conftest import ROOT
import host_check

PKG = os.path.join(ROOT, "scip-sdp_amd")
FIELDS = ["n", "nnz", "row", "col", "val", "minev", "cap", "nnz_out", "rowout", "colout", "valout"]


def _hdr():
    with open(os.path.join(ROOT, "include", "hipsdp.h")) as f:
        return f.read()


def _binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_ppmany", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_psd_project_many_is_declared_and_bound():
    hdr = _hdr()
    assert re.search(r"#define\s+HIPSDP_PSD_MANY_MAXJOBS\s+1024\b", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_psd_project_many\s*\(\s*int\s+device\s*,\s*int\s+count\s*,\s*hipsdp_psd_job\s*\*\s*jobs\s*,"
                     r"\s*double\s+epsilon\s*,\s*int\s+mode\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_psd_project_many_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    m = re.search(r"typedef\s+struct\s+hipsdp_psd_job\s*\{(.*?)\}\s*hipsdp_psd_job\s*;", hdr, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    names = [re.sub(r"[\s*]", "", d) for stmt in body.split(";") for d in re.sub(r"^\s*(const\s+)?(int|double)\b", "", stmt).split(",") if d.strip()]
    assert names == FIELDS, names
    with open(os.path.join(ROOT, "include", "hipsdp_units.h")) as f:
        assert not re.search(r"hipsdp_psd_project_many(_stats)?\s*\(", f.read())       # product symbols: declared in hipsdp.h alone
    mod = _binding()
    assert callable(mod.psd_project_many) and callable(mod.psd_project_many_stats)
    assert [f[0] for f in mod.PsdJob._fields_] == FIELDS


def test_binding_structure_has_the_layout_the_compiler_gives_the_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hipsdp.h"\nint main(void) { printf("%zu", sizeof(hipsdp_psd_job));\n'
                   + "".join('printf(" %%zu", offsetof(hipsdp_psd_job, %s));\n' % f for f in FIELDS) + "return 0; }\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    out = [int(x) for x in subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    mod = _binding()
    assert out[0] == C.sizeof(mod.PsdJob)
    assert out[1:] == [getattr(mod.PsdJob, f).offset for f in FIELDS]


def test_host_planning_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/psd_plan_check.cpp + csrc/hs_psd_plan.cpp, host compiler, -fsanitize=address,undefined:
    a program of its own with the runtimes linked in (nothing is loaded into python, nothing is preloaded)"""
    host_check.run_clean(tmp_path, "psd_plan_check.cpp", ["hs_psd_plan.cpp"], "psd plan check: ok")


def test_library_exports_the_new_symbols_and_checks_arguments_without_a_device(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_psd_project_many") and hasattr(lib, "hipsdp_psd_project_many_stats")
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_psd_project_many_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_psd_project_many_stats(None, None, None) == 0
    # host-only answers: nothing to do, and argument errors (the checks run before the device is looked at)
    assert lib.hipsdp_psd_project_many(0, 0, None, C.c_double(1e-9), 0) == 0
    assert lib.hipsdp_psd_project_many(0, 1, None, C.c_double(1e-9), 0) == 3
    assert lib.hipsdp_psd_project_many(0, -1, None, C.c_double(1e-9), 0) == 3
    tab = (hb.PsdJob * 1)()
    tab[0].n = 0
    assert lib.hipsdp_psd_project_many(0, 1, tab, C.c_double(1e-9), 0) == 3
    tab[0].n = 3
    assert lib.hipsdp_psd_project_many(0, 1, tab, C.c_double(1e-9), 2) == 3
    assert lib.hipsdp_psd_project_many(-1, 1, tab, C.c_double(1e-9), 0) == 3
    c2 = C.c_longlong(-1)
    assert lib.hipsdp_psd_project_many_stats(C.byref(c2), None, None) == 0 and c2.value == c.value


def test_the_kernels_are_built_from_their_own_source():
    with open(os.path.join(PKG, "Makefile")) as f:
        mk = f.read()
    assert "csrc/psd_many.hip" in mk and "csrc/hs_psd_plan.cpp" in mk
    with open(os.path.join(PKG, "csrc", "psd_many.hip")) as f:
        src = f.read()
    for k in ("k_pp_expand", "k_pp_recombine", "k_pp_write"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, src), k
    assert "atomicAdd" not in src and "hs_syev_small_many" in src and "hs_func_max_lds" in src
    with open(os.path.join(PKG, "csrc", "hs_psd_plan.cpp")) as f:
        assert "hip_runtime" not in f.read()
