"""CPU: the C ABI and the binding carry hipsdp_syevx / hipsdp_syevx_below with the documented signatures and limits, the unit entry
of the tridiagonalisation stays in the test library's header, and the new HIP source is part of the build."""
import os
import re
import importlib.util
from conftest import ROOT


def _hdr(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_syevx_is_declared_with_its_limits():
    hdr = _hdr("hipsdp.h")
    assert re.search(r"#define\s+HIPSDP_SYEVX_MAXN\s+512\b", hdr) and re.search(r"#define\s+HIPSDP_SYEVX_MAXK\s+32\b", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_syevx\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*A\s*,\s*int\s+il\s*,"
                     r"\s*int\s+iu\s*,\s*double\s*\*\s*lam\s*,\s*double\s*\*\s*V\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_syevx_below\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*A\s*,"
                     r"\s*double\s+bound\s*,\s*int\s+maxk\s*,\s*int\s*\*\s*count\s*,\s*int\s*\*\s*nbelow\s*,\s*double\s*\*\s*lam\s*,"
                     r"\s*double\s*\*\s*V\s*\)", hdr)


def test_tridiag_unit_is_a_test_entry_only():
    units = _hdr("hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_tridiag_unit\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*A\s*,"
                     r"\s*double\s*\*\s*d\s*,\s*double\s*\*\s*e\s*,\s*double\s*\*\s*Vrefl\s*,\s*double\s*\*\s*tau\s*\)", units)
    assert "hipsdp_tridiag_unit" not in _hdr("hipsdp.h")
    assert not re.search(r"hipsdp_syevx(_below)?\s*\(", units)


def test_library_exports_the_new_symbols(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_syevx") and hasattr(lib, "hipsdp_syevx_below")
    assert hasattr(hb.ulib(), "hipsdp_tridiag_unit") and not hasattr(lib, "hipsdp_tridiag_unit")
    # refused before any device work: the argument checks come first
    assert lib.hipsdp_syevx(0, 0, None, 1, 1, None, None) == 3
    assert lib.hipsdp_syevx_below(0, 513, None, hb.C.c_double(0.0), 1, None, None, None, None) == 3


def test_binding_has_both_wrappers():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_syevx", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.syevx) and callable(mod.syevx_below) and callable(mod.tridiag_unit)
    import inspect
    assert list(inspect.signature(mod.syevx).parameters) == ["A", "il", "iu", "vectors", "device"]
    assert list(inspect.signature(mod.syevx_below).parameters) == ["A", "bound", "maxk", "vectors", "device"]


def test_the_kernels_are_built_from_their_own_source():
    with open(os.path.join(ROOT, "scip-sdp_amd", "Makefile")) as f:
        assert "csrc/syevx.hip" in f.read()
    with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", "syevx.hip")) as f:
        src = f.read()
    assert src.count("__global__") >= 5
    # determinism: the only atomic of the solver is the integer count of the multisection, which syevx.hip and syevr.hip share
    # through hs_tridiag.h - one call in the three files together, in the header
    srcs = {}
    for name in ("syevx.hip", "syevr.hip", "hs_tridiag.h"):
        with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", name)) as f:
            srcs[name] = f.read()
    count = {name: len(re.findall(r"atomic\w*\s*\(", text)) for name, text in srcs.items()}
    assert count == {"syevx.hip": 0, "syevr.hip": 0, "hs_tridiag.h": 1}, count
    assert "atomicAdd(&cntb" in srcs["hs_tridiag.h"] and '#include "hs_tridiag.h"' in src
