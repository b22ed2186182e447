"""CPU: the C ABI and the binding carry hipsdp_syevr with the documented signature, the unit entry of its stages 2 + 3 stays in the
test library's header, the library exports it and refuses bad arguments before any device work, and the new HIP source is part of
the build."""
import os
import re
import inspect
import importlib.util
from conftest import ROOT


def _hdr(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_syevr_is_declared():
    hdr = _hdr("hipsdp.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_syevr\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*A\s*,"
                     r"\s*double\s*\*\s*lam\s*,\s*double\s*\*\s*V\s*\)", hdr)


def test_tvec_unit_is_a_test_entry_only():
    units = _hdr("hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_tvec_unit\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*const\s+double\s*\*\s*d\s*,"
                     r"\s*const\s+double\s*\*\s*e\s*,\s*double\s*\*\s*lam\s*,\s*double\s*\*\s*Z\s*\)", units)
    assert "hipsdp_tvec_unit" not in _hdr("hipsdp.h")
    assert not re.search(r"hipsdp_syevr\s*\(", units)


def test_library_exports_the_new_symbols(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_syevr")
    assert hasattr(hb.ulib(), "hipsdp_tvec_unit") and not hasattr(lib, "hipsdp_tvec_unit")
    # refused before any device work: the argument checks come first
    assert lib.hipsdp_syevr(0, 0, None, None, None) == 3
    assert lib.hipsdp_syevr(0, 513, None, None, None) == 3


def test_binding_has_the_wrappers():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_syevr", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.syevr) and callable(mod.tvec_unit)
    assert list(inspect.signature(mod.syevr).parameters) == ["A", "vectors", "device"]
    assert inspect.signature(mod.syevr).parameters["vectors"].default is True
    assert list(inspect.signature(mod.tvec_unit).parameters) == ["d", "e", "device"]


def test_the_kernels_are_built_from_their_own_source():
    with open(os.path.join(ROOT, "scip-sdp_amd", "Makefile")) as f:
        assert "csrc/syevr.hip" in f.read()
    with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", "syevr.hip")) as f:
        src = f.read()
    assert src.count("__global__") >= 6
    # determinism: the only atomic of the solver is the integer count of the multisection, which syevx.hip and syevr.hip share
    # through hs_tridiag.h - one call in the three files together, in the header
    srcs = {}
    for name in ("syevx.hip", "syevr.hip", "hs_tridiag.h"):
        with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", name)) as f:
            srcs[name] = f.read()
    count = {name: len(re.findall(r"atomic\w*\s*\(", text)) for name, text in srcs.items()}
    assert count == {"syevx.hip": 0, "syevr.hip": 0, "hs_tridiag.h": 1}, count
    assert "atomicAdd(&cntb" in srcs["hs_tridiag.h"] and '#include "hs_tridiag.h"' in src
    # stage 1 is the one of syevx.hip, not a copy
    assert "hs_syevx_tridiag_dev(" in src and "k_syevx_col" not in src
