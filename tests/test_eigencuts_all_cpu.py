"""CPU: the C ABI and the binding carry hipsdp_eigencuts_all / hipsdp_eigencuts_all_stats with the documented signatures, the unit
entry point of the batched decomposition stays in the test library's header, and the new HIP source is part of the build."""
import os
import re
import importlib.util
from conftest import ROOT


def _hdr(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_eigencuts_all_is_declared_and_bound():
    hdr = _hdr("hipsdp.h")
    d = r"\s*,\s*double\s*\*\s*"
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_eigencuts_all\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*double\s+tol\s*,\s*int\s+maxcuts\s*,\s*int\s*\*\s*ncuts" + d + "lmin" + d + "eigvals" + d + "coefs" + d + "lhs"
                     + d + r"vecs\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_eigencuts_all_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    units = _hdr("hipsdp_units.h")
    assert not re.search(r"hipsdp_eigencuts_all(_stats)?\s*\(", units)         # product symbols: declared in hipsdp.h alone
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_syev_many_unit\s*\(", units) and "hipsdp_syev_many_unit" not in hdr
    spec = importlib.util.spec_from_file_location("hipsdp_binding_ecall", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.Solver.eigencuts_all) and callable(mod.eigencuts_all_stats) and callable(mod.Solver.eigencuts_all_stats)


def test_library_exports_the_new_symbols(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_eigencuts_all") and hasattr(lib, "hipsdp_eigencuts_all_stats")
    assert hasattr(hb.ulib(), "hipsdp_syev_many_unit") and not hasattr(lib, "hipsdp_syev_many_unit")
    # no device work: the totals are readable before any call, and NULL outputs are allowed
    import ctypes as C
    c, l, r = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1)
    assert lib.hipsdp_eigencuts_all_stats(C.byref(c), C.byref(l), C.byref(r)) == 0
    assert c.value >= 0 and l.value >= 0 and r.value >= 0
    assert lib.hipsdp_eigencuts_all_stats(None, None, None) == 0
    assert lib.hipsdp_eigencuts_all(None, None, C.c_double(0.0), 0, None, None, None, None, None, None) == 3


def test_the_kernels_are_built_from_their_own_source():
    with open(os.path.join(ROOT, "scip-sdp_amd", "Makefile")) as f:
        assert "csrc/eigcuts.hip" in f.read()
    with open(os.path.join(ROOT, "scip-sdp_amd", "csrc", "eigcuts.hip")) as f:
        src = f.read()
    assert "__global__" in src and "atomicAdd" not in src
