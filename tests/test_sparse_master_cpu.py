"""CPU: the C ABI carries the master copy of blocks kept as triplets (hipsdp_master_define2, hipsdp_master_block_is_sparse,
hipsdp_master_gather_stats), the dump of a block's device structure is a unit entry and no product symbol, and the host side of the
triplet master (one-time sort into the three orders, index maps of a node: csrc/hs_sp_master.cpp) agrees with a plain restatement
in a stand-alone program under AddressSanitizer + UBSan."""
import os
import re
import importlib.util
from conftest import ROOT
import host_check

PKG = os.path.join(ROOT, "scip-sdp_amd")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding_spmaster", os.path.join(PKG, "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_new_calls_are_declared_and_bound():
    hdr = _read("include", "hipsdp.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_master_define2\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+nvars\s*,\s*int\s+nblocks\s*,"
                     r"\s*const\s+int\s*\*\s*blocksizes\s*,\s*const\s+int\s*\*\s*nblockvars\s*,\s*const\s+long\s+long\s*\*\s*nnz\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_master_block_is_sparse\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+master_block\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_master_gather_stats\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*long\s+long\s*\*\s*device_builds\s*,"
                     r"\s*long\s+long\s*\*\s*host_builds\s*,\s*long\s+long\s*\*\s*launches\s*,\s*long\s+long\s*\*\s*readbacks\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_master_define\s*\(", hdr)              # the dense form keeps its name and meaning
    mod = _binding()
    for name in ("master_define", "master_add_entries", "master_add_vars", "master_gather", "master_block_is_sparse", "master_gather_stats"):
        assert callable(getattr(mod.Solver, name)), name


def test_the_dump_is_a_unit_entry_and_not_a_product_symbol():
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparse_dump_unit\s*\(\s*hipsdp_solver\s*\*", _read("include", "hipsdp_units.h"))
    assert "hipsdp_sparse_dump_unit" not in _read("include", "hipsdp.h")


def test_library_exports_the_new_symbols(hb):
    lib = hb.lib()
    for name in ("hipsdp_master_define2", "hipsdp_master_block_is_sparse", "hipsdp_master_gather_stats"):
        assert hasattr(lib, name), name
    assert not hasattr(lib, "hipsdp_sparse_dump_unit")
    assert hasattr(hb.ulib(), "hipsdp_sparse_dump_unit")
    # host-only answers
    assert lib.hipsdp_master_block_is_sparse(None, 0) == 0
    assert lib.hipsdp_master_gather_stats(None, None, None, None, None) == 3


def test_host_side_of_the_triplet_master_runs_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program tests/harness/sp_master_check.cpp + csrc/hs_sp_master.cpp, host compiler, -fsanitize=address,undefined:
    a program of its own with the runtimes linked in (nothing is loaded into python, nothing is preloaded)"""
    host_check.run_clean(tmp_path, "sp_master_check.cpp", ["hs_sp_master.cpp"], "sp master check: ok")


def test_the_gather_is_built_from_its_own_sources():
    mk = _read("scip-sdp_amd", "Makefile")
    assert "csrc/sp_master.hip" in mk and "csrc/hs_sp_master.cpp" in mk
    src = _read("scip-sdp_amd", "csrc", "sp_master.hip")
    for k in ("k_spm_var", "k_spm_count_pos", "k_spm_scan_local", "k_spm_scan_top", "k_spm_scan_add", "k_spm_write_pos", "k_spm_order_pos",
              "k_spm_gather_dense"):
        assert re.search(r"__global__[^;{]*\b%s\s*\(" % k, src), k
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "atomicAdd" not in code and "__ballot" in code and "__popcll" in code      # no floating-point atomics (no atomics at all)
    assert "hip_runtime" not in _read("scip-sdp_amd", "csrc", "hs_sp_master.cpp")
    assert "hip_runtime" not in _read("scip-sdp_amd", "csrc", "hs_sp_master.h")
