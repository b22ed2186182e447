"""measured error levels of the Cholesky kernels: runs the cases of tests/test_gpu_chol.py (single block, fused outputs, blocked,
semidefinite, solves in sequence) in collecting mode and writes, per group of figures, the worst engine value (by value / bound), the
reference's figure on the same case and the bound (developer tool, GPU box)

    python tests/devtools/chol_levels.py [output file, default profiles/r13_chol_levels.txt]"""
import importlib.util, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "harness")); sys.path.insert(0, os.path.join(ROOT, "tests"))
spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
hb = importlib.util.module_from_spec(spec); spec.loader.exec_module(hb)
import chol_cases as cc
import test_gpu_chol as T

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r13_chol_levels.txt")
assert hb.device_count() > 0, "no HIP device visible"
missed = []
for fn, params in ((T.test_single_block_factorization_componentwise, cc.SINGLE), (T.test_fused_outputs_of_the_small_block_kernel, cc.SINGLE),
                   (T.test_blocked_factorization_both_forms, cc.BLOCKED), (T.test_semidefinite_mode_against_the_oracle, cc.PSD_SIZES),
                   (T.test_a_forced_pivot_above_the_noise_level_keeps_its_column, cc.KEPT_SIZES),
                   (T.test_solves_in_sequence_on_one_workspace, cc.SEQ_SIZES)):
    for p in params:
        try:
            fn(hb, p)
        except AssertionError as e:
            missed.append("%s[%s]: %s" % (fn.__name__, p, str(e)[:400]))
lines = ["Cholesky kernels (scip-sdp_amd/csrc/chol.hip) against LAPACK / ipm_ref.chol_psd: worst figure of every group of tests/test_gpu_chol.py",
         "(worst by engine / bound; reference = LAPACK's or the oracle's figure on the same case; componentwise figures in units of (n + 1) eps)",
         "",
         "%-36s %-11s %-11s %-11s %s" % ("group", "engine", "reference", "bound", "case")]
for g in sorted(cc.LEVELS):
    ratio, value, ref, bound, what = cc.LEVELS[g]
    lines.append("%-36s %-11.3e %-11s %-11.3e %s" % (g, value, "-" if ref is None else "%.3e" % ref, bound, what))
lines += ["", "missed bounds: %d" % len(missed)] + missed
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
