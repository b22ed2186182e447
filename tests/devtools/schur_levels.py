"""measured error levels of the Schur assembly: runs the iterate and exact cases of tests/test_gpu_schur_forms.py in collecting mode
and writes, per form, the worst F_device (by F_device / bound), F_numpy on the same case and their ratio, and how many exact cases
came back with the bits of numpy and the predicted counters (developer tool, GPU box)

    python tests/devtools/schur_levels.py [output file, default profiles/r18_schur_levels.txt]"""
import importlib.util, os, sys
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "harness")); sys.path.insert(0, os.path.join(ROOT, "tests"))
spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
hb = importlib.util.module_from_spec(spec); spec.loader.exec_module(hb)
import schur_cases as sc
import test_gpu_schur_forms as T

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r18_schur_levels.txt")
assert hb.device_count() > 0, "no HIP device visible"
assert sc.longdouble_ok(), "numpy.longdouble has no 64-bit mantissa here"
missed = []
for m1, n in sc.ITERATE:
    for cond in sc.CONDS:
        T.iterate_figures(hb, m1, n, cond, missed)
exact_runs, exact_bad, used = 0, [], []
cases = [(f, m1, n, p, 0.0) for m1, n in sc.LADDER for f, p in ((0, 1), (1, 2), (2, 2), (3, 1), (4, 64))]
cases += [(1,) + s + (0.0,) for s in sc.FORM1] + [(2,) + s + (0.0,) for s in sc.FORM2] + [(4,) + s + (0.0,) for s in sc.FORM4]
cases += [(3,) + s + (1, w) for s in sc.FORM3 for w in (0.0, sc.chunk_gbytes(s[1]))]
for form, m1, n, parts, ws in cases:
    before = len(exact_bad)
    T.run_exact(hb, form, m1, n, parts=parts, ws=ws, bad=exact_bad)
    exact_runs += 1
    if form == 0:
        A, R, G, _, _ = sc.exact(m1, n)
        used.append("(%d, %d): %s" % (m1, n, hb.schur_form_unit(0, A, R, G)[1]))
lines = ["Schur assembly (scip-sdp_amd/csrc/schur.hip), every form through hipsdp_schur_form_unit / hipsdp_schur_small_unit: worst figure per form",
         "of tests/test_gpu_schur_forms.py.  F = max_ij |M - M_ref|_ij / (eps B_ij), M_ref in extended precision on the operands handed to the",
         "device, B the abs-value chain of the form; iterate family: n in %s, cond in %s" % ([s[1] for s in sc.ITERATE], list(sc.CONDS)),
         "(worst by F_device / bound; F_numpy = float64 numpy on the same case; ' / numpy': bound = %g F_numpy, ' / cap': bound = n^2 + 2 n + 2)" % sc.MARGIN,
         "",
         "%-42s %-11s %-11s %-9s %-11s %s" % ("group", "F_device", "F_numpy", "ratio", "bound", "case")]
for g in sorted(sc.LEVELS):
    ratio, value, ref, bound, what = sc.LEVELS[g]
    lines.append("%-42s %-11.3e %-11s %-9s %-11.3e %s" % (g, value, "-" if ref is None else "%.3e" % ref,
                                                         "-" if not ref else "%.2f" % (value / ref), bound, what))
lines += ["", "missed bounds: %d" % len(missed)] + [str(m) for m in missed]
lines += ["", "exact family: %d runs, %d findings (bits of numpy, symmetric, counters as predicted)" % (exact_runs, len(exact_bad))] + [str(b) for b in exact_bad]
lines += ["counters of hs_schur_W (persistent kernels, of these paired-band, Gram kernel): " + "; ".join(used)]
with open(out, "w") as f:
    f.write("\n".join(lines) + "\n")
print("\n".join(lines))
