"""check_y_many_rate.py - time of the feasibility check of `count` candidate points: ONE hipsdp_check_y_many call against (a) the loop
over the candidates of hipsdp_eigencuts_all(maxcuts = 0) - hipsdp_eigencuts_all_large(maxcuts = 0) above 128 rows -, which is what the
project offered before this call, and (b) numpy (Z formed by tensordot, eigvalsh) on one host core.

Shapes: 32 blocks of 12 rows; 4 blocks of 40 rows; 2 blocks of 128 rows; 4 blocks of 200 rows; 8 blocks of 512 rows (count <= 8).
count in 1, 8, 64, 256.  Every figure is the median of three timed calls after one warm-up call, host clock around a call that ends in
its read-back.  (b) is a loop, linear in count: it is timed on min(count, 8) candidates and scaled.

    HIPSDP_LIB=<libhipsdp.so of the parent commit> python tests/devtools/check_y_many_rate.py --loop-json FILE
                                 the loop (a) alone, figures to FILE: the baseline is never the new build
    python tests/devtools/check_y_many_rate.py [--baseline FILE] [--out profiles/r28_check_y_many_rate.txt]

The last column is the bytes of all constraint matrices over the time of the call: a LOWER bound of the bandwidth of k_cm_form_z's one
pass (the call also runs the eigenvalue kernels); for the kernel's own time use rocprofv3 --kernel-trace --stats in a run of its own."""
import argparse
import importlib.util
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "harness"))

SHAPES = [("32 blocks of 12", [12] * 32, 40, 256), ("4 blocks of 40", [40] * 4, 40, 256), ("2 blocks of 128", [128] * 2, 1000, 256),
          ("4 blocks of 200", [200] * 4, 100, 256), ("8 blocks of 512", [512] * 8, 8, 8)]
COUNTS = [1, 8, 64, 256]


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def problem(ns, m, seed):
    """entries of order 1 / sqrt(n), points of order 1: Z(y) indefinite, as at a rounded point"""
    rng = np.random.default_rng(seed)
    blocks = []
    for n in ns:
        R = rng.standard_normal((m + 1, n, n)) / np.sqrt(n)
        blocks.append((R + R.transpose(0, 2, 1)) / 2.0)
    return blocks, rng.uniform(-1.0, 1.0, (max(COUNTS), m))


def med3(fn):
    fn()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-json", default=None)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into the list of shapes (default: all)")
    a = ap.parse_args()
    import ipm_ref
    hb = binding()
    picked = range(len(SHAPES)) if a.shapes is None else [int(t) for t in a.shapes.split(",")]
    rows = []
    for si in picked:
        name, ns, m, cmax = SHAPES[si]
        blocks, Y = problem(ns, m, si)
        s = hb.Solver(0)
        s.load_core(ipm_ref.CoreProblem(np.zeros(m), blocks, None, None))
        large = ns[0] > 128
        one = (lambda y: s.eigencuts_all_large(y, 1e-6, 0)) if large else (lambda y: s.eigencuts_all(y, 1e-6, 0))
        for count in [c for c in COUNTS if c <= cmax]:
            row = dict(name=name, blocks=len(ns), n=ns[0], m=m, count=count, lib=hb.LIBPATH)
            row["loop_ms"] = med3(lambda: [one(Y[j]) for j in range(count)])
            if a.loop_json is None:
                st0 = hb.check_y_many_stats()
                lmin, _, served = s.check_y_many(Y[:count])
                st1 = hb.check_y_many_stats()
                assert np.all(served == 0)
                ref = np.array([r[0] for r in one(Y[0])])
                assert np.max(np.abs(lmin[0] - ref)) <= 1e-10 * max(1.0, np.max(np.abs(ref)))
                row["launches"], row["readbacks"] = st1[1] - st0[1], st1[2] - st0[2]
                row["many_ms"] = med3(lambda: s.check_y_many(Y[:count]))
                k = min(count, 8)
                t0 = time.perf_counter()
                for j in range(k):
                    for A in blocks:
                        np.linalg.eigvalsh(np.tensordot(Y[j], A[1:], axes=(0, 0)) - A[0])
                row["host_ms"] = 1e3 * (time.perf_counter() - t0) * count / k
                row["bytes_A"] = int(sum(8 * A.size for A in blocks))
            rows.append(row)
            print(json.dumps(row), flush=True)
        s.close()
    if a.loop_json is not None:
        with open(a.loop_json, "w") as f:
            json.dump(rows, f)
        return
    base = {}
    if a.baseline is not None:
        with open(a.baseline) as f:
            base = {(r["name"], r["count"]): r for r in json.load(f)}
    lines = ["# feasibility of `count` candidate points: median ms of 3 calls after a warm-up; ratio = loop (a) of the parent library / hipsdp_check_y_many",
             "# shape              m  count | check_y_many | (a) loop of eigencuts_all[_large](maxcuts = 0): parent library | this build | ratio | (b) numpy, 1 core | launches read-backs | A bytes / t"]
    for r in rows:
        p = base.get((r["name"], r["count"]))
        ptxt = "%10.3f" % p["loop_ms"] if p else "(not measured)"
        ratio = "%7.2f" % (p["loop_ms"] / r["many_ms"]) if p else "    n/a"
        lines.append("%-18s %5d %5d | %12.3f | %14s | %10.3f | %s | %10.1f | %d %d | %.1f GB/s" % (
            r["name"], r["m"], r["count"], r["many_ms"], ptxt, r["loop_ms"], ratio, r["host_ms"], r["launches"], r["readbacks"],
            r["bytes_A"] / (r["many_ms"] * 1e-3) / 1e9))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
