"""sparsecuts_variants_rate.py - what the reference's three switches cost on the device: hipsdp_sparsecuts_all_ex with variant 0
(= hipsdp_sparsecuts_all), 1 (recomputesparseev), 2 (recomputeinitial), 4 (exacttrans) and 7 (all three) against the numpy restatement
(tests/harness/sparsecuts_variants_ref.py) on one host core.

Problems: the three families of tests/harness/sparsecuts_variants_cases.py that the README row quotes - 32 blocks of 12 rows at
target size 4, 4 blocks of 40 rows at size 10, the nine blocks of 3 .. 128 rows at size 10 (tol = feastol = 1e-6, maxcuts 5).  Per
problem and variant the median of --calls calls after --warmup calls, repeated --reps times (the spread of the repetitions is printed
beside the median); the restatement is timed --host-calls times.  Launches and read-backs are the differences of the call's stats
(hipsdp_sparsecuts_all_stats for variant 0, hipsdp_sparsecuts_ex_stats otherwise) over one call.

    python tests/devtools/sparsecuts_variants_rate.py [--out profiles/r20_sparsecuts_variants_rate.txt]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
PROBLEMS = [("r12", 4, "32 blocks of 12"), ("b40", 10, "4 blocks of 40"), ("f0", 10, "9 blocks 3..128")]
VARIANTS = [0, 1, 2, 4, 7]


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, calls, warmup, reps):
    """medians (ms) of `reps` repetitions of `calls` calls"""
    for _ in range(warmup):
        fn()
    meds = []
    for _ in range(reps):
        ts = []
        for _ in range(calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        meds.append(1e3 * float(np.median(ts)))
    return meds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sparsecuts_variants_ref as V
    import sparsecuts_variants_cases as K
    import test_gpu_sparsecuts_all as T
    hb = binding()
    rows = []
    for name, size, label in PROBLEMS:
        blocks, ys, y, b = K.family(name)
        s = T.load_dense(hb, blocks, b)
        sizes = [size] * len(blocks)
        base = None
        for variant in VARIANTS:
            call = lambda: s.sparsecuts_all_ex(y, sizes, K.TOL, K.FEASTOL, K.MAXCUTS, variant)
            stats = hb.sparsecuts_all_stats if variant == 0 else hb.sparsecuts_ex_stats
            call()
            st0 = stats()
            res = call()
            st1 = stats()
            row = dict(name=label, blocks=len(blocks), size=size, variant=variant, cuts=int(sum(max(r[0], 0) for r in res)),
                       iters=int(sum(r[6] for r in res)), launches=st1[1] - st0[1], readbacks=st1[2] - st0[2])
            row["ms"] = timed(call, a.calls, a.warmup, a.reps)
            row["host_ms"] = timed(lambda: [V.sparse_cuts_dense_ex(A, y, size, K.TOL, K.FEASTOL, K.MAXCUTS, variant) for A in blocks],
                                   a.host_calls, 1, 1)
            if variant == 0:
                base = float(np.median(row["ms"]))
            row["over0"] = float(np.median(row["ms"])) / base
            rows.append(row)
        s.close()
    med = lambda v: float(np.median(v))
    lines = ["# sparse eigenvector cuts of all blocks with the switches recomputesparseev (1), recomputeinitial (2), exacttrans (4) "
             "(tol = feastol 1e-6, maxcuts 5): median ms of %d calls, [min .. max] of %d repetitions" % (a.calls, a.reps),
             "# problem          blocks size variant cuts TPower-iterations | sparsecuts_all_ex     | x variant 0 | restatement, 1 core "
             "| host / device | launches read-backs"]
    for r in rows:
        lines.append("%-18s %5d %4d %7d %4d %7d | %8.3f [%.3f .. %.3f] | %6.2f | %9.2f | %6.2f | %d %d" % (
            r["name"], r["blocks"], r["size"], r["variant"], r["cuts"], r["iters"], med(r["ms"]), min(r["ms"]), max(r["ms"]), r["over0"],
            med(r["host_ms"]), med(r["host_ms"]) / med(r["ms"]), r["launches"], r["readbacks"]))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
