"""sparsecuts_all_rate.py - time of the sparse eigenvector cuts of all blocks in one call: hipsdp_sparsecuts_all against the numpy
restatement (tests/harness/sparsecuts_ref.py) on one host core, with hipsdp_eigencuts_all on the same family for scale.

Problems: the four families of tests/test_gpu_sparsecuts_all.py at target size 4 and 10 (tol = feastol = 1e-6, maxcuts 5; the
blocks of 150 and 200 rows of the fourth family are not served and take no part in either column of the sparse cuts).  Per problem
the median of --calls calls after --warmup calls, repeated --reps times (the spread of the repetitions is printed beside the
median); the restatement is timed --host-calls times.  The launch and read-back counts are the differences of
hipsdp_sparsecuts_all_stats over one call.

    python tests/devtools/sparsecuts_all_rate.py [--out profiles/r16_sparsecuts_all_rate.txt]"""
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
NAMES = ["9 blocks 3..128", "32 blocks of 12", "4 blocks of 40", "16,(150),48,(200),10"]


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
    import sparsecuts_ref as R
    import test_gpu_sparsecuts_all as T
    hb = binding()
    rows = []
    for fam in range(4):
        blocks, ys, y, b = T.family(fam)
        s = T.load_dense(hb, blocks, b)
        nb = len(blocks)
        ec = timed(lambda: s.eigencuts_all(y, T.TOL, T.MAXCUTS), a.calls, a.warmup, a.reps)
        for size in (4, 10):
            sizes = [size] * nb
            s.sparsecuts_all(y, sizes, T.TOL, T.FEASTOL, T.MAXCUTS)
            st0 = hb.sparsecuts_all_stats()
            res = s.sparsecuts_all(y, sizes, T.TOL, T.FEASTOL, T.MAXCUTS)
            st1 = hb.sparsecuts_all_stats()
            row = dict(name=NAMES[fam], blocks=nb, size=size, cuts=int(sum(max(r[0], 0) for r in res)), iters=int(sum(r[6] for r in res)),
                       launches=st1[1] - st0[1], readbacks=st1[2] - st0[2], ec_ms=ec)
            row["all_ms"] = timed(lambda: s.sparsecuts_all(y, sizes, T.TOL, T.FEASTOL, T.MAXCUTS), a.calls, a.warmup, a.reps)
            row["all0_ms"] = timed(lambda: s.sparsecuts_all(y, sizes, T.TOL, T.FEASTOL, 0), a.calls, a.warmup, a.reps)
            host = [A for A in blocks if A.shape[1] <= 128]
            row["host_ms"] = timed(lambda: [R.sparse_cuts_dense(A, y, size, T.TOL, T.FEASTOL, T.MAXCUTS) for A in host], a.host_calls, 1, 1)
            rows.append(row)
        s.close()
    med = lambda v: float(np.median(v))
    lines = ["# sparse eigenvector cuts of all blocks (tol = feastol 1e-6, maxcuts 5): median ms of %d calls, [min .. max] of %d repetitions"
             % (a.calls, a.reps),
             "# problem              blocks size cuts TPower-iterations | sparsecuts_all        | same, maxcuts = 0     | restatement, 1 core "
             "| eigencuts_all (dense cuts) | launches read-backs"]
    for r in rows:
        lines.append("%-22s %5d %4d %4d %7d | %8.3f [%.3f .. %.3f] | %8.3f [%.3f .. %.3f] | %9.2f | %8.3f [%.3f .. %.3f] | %d %d" % (
            r["name"], r["blocks"], r["size"], r["cuts"], r["iters"], med(r["all_ms"]), min(r["all_ms"]), max(r["all_ms"]),
            med(r["all0_ms"]), min(r["all0_ms"]), max(r["all0_ms"]), med(r["host_ms"]), med(r["ec_ms"]), min(r["ec_ms"]), max(r["ec_ms"]),
            r["launches"], r["readbacks"]))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
