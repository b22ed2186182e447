"""sparsecuts_large_rate.py - time of the sparse eigenvector cuts of ONE block of 129 .. 512 rows: hipsdp_sparsecuts against the
numpy restatement (tests/harness/sparsecuts_ref.py, its eigh included) on one host core, with hipsdp_eigencuts (dense cuts) on the
same block for scale.

Problems: the rows of tests/harness/sparsecuts_large_cases.TABLE with 150, 200, 257 and 512 rows (tol = feastol = 1e-6, maxcuts 5),
each block loaded dense and alone.  Per problem the median of --calls calls after --warmup calls, repeated --reps times (the spread
of the repetitions is printed beside the median); the restatement is timed --host-calls times, hipsdp_eigencuts --calls / 3 times.
The same call with maxcuts = 0 stops behind the smallest eigenvalue: it is the share of Z(y) and the tridiagonalisation; the
difference to the full call, over the TPower iterations, bounds the cost of one iteration from above (it also holds the two vector
launches, the second eigenvalue, the fill of MT and the coefficients).  The launch and read-back counts are the differences of
hipsdp_sparsecuts_stats over one call.

    python tests/devtools/sparsecuts_large_rate.py [--out profiles/r17_sparsecuts_large_rate.txt]"""
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
ROWS = ("f4b1", "f4b3", "n257", "n512")


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
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ipm_ref
    import sparsecuts_ref as R
    import sparsecuts_large_cases as L
    hb = binding()
    rows = []
    for name, spec, size, cuts, its in L.TABLE:
        if name not in ROWS:
            continue
        A, ys, y, b = L.block(spec)
        n = A.shape[1]
        s = hb.Solver(0)
        s.load_core(ipm_ref.CoreProblem(b, [A], None, None))
        s.sparsecuts(0, y, size, L.TOL, L.FEASTOL, L.MAXCUTS)
        st0 = hb.sparsecuts_stats()
        res = s.sparsecuts(0, y, size, L.TOL, L.FEASTOL, L.MAXCUTS)
        st1 = hb.sparsecuts_stats()
        row = dict(name=name, n=n, size=size, cuts=int(res[0]), iters=int(res[6]), launches=st1[1] - st0[1], readbacks=st1[2] - st0[2])
        assert (row["cuts"], row["iters"]) == (cuts, its), row
        row["one_ms"] = timed(lambda: s.sparsecuts(0, y, size, L.TOL, L.FEASTOL, L.MAXCUTS), a.calls, a.warmup, a.reps)
        row["one0_ms"] = timed(lambda: s.sparsecuts(0, y, size, L.TOL, L.FEASTOL, 0), a.calls, a.warmup, a.reps)
        row["ec_ms"] = timed(lambda: s.eigencuts(0, y, L.TOL, L.MAXCUTS), max(1, a.calls // 3), 2, a.reps)
        row["host_ms"] = timed(lambda: R.sparse_cuts_dense(A, y, size, L.TOL, L.FEASTOL, L.MAXCUTS), a.host_calls, 1, 1)
        s.close()
        rows.append(row)
    med = lambda v: float(np.median(v))
    lines = ["# sparse eigenvector cuts of one block (tol = feastol 1e-6, maxcuts 5): median ms of %d calls, [min .. max] of %d repetitions"
             % (a.calls, a.reps),
             "# rows size cuts TPower-iterations | sparsecuts             | same, maxcuts = 0       | us per iteration (difference) "
             "| restatement, 1 core | eigencuts (dense cuts)  | launches read-backs"]
    for r in rows:
        per = 1e3 * (med(r["one_ms"]) - med(r["one0_ms"])) / max(1, r["iters"])
        lines.append("%5d %4d %4d %7d | %8.3f [%.3f .. %.3f] | %8.3f [%.3f .. %.3f] | %7.2f | %9.2f | %8.3f [%.3f .. %.3f] | %d %d" % (
            r["n"], r["size"], r["cuts"], r["iters"], med(r["one_ms"]), min(r["one_ms"]), max(r["one_ms"]),
            med(r["one0_ms"]), min(r["one0_ms"]), max(r["one0_ms"]), per, med(r["host_ms"]), med(r["ec_ms"]), min(r["ec_ms"]),
            max(r["ec_ms"]), r["launches"], r["readbacks"]))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
