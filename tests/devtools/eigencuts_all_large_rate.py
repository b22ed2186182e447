"""eigencuts_all_large_rate.py - what hipsdp_eigencuts_all_large costs: the dense eigenvector cuts of all blocks of 129 .. 512 rows in
one call.

Problems (m = 25, tol 1e-6, maxcuts 5): one block of 512 rows; 4 blocks of 200 rows; 8 blocks of 512 rows; family "f3" of tests/harness/
sparsecuts_variants_cases.py (blocks of 16, 150, 48, 200, 10 rows: two are served).  Per problem the median of --calls calls after
--warmup calls, repeated --reps times (the spread of the repetitions is printed beside the median).  Beside the call
  - what a caller had before: hipsdp_eigencuts_all on the same solver, which serves these blocks one after the other on the per-block
    path - with this build and, --parent-lib PATH, with another build of libhipsdp.so, loaded through HIPSDP_LIB in a child process of
    this script: the parent commit, which has no hipsdp_eigencuts_all_large, on the same box;
  - the numpy oracle (oracle/eigcuts_ref.cuts_dense) on one host core, --host-calls times.
The share of the coefficient launch is the call's time minus the time of the same call with maxcuts = 0 (which leaves out the two
vector launches as well: an upper bound).  Launches and read-backs are the differences of hipsdp_eigencuts_all_large_stats over one call.
The pass mark, per row: the call is faster than the parent's hipsdp_eigencuts_all by more than the larger of the two spreads.

    python tests/devtools/eigencuts_all_large_rate.py [--parent-lib PATH] [--out profiles/r26_eigencuts_all_large_rate.txt]"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "harness"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
M = 25
#            label                 rows of the blocks (None: family f3)
PROBLEMS = [("1 block of 512", [512]), ("4 blocks of 200", [200] * 4), ("8 blocks of 512", [512] * 8), ("f3: 150 and 200", None)]
TOL, MAXCUTS = 1e-6, 5


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def problem(ns):
    """(blocks, ys, y, b): f3, or blocks built the way its family is - block k is instances.planted_dense(n_k, 25, seed = 31000 + k)
    with the constant matrix rebuilt around the ys of block 0, y = ys + 0.7 N(0, 1)"""
    import instances
    import sparsecuts_variants_cases as K
    if ns is None:
        return K.family("f3")
    blocks, ys, b = [], None, np.zeros(M)
    for k, n in enumerate(ns):
        _, A, ysk, Xs, Zs = instances.planted_dense(n, M, seed=31000 + k)
        if k == 0:
            ys = ysk
        A = A.copy()
        A0 = np.tensordot(ys, A[1:], axes=(0, 0)) - Zs
        A[0] = 0.5 * (A0 + A0.T)
        b += A[1:].reshape(M, -1) @ Xs.reshape(-1)
        blocks.append(A)
    return blocks, ys, ys + 0.7 * np.random.default_rng(len(ns)).standard_normal(M), b


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


def before(a, hb):
    """hipsdp_eigencuts_all on every problem (the per-block path for its large blocks): {label: medians}"""
    import test_gpu_eigencuts_all as T
    out = {}
    for label, ns in PROBLEMS:
        blocks, ys, y, b = problem(ns)
        s = T.load_dense(hb, blocks, b)
        out[label] = timed(lambda: s.eigencuts_all(y, TOL, MAXCUTS), a.calls, a.warmup, a.reps)
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--before-only", action="store_true", help="print the timings of hipsdp_eigencuts_all as JSON and stop (the child of --parent-lib)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hb = binding()
    if a.before_only:
        print(json.dumps(before(a, hb)))
        return
    import eigcuts_ref
    import test_gpu_eigencuts_all as T
    parent = None
    if a.parent_lib:
        env = dict(os.environ)
        env["HIPSDP_LIB"] = os.path.abspath(a.parent_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--before-only", "--calls", str(a.calls), "--warmup", str(a.warmup),
                            "--reps", str(a.reps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit("the child with the parent library failed")
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    mine = before(a, hb)
    med = lambda v: float(np.median(v))
    rows = []
    for label, ns in PROBLEMS:
        blocks, ys, y, b = problem(ns)
        large = [k for k, A in enumerate(blocks) if 128 < A.shape[1] <= 512]
        s = T.load_dense(hb, blocks, b)
        call = lambda: s.eigencuts_all_large(y, TOL, MAXCUTS)
        call()
        st0 = hb.eigencuts_all_large_stats()
        res = call()
        st1 = hb.eigencuts_all_large_stats()
        row = dict(name=label, blocks=len(large), cuts=int(sum(len(r[1]) for r in res if r is not None)), launches=st1[1] - st0[1],
                   readbacks=st1[2] - st0[2])
        row["ms"] = timed(call, a.calls, a.warmup, a.reps)
        row["feas_ms"] = timed(lambda: s.eigencuts_all_large(y, TOL, 0), a.calls, a.warmup, a.reps)
        row["before_ms"] = mine[label]
        row["parent_ms"] = parent[label] if parent else None
        row["host_ms"] = timed(lambda: [eigcuts_ref.cuts_dense(blocks[k], y, TOL, MAXCUTS) for k in large], a.host_calls, 0, 1)
        rows.append(row)
        s.close()
    rng = lambda v: "%.3f [%.3f .. %.3f]" % (med(v), min(v), max(v))
    lines = ["# dense eigenvector cuts of all blocks of 129 .. 512 rows in one call (hipsdp_eigencuts_all_large; m = 25, tol 1e-6, maxcuts 5): "
             "median ms of %d calls, [min .. max] of %d repetitions" % (a.calls, a.reps),
             "# problem          served cuts | the call | maxcuts = 0 | vectors + coefficients: share of the call | hipsdp_eigencuts_all, this build"
             " | parent build | numpy oracle, 1 core | launches read-backs | faster than the parent by more than the spreads"]
    for r in rows:
        ref = r["parent_ms"] or r["before_ms"]
        margin = med(ref) - med(r["ms"])
        spread = max(max(r["ms"]) - min(r["ms"]), max(ref) - min(ref))
        verdict = "%s (margin %.3f, spread %.3f%s)" % ("PASS" if margin > spread else "FAIL", margin, spread, "" if r["parent_ms"] else "; this build, no parent given")
        share = (med(r["ms"]) - med(r["feas_ms"])) / med(r["ms"])
        lines.append("%-18s %5d %4d | %s | %s | %.3f ms = %.1f %% | %s | %s | %.1f (x %.1f) | %d %d | %s" %
                     (r["name"], r["blocks"], r["cuts"], rng(r["ms"]), rng(r["feas_ms"]), med(r["ms"]) - med(r["feas_ms"]), 100.0 * share,
                      rng(r["before_ms"]), ("%s (x %.2f)" % (rng(r["parent_ms"]), med(r["parent_ms"]) / med(r["ms"]))) if r["parent_ms"] else "-",
                      med(r["host_ms"]), med(r["host_ms"]) / med(r["ms"]), r["launches"], r["readbacks"], verdict))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
