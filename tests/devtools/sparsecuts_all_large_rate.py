"""sparsecuts_all_large_rate.py - what hipsdp_sparsecuts_all_large costs: the sparse cuts of all blocks of 129 .. 512 rows in one call,
variants 0 (default loop), 1 (recomputesparseev), 2 (recomputeinitial), 4 (exacttrans) and 7 (all three).

Problems (m = 25, tol = feastol = 1e-6, maxcuts 5): 4 blocks of 200 rows at target size 10; family "f3" of tests/harness/
sparsecuts_variants_cases.py (blocks of 16, 150, 48, 200, 10 rows: two are served) at size 10; one block of 512 rows at size 24; 8 blocks
of 512 rows at size 24.  Per problem and variant the median of --calls calls after --warmup calls, repeated --reps times (the spread
of the repetitions is printed beside the median).  Beside them
  - variant 0: the loop of hipsdp_sparsecuts over the same blocks, with this build and - --parent-lib PATH - with another build of
    libhipsdp.so, loaded through HIPSDP_LIB in a child process of this script: the parent commit, which has no
    hipsdp_sparsecuts_all_large, on the same box;
  - the other variants: the numpy restatement (tests/harness/sparsecuts_variants_ref.py) on one host core, --host-calls times.
Launches and read-backs are the differences of hipsdp_sparsecuts_all_large_stats over one call.  The pass mark: at variant 0 with 4
blocks of 200 rows the call is faster than the parent's loop by more than three times the spread of the repetitions.

    python tests/devtools/sparsecuts_all_large_rate.py [--parent-lib PATH] [--out profiles/r25_sparsecuts_all_large_rate.txt]"""
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
#            label                 rows of the blocks (None: family f3)   size
PROBLEMS = [("4 blocks of 200", [200] * 4, 10), ("f3: 150 and 200", None, 10), ("1 block of 512", [512], 24), ("8 blocks of 512", [512] * 8, 24)]
VARIANTS = [0, 1, 2, 4, 7]
TOL, FEASTOL, MAXCUTS = 1e-6, 1e-6, 5


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


def loops(a, hb):
    """the loop of hipsdp_sparsecuts over the large blocks of every problem: {label: medians}"""
    import test_gpu_sparsecuts_all as T
    out = {}
    for label, ns, size in PROBLEMS:
        blocks, ys, y, b = problem(ns)
        large = [k for k, A in enumerate(blocks) if 128 < A.shape[1] <= 512]
        s = T.load_dense(hb, blocks, b)
        out[label] = timed(lambda: [s.sparsecuts(k, y, size, TOL, FEASTOL, MAXCUTS) for k in large], a.calls, a.warmup, a.reps)
        s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=1)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--loop-only", action="store_true", help="print the loop timings as JSON and stop (the child of --parent-lib)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hb = binding()
    if a.loop_only:
        print(json.dumps(loops(a, hb)))
        return
    import sparsecuts_variants_ref as V
    import test_gpu_sparsecuts_all as T
    parent = None
    if a.parent_lib:
        env = dict(os.environ)
        env["HIPSDP_LIB"] = os.path.abspath(a.parent_lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", "--calls", str(a.calls), "--warmup", str(a.warmup),
                            "--reps", str(a.reps)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-3000:])
            raise SystemExit("the child with the parent library failed")
        parent = json.loads(r.stdout.strip().splitlines()[-1])
    mine = loops(a, hb)
    med = lambda v: float(np.median(v))
    rows = []
    for label, ns, size in PROBLEMS:
        blocks, ys, y, b = problem(ns)
        large = [k for k, A in enumerate(blocks) if 128 < A.shape[1] <= 512]
        s = T.load_dense(hb, blocks, b)
        sizes = [size] * len(blocks)
        for variant in VARIANTS:
            call = lambda: s.sparsecuts_all_large(y, sizes, TOL, FEASTOL, MAXCUTS, variant)
            call()
            st0 = hb.sparsecuts_all_large_stats()
            res = call()
            st1 = hb.sparsecuts_all_large_stats()
            row = dict(name=label, blocks=len(large), size=size, variant=variant, cuts=int(sum(max(r[0], 0) for r in res)),
                       iters=int(sum(r[6] for r in res)), launches=st1[1] - st0[1], readbacks=st1[2] - st0[2])
            row["ms"] = timed(call, a.calls, a.warmup, a.reps)
            if variant == 0:
                row["loop_ms"] = mine[label]
                row["parent_ms"] = parent[label] if parent else None
            else:
                row["host_ms"] = timed(lambda: [V.sparse_cuts_dense_ex(blocks[k], y, size, TOL, FEASTOL, MAXCUTS, variant) for k in large],
                                       a.host_calls, 0, 1)
            rows.append(row)
        s.close()
    rng = lambda v: "%.3f [%.3f .. %.3f]" % (med(v), min(v), max(v))
    lines = ["# sparse eigenvector cuts of all blocks of 129 .. 512 rows in one call (hipsdp_sparsecuts_all_large; m = 25, tol = feastol 1e-6, "
             "maxcuts 5): median ms of %d calls, [min .. max] of %d repetitions" % (a.calls, a.reps),
             "# problem          served size variant cuts TPower-iterations | the call | beside it | launches read-backs"]
    for r in rows:
        if r["variant"] == 0:
            beside = "loop of hipsdp_sparsecuts, this build: %s" % rng(r["loop_ms"])
            if r["parent_ms"]:
                beside += "; parent build: %s (x %.2f)" % (rng(r["parent_ms"]), med(r["parent_ms"]) / med(r["ms"]))
        else:
            beside = "restatement, 1 core: %.1f (x %.1f)" % (med(r["host_ms"]), med(r["host_ms"]) / med(r["ms"]))
        lines.append("%-18s %5d %4d %7d %4d %7d | %s | %s | %d %d" % (r["name"], r["blocks"], r["size"], r["variant"], r["cuts"], r["iters"],
                                                                   rng(r["ms"]), beside, r["launches"], r["readbacks"]))
    r0 = rows[0]
    ref = r0["parent_ms"] or r0["loop_ms"]
    margin = med(ref) - med(r0["ms"])
    spread = max(max(r0["ms"]) - min(r0["ms"]), max(ref) - min(ref))
    lines.append("# pass mark (variant 0, 4 blocks of 200 rows): the call %.3f ms, the %s loop %.3f ms, margin %.3f ms, spread of the repetitions "
                 "%.3f ms: %s" % (med(r0["ms"]), "parent's" if r0["parent_ms"] else "present build's", med(ref), margin, spread,
                                  "PASS" if margin > 3.0 * spread else "FAIL"))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
