"""onevar_all_rate.py - time of a round of one-variable SDPs over ALL blocks of a solver: hipsdp_onevar_bounds_all against
  (a) the loop of hipsdp_onevar_bounds over the blocks - what a caller had before the call existed - on the library under test and,
      with --loop-lib, on the PARENT commit's build (a child process with HIPSDP_LIB=<that libhipsdp.so>),
  (b) the numpy restatement (tests/onevar_cases.py) on one host core.
For the EXTREMES-only round (a) is a loop of hipsdp_syevi_small, two calls per matrix (ith = 1 and ith = n, no eigenvector): the
SCIPlapackComputeIthEigenvalue calls of computeAllmatricespsd and of the lock computation; (b) is numpy.linalg.eigvalsh.

Rounds (u = ub, feastol 1e-6, all variables of every block): 32 blocks of 12 rows (m = 12), 4 blocks of 40 rows (m = 30), the
five-block mix of the tests (3, 17, 64, 65, 128 rows, m = 6), 2 blocks of 128 rows (m = 12), and EXTREMES over the 32 blocks of 12
rows.  Per round the median of --calls calls after --warmup calls, repeated --reps times (the spread of the repetitions is printed
beside the median); (b) is timed --host-calls times.  Launches and read-backs are the differences of the two stats calls over one
round.

    python tests/devtools/onevar_all_rate.py [--loop-lib PARENT/libhipsdp.so] [--out profiles/r23_onevar_bounds_all_rate.txt]"""
import argparse
import ctypes as C
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
# name, [(rows, rank)], m, EXTREMES only
ROUNDS = [("32 x 12 rows", [(12, 2)] * 32, 12, False), ("4 x 40 rows", [(40, 4)] * 4, 30, False),
          ("3 17 64 65 128 rows", None, 6, False), ("2 x 128 rows", [(128, 12)] * 2, 12, False),
          ("EXTREMES, 32 x 12 rows", [(12, 2)] * 32, 12, True)]


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


def round_data(K, KA, spec, m):
    """(blocks, lb, ub): equal blocks differ by their seed, so no two blocks of a round hold the same matrices"""
    if spec is None:
        return KA.multi_family(1, 0.6, 0.0, 0)
    seen = {}
    rng = np.random.default_rng([m, 1, 77])
    ub = rng.uniform(0.5, 2.0, m)
    lb = np.where(rng.uniform(0.0, 1.0, m) < 0.5, -rng.uniform(0.0, 0.5, m), 0.0)
    blocks = []
    for n, rank in spec:
        seen[n] = seen.get(n, 0) + 1
        A = np.array(K.family(n, m, rank, seen[n], 0.0, 0.0, 0)[0])
        A[0] = 0.6 * np.tensordot(ub, A[1:], axes=1)
        blocks.append(A)
    return blocks, lb, ub


def load(hb, blocks, m):
    import ipm_ref
    s = hb.Solver(0)
    s.load_core(ipm_ref.CoreProblem(np.ones(m), list(blocks), None, None))
    return s


def loop_of_blocks(s, nb, lb, ub, feastol):
    return [s.onevar_bounds(b, ub, lb, ub, feastol) for b in range(nb)]


def loop_of_syevi(lib, mats):
    """two hipsdp_syevi_small calls per matrix: the smallest and the largest eigenvalue, no eigenvector"""
    val = C.c_double(0.0)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out = []
    for M in mats:
        n = M.shape[0]
        pair = []
        for ith in (1, n):
            rc = lib.hipsdp_syevi_small(0, n, pd(M), ith, C.byref(val), None)
            assert rc == 0, rc
            pair.append(val.value)
        out.append(pair)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--loop-lib", default=None, help="libhipsdp.so of the parent commit: the loops once more on it, in a child process")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import onevar_cases as K
    import onevar_all_cases as KA
    hb = binding()
    lib = hb.lib()
    other = None
    if a.loop_lib and not a.loop_only:
        env = dict(os.environ, HIPSDP_LIB=os.path.abspath(a.loop_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", "--calls", str(a.calls), "--warmup", str(a.warmup),
                            "--reps", str(a.reps)], env=env, stdout=subprocess.PIPE, text=True, timeout=500)
        other = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None
    rows, loops = [], {}
    for name, spec, m, extremes in ROUNDS:
        blocks, lb, ub = round_data(K, KA, spec, m)
        nb = len(blocks)
        s = load(hb, blocks, m)
        mats = [np.ascontiguousarray(A[i + 1]) for A in blocks for i in range(m)]
        if extremes:
            loop = lambda: loop_of_syevi(lib, mats)
        else:
            loop = lambda: loop_of_blocks(s, nb, lb, ub, K.FEASTOL)
        loop_ms = timed(loop, a.calls, a.warmup, a.reps)
        loops[name] = loop_ms
        if a.loop_only:
            s.close()
            continue
        lbj, ubj = np.tile(lb, nb), np.tile(ub, nb)
        kind = np.full(nb * m, KA.EXTREMES, dtype=np.int32) if extremes else None
        call = lambda: s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, kind=kind)
        call()
        c0, o0 = hb.onevar_bounds_all_stats(), hb.onevar_bounds_stats()
        res = call()
        c1 = hb.onevar_bounds_all_stats()
        ref = loop()
        o1 = hb.onevar_bounds_stats()
        if extremes:
            same = bool(np.max(np.abs(res[2] - np.array([p[0] for p in ref]))) <= 1e-12 * np.max(np.abs(res[1]))
                        and np.max(np.abs(res[1] - np.array([p[1] for p in ref]))) <= 1e-12 * np.max(np.abs(res[1])))
            numpy_fn = lambda: [np.linalg.eigvalsh(M)[[0, -1]] for M in mats]
            loop_launches, loop_readbacks = 2 * len(mats), 2 * len(mats)
        else:
            same = all(np.concatenate([p[k] for p in ref]).tobytes() == np.asarray(res[k]).tobytes() for k in range(5))
            numpy_fn = lambda: [K.onevar_ref(K.z_of(A, ub), A[i + 1], ub[i], K.NEWTON, lb[i], ub[i], K.FEASTOL) for A in blocks
                                for i in range(m)]
            loop_launches, loop_readbacks = o1[1] - o0[1], o1[2] - o0[2]
        row = dict(name=name, blocks=nb, jobs=nb * m, evals=int(res[4].sum()), launches=c1[1] - c0[1], readbacks=c1[2] - c0[2],
                   loop_launches=loop_launches, loop_readbacks=loop_readbacks, same=same, loop_ms=loop_ms,
                   parent_ms=None if other is None else other[name],
                   statuses=[int(np.sum(res[0] == k)) for k in (K.LB, K.INNER, K.INFEASIBLE, KA.DONE)])
        row["call_ms"] = timed(call, a.calls, a.warmup, a.reps)
        row["numpy_ms"] = timed(numpy_fn, a.host_calls, 1, 1)
        rows.append(row)
        s.close()
    if a.loop_only:
        print(json.dumps(loops))
        return
    med = lambda v: float(np.median(v))
    lines = ["# a round of one-variable SDPs over all blocks (u = ub, feastol 1e-6, every variable of every block): median ms of %d calls, "
             "[min .. max] of %d repetitions; restatement: median of %d" % (a.calls, a.reps, a.host_calls),
             "# (a) the loop of hipsdp_onevar_bounds over the blocks (EXTREMES: of hipsdp_syevi_small, two per matrix) on this build, "
             "(a') the same loop on the parent commit's build%s" % ("" if other is not None else " - NOT MEASURED (no --loop-lib)"),
             "# round                   blocks jobs LB/INNER/INFEASIBLE/DONE evaluations | onevar_bounds_all      launches read-backs | "
             "(a) loop ms              launches read-backs  ratio | (a') parent ms  ratio | restatement, 1 core  ratio | same results"]
    for r in rows:
        pm = r["parent_ms"]
        lines.append("%-25s %5d %5d %3d/%3d/%3d/%3d %8d | %8.3f [%.3f .. %.3f] %4d %4d | %8.3f [%.3f .. %.3f] %4d %4d %6.1fx | %9s %7s | "
                     "%9.2f %7.1fx | %s" % (
                         r["name"], r["blocks"], r["jobs"], r["statuses"][0], r["statuses"][1], r["statuses"][2], r["statuses"][3],
                         r["evals"], med(r["call_ms"]), min(r["call_ms"]), max(r["call_ms"]), r["launches"], r["readbacks"],
                         med(r["loop_ms"]), min(r["loop_ms"]), max(r["loop_ms"]), r["loop_launches"], r["loop_readbacks"],
                         med(r["loop_ms"]) / med(r["call_ms"]), "-" if pm is None else "%.3f" % med(pm),
                         "-" if pm is None else "%.1fx" % (med(pm) / med(r["call_ms"])), med(r["numpy_ms"]),
                         med(r["numpy_ms"]) / med(r["call_ms"]), "bits equal" if r["same"] and "EXTREMES" not in r["name"] else
                         ("within 1e-12" if r["same"] else "DIFFERENT")))
    lines.append("# not measured: blocks kept as nonzeros or as packed triangles alone, rounds with u = 0 (tightenMatrices), rounds inside a "
                 "running branch-and-bound, more than one host thread, the call beside other work on the device")
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
