"""onevar_rate.py - time of all one-variable SDPs of a block in one call: hipsdp_onevar_bounds against
  (a) the same Newton loop on the host with one hipsdp_syevi_small per evaluation - what a caller had before the call existed (the
      SCIPlapackComputeIthEigenvalue of lapack_interface_hip.c inside SCIPsolveOneVarSDPDense: a launch and a host wait per eigenpair;
      the host forms M(mu) and the supergradient with numpy),
  (b) the numpy restatement (tests/onevar_cases.py) on one host core.

Blocks of the family of tests/onevar_cases.py (t = 0.6, seed 1, u = ub, feastol 1e-6): 12 rows with 32 jobs, 40 rows with 30 jobs,
128 rows with 12 jobs.  Per block the median of --calls calls after --warmup calls, repeated --reps times (the spread of the
repetitions is printed beside the median); (a) and (b) are timed --host-calls times.  Launches and read-backs are the differences of
hipsdp_onevar_bounds_stats over one call; the evaluations are the sum of the call's evals.

    python tests/devtools/onevar_rate.py [--out profiles/r21_onevar_bounds_rate.txt]"""
import argparse
import ctypes as C
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
BLOCKS = [(12, 32, 2), (40, 30, 4), (128, 12, 12)]           # (rows, jobs, rank)


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


def per_evaluation_loop(lib, K, Z, A, lb, ub, feastol):
    """the Newton loop of every variable on the host, the eigenpair of every evaluation by one hipsdp_syevi_small"""
    n = Z.shape[0]
    val = C.c_double(0.0)
    vec = np.zeros(n)
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    out, evals = [], 0
    for i in range(len(lb)):
        Ai, ui = A[i + 1], ub[i]

        def f(mu):
            M = np.ascontiguousarray(Z + (mu - ui) * Ai)
            rc = lib.hipsdp_syevi_small(0, n, pd(M), 1, C.byref(val), pd(vec))
            assert rc == 0, rc
            return val.value, float(vec @ Ai @ vec)

        cnt = 1
        ev, g = f(ub[i])
        if ev < -feastol and g > 0.0:
            out.append((K.INFEASIBLE, ub[i])); evals += cnt
            continue
        ev, g = f(lb[i]); cnt += 1
        if ev >= -feastol:
            out.append((K.LB, lb[i])); evals += cnt
            continue
        if g <= 0.0:
            out.append((K.INFEASIBLE, lb[i])); evals += cnt
            continue
        mu = lb[i]
        while ev < -feastol and g > 0.0 and cnt < 100:
            mu = mu - (feastol / 2.0 + ev) / g
            if mu > ub[i]:
                break
            ev, g = f(mu); cnt += 1
        out.append((K.INFEASIBLE if ev < -feastol else K.INNER, mu)); evals += cnt
    return out, evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import onevar_cases as K
    import test_gpu_sparsecuts_all as T
    hb = binding()
    lib = hb.lib()
    rows = []
    for n, m, rank in BLOCKS:
        A, lb, ub = K.family(n, m, rank, 1, 0.6, 0.0, 0)
        Z = K.z_of(A, ub)
        s = T.load_dense(hb, [A], np.ones(m))
        s.onevar_bounds(0, ub, lb, ub, K.FEASTOL)
        st0 = hb.onevar_bounds_stats()
        res = s.onevar_bounds(0, ub, lb, ub, K.FEASTOL)
        st1 = hb.onevar_bounds_stats()
        loop, loop_evals = per_evaluation_loop(lib, K, Z, A, lb, ub, K.FEASTOL)
        row = dict(n=n, jobs=m, evals=int(res[4].sum()), loop_evals=loop_evals, launches=st1[1] - st0[1], readbacks=st1[2] - st0[2],
                   same_status=int(sum(int(res[0][i]) == loop[i][0] for i in range(m))),
                   statuses=[int(np.sum(res[0] == k)) for k in (K.LB, K.INNER, K.INFEASIBLE)])
        row["call_ms"] = timed(lambda: s.onevar_bounds(0, ub, lb, ub, K.FEASTOL), a.calls, a.warmup, a.reps)
        row["loop_ms"] = timed(lambda: per_evaluation_loop(lib, K, Z, A, lb, ub, K.FEASTOL), a.host_calls, 1, 1)
        row["numpy_ms"] = timed(lambda: [K.onevar_ref(Z, A[i + 1], ub[i], K.NEWTON, lb[i], ub[i], K.FEASTOL) for i in range(m)],
                                a.host_calls, 1, 1)
        rows.append(row)
        s.close()
    med = lambda v: float(np.median(v))
    lines = ["# all one-variable SDPs of a block (u = ub, feastol 1e-6): median ms of %d calls, [min .. max] of %d repetitions; host columns: "
             "median of %d" % (a.calls, a.reps, a.host_calls),
             "# rows jobs LB/INNER/INFEASIBLE evaluations | onevar_bounds         | host loop, one syevi_small per evaluation | ratio "
             "| restatement, 1 core | launches read-backs"]
    for r in rows:
        lines.append("%5d %4d %3d/%3d/%3d %7d | %8.3f [%.3f .. %.3f] | %9.3f (%d evaluations, %d statuses equal) | %5.1fx | %9.2f | %d %d" % (
            r["n"], r["jobs"], r["statuses"][0], r["statuses"][1], r["statuses"][2], r["evals"], med(r["call_ms"]), min(r["call_ms"]),
            max(r["call_ms"]), med(r["loop_ms"]), r["loop_evals"], r["same_status"], med(r["loop_ms"]) / med(r["call_ms"]),
            med(r["numpy_ms"]), r["launches"], r["readbacks"]))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
