"""onevar_large_rate.py - time of a round of one-variable SDPs on blocks of 129 .. 512 rows: hipsdp_onevar_bounds_large against
  (a') what a caller had before the call existed: the Newton loop of every job ON THE HOST with one hipsdp_syevx(il = iu = 1) per
       evaluation (M(mu) formed with numpy, g = v^T A_i v with numpy), run on the PARENT commit's build in a child process with
       HIPSDP_LIB=<that libhipsdp.so> (--parent-lib) - and, as (a), on the library under test,
  (b)  the numpy restatement (tests/onevar_cases.py) on one host core.
Rounds (u = ub, feastol 1e-6, all variables of every block, blocks loaded dense): one block of 512 rows (m = 4), one of 257 rows
(m = 12), one of 129 rows (m = 32), four blocks of 200 rows (m = 12), one block of 512 rows with m = 64.  The call: median ms of
--calls calls after --warmup, [min .. max] of --reps repetitions; the host loop: median of --loop-calls calls (it takes up to a
second per call); (b): one run.  Launches and read-backs are the differences of the stats call over one round; R = max evals.

--regress: hipsdp_syevx (512 rows, one pair) and hipsdp_sparsecuts (512 rows, size 24) - whose column kernel is re-expressed over a
shared body - on this build and on the parent's in turn (A B A B), each run a process of its own.  --out APPENDS, so that the two
runs (the rounds, then --regress) make one file; every child process has a time limit.

    python tests/devtools/onevar_large_rate.py [--parent-lib PARENT/libhipsdp.so] [--regress] [--out profiles/r24_onevar_large_rate.txt]"""
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
# name, [(rows, rank)], m
ROUNDS = [("1 x 512 rows, m = 4", [(512, 16)], 4), ("1 x 257 rows, m = 12", [(257, 12)], 12), ("1 x 129 rows, m = 32", [(129, 10)], 32),
          ("4 x 200 rows, m = 12", [(200, 12)] * 4, 12), ("1 x 512 rows, m = 64", [(512, 16)], 64)]


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, calls, warmup, reps):
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


def round_data(K, spec, m):
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


def host_loop(hb, K, blocks, lb, ub, feastol):
    """the Newton loop of every job on the host, the eigenpair of an evaluation by hipsdp_syevx(il = iu = 1); returns (status,
    optval, evals) per job"""
    out = []
    for A in blocks:
        Z = K.z_of(A, ub)
        for i in range(len(ub)):
            Ai, ev = A[i + 1], [0]

            def f(mu):
                ev[0] += 1
                lam, V = hb.syevx(np.ascontiguousarray(Z + (mu - ub[i]) * Ai), 1, 1)
                return float(lam[0]), float(V[0] @ Ai @ V[0])
            e, g = f(ub[i])
            if e < -feastol and g > 0.0:
                out.append((K.INFEASIBLE, ub[i], ev[0])); continue
            e, g = f(lb[i])
            if e >= -feastol:
                out.append((K.LB, lb[i], ev[0])); continue
            if g <= 0.0:
                out.append((K.INFEASIBLE, lb[i], ev[0])); continue
            mu, st = lb[i], None
            while e < -feastol and g > 0.0 and ev[0] < 100:
                nxt = mu - (feastol / 2.0 + e) / g
                if nxt > ub[i]:
                    st = (K.INFEASIBLE, nxt, ev[0]); break
                mu = nxt
                e, g = f(mu)
            out.append(st if st is not None else ((K.INFEASIBLE if e < -feastol else K.INNER), mu, ev[0]))
    return out


def regress_child(hb, K, calls, warmup, reps):
    import ipm_ref
    rng = np.random.default_rng(512)
    B = rng.standard_normal((512, 512))
    M = np.ascontiguousarray(0.5 * (B + B.T))
    sx = timed(lambda: hb.syevx(M, 1, 1), calls, warmup, reps)
    A, lb, ub = K.family(512, 4, 16, 1, 1.2, 0.0, 0)
    s = hb.Solver(0)
    s.load_core(ipm_ref.CoreProblem(np.ones(4), [np.array(A)], None, None))
    y = np.array(ub)
    res = s.sparsecuts(0, y, 24, 1e-6, 1e-6, 5)
    sc = timed(lambda: s.sparsecuts(0, y, 24, 1e-6, 1e-6, 5), calls, warmup, reps)
    s.close()
    print(json.dumps(dict(syevx=sx, sparsecuts=sc, ncuts=int(res[0]))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-calls", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libhipsdp.so of the parent commit")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--regress", action="store_true")
    ap.add_argument("--regress-child", action="store_true")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import onevar_cases as K
    hb = binding()
    if a.regress_child:
        regress_child(hb, K, a.calls, a.warmup, a.reps)
        return
    me = [sys.executable, os.path.abspath(__file__)]
    lines = []
    if a.regress:
        runs = []
        for k in range(4):
            env = dict(os.environ)
            env.pop("HIPSDP_LIB", None)
            if k % 2 == 1:
                if not a.parent_lib:
                    continue
                env["HIPSDP_LIB"] = os.path.abspath(a.parent_lib)
            r = subprocess.run(me + ["--regress-child", "--calls", str(a.calls), "--warmup", str(a.warmup), "--reps", str(a.reps)], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit("regression child %d failed" % k)
            runs.append(("parent" if k % 2 else "this", json.loads(r.stdout.strip().splitlines()[-1])))
        lines.append("# regression check, A B A B, a process per run: median ms of %d calls, median over %d repetitions [min .. max]" % (a.calls, a.reps))
        for key, what in (("syevx", "hipsdp_syevx, 512 rows, il = iu = 1"), ("sparsecuts", "hipsdp_sparsecuts, 512 rows, size 24, maxcuts 5")):
            lines.append("%-50s " % what + "   ".join("%s %.3f [%.3f .. %.3f]" % (who, float(np.median(d[key])), min(d[key]), max(d[key]))
                                                      for who, d in runs))
    other = None
    if a.parent_lib and not a.loop_only and not a.regress:
        env = dict(os.environ, HIPSDP_LIB=os.path.abspath(a.parent_lib))
        r = subprocess.run(me + ["--loop-only", "--loop-calls", str(a.loop_calls)], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
        other = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None
    rows, loops = [], {}
    for name, spec, m in ([] if a.regress else ROUNDS):
        blocks, lb, ub = round_data(K, spec, m)
        nb = len(blocks)
        loop = lambda: host_loop(hb, K, blocks, lb, ub, K.FEASTOL)
        loops[name] = timed(loop, a.loop_calls, 1, 1)
        if a.loop_only:
            continue
        import ipm_ref
        s = hb.Solver(0)
        s.load_core(ipm_ref.CoreProblem(np.ones(m), list(blocks), None, None))
        lbj, ubj = np.tile(lb, nb), np.tile(ub, nb)
        call = lambda: s.onevar_bounds_large(ub, lbj, ubj, K.FEASTOL)
        call()
        c0 = hb.onevar_bounds_large_stats()
        res = call()
        c1 = hb.onevar_bounds_large_stats()
        ref = loop()
        same = all(int(res[0][j]) == ref[j][0] and int(res[4][j]) == ref[j][2] for j in range(nb * m))
        row = dict(name=name, blocks=nb, jobs=nb * m, evals=int(res[4].sum()), R=int(res[4].max()), launches=c1[1] - c0[1],
                   readbacks=c1[2] - c0[2], same=same, loop_ms=loops[name], parent_ms=None if other is None else other[name],
                   statuses=[int(np.sum(res[0] == k)) for k in (K.LB, K.INNER, K.INFEASIBLE)])
        row["call_ms"] = timed(call, a.calls, a.warmup, a.reps)
        row["numpy_ms"] = None if a.no_numpy else timed(
            lambda: [K.onevar_ref(K.z_of(A, ub), A[i + 1], ub[i], K.NEWTON, lb[i], ub[i], K.FEASTOL) for A in blocks for i in range(m)], 1, 0, 1)
        rows.append(row)
        s.close()
    if a.loop_only:
        print(json.dumps(loops))
        return
    med = lambda v: float(np.median(v))
    if rows:
        lines += ["# a round of one-variable SDPs on blocks of 129 .. 512 rows (u = ub, feastol 1e-6, every variable of every block, blocks "
                  "loaded dense): hipsdp_onevar_bounds_large, median ms of %d calls, [min .. max] of %d repetitions" % (a.calls, a.reps),
                  "# (a) the Newton loop on the host with one hipsdp_syevx(il = iu = 1) per evaluation on this build, (a') the same on the parent "
                  "commit's build%s: median of %d calls; restatement: one run on one core" % (
                      "" if other is not None else " - NOT MEASURED (no --parent-lib)", a.loop_calls),
                  "# round                  blocks jobs LB/INNER/INFEASIBLE evaluations R | onevar_bounds_large        launches read-backs | "
                  "(a) host loop ms  ratio | (a') parent ms  ratio | restatement, 1 core  ratio | status and evals equal the host loop's"]
        for r in rows:
            pm, nm = r["parent_ms"], r["numpy_ms"]
            lines.append("%-24s %5d %5d %3d/%3d/%3d %8d %2d | %8.3f [%.3f .. %.3f] %6d %4d | %9.2f %6.1fx | %9s %7s | %9s %7s | %s" % (
                r["name"], r["blocks"], r["jobs"], r["statuses"][0], r["statuses"][1], r["statuses"][2], r["evals"], r["R"],
                med(r["call_ms"]), min(r["call_ms"]), max(r["call_ms"]), r["launches"], r["readbacks"],
                med(r["loop_ms"]), med(r["loop_ms"]) / med(r["call_ms"]),
                "-" if pm is None else "%.2f" % med(pm), "-" if pm is None else "%.1fx" % (med(pm) / med(r["call_ms"])),
                "-" if nm is None else "%.1f" % med(nm), "-" if nm is None else "%.1fx" % (med(nm) / med(r["call_ms"])),
                "yes" if r["same"] else "NO"))
        lines.append("# not measured: blocks kept as nonzeros or as packed triangles alone, rounds with u = 0, TWOPOINT and EXTREMES rounds, "
                     "several chunks, the time per kernel (no trace was taken), more than one host thread, the call inside SCIP-SDP's presolving")
    txt = "\n".join(lines)
    print(txt)
    if rows:
        print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "a") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
