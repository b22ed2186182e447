"""solve_objectives_rate.py - hipsdp_solve_objectives against what it replaces, on the bound-tightening workloads.

Two workloads: the root of example_TT (m = 37) with the objective cutoff row at the known optimum + 1 and the 74 objectives +-e_v,
the root of example_MkP (m = 105) with 210.  Timed, call alone (loading is not), median of --reps after a warm-up:

   call   ONE hipsdp_solve_objectives on one loaded solver
   (a)    the loop of hipsdp_set_obj + hipsdp_solve + hipsdp_get_y on one loaded solver; with --loop-lib PATH the same loop once more
          in a child process on another build of libhipsdp.so (the commit before the call existed), same box
   (b)    hipsdp_solve_many on K solvers, each loaded with the problem and one of the objectives (+ hipsdp_get_y each)
   (c)    one host core on oracle/cpu_ref.c

and the device memory the loaded solvers of the call and of (b) take (hipsdp_mem_info).  Prints a table and one JSON line.

    python tests/devtools/solve_objectives_rate.py [--reps 3] [--out profiles/r22_solve_objectives_rate.txt] [--loop-lib PATH]
    python tests/devtools/solve_objectives_rate.py --trace        (one call per workload, for rocprofv3 --kernel-trace --stats)
    python tests/devtools/solve_objectives_rate.py --loop-only    (what the child process of --loop-lib runs: one JSON line)
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "harness"), os.path.join(ROOT, "tests")]
import importlib.util  # noqa: E402
import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL = dict(gaptol=1e-6, feastol=1e-6)
WORK = [("example_TT.dat-s.gz", 2.11803), ("example_MkP.dat-s.gz", -95.0)]


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def workload(name, optimum):
    """the root with the cutoff row and all 2 m objectives, in the reference's order (min y_v, max y_v per variable)"""
    import bnb
    import obbt
    import sdpa_io
    import sdpi_prepare
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", name))
    P = sdpi_prepare.prepare(bnb.instance_to_sdpi(inst))
    node = obbt.node_with_cutoff(P, optimum + 1.0)
    m = node.core.m
    B = np.zeros((2 * m, m))
    for k in range(m):
        B[2 * k, k] = 1.0
        B[2 * k + 1, k] = -1.0
    return node.core, B


def free_bytes(hb):
    fr, tot = C.c_double(0), C.c_double(0)
    assert hb.lib().hipsdp_mem_info(0, C.byref(fr), C.byref(tot)) == 0
    return fr.value


def time_loop(hb, core, B, reps):
    s = hb.Solver(0)
    s.load_core(core)
    ts, infos, Y = [], None, np.zeros(B.shape)
    for r in range(reps + 1):
        t0 = time.perf_counter()
        infos = []
        for j, bj in enumerate(B):
            s.set_obj(bj)
            infos.append(s.solve(**TOL))
            Y[j] = s.y()
        ts.append(time.perf_counter() - t0)
    s.close()
    return float(np.median(ts[1:])), infos, Y


def time_call(hb, core, B, reps):
    f0 = free_bytes(hb)
    s = hb.Solver(0)
    s.load_core(core)
    ts = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        infos, Y = s.solve_objectives(B, **TOL)
        ts.append(time.perf_counter() - t0)
    used = f0 - free_bytes(hb)
    s.close()
    return float(np.median(ts[1:])), infos, Y, used


def time_many(hb, core, B, reps):
    f0 = free_bytes(hb)
    pool = [hb.Solver(0) for _ in B]
    ts = []
    for r in range(reps + 1):
        for s, bj in zip(pool, B):
            s.load_core(core)
            s.set_obj(bj)
        t0 = time.perf_counter()
        infos = hb.solve_many(pool, TOL)
        Y = np.array([s.y() for s in pool])
        ts.append(time.perf_counter() - t0)
    used = f0 - free_bytes(hb)
    for s in pool:
        s.close()
    return float(np.median(ts[1:])), infos, Y, used


def time_cpu(core, B):
    import cpu_ref
    import ipm_ref
    t0 = time.perf_counter()
    its = []
    for bj in B:
        info, y = cpu_ref.solve(ipm_ref.CoreProblem(bj, core.blocks, core.D, core.c), gaptol=TOL["gaptol"], feastol=TOL["feastol"])
        its.append(info.iterations)
    return time.perf_counter() - t0, its


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--loop-lib", default=None, help="another libhipsdp.so: the loop once more on it, in a child process")
    ap.add_argument("--loop-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    hb = binding()
    works = [(name,) + workload(name, opt) for name, opt in WORK]
    if a.loop_only:
        print(json.dumps({name: time_loop(hb, core, B, a.reps)[0] for name, core, B in works}))
        return
    if a.trace:
        for name, core, B in works:
            s = hb.Solver(0)
            s.load_core(core)
            t0 = time.perf_counter()
            s.solve_objectives(B, **TOL)
            print("trace %s: %d objectives, %.3f ms" % (name, len(B), 1e3 * (time.perf_counter() - t0)))
            s.close()
        return
    other = None
    if a.loop_lib:
        env = dict(os.environ, HIPSDP_LIB=os.path.abspath(a.loop_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", "--reps", str(a.reps)], env=env,
                           stdout=subprocess.PIPE, text=True, timeout=600)
        other = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else None
    rows = []
    for name, core, B in works:
        n = len(B)
        t_loop, il, Yl = time_loop(hb, core, B, a.reps)
        t_call, ic, Yc, mem_call = time_call(hb, core, B, a.reps)
        t_many, im, Ym, mem_many = time_many(hb, core, B, a.reps)
        t_cpu, its_cpu = time_cpu(core, B)
        its = [i.iterations for i in ic]
        same = [i.iterations for i in il] == its and [i.status for i in il] == [i.status for i in ic] and np.array_equal(Yl, Yc)
        st0 = hb.solve_objectives_stats()
        rows.append(dict(name=name, objectives=n, m=core.m, q=core.q, call_ms=1e3 * t_call, loop_ms=1e3 * t_loop,
                         loop_other_ms=None if other is None else 1e3 * other[name], many_ms=1e3 * t_many, cpu_ms=1e3 * t_cpu,
                         iters_mean=float(np.mean(its)), iters_max=int(np.max(its)), cpu_iters_mean=float(np.mean(its_cpu)),
                         optimal=int(sum(1 for i in ic if i.status == 0)), bits_equal_loop=bool(same),
                         mem_call_bytes=mem_call, mem_many_bytes=mem_many, stats=list(st0)))
    lines = ["# hipsdp_solve_objectives on the bound-tightening workloads: the root with the cutoff row at the known optimum + 1 and the",
             "# 2 m objectives +-e_v; the call alone timed, median of %d after a warm-up.  (a) loop of set_obj + solve + get_y on one solver" % a.reps,
             "# [(a') the same loop on the library given by --loop-lib], (b) solve_many on 2 m solvers, (c) one host core, oracle/cpu_ref.c",
             "# instance                objectives   call ms   (a) loop ms   x   (a') ms    x   (b) many ms   x   (c) cpu ms   x  | iters mean max | optimal | bits = loop | device bytes call / (b)"]
    for r in rows:
        lo = r["loop_other_ms"]
        lines.append("%-26s %6d %11.3f %11.3f %6.1f %9s %6s %10.3f %6.2f %10.1f %6.1f  | %6.2f %4d | %5d | %s | %.0f / %.0f" % (
            r["name"], r["objectives"], r["call_ms"], r["loop_ms"], r["loop_ms"] / r["call_ms"], "-" if lo is None else "%.3f" % lo,
            "-" if lo is None else "%.1f" % (lo / r["call_ms"]), r["many_ms"], r["many_ms"] / r["call_ms"], r["cpu_ms"],
            r["cpu_ms"] / r["call_ms"], r["iters_mean"], r["iters_max"], r["optimal"], r["bits_equal_loop"], r["mem_call_bytes"],
            r["mem_many_bytes"]))
    r0 = rows[0]
    base = r0["loop_other_ms"] if r0["loop_other_ms"] is not None else r0["loop_ms"]
    lines.append("# %s, %d objectives: %.2f x faster than the loop (pass mark 8 x); against solve_many on %d solvers %.3f x" % (
        r0["name"], r0["objectives"], base / r0["call_ms"], r0["objectives"], r0["many_ms"] / r0["call_ms"]))
    txt = "\n".join(lines) + "\n"
    print(txt)
    print(json.dumps(dict(rows=rows)))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)


if __name__ == "__main__":
    main()
