"""solve_many_rate.py - node solves per second of hipsdp_solve_many against K sequential hipsdp_solve calls.

One serial engine run of example_TT's branch-and-bound (tests/harness/bnb.py, node relaxations through the binding's hipsdp_solve)
records its first node problems as core problems (sdpi_prepare.to_core); with the roots of example_MkP, example_small and
example_tightenmatrices at the end they make 512 problems, loaded into 512 solvers.  For K in 1, 8, 32, 64, 128, 256, 512 the first K
are solved by ONE hipsdp_solve_many call, and again by K hipsdp_solve calls; only the calls are timed (loading is not).  Prints a table
and one JSON line.

    python tests/devtools/solve_many_rate.py [--reps 5] [--out profiles/r07_solve_many_rate.txt]
    python tests/devtools/solve_many_rate.py --trace K1,K2     (one call per K, for rocprofv3 --kernel-trace --stats)
    python tests/devtools/solve_many_rate.py --summarize-trace DIR --out FILE   (the solve1 dispatches of a kernel trace)
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests", "harness"), os.path.join(ROOT, "tests")]
import importlib.util  # noqa: E402
import numpy as np  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
KS = [1, 8, 32, 64, 128, 256, 512]
TOL = dict(gaptol=1e-6, feastol=1e-6)


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def record_problems(hb, total=512):
    """example_TT's first total - 3 node problems (one serial run, hipsdp_solve), then three roots"""
    import bnb
    import ipm_ref
    import sdpa_io
    import sdpi_prepare
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", "example_TT.dat-s.gz"))
    prob = bnb.instance_to_sdpi(inst)
    cores = []
    s = hb.Solver(0)

    def solve(P):
        b, blk, D, c, maps = sdpi_prepare.to_core(P)
        core = ipm_ref.CoreProblem(b, blk, D, c)
        if len(cores) < total - 3:
            cores.append(core)
        s.load_core(core)
        info = s.solve(**TOL)
        if info.status in (1, 3):
            return bnb.NodeResult('infeasible')
        if info.status != 0:
            return bnb.NodeResult('failed')
        y = np.array(P.lb, dtype=float)
        for k, v in enumerate(maps["active"]):
            y[v] = s.y()[k]
        return bnb.NodeResult('optimal', float(P.prob.obj @ y), y)
    best, y, nodes, failed = bnb.branch_and_bound(prob, inst.intvars, solve)
    s.close()
    ntt = len(cores)
    for name in ("example_MkP.dat-s.gz", "example_small.dat-s", "example_tightenmatrices.dat-s"):
        inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", name))
        D, c = sdpa_io.lp_dense(inst)
        cores.append(ipm_ref.CoreProblem(inst.obj, sdpa_io.dense_blocks(inst), D, c))
    return cores, ntt, nodes


def loaded(hb, pool, cores):
    for s, c in zip(pool, cores):
        s.load_core(c)


def run_many(hb, pool, cores, K):
    loaded(hb, pool[:K], cores[:K])
    t0 = time.perf_counter()
    infos = hb.solve_many(pool[:K], TOL)
    return time.perf_counter() - t0, infos, [s.solve_path() for s in pool[:K]]


def run_seq(hb, pool, cores, K):
    loaded(hb, pool[:K], cores[:K])
    t0 = time.perf_counter()
    infos = [s.solve(**TOL) for s in pool[:K]]
    return time.perf_counter() - t0, infos


def summarize_trace(d, out):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if "solve1" in r.get("Kernel_Name", ""):
                    rows.append(r)
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    single = [r for r in rows if "_many" not in r["Kernel_Name"]]
    lines = ["# one-launch kernel dispatches of tests/devtools/solve_many_rate.py --trace (rocprofv3 --kernel-trace --stats)",
             "# the serial run that records the tree: %d single-launch dispatches (grid = one workgroup), mean %.1f us" % (
                 len(single), np.mean([(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in single]) if single else 0.0),
             "# then one hipsdp_solve_many call per K: kernel, grid (threads), workgroup, LDS bytes, duration us"]
    for r in rows:
        if "_many" not in r["Kernel_Name"]:
            continue
        lines.append("%-60s grid %6s x %s x %s  wg %s  lds %s  %.1f us" % (
            r["Kernel_Name"][:60], r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Grid_Size_Y", "1"), r.get("Grid_Size_Z", "1"),
            r.get("Workgroup_Size_X", r.get("Workgroup_Size", "?")), r.get("LDS_Block_Size", r.get("Group_Segment_Size", "?")),
            (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        lines.append("")
        lines.append("# " + os.path.basename(f))
        with open(f) as fh:
            for ln in fh:
                if "solve1" in ln or ln.startswith('"Name"') or ln.startswith("Name"):
                    lines.append(ln.rstrip())
    txt = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as fh:
            fh.write(txt)
    print(txt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", default=None, help="comma-separated K: one solve_many call each, nothing else timed")
    ap.add_argument("--summarize-trace", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.summarize_trace:
        summarize_trace(a.summarize_trace, a.out)
        return
    hb = binding()
    t0 = time.perf_counter()
    cores, ntt, tree_nodes = record_problems(hb)
    t_rec = time.perf_counter() - t0
    pool = [hb.Solver(0) for _ in cores]
    if a.trace:
        for K in [int(k) for k in a.trace.split(",")]:
            dt, infos, paths = run_many(hb, pool, cores, K)
            print("trace K=%d: %.3f ms, %d of %d in the one launch" % (K, dt * 1e3, sum(paths), K))
        for s in pool:
            s.close()
        return
    run_many(hb, pool, cores, len(cores))                  # (first launch of every instance: attributes, code load)
    rows = []
    for K in KS:
        K = min(K, len(cores))
        tm, ts = [], []
        for _ in range(a.reps):
            dt, infos, paths = run_many(hb, pool, cores, K)
            tm.append(dt)
            ds, infos_s = run_seq(hb, pool, cores, K)
            ts.append(ds)
        its = [i.iterations for i in infos]
        assert [i.iterations for i in infos_s] == its and [i.status for i in infos_s] == [i.status for i in infos]
        tmed, smed = float(np.median(tm)), float(np.median(ts))
        rows.append(dict(K=K, many_ms=tmed * 1e3, many_solves_per_s=K / tmed, seq_ms=smed * 1e3, seq_solves_per_s=K / smed,
                         iters_mean=float(np.mean(its)), iters_max=int(np.max(its)), one_launch=int(sum(paths))))
    base = rows[0]["many_solves_per_s"]
    lines = ["# hipsdp_solve_many against K x hipsdp_solve: %d problems = example_TT's first %d node problems (tree of %d nodes, "
             "recorded in %.1f s) + the roots of example_MkP, example_small, example_tightenmatrices; median of %d repetitions, "
             "loading not timed" % (len(cores), ntt, tree_nodes, t_rec, a.reps),
             "#    K   solve_many ms   solves/s   x K=1   |  K x solve ms   solves/s   |  iters mean  max  | in the one launch"]
    for r in rows:
        lines.append("%6d   %12.3f %10.0f %7.2f   | %12.3f %10.0f   | %8.2f %5d   | %d" % (
            r["K"], r["many_ms"], r["many_solves_per_s"], r["many_solves_per_s"] / base, r["seq_ms"], r["seq_solves_per_s"],
            r["iters_mean"], r["iters_max"], r["one_launch"]))
    r64 = [r for r in rows if r["K"] == 64]
    if r64:
        lines.append("# K = 64: %.2f x the K = 1 rate (pass mark 8 x)" % (r64[0]["many_solves_per_s"] / base))
    txt = "\n".join(lines) + "\n"
    print(txt)
    print(json.dumps(dict(rows=rows, problems=len(cores), tt_nodes=ntt)))
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(txt)
    for s in pool:
        s.close()


if __name__ == "__main__":
    main()
