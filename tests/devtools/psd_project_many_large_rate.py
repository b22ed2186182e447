"""psd_project_many_large_rate.py - time of the PSD projections of blocks of 129 .. 512 rows: hipsdp_psd_project_many_large against
hipsdp_psd_project_many of the PARENT commit's library on the same jobs (there every such job takes the single-call chain with the
block-Jacobi decomposition, one after the other) and against the numpy restatement (oracle/psd_project_ref.spectral) on one host core.

Shapes: 1 and 8 jobs of 512 rows, 4 of 200, 150 + 200 mixed, 2 of 129 - each on `random` inputs (dense random symmetric, the generator
of tests/harness/psd_many_cases.py) and on `low_rank_shifted` ones (rank n / 10, shift -0.01: what a warm start's X or Z looks like).
Mode 1, minev 1e-4, epsilon 1e-9.  The ctypes arguments are built once: the timed region is the C call alone.  Per shape the median of
--calls calls after --warmup calls, repeated --reps times (the spread of the repetitions beside the median); numpy is timed with
--calls / 6 calls per repetition.

    HIPSDP_LIB=<libhipsdp.so of the parent commit> python tests/devtools/psd_project_many_large_rate.py --parent-json FILE
        hipsdp_psd_project_many of that library only, figures to FILE (the baseline is never the new build)
    python tests/devtools/psd_project_many_large_rate.py [--parent FILE] [--out profiles/r27_psd_project_many_large_rate.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/devtools/psd_project_many_large_rate.py --only 8x512 --no-host --calls 5 --reps 1
        the stage shares; --kernels-csv DIR/..._kernel_stats.csv --kernels-out profiles/r27_psd_project_many_large_kernels.txt
        then turns the statistics into microseconds per call"""
import argparse
import csv
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
MINEV, EPS, MODE = 1e-4, 1e-9, 1
SHAPES = [("1x512", "1 job of 512 rows", [512]), ("8x512", "8 jobs of 512 rows", [512] * 8), ("4x200", "4 jobs of 200 rows", [200] * 4),
          ("150+200", "150 + 200 rows", [150, 200]), ("2x129", "2 jobs of 129 rows", [129, 129])]
KINDS = ("random", "low_rank_shifted")


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


class Jobs:
    """the arrays of the jobs of a shape and the job table, built once"""
    def __init__(self, hb, kind, ns):
        import psd_large_cases as cases
        PI, PD = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self.data = []
        for k, n in enumerate(ns):
            if kind == "random":
                row, col, val, _ = cases.random_sparse_sym(n, 6000 + 17 * n + k, 1.0)
            else:
                j = cases.low_rank_shifted(n, n // 10, -0.01, seed=6500 + 17 * n + k)
                row, col, val = j.row, j.col, j.val
            cap = n * (n + 1) // 2
            self.data.append((n, row, col, val, np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap)))
        self.tab = (hb.PsdJob * len(ns))()
        for k, d in enumerate(self.data):
            t = self.tab[k]
            t.n, t.nnz, t.minev, t.cap = d[0], len(d[3]), MINEV, len(d[6])
            t.row, t.col, t.val = d[1].ctypes.data_as(PI), d[2].ctypes.data_as(PI), d[3].ctypes.data_as(PD)
            t.rowout, t.colout, t.valout = d[4].ctypes.data_as(PI), d[5].ctypes.data_as(PI), d[6].ctypes.data_as(PD)


def kernels_table(path, calls, out):
    """the statistics file of a rocprofv3 --kernel-trace --stats run over `calls` calls of the 8 x 512 shape -> microseconds per call"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split()[-1]
            rows.append((name, int(r["Calls"]), float(r["TotalDurationNs"])))
    total = sum(t for _, _, t in rows)
    lines = ["# hipsdp_psd_project_many_large, kernel trace of %d calls (rocprofv3 --kernel-trace --stats; one MI355X, 8 jobs of 512 rows,"
             " low_rank_shifted, mode 1): microseconds per call" % calls,
             "# kernel                        launches per call | us per call | share of the kernel time"]
    for name, n, t in sorted(rows, key=lambda x: -x[2]):
        lines.append("%-34s %12.1f | %11.1f | %5.1f %%" % (name, n / calls, 1e-3 * t / calls, 100.0 * t / total))
    lines.append("# sum of the kernels %39.1f" % (1e-3 * total / calls))
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--kind", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--parent-json", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-csv", default=None)
    ap.add_argument("--kernels-out", default=None)
    a = ap.parse_args()
    if a.kernels_csv is not None:
        kernels_table(a.kernels_csv, a.calls * a.reps + a.warmup + 1, a.kernels_out)
        return
    import psd_project_ref as ref
    hb = binding()
    lib = hb.lib()
    if hb.device_count() <= 0:
        raise RuntimeError("no HIP device visible: this is a measurement on the GPU")
    eps = C.c_double(EPS)
    rows = []
    for key, name, ns in SHAPES:
        if a.only is not None and key != a.only:
            continue
        for kind in KINDS:
            if a.kind is not None and kind != a.kind:
                continue
            J = Jobs(hb, kind, ns)
            row = dict(key=key, name=name, kind=kind, jobs=len(ns), lib=hb.LIBPATH)
            if a.parent_json is not None:
                def many():
                    if lib.hipsdp_psd_project_many(0, len(ns), J.tab, eps, MODE) != 0:
                        raise RuntimeError("hipsdp_psd_project_many failed")
                row["many_ms"] = timed(many, a.calls, a.warmup, a.reps)
            else:
                def large():
                    if lib.hipsdp_psd_project_many_large(0, len(ns), J.tab, eps, MODE) != 0:
                        raise RuntimeError("hipsdp_psd_project_many_large failed")
                st0 = hb.psd_project_many_large_stats()
                large()
                st1 = hb.psd_project_many_large_stats()
                row["launches"], row["readbacks"] = st1[1] - st0[1], st1[2] - st0[2]
                row["large_ms"] = timed(large, a.calls, a.warmup, a.reps)
                if not a.no_host:
                    row["host_ms"] = timed(lambda: [ref.spectral(d[0], d[1], d[2], d[3], MINEV) for d in J.data], max(1, a.calls // 6), 1, a.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.parent_json is not None:
        with open(a.parent_json, "w") as f:
            json.dump(rows, f)
        return
    base = {}
    if a.parent is not None:
        with open(a.parent) as f:
            base = {(r["key"], r["kind"]): r for r in json.load(f)}
    med = lambda v: float(np.median(v))
    lines = ["# PSD projections of blocks of 129 .. 512 rows (mode %d, minev %g, epsilon %g): median ms of %d calls, [min .. max] of %d repetitions"
             % (MODE, MINEV, EPS, a.calls, a.reps),
             "# shape              input            jobs | hipsdp_psd_project_many_large | hipsdp_psd_project_many, parent library      | numpy spectral, 1 core | launches read-backs"]
    for r in rows:
        p = base.get((r["key"], r["kind"]))
        ptxt = "(not measured)"
        if p is not None:
            ptxt = "%8.3f [%.3f .. %.3f] (x %.2f)" % (med(p["many_ms"]), min(p["many_ms"]), max(p["many_ms"]), med(p["many_ms"]) / med(r["large_ms"]))
        htxt = "(not measured)"
        if "host_ms" in r:
            htxt = "%8.1f (x %.1f)" % (med(r["host_ms"]), med(r["host_ms"]) / med(r["large_ms"]))
        lines.append("%-20s %-16s %4d | %8.3f [%.3f .. %.3f] | %-42s | %-20s | %d %d" % (
            r["name"], r["kind"], r["jobs"], med(r["large_ms"]), min(r["large_ms"]), max(r["large_ms"]), ptxt, htxt, r["launches"], r["readbacks"]))
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
