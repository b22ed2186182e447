"""psd_project_many_rate.py - time of the PSD projections of all blocks of one or many nodes: hipsdp_psd_project_many against the loop
of hipsdp_psd_project calls over the same jobs and against the numpy restatement (oracle/psd_project_ref.chain) on one host core.

Problems: 1 job of 10 rows; 2 x 32 jobs of 12 rows; 2 x 4 jobs of 40 rows; 128 jobs of 10 rows (Z and X of 64 example_TT nodes);
2 jobs of 128 rows.  Dense random symmetric matrices (the generator of tests/harness/psd_many_cases.py, one seed per job), minev 1e-4,
epsilon 1e-9, mode 0.  The ctypes arguments are built once: the timed region is the C call (or the loop of C calls) alone.  Per
problem, the median of --calls calls after --warmup calls, repeated --reps times (the spread of the repetitions beside the median).

    python tests/devtools/psd_project_many_rate.py --loop-json FILE     the loop of single calls only, figures to FILE.  Run it with
                                                                        HIPSDP_LIB=<libhipsdp.so of the parent commit>:
                                                                        the baseline is never the new build
    python tests/devtools/psd_project_many_rate.py [--baseline FILE] [--out profiles/r12_psd_project_many_rate.txt]

Pass marks (printed per problem): with several jobs the batched median is below the parent loop's and numpy's by more than the
measured spread; with one job it is not above the parent's single call by more than the spread."""
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
MINEV, EPS, MODE = 1e-4, 1e-9, 0
PROBLEMS = [("1 job of 10 rows", 1, 10), ("2 x 32 jobs of 12 rows", 64, 12), ("2 x 4 jobs of 40 rows", 8, 40),
            ("128 jobs of 10 rows", 128, 10), ("2 jobs of 128 rows", 2, 128)]


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(fn, a):
    """medians (ms) of a.reps repetitions of a.calls calls"""
    for _ in range(a.warmup):
        fn()
    meds = []
    for _ in range(a.reps):
        ts = []
        for _ in range(a.calls):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        meds.append(1e3 * float(np.median(ts)))
    return meds


class Jobs:
    """the arrays of `count` jobs of n rows and the ctypes arguments of both entry points, built once"""
    def __init__(self, count, n):
        import psd_many_cases as cases
        PI, PD = C.POINTER(C.c_int), C.POINTER(C.c_double)
        self.n, self.count = n, count
        cap = n * (n + 1) // 2
        self.data = []
        for k in range(count):
            row, col, val, _ = cases.random_sparse_sym(n, 5000 + 131 * n + k, 1.0)
            self.data.append((row, col, val, np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap), C.c_int(0)))
        self.single = [(0, n, len(d[2]), d[0].ctypes.data_as(PI), d[1].ctypes.data_as(PI), d[2].ctypes.data_as(PD), C.c_double(MINEV),
                        C.c_double(EPS), MODE, cap, C.byref(d[6]), d[3].ctypes.data_as(PI), d[4].ctypes.data_as(PI), d[5].ctypes.data_as(PD))
                       for d in self.data]

    def table(self, hb):
        PI, PD = C.POINTER(C.c_int), C.POINTER(C.c_double)
        tab = (hb.PsdJob * self.count)()
        for k, d in enumerate(self.data):
            tab[k].n, tab[k].nnz, tab[k].minev, tab[k].cap = self.n, len(d[2]), MINEV, len(d[5])
            tab[k].row, tab[k].col, tab[k].val = d[0].ctypes.data_as(PI), d[1].ctypes.data_as(PI), d[2].ctypes.data_as(PD)
            tab[k].rowout, tab[k].colout, tab[k].valout = d[3].ctypes.data_as(PI), d[4].ctypes.data_as(PI), d[5].ctypes.data_as(PD)
        return tab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--loop-json", default=None)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import psd_project_ref as ref
    hb = binding()
    lib = hb.lib()
    if hb.device_count() <= 0:
        raise RuntimeError("no HIP device visible: this is a measurement on the GPU")
    rows = []
    for name, count, n in PROBLEMS:
        J = Jobs(count, n)

        def loop():
            for args in J.single:
                if lib.hipsdp_psd_project(*args) != 0:
                    raise RuntimeError("hipsdp_psd_project failed")

        row = dict(name=name, jobs=count, n=n, loop_ms=timed(loop, a), lib=hb.LIBPATH)
        if a.loop_json is None:
            tab = J.table(hb)
            eps = C.c_double(EPS)

            def many():
                if lib.hipsdp_psd_project_many(0, count, tab, eps, MODE) != 0:
                    raise RuntimeError("hipsdp_psd_project_many failed")

            st0 = hb.psd_project_many_stats()
            many()
            st1 = hb.psd_project_many_stats()
            row["launches"], row["readbacks"] = st1[1] - st0[1], st1[2] - st0[2]
            row["many_ms"] = timed(many, a)
            row["host_ms"] = timed(lambda: [ref.chain(n, d[0], d[1], d[2], MINEV) for d in J.data], a)
        rows.append(row)
    if a.loop_json is not None:
        with open(a.loop_json, "w") as f:
            json.dump(rows, f)
        print(json.dumps(rows))
        return
    base = {}
    if a.baseline is not None:
        with open(a.baseline) as f:
            base = {r["name"]: r for r in json.load(f)}
    med = lambda v: float(np.median(v))
    spread = lambda v: max(v) - min(v)
    lines = ["# PSD projections (mode %d, minev %g, epsilon %g): median ms of %d calls, [min .. max] of %d repetitions" % (MODE, MINEV, EPS, a.calls, a.reps),
             "# problem                 jobs | psd_project_many      | loop of psd_project, parent library | loop, this build | numpy chain, 1 core | launches read-backs | pass mark"]
    for r in rows:
        p = base.get(r["name"])
        ptxt = "%8.3f [%.3f .. %.3f]" % (med(p["loop_ms"]), min(p["loop_ms"]), max(p["loop_ms"])) if p else "     (not measured)     "
        if p is None:
            mark = "parent not measured"
        elif r["jobs"] > 1:
            sp = max(spread(r["many_ms"]), spread(p["loop_ms"]), spread(r["host_ms"]))
            ok = med(r["many_ms"]) + sp < med(p["loop_ms"]) and med(r["many_ms"]) + sp < med(r["host_ms"])
            mark = "below parent loop and numpy by more than the spread: %s" % ("yes" if ok else "NO")
        else:
            sp = max(spread(r["many_ms"]), spread(p["loop_ms"]))
            ok = med(r["many_ms"]) <= med(p["loop_ms"]) + sp
            mark = "not above the parent's single call by more than the spread: %s; %s numpy" % (
                "yes" if ok else "NO", "above" if med(r["many_ms"]) > med(r["host_ms"]) else "below")
        lines.append("%-25s %4d | %8.3f [%.3f .. %.3f] | %s | %8.3f | %8.3f [%.3f .. %.3f] | %d %d | %s" % (
            r["name"], r["jobs"], med(r["many_ms"]), min(r["many_ms"]), max(r["many_ms"]), ptxt, med(r["loop_ms"]),
            med(r["host_ms"]), min(r["host_ms"]), max(r["host_ms"]), r["launches"], r["readbacks"], mark))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows, baseline=list(base.values()))))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
