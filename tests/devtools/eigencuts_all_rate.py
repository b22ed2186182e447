"""eigencuts_all_rate.py - time of one separation round over all blocks: hipsdp_eigencuts_all against the loop of per-block
hipsdp_eigencuts calls and against the numpy restatement on one host core.

Problems: the three batched families of tests/test_gpu_eigencuts_all.py (9 mixed blocks of 3 .. 128 rows; 32 blocks of 12 rows;
4 blocks of 40 rows), one block of 40 rows, and the root of example_TT loaded as a core problem.  Per problem, the median of
--calls calls after --warmup calls, repeated --reps times (the spread of the repetitions is printed beside the median).

    python tests/devtools/eigencuts_all_rate.py --per-block-json FILE      the loop of per-block calls only, figures to FILE.  Run
                                                                           it with HIPSDP_LIB=<libhipsdp.so of the parent commit>
                                                                           (DESIGN 7): the baseline is never the new build
    python tests/devtools/eigencuts_all_rate.py [--baseline FILE] [--out profiles/r09_eigencuts_all_rate.txt]

"step 4" is not timed by itself: the column is the bytes of A over t(maxcuts = 5) - t(maxcuts = 0) - the second call skips the
sweep over A (and reads back less), so the figure is a LOWER bound of the sweep's bandwidth.  The launch count of the stats call is
printed; compare it once with the kernel count of `rocprofv3 --kernel-trace --stats -- python ... --calls 1 --warmup 0 --reps 1`."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TOL, MAXCUTS = 1e-6, 5


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def problems():
    """[(name, blocks, y, b, D, c)]"""
    import test_gpu_eigencuts_all as T
    out = []
    for name, fam in [("9 blocks 3..128", T.FAMILIES[0]), ("32 blocks of 12", T.FAMILIES[1]), ("4 blocks of 40", T.FAMILIES[2]),
                      ("1 block of 40", ([40], 15, (), 1, 5))]:
        blocks, ys, y, b = T.family(fam[0], fam[1], fam[2], fam[3])
        out.append((name, blocks, y, b, None, None))
    import bnb
    import sdpa_io
    import sdpi_prepare
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", "example_TT.dat-s.gz"))
    b, blk, D, c, _ = sdpi_prepare.to_core(sdpi_prepare.prepare(bnb.instance_to_sdpi(inst)))
    y = 0.7 * np.random.default_rng(0).standard_normal(len(b))
    out.append(("example_TT root", [np.asarray(A) for A in blk], y, b, D, c))
    return out


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--per-block-json", default=None)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ipm_ref
    import eigcuts_ref
    hb = binding()
    rows = []
    for name, blocks, y, b, D, c in problems():
        s = hb.Solver(0)
        s.load_core(ipm_ref.CoreProblem(b, blocks, D, c))
        nb = len(blocks)
        loop = timed(lambda: [s.eigencuts(k, y, TOL, MAXCUTS) for k in range(nb)], a)
        row = dict(name=name, blocks=nb, loop_ms=loop, lib=hb.LIBPATH)
        if a.per_block_json is None:
            st0 = hb.eigencuts_all_stats()
            res = s.eigencuts_all(y, TOL, MAXCUTS)
            st1 = hb.eigencuts_all_stats()
            row["cuts"] = int(sum(len(r[1]) for r in res))
            row["launches"], row["readbacks"] = st1[1] - st0[1], st1[2] - st0[2]
            row["all_ms"] = timed(lambda: s.eigencuts_all(y, TOL, MAXCUTS), a)
            row["all0_ms"] = timed(lambda: s.eigencuts_all(y, TOL, 0), a)
            row["host_ms"] = timed(lambda: [eigcuts_ref.cuts_dense(A, y, TOL, MAXCUTS) for A in blocks], a)
            row["bytes_A"] = int(sum(8 * A.size for A in blocks))
        rows.append(row)
        s.close()
    if a.per_block_json is not None:
        with open(a.per_block_json, "w") as f:
            json.dump(rows, f)
        print(json.dumps(rows))
        return
    base = {}
    if a.baseline is not None:
        with open(a.baseline) as f:
            base = {r["name"]: r for r in json.load(f)}
    med = lambda v: float(np.median(v))
    lines = ["# one separation round (tol %g, maxcuts %d): median ms of %d calls, [min .. max] of %d repetitions" % (TOL, MAXCUTS, a.calls, a.reps),
             "# problem            blocks cuts | eigencuts_all        | per-block loop, parent library | per-block loop, this build | host oracle, 1 core | launches read-backs | A bytes / (t - t(maxcuts=0))"]
    for r in rows:
        p = base.get(r["name"])
        ptxt = "%8.3f [%.3f .. %.3f]" % (med(p["loop_ms"]), min(p["loop_ms"]), max(p["loop_ms"])) if p else "     (not measured)     "
        d = med(r["all_ms"]) - med(r["all0_ms"])
        bw = "%.1f GB/s" % (r["bytes_A"] / (d * 1e-3) / 1e9) if d > 0 else "n/a"
        lines.append("%-20s %5d %4d | %8.3f [%.3f .. %.3f] | %s | %8.3f | %8.3f | %d %d | %s" % (
            r["name"], r["blocks"], r["cuts"], med(r["all_ms"]), min(r["all_ms"]), max(r["all_ms"]), ptxt, med(r["loop_ms"]),
            med(r["host_ms"]), r["launches"], r["readbacks"], bw))
    txt = "\n".join(lines)
    print(txt)
    print(json.dumps(dict(rows=rows, baseline=list(base.values()))))
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
