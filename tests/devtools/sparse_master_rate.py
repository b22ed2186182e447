"""sparse_master_rate.py - what it costs to prepare a block kept as nonzeros for a node: the direct load (hipsdp_set_shape2,
hipsdp_add_entries of the node's triplets, structure built on the host by hs_sp_build at the first use) against the gather from the
master copy kept as triplets (hipsdp_set_shape2, hipsdp_master_gather: structure built on the device).

Sizes (n rows, m variables, k lower nonzeros per matrix): (150, 60, 3), (500, 2000, 3), (500, 2000, 50) - instances.planted_sparse -
and (300, 2000, 500): 10^6 triplets at random positions.  Per size 30 nodes: the root, then nodes with a random tenth of the variables
fixed and two in a hundred rows removed.  The triplets of every node are marshalled BEFORE the clock starts (the solver interface
does that in C per node on the direct path and not at all on the gather path: the direct figure is flattered by it).

The structure of the direct path is built by the first call that uses it, so both paths are timed from hipsdp_set_shape2 to the return
of a first hipsdp_check_y_tol, and the median time of the same call repeated on the finished structure is subtracted.  The gather
returns when its structure is ready (it ends with the read-back of the counts), so its time without any consumer is given as well.
Figures: median over the 30 nodes, repeated --reps times (smallest and largest median = the spread).  The solve time of the root
(general path, tolerances 1e-5) stands beside them where the cost rule would keep the block as nonzeros.

    HIPSDP_LIB=<libhipsdp.so of the parent commit> python tests/devtools/sparse_master_rate.py --direct-json FILE
                                  the direct path only, figures to FILE: the baseline is never the new build
    python tests/devtools/sparse_master_rate.py [--baseline FILE] [--out profiles/r15_sparse_master_rate.txt]

One verdict line per size: "faster" when the gather's median is below the parent's direct median by more than the larger of the two
spreads, "slower" when it is above by more than that, "no difference" otherwise.  No pass mark: a loss is reported as a loss."""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "harness"))
import instances
import sp_master_cases as cases

SIZES = [(150, 60, 3), (500, 2000, 3), (500, 2000, 50), (300, 2000, 500)]
NODES = 30
PI, PD = C.POINTER(C.c_int), C.POINTER(C.c_double)


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def slots_of(n, m, k):
    if k <= 50:
        b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=1500 + n + m + k)
        var, row, col, val = coo
        order = np.argsort(var, kind="stable")
        cut = np.searchsorted(var[order], np.arange(1, m + 2))
        return [(row[order][cut[v]:cut[v + 1]], col[order][cut[v]:cut[v + 1]], val[order][cut[v]:cut[v + 1]]) for v in range(m)], b, A0
    return cases._random_slots(n, m, k, n * (n + 1) // 2, 1500 + n + m + k), np.ones(m), -np.eye(n)


def nodes_of(n, m):
    rng = np.random.default_rng(n + m)
    out = [cases.Node("root", range(m), range(n))]
    for i in range(1, NODES):
        act = sorted(rng.choice(m, size=m - max(1, m // 10), replace=False).tolist())
        kept = sorted(rng.choice(n, size=n - max(1, n // 50), replace=False).tolist())
        out.append(cases.Node("node%d" % i, act, kept))
    return out


class Prepared:
    """ctypes arguments of both paths for one node, built once"""
    def __init__(self, n, slots, node):
        self.m, self.nk = node.m, len(node.kept)
        var, row, col, val = cases.marshal(slots, n, node)
        self.coo = [np.ascontiguousarray(a) for a in (var, row, col, val)]
        self.nnz = (C.c_longlong * 1)(len(val))
        self.bs = (C.c_int * 1)(self.nk)
        self.act = np.array(node.act, dtype=np.int32)
        self.kept = np.array(node.kept, dtype=np.int32)
        self.y = np.zeros(self.m)
        self.lmin = np.zeros(1)
        self.viol = C.c_double(0.0)


def run_path(hb, n, slots, nodes, gathered, reps):
    """[(median total, median consumer alone, median gather alone)] per repetition, ms"""
    lib = hb.lib()
    prep = [Prepared(n, slots, nd) for nd in nodes]
    s = hb.Solver(0)
    s.sparse_policy(2)
    if gathered:
        s.master_define(len(slots), [n], [len(slots)], nnz=[sum(len(v) for _, _, v in slots)])
        assert s.master_add_vars(0, [r for r, _, _ in slots], [c for _, c, _ in slots], [v for _, _, v in slots]) == 0
    out = []
    for rep in range(reps + 1):                      # (the first repetition warms up: allocations, the sort of the master)
        tot, use, gat = [], [], []
        for p in prep:
            t0 = time.perf_counter()
            rc = lib.hipsdp_set_shape2(s.h, p.m, 1, p.bs, 0, p.nnz)
            if gathered:
                rc |= lib.hipsdp_master_gather(s.h, 0, 0, len(p.act), p.act.ctypes.data_as(PI), p.nk, p.kept.ctypes.data_as(PI))
                t1 = time.perf_counter()
            else:
                rc |= lib.hipsdp_add_entries(s.h, 0, C.c_longlong(len(p.coo[3])), p.coo[0].ctypes.data_as(PI), p.coo[1].ctypes.data_as(PI),
                                             p.coo[2].ctypes.data_as(PI), p.coo[3].ctypes.data_as(PD))
                t1 = t0
            rc |= lib.hipsdp_check_y_tol(s.h, p.y.ctypes.data_as(PD), C.c_double(1.0), p.lmin.ctypes.data_as(PD), C.byref(p.viol))
            t2 = time.perf_counter()
            rc |= lib.hipsdp_check_y_tol(s.h, p.y.ctypes.data_as(PD), C.c_double(1.0), p.lmin.ctypes.data_as(PD), C.byref(p.viol))
            t3 = time.perf_counter()
            assert rc == 0, (rc, s.last_error())
            tot.append(t2 - t0); use.append(t3 - t2); gat.append(t1 - t0)
        if rep > 0:
            out.append((1e3 * float(np.median(tot)), 1e3 * float(np.median(use)), 1e3 * float(np.median(gat))))
    stats = s.master_gather_stats() if hasattr(lib, "hipsdp_master_gather_stats") else None
    s.close()
    return out, stats


def solve_root(hb, n, m, slots, b, A0):
    node = cases.Node("root", range(m), range(n))
    var, row, col, val = cases.marshal(slots, n, node)
    s = hb.Solver(0)
    s.sparse_policy(2)
    s.load_sparse(m, n, b, (var, row, col, val), A0)
    info = s.solve(gaptol=1e-5, feastol=1e-5)
    s.close()
    return info.status, info.iterations, 1e3 * info.solve_seconds


def figures(runs):
    """median of the repetitions' (total - consumer) and its spread, and the same of the gather alone"""
    prep = [t - u for t, u, _ in runs]
    gat = [g for _, _, g in runs]
    return dict(prep=float(np.median(prep)), prep_lo=min(prep), prep_hi=max(prep), alone=float(np.median(gat)), alone_lo=min(gat),
                alone_hi=max(gat))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--direct-json")
    ap.add_argument("--baseline")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_sparse_master_rate.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="0,1,2,3")
    a = ap.parse_args()
    hb = binding()
    base = json.load(open(a.baseline)) if a.baseline else {}
    lines, res = [], {}
    for i in [int(x) for x in a.sizes.split(",")]:
        n, m, k = SIZES[i]
        key = "%d,%d,%d" % (n, m, k)
        slots, b, A0 = slots_of(n, m, k)
        nodes = nodes_of(n, m)
        d, _ = run_path(hb, n, slots, nodes, False, a.reps)
        res[key] = dict(direct=figures(d), lib=hb.LIBPATH)
        print("n %d m %d k %d: direct %.3f ms [%.3f, %.3f]" % (n, m, k, res[key]["direct"]["prep"], res[key]["direct"]["prep_lo"],
                                                              res[key]["direct"]["prep_hi"]), flush=True)
        if a.direct_json:
            continue
        g, stats = run_path(hb, n, slots, nodes, True, a.reps)
        G, D = figures(g), res[key]["direct"]
        P = base.get(key, {}).get("direct")
        sol = solve_root(hb, n, m, slots, b, A0) if k <= 50 else None
        lines.append("n = %d, m = %d, k = %d (%d triplets, %d nodes, %d repetitions)" % (n, m, k, m * k, NODES, a.reps))
        if P is not None:
            lines.append("   direct load, parent commit      %9.3f ms   [%.3f, %.3f]" % (P["prep"], P["prep_lo"], P["prep_hi"]))
        lines.append("   direct load, this build         %9.3f ms   [%.3f, %.3f]" % (D["prep"], D["prep_lo"], D["prep_hi"]))
        lines.append("   gather, this build              %9.3f ms   [%.3f, %.3f]" % (G["prep"], G["prep_lo"], G["prep_hi"]))
        lines.append("   gather alone (to its return)    %9.3f ms   [%.3f, %.3f]" % (G["alone"], G["alone_lo"], G["alone_hi"]))
        lines.append("   per gather: %.1f launches, %.1f read-backs; host builds %d" % (stats[2] / stats[0], stats[3] / stats[0], stats[1]))
        lines.append("   solve of the root               " + ("%9.3f ms   (status %d, %d iterations)" % (sol[2], sol[0], sol[1]) if sol
                     else "not solved: the cost rule keeps a block this dense as a dense array"))
        ref = P if P is not None else D
        spread = max(ref["prep_hi"] - ref["prep_lo"], G["prep_hi"] - G["prep_lo"])
        verdict = "faster" if G["prep"] < ref["prep"] - spread else ("slower" if G["prep"] > ref["prep"] + spread else "no difference")
        lines.append("   verdict: the gather is %s than the direct load of %s (%.3f against %.3f ms, spread %.3f ms)"
                     % (verdict, "the parent commit" if P is not None else "this build", G["prep"], ref["prep"], spread))
        print("\n".join(lines[-8:]), flush=True)
    if a.direct_json:
        json.dump(res, open(a.direct_json, "w"), indent=1)
        return
    with open(a.out, "w") as f:
        f.write("Preparation of a block kept as nonzeros for a node: direct load against the gather from the triplet master\n"
                "(tests/devtools/sparse_master_rate.py; time from hipsdp_set_shape2 to the structure being ready on the device)\n\n")
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
