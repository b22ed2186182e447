"""rounding_frame_rate.py - time of stage 1 of the primal rounding problem: ONE hipsdp_rounding_frame call over all blocks against
(a) what the project offered before the call: hipsdp_syev_small (up to 128 rows) / hipsdp_syevr (above) per block for the decompositions,
    and the coefficient loops in numpy on one core (per matrix sum((V A_i) * V, axis 1): BLAS, one thread);
(b) the numpy restatement alone (eigh per block and the same coefficient loops).
The two eigen entries of (a) are the same code in the parent commit and in this build, so (a) is timed with this build's library.

Shapes: 32 blocks of 12 rows; 4 blocks of 40; 2 blocks of 128 with m = 1000; 4 blocks of 200; one and 8 blocks of 512 with m = 1000; one
block of 512 with m = 20 (the K-split case).  Every figure is the median of three timed calls after one warm-up call, host clock around a
call that ends in its read-back.  (a) and (b) are loops over the matrices: above 128 rows their coefficient part is timed on 8 matrices
per block and scaled to m + 1.

    python tests/devtools/rounding_frame_rate.py [--shapes 0,1,..] [--out profiles/r29_rounding_frame_rate.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tests/devtools/rounding_frame_rate.py --trace 4 --calls 5
        five calls of one shape and nothing else; then
    python tests/devtools/rounding_frame_rate.py --kernels-csv DIR/.../..._kernel_stats.csv --trace 4 --calls 5 --kernels-out FILE
        the kernel shares, and for k_rf_coefs_mc the executed flops (every tile runs 64 x 64 x 16 multiply-adds per panel, padding
        included) over its kernel time as a fraction of the 78.6 TFLOP/s of the FP64 matrix cores."""
import argparse
import csv
import importlib.util
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "harness"))

SHAPES = [("32 blocks of 12", [12] * 32, 40), ("4 blocks of 40", [40] * 4, 40), ("2 blocks of 128", [128] * 2, 1000),
          ("4 blocks of 200", [200] * 4, 100), ("1 block of 512", [512], 1000), ("8 blocks of 512", [512] * 8, 1000),
          ("1 block of 512, K-split", [512], 20)]
PEAK = 78.6e12


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def problem(ns, m, seed):
    rng = np.random.default_rng(seed)
    blocks, X = [], []
    for n in ns:
        if blocks and (m + 1) * n * n > 1 << 26:
            blocks.append(blocks[0])                   # (blocks of gigabytes: one set of matrices on the host, a copy per block on the device)
        else:
            R = rng.standard_normal((m + 1, n, n)) / np.sqrt(n)
            blocks.append((R + R.transpose(0, 2, 1)) / 2.0)
        R = rng.standard_normal((n, n)) / np.sqrt(n)
        X.append((R + R.T) / 2.0)
    return blocks, X


def med3(fn):
    fn()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def coef_loops(V, A, cap):
    """seconds of the coefficient loops of one block, scaled to all its matrices when only `cap` of them are timed"""
    k = A.shape[0] if cap is None else min(cap, A.shape[0])
    t0 = time.perf_counter()
    for i in range(k):
        np.sum((V @ A[i]) * V, axis=1)
    return (time.perf_counter() - t0) * A.shape[0] / k


def slices_of(n, m):
    """hs_rf_slice_rule of csrc/hs_round_plan.h for a packed block (the form of a dense-loaded block above 64 rows)"""
    klen = n * (n + 1) // 2
    tiles = -(-n // 64) * -(-(m + 1) // 64)
    panels = -(-klen // 16)
    want = max(1, min(-(-512 // tiles), panels // 64, 64))
    pps = max(1, -(-panels // want))
    return -(-panels // pps), pps, panels


def mc_flops(ns, m):
    """multiply-adds x 2 the matrix-core launch executes for the blocks above 64 rows"""
    total = 0
    for n in ns:
        if n <= 64:
            continue
        sl, pps, panels = slices_of(n, m)
        tiles = -(-n // 64) * -(-(m + 1) // 64)
        total += 2 * tiles * panels * 64 * 64 * 16
    return total


def kernels_report(a):
    name, ns, m = SHAPES[a.trace]
    rows = []
    with open(a.kernels_csv) as f:
        for r in csv.DictReader(f):
            rows.append((r["Name"].replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split()[-1], int(r["Calls"]), float(r["TotalDurationNs"])))
    total = sum(r[2] for r in rows)
    lines = ["# hipsdp_rounding_frame, %s, m = %d: kernel trace of %d calls (rocprofv3 --kernel-trace --stats, a run of its own; one MI355X);"
             % (name, m, a.calls), "# microseconds per call and share of the kernel time of a call", "# kernel | launches per call | us per call | share"]
    for nm, calls, ns_total in sorted(rows, key=lambda r: -r[2]):
        lines.append("%-60s | %6.1f | %10.1f | %5.1f%%" % (nm[:60], calls / a.calls, ns_total / a.calls / 1e3, 100.0 * ns_total / total))
    mc = [r for r in rows if "k_rf_coefs_mc" in r[0]]
    if mc:
        t = mc[0][2] / a.calls * 1e-9
        fl = mc_flops(ns, m)
        lines.append("# k_rf_coefs_mc: %.3e executed flops per call (padded tiles included) / %.1f us = %.2f TFLOP/s = %.1f%% of %.1f TFLOP/s"
                     % (fl, t * 1e6, fl / t / 1e12, 100.0 * fl / t / PEAK, PEAK / 1e12))
        lines.append("# (kernel time from the trace, not from HIP events: the call owns its stream and offers no event hook)")
    txt = "\n".join(lines)
    print(txt)
    if a.kernels_out:
        with open(a.kernels_out, "w") as f:
            f.write(txt + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into the list of shapes (default: all)")
    ap.add_argument("--trace", type=int, default=None, help="index of one shape: --calls calls of it and nothing else")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--kernels-csv", default=None)
    ap.add_argument("--kernels-out", default=None)
    a = ap.parse_args()
    if a.kernels_csv is not None:
        return kernels_report(a)
    import ipm_ref
    hb = binding()
    if a.trace is not None:
        name, ns, m = SHAPES[a.trace]
        blocks, X = problem(ns, m, a.trace)
        s = hb.Solver(0)
        s.load_core(ipm_ref.CoreProblem(np.zeros(m), blocks, None, None))
        for _ in range(a.calls):
            s.rounding_frame(X)
        s.close()
        return
    picked = range(len(SHAPES)) if a.shapes is None else [int(t) for t in a.shapes.split(",")]
    lines = ["# stage 1 of the primal rounding problem: median ms of 3 calls after a warm-up, one MI355X; (a) = hipsdp_syev_small / hipsdp_syevr per",
             "# block + numpy coefficient loops on one core, (b) = numpy alone (eigh + the same loops); above 128 rows the loops are timed on 8",
             "# matrices per block and scaled; recombine = ONE hipsdp_rounding_recombine (mode 0) on the frame",
             "# shape                     m | rounding_frame | (a) eig entries + numpy loops | (a) / new | (b) numpy | (b) / new | launches read-backs | recombine"]
    for si in picked:
        name, ns, m = SHAPES[si]
        blocks, X = problem(ns, m, si)
        s = hb.Solver(0)
        s.load_core(ipm_ref.CoreProblem(np.zeros(m), blocks, None, None))
        st0 = hb.rounding_stats()
        eig, obj, coefs, vecs, served = s.rounding_frame(X)
        st1 = hb.rounding_stats()
        assert np.all(served == 0)
        n0 = ns[0]
        V0 = vecs[:n0 * n0].reshape(n0, n0)
        want = np.sum((V0 @ blocks[0][1]) * V0, axis=1)
        assert np.max(np.abs(coefs[:n0, 0] - want)) <= 1e-9, name
        new_ms = med3(lambda: s.rounding_frame(X))
        rec_ms = med3(lambda: s.rounding_recombine(eig, 1e-9, 0))
        cap = 8 if n0 > 128 else None
        eig_fn = (lambda M: hb.syevr(M)) if n0 > 128 else (lambda M: hb.syev(M))
        pairs = [eig_fn(M) for M in X]
        eig_ms = med3(lambda: [eig_fn(M) for M in X])
        loops_ms = 1e3 * sum(coef_loops(V, A, cap) for (_, V), A in zip(pairs, blocks))
        t0 = time.perf_counter()
        for M in X:
            np.linalg.eigh(M)
        eigh_ms = 1e3 * (time.perf_counter() - t0)
        a_ms, b_ms = eig_ms + loops_ms, eigh_ms + loops_ms
        s.close()
        lines.append("%-24s %5d | %14.3f | %12.3f (%.3f + %.3f) | %7.2f | %10.1f | %7.2f | %d %d | %.3f" % (
            name, m, new_ms, a_ms, eig_ms, loops_ms, a_ms / new_ms, b_ms, b_ms / new_ms, st1[1] - st0[1], st1[2] - st0[2], rec_ms))
        print(lines[-1], flush=True)
    txt = "\n".join(lines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
