"""syevx_time.py - time of a selected-eigenpair request above 128 rows: hipsdp_syevx / hipsdp_syevx_below against what a caller pays
today (hipsdp_syev, the full block-Jacobi decomposition) and against one host core.

Sizes 129, 200, 300, 400, 500, 512; a random full-rank matrix and the low_rank_shifted matrix of
test_block_jacobi_on_clustered_spectra; requests: smallest pair, smallest five pairs, smallest five values only, and
hipsdp_syevx_below at a bound with five eigenvalues below it (maxk = 5).  Per figure: the median of --calls calls after --warmup
calls, repeated --reps times; the spread (max - min) of the repetitions stands beside the median.

    python tests/devtools/syevx_time.py --syev-json FILE      hipsdp_syev alone, figures to FILE.  Run it with
                                                              HIPSDP_LIB=<libhipsdp.so of the parent commit>: the
                                                              baseline is never the new build
    python tests/devtools/syevx_time.py [--baseline FILE] [--out profiles/r10_syevx_time.txt]

Without --baseline the hipsdp_syev column comes from the library under test (the function is unchanged by the selected-eigenpair
path) and the table says so.  The kernel count of a call is by construction n + 1 for values (one set-up launch, n - 1 columns, the
multisection) and n + 3 with vectors; compare once with `rocprofv3 --kernel-trace --stats -- python ... --calls 1 --warmup 0 --reps 1`."""
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
SIZES = [129, 200, 300, 400, 500, 512]


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def matrices(n):
    rng = np.random.default_rng(300 + n)
    out = {"random": (lambda G: G + G.T)(rng.standard_normal((n, n))),
           "low_rank_shifted": (lambda B: B @ B.T - 0.01 * np.eye(n))(rng.standard_normal((n, n // 10)))}
    return {k: np.ascontiguousarray(0.5 * (W + W.T)) for k, W in out.items()}


def timed(fn, a):
    """median (ms) over the repetitions and their spread"""
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
    return float(np.median(meds)), float(max(meds) - min(meds))


def host_eigh():
    try:
        from scipy.linalg import eigh
        return "scipy.linalg.eigh(subset_by_index)", lambda W, k, vec: eigh(W, subset_by_index=[0, k - 1], eigvals_only=not vec)
    except ImportError:
        return "numpy.linalg.eigh (all pairs)", lambda W, k, vec: (np.linalg.eigh(W) if vec else np.linalg.eigvalsh(W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--syev-json", default=None)
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hb = binding()
    assert hb.device_count() > 0, "no HIP device"
    if a.syev_json:
        res = {}
        for n in SIZES:
            for name, W in matrices(n).items():
                res["%d %s" % (n, name)] = timed(lambda: hb.syev(W), a)
        with open(a.syev_json, "w") as f:
            json.dump({"lib": hb.LIBPATH, "syev_ms": res}, f)
        return
    base = None
    if a.baseline:
        with open(a.baseline) as f:
            base = json.load(f)
    hname, heigh = host_eigh()
    lines = ["selected eigenpairs above 128 rows: median ms of %d calls (spread of %d repetitions)" % (a.calls, a.reps),
             "hipsdp_syev: %s" % ("library of the parent commit (HIPSDP_LIB)" if base else "library under test (hipsdp_syev is the same code in both)"),
             "host: %s, one core" % hname,
             "kernels per call: n + 3 with vectors, n + 1 values only",
             "",
             "%4s %-17s | %-15s %-15s %-15s %-15s | %-16s | %-9s %-9s | kernels" % ("n", "matrix", "syevx k=1", "syevx k=5", "k=5 values", "below, 5 of 5",
                                                                                  "hipsdp_syev", "host k=1", "host k=5")]
    verdict = []
    for n in SIZES:
        for name, W in matrices(n).items():
            ev = np.linalg.eigvalsh(W)
            bound = 0.5 * (ev[4] + ev[5]) if ev[5] - ev[4] > 1e-8 else ev[4] + 1e-8
            t1 = timed(lambda: hb.syevx(W, 1, 1), a)
            t5 = timed(lambda: hb.syevx(W, 1, 5), a)
            t5v = timed(lambda: hb.syevx(W, 1, 5, vectors=False), a)
            tb = timed(lambda: hb.syevx_below(W, bound, 5), a)
            ts = tuple(base["syev_ms"]["%d %s" % (n, name)]) if base else timed(lambda: hb.syev(W), a)
            h1 = timed(lambda: heigh(W, 1, True), a)
            h5 = timed(lambda: heigh(W, 5, True), a)
            f = lambda t: "%7.3f (%5.3f)" % t
            lines.append("%4d %-17s | %s %s %s %s | %s  | %9.3f %9.3f | %d / %d" % (n, name, f(t1), f(t5), f(t5v), f(tb), f(ts), h1[0], h5[0], n + 3, n + 1))
            if n in (200, 500):
                for k, t in ((1, t1), (5, t5)):
                    ok = t[0] + max(t[1], ts[1]) < ts[0]
                    verdict.append("n = %d, %s, k = %d: %.3f ms against %.3f ms of hipsdp_syev - %s" %
                                   (n, name, k, t[0], ts[0], "below by more than the spread" if ok else "NOT below by more than the spread"))
    lines += ["", "claim (median below hipsdp_syev's by more than the spread, n = 200 and 500, k = 1 and 5, both matrices):"] + verdict
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
