"""syevr_time.py - time of a FULL eigendecomposition above 128 rows: hipsdp_syevr (tridiagonal form, csrc/syevr.hip) against what a
caller gets today (hipsdp_syev, the block-Jacobi decomposition) and against numpy.linalg.eigh on one host core.

Sizes 129, 200, 257, 400, 500, 512; a random full-rank matrix, the low_rank_shifted matrix and the graded matrix of
tests/test_gpu_syevr.py; with and without vectors.  Per figure: the median of --calls calls (host clock around the call, which ends
in a synchronisation of its stream and includes both transfers) after --warmup calls, repeated --reps times; the spread (max - min)
of the repetitions stands beside the median.

    python tests/devtools/syevr_time.py --syev-json FILE      hipsdp_syev alone, figures to FILE.  Run it with
                                                              HIPSDP_LIB=<libhipsdp.so of the parent commit>: the
                                                              baseline is never the new build
    python tests/devtools/syevr_time.py --profile-run         five calls with vectors per matrix at n = 512 and nothing else: the
                                                              program of a SEPARATE run under
                                                              `rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python ...`
    python tests/devtools/syevr_time.py [--baseline FILE] [--kernel-trace DIR/NAME_kernel_trace.csv] [--out profiles/r11_syevr_time.txt]

With --kernel-trace the share of each stage at n = 512 is printed per matrix from the kernel times of that trace (a call starts at
its k_syevx_init).  Without --baseline the hipsdp_syev column comes from the library under test (hipsdp_syev is not rerouted, the same
code in both) and the table says so."""
import argparse
import csv
import importlib.util
import json
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SIZES = [129, 200, 257, 400, 500, 512]
NAMES = ["random", "low_rank_shifted", "graded"]
PROFILE_N, PROFILE_CALLS = 512, 5
ASKS = {200: 3.0, 500: 8.0}                                 # the asks of the verdict, ms
STAGES = [("1 tridiagonalisation", ("k_syevx_init", "k_syevx_col")), ("2 eigenvalues, tables", ("k_syevr_values", "k_syevr_order")),
          ("3 step", ("k_syevr_step",)), ("3 orthogonalisation", ("k_syevr_ortho_prev", "k_syevr_ortho_panel")),
          ("4 back-transformation", ("k_syevr_back",))]


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def matrices(n):
    """the matrices of spectra(n) in tests/harness/eig_cases.py (same generator, same order of draws)"""
    rng = np.random.default_rng(300 + n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    out = {"low_rank_shifted": (lambda B: B @ B.T - 0.01 * np.eye(n))(rng.standard_normal((n, n // 10)))}
    rng.standard_normal(n)                                   # (rank_one)
    out["random"] = (lambda G: G + G.T)(rng.standard_normal((n, n)))
    out["graded"] = (Q * 10.0 ** np.linspace(-6, 6, n)) @ Q.T
    return {k: np.ascontiguousarray(0.5 * (out[k] + out[k].T)) for k in NAMES}


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


def stage_shares(path):
    """per matrix of the profile run: [(stage, microseconds per call, share)] and the kernels per call"""
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((float(r["Start_Timestamp"]), float(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls = []
    for t0, t1, name in rows:
        if "k_syevx_init" in name:
            calls.append([])
        if calls and ("k_syevx_" in name or "k_syevr_" in name):
            calls[-1].append((name, t1 - t0))
    assert len(calls) == PROFILE_CALLS * len(NAMES), "the trace is not one of --profile-run: %d calls" % len(calls)
    out = {}
    for m, mat in enumerate(NAMES):
        mine = calls[m * PROFILE_CALLS + 1:(m + 1) * PROFILE_CALLS]          # (the first call of a matrix is the warm-up)
        tot = {s: 0.0 for s, _ in STAGES}
        for c in mine:
            for name, dt in c:
                for s, keys in STAGES:
                    if any(k in name for k in keys):
                        tot[s] += dt
        total = sum(tot.values())
        out[mat] = ([(s, 1e-3 * tot[s] / len(mine), tot[s] / total) for s, _ in STAGES], len(mine[0]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--syev-json", default=None)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--kernel-trace", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hb = binding()
    assert hb.device_count() > 0, "no HIP device"
    if a.profile_run:
        mats = matrices(PROFILE_N)
        for name in NAMES:
            for _ in range(PROFILE_CALLS):
                hb.syevr(mats[name])
        return
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
    lines = ["all eigenpairs above 128 rows: median ms of %d calls, transfers included (spread of %d repetitions)" % (a.calls, a.reps),
             "hipsdp_syev: %s" % ("library of the parent commit (HIPSDP_LIB)" if base else "library under test (hipsdp_syev is the same code in both)"),
             "host: numpy.linalg.eigh / eigvalsh, one core",
             "kernels per call: n + 6 + 6 ceil(n / 32) with vectors, n + 2 values only",
             "",
             "%4s %-17s | %-15s %-15s | %-15s | %-9s %-9s | kernels" % ("n", "matrix", "syevr", "syevr values", "hipsdp_syev", "eigh", "eigvalsh")]
    verdict = []
    for n in SIZES:
        for name, W in matrices(n).items():
            tv = timed(lambda: hb.syevr(W), a)
            t0 = timed(lambda: hb.syevr(W, vectors=False), a)
            ts = tuple(base["syev_ms"]["%d %s" % (n, name)]) if base else timed(lambda: hb.syev(W), a)
            hv = timed(lambda: np.linalg.eigh(W), a)
            h0 = timed(lambda: np.linalg.eigvalsh(W), a)
            f = lambda t: "%7.3f (%5.3f)" % t
            lines.append("%4d %-17s | %s %s | %s | %9.3f %9.3f | %d / %d" % (n, name, f(tv), f(t0), f(ts), hv[0], h0[0], n + 6 + 6 * ((n + 31) // 32), n + 2))
            ok = tv[0] + max(tv[1], ts[1]) < ts[0]
            v = "n = %d, %s: %.3f ms against %.3f ms of hipsdp_syev - %s" % (n, name, tv[0], ts[0], "FASTER (below by more than the spread)" if ok
                                                                              else "NOT faster (not below by more than the spread)")
            v += "; host eigh %.3f ms - %s" % (hv[0], "below the host" if tv[0] < hv[0] else "LOSES to the host")
            if n in ASKS:
                v += "; ask <= %.0f ms - %s" % (ASKS[n], "met" if tv[0] <= ASKS[n] else "NOT met")
            verdict.append(v)
    lines += ["", "verdict, with vectors (faster = median below hipsdp_syev's by more than the larger of the two spreads):"] + verdict
    if a.kernel_trace:
        lines += ["", "share of each stage at n = %d, with vectors: kernel time per call from a separate kernel trace (%d calls per matrix, the first left out)"
                  % (PROFILE_N, PROFILE_CALLS)]
        for mat, (st, nk) in stage_shares(a.kernel_trace).items():
            lines.append("  %s (%d kernels per call, %.3f ms of kernel time):" % (mat, nk, 1e-3 * sum(us for _, us, _ in st)))
            for s, us, share in st:
                lines.append("    %-24s %9.1f us  %5.1f %%" % (s, us, 100.0 * share))
            big = max(st, key=lambda x: x[1])
            lines.append("    largest: %s" % big[0])
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
