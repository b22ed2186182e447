"""rank1_check_rate.py - time of the rank-1 part of CONSCHECK for `count` candidate points: ONE hipsdp_rank1_check_many call against
  (a) what the library offered before it, per candidate and block: Z in numpy, hipsdp_syevi_small up to 128 rows / hipsdp_syevx above for
      the indices 1 and n - 1 (the path of SCIPlapackComputeIthEigenvalue), and the two minor scans vectorised in numpy on one core
      (those entries are unchanged, so this build's library runs them);
  (b) numpy alone on one core: eigvalsh and the same scans.
and ONE hipsdp_rank1_approx call against Z in numpy, hipsdp_syev_small up to 128 rows / hipsdp_syevr above, and the right-hand side in
numpy.

Shapes: 6 blocks of 3 rows, m = 51 (example_rank1_*.cbf); 32 blocks of 12, m = 40; 2 blocks of 128, m = 100; 4 blocks of 200, m = 100;
one block of 512, m = 100.  count 1 and 64 (8 at 512 rows).  The new calls: median of three timed calls after one warm-up, host clock
around a call that ends in its read-back, with the smallest and the largest of the three beside it.  (a) and (b) are loops, linear in
count: they are timed the same way on min(count, 8) candidates and scaled.

    python tests/devtools/rank1_check_rate.py [--out profiles/r30_rank1_check_rate.txt] [--shapes 0,1]"""
import argparse
import ctypes as C
import importlib.util
import os
import sys
import time

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("OPENBLAS_NUM_THREADS", "1")
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests", "harness"))

SHAPES = [("6 blocks of 3", [3] * 6, 51, 64), ("32 blocks of 12", [12] * 32, 40, 64), ("2 blocks of 128", [128] * 2, 100, 64),
          ("4 blocks of 200", [200] * 4, 100, 64), ("1 block of 512", [512], 100, 8)]
FEASTOL = 1e-6


def binding():
    spec = importlib.util.spec_from_file_location("hipsdp_binding", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def problem(ns, m, seed):
    """entries of order 1 / sqrt(n), points of order 1: Z(y) indefinite, as at a rounded point"""
    rng = np.random.default_rng(seed)
    blocks = []
    for n in ns:
        R = rng.standard_normal((m + 1, n, n)) / np.sqrt(n)
        blocks.append((R + R.transpose(0, 2, 1)) / 2.0)
    return blocks, rng.uniform(-1.0, 1.0, (64, m))


def three(fn):
    """(median, smallest, largest) ms of three calls after a warm-up"""
    fn()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated indices into the list of shapes (default: all)")
    a = ap.parse_args()
    import ipm_ref
    import rank1_cases as r1
    hb = binding()
    lib = hb.lib()
    dp = lambda x: x.ctypes.data_as(C.POINTER(C.c_double))

    def ith(Z, i):
        n = Z.shape[0]
        if n <= 128:
            ev = C.c_double(0.0)
            assert lib.hipsdp_syevi_small(0, n, dp(Z), int(i), C.byref(ev), None) == 0
            return ev.value
        return hb.syevx(Z, i, i, vectors=False)[0][0]

    def old_check(blocks, Y):
        out = []
        for y in Y:
            for A in blocks:
                Z = np.ascontiguousarray(r1.zmat(A, y))
                n = Z.shape[0]
                out.append((ith(Z, 1), ith(Z, n - 1), r1.scan_ev(Z), r1.scan_det(Z, FEASTOL)))
        return out

    def numpy_check(blocks, Y):
        out = []
        for y in Y:
            for A in blocks:
                Z = r1.zmat(A, y)
                w = np.linalg.eigvalsh(Z)
                out.append((w[0], w[-2], r1.scan_ev(Z), r1.scan_det(Z, FEASTOL)))
        return out

    def old_approx(blocks, y):
        out = []
        for A in blocks:
            Z = np.ascontiguousarray(r1.zmat(A, y))
            n = Z.shape[0]
            if n <= 128:
                lam, V = np.zeros(n), np.zeros((n, n))
                assert lib.hipsdp_syev_small(0, n, dp(Z), dp(lam), dp(V)) == 0
            else:
                lam, V = hb.syevr(Z)
            out.append(r1.rhs(A[0], lam[-1], V[-1]))
        return out

    picked = range(len(SHAPES)) if a.shapes is None else [int(t) for t in a.shapes.split(",")]
    lines = ["# rank-1 part of CONSCHECK for `count` points: ms, median of 3 calls after a warm-up [smallest, largest]; (a) and (b) timed on",
             "# min(count, 8) points and scaled; ratio = (a) / hipsdp_rank1_check_many; wins: (a) median > the call's LARGEST repetition",
             "# shape              m  count | rank1_check_many [min, max] | (a) syevi_small / syevx x 2 + numpy scans | ratio | wins | (b) numpy alone | launches read-backs"]
    alines = ["# hipsdp_rank1_approx (one point, all blocks): ms as above; (a) Z in numpy, hipsdp_syev_small / hipsdp_syevr, rhs in numpy",
              "# shape              m | rank1_approx [min, max] | (a) | ratio | launches read-backs"]
    for si in picked:
        name, ns, m, cmax = SHAPES[si]
        blocks, Y = problem(ns, m, si)
        s = hb.Solver(0)
        s.load_core(ipm_ref.CoreProblem(np.zeros(m), blocks, None, None))
        for count in (1, cmax):
            st0 = hb.rank1_check_many_stats()
            res = s.rank1_check_many(Y[:count], FEASTOL)
            st1 = hb.rank1_check_many_stats()
            assert np.all(res[5] == 0)
            ref = numpy_check(blocks, Y[:1])
            for b in range(len(ns)):
                top = max(abs(res[0][0, b, 0]), abs(res[0][0, b, 2]))
                assert abs(res[0][0, b, 0] - ref[b][0]) <= 1e-10 * top and abs(res[0][0, b, 1] - ref[b][1]) <= 1e-10 * top
                assert abs(res[1][0, b] - ref[b][2][0]) <= 1e-10 * top
            new = three(lambda: s.rank1_check_many(Y[:count], FEASTOL))
            k = min(count, 8)
            old = three(lambda: old_check(blocks, Y[:k]))
            host = three(lambda: numpy_check(blocks, Y[:k]))
            f = count / k
            lines.append("%-18s %5d %5d | %10.3f [%.3f, %.3f] | %10.3f [%.3f, %.3f] | %7.2f | %-4s | %10.3f | %d %d" % (
                name, m, count, new[0], new[1], new[2], old[0] * f, old[1] * f, old[2] * f, old[0] * f / new[0],
                "yes" if old[0] * f > new[2] else "NO", host[0] * f, st1[1] - st0[1], st1[2] - st0[2]))
            print(lines[-1], flush=True)
        st0 = hb.rank1_approx_stats()
        out, served = s.rank1_approx(Y[0])
        st1 = hb.rank1_approx_stats()
        assert np.all(served == 0)
        want = old_approx(blocks, Y[0])
        for b in range(len(ns)):
            # (the sign of the vector is free: the right-hand side does not see it)
            assert np.max(np.abs(out[b][2] - want[b])) <= 1e-8 * max(1.0, abs(out[b][0])), (name, b)
        new = three(lambda: s.rank1_approx(Y[0]))
        old = three(lambda: old_approx(blocks, Y[0]))
        alines.append("%-18s %5d | %10.3f [%.3f, %.3f] | %10.3f [%.3f, %.3f] | %7.2f | %d %d" % (
            name, m, new[0], new[1], new[2], old[0], old[1], old[2], old[0] / new[0], st1[1] - st0[1], st1[2] - st0[2]))
        print(alines[-1], flush=True)
        s.close()
    txt = "\n".join(lines + alines)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
