"""CPU: the host Lanczos reference of the GPU tests (tests/harness/lanczos_ref.py) on every family and size those tests use - the
evidence that the matrices are benign for the reference itself, so that what tests/test_gpu_lanczos.py and
tests/test_gpu_check_y_routes.py compare a kernel with does not depend on the reference's own rounding:

 - the float64 and the longdouble run agree in theta and in resid to 1e-13 max |lambda| (lambda: numpy's eigvalsh) at every step count;
 - a Ritz value never undershoots: theta >= lambda_1 - 1e-13 max |lambda|;
 - the residual bound holds: some eigenvalue lies within resid + 1e-13 max |lambda| of theta;
 - the matrix made against the start vector stops after one step with theta = 1 and resid = 0 while its smallest eigenvalue is -1:
   what a run that stops before n steps can miss (hipsdp_check_y sends such a block to the tridiagonal path).

The GPU tests hold the kernels to 1e-12 max |lambda|, ten times the spread allowed here."""
import numpy as np
import pytest

import lanczos_ref as lr

_SPECTRA = {}


def eig(name, n):
    """eigvalsh of a family's matrix, once per process"""
    if (name, n) not in _SPECTRA:
        _SPECTRA[(name, n)] = np.linalg.eigvalsh(lr.matrix(name, n))
    return _SPECTRA[(name, n)]


def check(lam, scale, r64, rld, n, what):
    worst = [0.0, 0.0]
    for steps in lr.STEPS:
        k = lr.steps_of(n, steps)
        t64, s64, d64 = lr.ritz(r64, k)
        tld, sld, dld = lr.ritz(rld, k)
        bound = 1e-13 * scale
        assert abs(t64 - tld) <= bound and abs(s64 - sld) <= bound, (what, steps, t64, tld, s64, sld, d64, dld)
        for t, s in ((t64, s64), (tld, sld)):
            assert t >= lam[0] - bound, (what, steps, t, lam[0])
            assert np.min(np.abs(lam - t)) <= s + bound, (what, steps, t, s)
        if scale > 0.0:
            worst = [max(worst[0], abs(t64 - tld) / scale), max(worst[1], abs(s64 - sld) / scale)]
    return worst


# every family at every size of tests/test_gpu_lanczos.py, and all of them at the 513 rows where tests/test_gpu_check_y_routes.py takes
# its slack from the 250-step reference
CASES = [(name, n) for name in lr.FAMILIES for n in lr.SIZES] + [(name, 513) for name in lr.FAMILIES + lr.TOL_FAMILIES]


@pytest.mark.parametrize("name,n", CASES)
def test_the_two_precisions_agree_and_the_ritz_theorems_hold(name, n):
    W = lr.matrix(name, n)
    lam = eig(name, n)
    scale = float(np.max(np.abs(lam)))
    r64 = lr.run(W, 0, np.float64)
    rld = lr.run(W, 0, np.longdouble)
    worst = check(lam, scale, r64, rld, n, (name, n))
    print("%s n = %d: float64 against longdouble, largest |theta - theta'| / max |lambda| = %.3g, |resid - resid'| / max |lambda| = %.3g, "
          "%d and %d steps" % (name, n, worst[0], worst[1], len(r64.alpha), len(rld.alpha)))
    if name in ("identity", "zero"):
        assert r64.broke == 0 and rld.broke == 0
    if name in ("wigner", "neg1", "graded"):
        assert r64.broke in (-1, n - 1) and rld.broke in (-1, n - 1)          # (the n-th step finds nothing left: beta = 0)


def test_the_run_of_8193_rows():
    """the matrix of the launch-per-step case, H diag(d) H: 24 steps in both precisions (the longdouble product row chunk by row
    chunk), against d"""
    W, d = lr.reflected_diag(lr.BIG_N)
    n = lr.BIG_N
    scale = float(np.max(np.abs(d)))

    def mv(q):
        out = np.empty(n, dtype=np.longdouble)
        for r in range(0, n, 512):
            out[r:r + 512] = W[r:r + 512].astype(np.longdouble) @ q
        return out
    r64 = lr.run(W, lr.BIG_STEPS, np.float64)
    rld = lr.run(n, lr.BIG_STEPS, np.longdouble, matvec=mv)
    t64, s64, d64 = lr.ritz(r64, lr.BIG_STEPS)
    tld, sld, dld = lr.ritz(rld, lr.BIG_STEPS)
    print("8193 rows: theta %.17g / %.17g, resid %.3g / %.3g" % (t64, tld, s64, sld))
    assert d64 == dld == lr.BIG_STEPS
    assert abs(t64 - tld) <= 1e-13 * scale and abs(s64 - sld) <= 1e-13 * scale
    assert t64 >= d[0] - 1e-13 * scale and np.min(np.abs(d - t64)) <= s64 + 1e-13 * scale


@pytest.mark.parametrize("n", [17, 100, 200])
def test_the_matrix_made_against_the_start_vector_stops_after_one_step(n):
    W = lr.adversarial(n, np.random.default_rng([5, n]))
    lam = np.linalg.eigvalsh(W)
    assert abs(lam[0] + 1.0) <= 1e-14 and abs(lam[1] - 1.0) <= 1e-14
    for dtype in (np.float64, np.longdouble):
        theta, resid, done = lr.lanczos(W, 0, dtype)
        assert abs(theta - 1.0) <= 1e-15 and resid == 0.0 and done == 1, (theta, resid, done)
