"""GPU: hipsdp_check_y / hipsdp_check_y_tol - the product's accept decision, is lambda_min(Z(y)) >= -tol - at every route check_y_impl
(csrc/ipm.hip) takes, against numpy's eigvalsh of a Z(y) that is known on the host.

   rows       no tolerance                                         tol > 0
   1 - 16     k_lmin_tiny, exact                                   the same
   17 - 64    Lanczos, min(n, 250) steps, theta - resid;           the same
              a run that stopped before n steps: hs_syevx_dev
   65 - 200   as 17 - 64                                           Cholesky of Z + 0.999 tol I: success returns -0.999 tol, failure
   201 - 512  hs_syevx_dev, the first eigenvalue                   the full decomposition (one launch up to 128 rows, block
   > 512      Cholesky of Z - sigma I, sigma = theta - resid       Jacobi above)
              - 1e-9 (1 + |theta|): success returns sigma,
              failure the block Jacobi

A single block is the problem m = 1, A_1 = S, A_0 = 0, y = [1]: Z = S exactly.  Mixed problems have m = 3 and a random y, A_0 chosen so
that Z(y) is the wanted matrix to rounding; their reference is numpy's Z(y) (zmat of tests/harness/check_y_cases.py).

Bounds, scale = max |lambda| of eigvalsh: |lmin - lambda_1| <= 1e-12 scale wherever the eigenvalue itself is returned - the header's
contract, check_lmin's bound.  The zero matrix has scale 0 and is held to the absolute 1e-200 (the figure its Lanczos test uses).  Above
512 rows without a tolerance the call returns a certified lower bound: it must not exceed lambda_1 (soundness), and it may lie below by
what the code's own sigma is allowed - the distance of the 250-step Ritz value of the host reference (tests/harness/lanczos_ref.py) from
lambda_1, its residual bound and the margin 1e-9 (1 + |theta|)."""
import numpy as np
import pytest

import instances
import ipm_ref
import lanczos_ref as lr
from check_y_cases import load, zmat

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 16, 17, 64, 65, 128, 129, 200, 201, 512, 513]
NAMES = lr.FAMILIES + lr.TOL_FAMILIES
TOL = 1e-5
U = 2.0 ** -53


def hexes(a):
    return [float(v).hex() for v in np.asarray(a).reshape(-1)]


def single(gpu, S):
    """the solver whose Z([1]) is S"""
    n = S.shape[0]
    A = np.zeros((2, n, n))
    A[1] = S
    return load(gpu, [A], 1, "dense")


def bound_of(scale):
    return 1e-12 * scale if scale > 0.0 else 1e-200


def check_exact(lmin, lam, what):
    scale = float(np.max(np.abs(lam)))
    print("%s: lmin %.17g, lambda_1 %.17g, |lmin - lambda_1| / max |lambda| = %.3g" %
          (what, lmin, lam[0], abs(lmin - lam[0]) / max(scale, 1e-300)))
    assert abs(lmin - lam[0]) <= bound_of(scale), (what, lmin, lam[0])


def check_with_tolerance(lmin, lam, n, what):
    """n <= 64: the eigenvalue.  Above: -0.999 tol where the factorization of Z + 0.999 tol I succeeds, the eigenvalue where the point
    violates the tolerance.  No family lies within 4e-6 of the threshold."""
    assert abs(lam[0] + 0.999 * TOL) >= 4e-6
    if n <= 64 or lam[0] < -0.999 * TOL:
        check_exact(lmin, lam, what)
        if lam[0] < -TOL:
            assert lmin < -TOL, (what, lmin)
    else:
        print("%s: lmin %.17g, lambda_1 %.17g: the certified bound" % (what, lmin, lam[0]))
        assert abs(lmin + 0.999e-5) <= 1e-18, (what, lmin)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", NAMES)
def test_a_single_block_at_every_route(gpu, name, n):
    """Without a tolerance and with tol = 1e-5, two calls each (identical bits).  At 513 rows the test cannot see whether the
    factorization certified sigma or the block Jacobi computed the eigenvalue: both outcomes satisfy the two inequalities, and
    `graded`, where 250 steps have not converged, is there so that either is plausible."""
    S = lr.matrix(name, n)
    lam = np.linalg.eigvalsh(S)
    scale = float(np.max(np.abs(lam)))
    s = single(gpu, S)
    y = np.ones(1)
    lmin, viol = s.check_y(y)
    again, _ = s.check_y(y)
    lmin_t, viol_t = s.check_y(y, tol=TOL)
    again_t, _ = s.check_y(y, tol=TOL)
    back, _ = s.check_y(y)
    s.close()
    assert viol == 0.0 and viol_t == 0.0
    assert hexes(again) == hexes(lmin) == hexes(back) and hexes(again_t) == hexes(lmin_t)
    what = "%s n = %d" % (name, n)
    if n <= 512:
        check_exact(lmin[0], lam, what)
    else:
        t_ref, r_ref, _ = lr.lanczos(S, 250)
        slack = (t_ref - lam[0]) + r_ref + 1e-9 * (1.0 + abs(t_ref)) + bound_of(scale)
        print("%s: lmin %.17g, lambda_1 %.17g, lambda_1 - lmin = %.3g, allowed %.3g (theta_ref - lambda_1 = %.3g, resid_ref = %.3g)" %
              (what, lmin[0], lam[0], lam[0] - lmin[0], slack, t_ref - lam[0], r_ref))
        assert lmin[0] <= lam[0] + bound_of(scale), (what, lmin[0], lam[0])                 # sound: never above the eigenvalue
        assert lmin[0] >= lam[0] - slack, (what, lmin[0], lam[0], slack)                    # tight: within the slack of sigma
    check_with_tolerance(lmin_t[0], lam, n, what + " tol")
    if name == "outside" and n > 64:
        assert lmin_t[0] < -TOL
    if name in ("optlike", "inside") and n > 64:
        assert abs(lmin_t[0] + 0.999e-5) <= 1e-18


@pytest.mark.parametrize("n", [17, 100, 200])
def test_a_run_that_stops_early_does_not_decide(gpu, n):
    """Z = I - 2 u u^T with u orthogonal to the Lanczos start vector: the run stops after one step with theta = 1 and resid = 0
    (tests/test_lanczos_ref_cpu.py) while lambda_1 = -1.  A run of fewer than n steps has not seen the whole space: the block's
    eigenvalue comes from the tridiagonal path."""
    S = lr.adversarial(n, np.random.default_rng([5, n]))
    t_ref, r_ref, d_ref = lr.lanczos(S, 250)
    assert abs(t_ref - 1.0) <= 1e-15 and r_ref == 0.0 and d_ref == 1
    s = single(gpu, S)
    lmin, _ = s.check_y(np.ones(1))
    lmin_t, _ = s.check_y(np.ones(1), tol=TOL)
    s.close()
    print("n = %d: lmin %.17g, with a tolerance %.17g" % (n, lmin[0], lmin_t[0]))
    assert abs(lmin[0] + 1.0) <= 1e-12
    assert abs(lmin_t[0] + 1.0) <= 1e-12


# ---- mixed problems ----------------------------------------------------------------------------------------------------------------------

MIXED = [(16, "diag"), (17, "neg1"), (64, "graded"), (65, "wigner"), (200, "optlike"), (201, "outside")]
_MIXED = {}


def mixed_problem():
    """m = 3, blocks of the sizes and families of MIXED: A_0 = sum_i y_i A_i - S, so that Z(y) is S to rounding; the reference is the
    spectrum of numpy's Z(y).  Made once."""
    if not _MIXED:
        rng = np.random.default_rng(31)
        m = 3
        y = rng.uniform(-1.0, 1.0, m)
        blocks = []
        for n, name in MIXED:
            A = np.zeros((m + 1, n, n))
            for i in range(1, m + 1):
                R = rng.standard_normal((n, n))
                A[i] = (R + R.T) / (2.0 * np.sqrt(n))
            A[0] = np.tensordot(y, A[1:], axes=(0, 0)) - lr.matrix(name, n)
            A[0] = 0.5 * (A[0] + A[0].T)
            blocks.append(A)
        _MIXED.update(m=m, y=y, blocks=blocks, lam=[np.linalg.eigvalsh(zmat(A, y)) for A in blocks])
    return _MIXED


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_a_mixed_problem_and_its_blocks_in_reverse_order(gpu, form):
    """every block within its route's bound, with and without a tolerance; the same blocks loaded in reverse order give the same numbers
    per block (the Lanczos workspace and the scalar slots are shared across blocks: nothing of one block may reach another)"""
    P = mixed_problem()
    m, y, blocks, lam = P["m"], P["y"], P["blocks"], P["lam"]
    s = load(gpu, blocks, m, form)
    lmin, viol = s.check_y(y)
    lmin_t, _ = s.check_y(y, tol=TOL)
    s.close()
    s = load(gpu, blocks[::-1], m, form)
    rev, _ = s.check_y(y)
    rev_t, _ = s.check_y(y, tol=TOL)
    s.close()
    assert viol == 0.0
    for k, (n, name) in enumerate(MIXED):
        what = "%s block %d (%s, %d rows)" % (form, k, name, n)
        check_exact(lmin[k], lam[k], what)
        check_with_tolerance(lmin_t[k], lam[k], n, what + " tol")
    assert hexes(rev[::-1]) == hexes(lmin) and hexes(rev_t[::-1]) == hexes(lmin_t)


def test_check_y_and_check_y_many_agree(gpu):
    P = mixed_problem()
    m, blocks, lam = P["m"], P["blocks"], P["lam"]
    rng = np.random.default_rng(32)
    Y = np.vstack([P["y"], rng.uniform(-1.0, 1.0, (2, m))])
    s = load(gpu, blocks, m, "dense")
    many, _, served = s.check_y_many(Y)
    assert list(served) == [0] * len(blocks)
    for j, y in enumerate(Y):
        one, _ = s.check_y(y)
        for k, A in enumerate(blocks):
            w = np.linalg.eigvalsh(zmat(A, y))
            top = max(abs(w[0]), abs(w[-1]))
            print("point %d block %d: check_y %.17g, check_y_many %.17g, lambda_1 %.17g" % (j, k, one[k], many[j, k], w[0]))
            assert abs(one[k] - many[j, k]) <= 2e-12 * top, (j, k, one[k], many[j, k])
            assert abs(one[k] - w[0]) <= 1e-12 * top, (j, k, one[k], w[0])
    s.close()


@pytest.mark.parametrize("q", [1, 86])
def test_lpviol_matches_numpy(gpu, q):
    """max(0, -min(D y - c)) within the rounding bound of a sum of m + 1 terms, 4 (m + 1) 2^-53 max_r (|c_r| + sum_i |D_ri y_i|): a point
    of small integers where row r is violated by 0.75, met exactly or has a slack of 0.5 by r mod 3 (exact in every arithmetic), points of
    order 1, and a problem every row of which has slack"""
    m = 5
    rng = np.random.default_rng([q, m, 3])
    Y = rng.uniform(-1.0, 1.0, (4, m))
    Y[0] = rng.integers(-2, 3, m)
    D = rng.integers(-3, 4, (q, m)).astype(np.float64)
    c = D @ Y[0] + np.array([(0.75, 0.0, -0.5)[r % 3] for r in range(q)])
    A = np.zeros((m + 1, 3, 3))
    A[0] = -np.eye(3)
    s = load(gpu, [A], m, "dense", D, c)
    for j, y in enumerate(Y):
        lmin, viol = s.check_y(y)
        _, viol_t = s.check_y(y, tol=TOL)
        ref = max(0.0, float(np.max(c - D @ y)))
        bound = 4 * (m + 1) * U * float(np.max(np.abs(c) + np.abs(D) @ np.abs(y)))
        print("q = %d point %d: lpviol %.17g, numpy %.17g, bound %.3g" % (q, j, viol, ref, bound))
        assert abs(viol - ref) <= bound and float(viol).hex() == float(viol_t).hex()
        assert abs(lmin[0] - 1.0) <= 1e-12
    assert s.check_y(Y[0])[1] == 0.75
    s.close()
    s = load(gpu, [A], m, "dense", D, c - 1.0)
    assert s.check_y(Y[0])[1] == 0.0
    s.close()


def test_check_y_leaves_nothing_behind_for_the_next_solve(gpu):
    """solve, check_y, solve gives the bits of y of solve, solve: the check shares the Lanczos workspace and the scalar slots with the
    solve loop (a block of 100 rows: the step lengths of the loop run the Lanczos kernels on that workspace)"""
    b, A, ys, Xs, Zs = instances.planted_dense(100, 30)
    core = ipm_ref.CoreProblem(b, [A])
    point = ys + 0.25
    out = []
    for between in (False, True):
        s = gpu.Solver(0)
        s.load_core(core)
        assert s.solve(gaptol=1e-6, feastol=1e-6).status == 0
        y1 = s.y()
        if between:
            lam = np.linalg.eigvalsh(zmat(A, point))
            lmin, _ = s.check_y(point)
            check_exact(lmin[0], lam, "between two solves")
            s.check_y(point, tol=TOL)
        assert s.solve(gaptol=1e-6, feastol=1e-6).status == 0
        out.append((y1, s.y()))
        s.close()
    assert hexes(out[0][0]) == hexes(out[1][0]) and hexes(out[0][1]) == hexes(out[1][1])
