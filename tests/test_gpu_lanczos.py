"""GPU: the Lanczos kernels of csrc/eig.hip through hs_lanczos_lmin2 as the engine calls it without a solver's exchange vectors
(hipsdp_lambda_min2_unit: k_lmin_tiny up to 16 rows, k_lanczos_fused with one or two matrices per launch up to 8192 rows, a launch per
step above) against a host Lanczos that follows the kernel step by step (tests/harness/lanczos_ref.py) and against numpy's eigvalsh.

Sizes, step counts, families: lanczos_ref.SIZES / STEPS / FAMILIES, every combination.  At 16 rows the exact kernel answers whatever
the step count is, so there the reference is eigvalsh itself: theta = lambda_1, resid = 0, steps_done = n.

Bounds, with scale = max |lambda| of eigvalsh: 1e-12 scale, this project's eigenvalue bound (tests/test_gpu_eig_structured.py,
check_lmin of tests/harness/check_y_cases.py), for theta and resid against the reference and for the two theorems a Ritz value obeys
(it never undershoots lambda_1; some eigenvalue lies within resid of it).  The reference's own spread between float64 and longdouble is
below 1e-15 scale on these matrices (tests/test_lanczos_ref_cpu.py), and the breakdown threshold of 1e-13 scale bounds what a component
dropped on one side and kept on the other can move.  The zero matrix has scale 0: its outputs are held to the absolute 1e-200."""
import numpy as np
import pytest

import lanczos_ref as lr

pytestmark = pytest.mark.gpu

NO_BREAKDOWN = ("wigner", "neg1", "graded", "neg1_up", "neg1_down")      # steps_done = min(steps, n, 250)
ONE_STEP = ("identity", "zero")                                          # the first step finds beta = 0


def bits(*vals):
    return [float(v).hex() for v in vals]


def expected(name, n, lam, run, steps):
    """(theta, resid, steps_done) the device should report"""
    if n <= 16:
        return float(lam[0]), 0.0, n
    return lr.ritz(run, lr.steps_of(n, steps))


@pytest.mark.parametrize("n", lr.SIZES)
@pytest.mark.parametrize("name", lr.FAMILIES)
def test_lanczos_matches_the_krylov_reference_and_eigvalsh(gpu, name, n):
    W = lr.matrix(name, n)
    other = lr.matrix("neg1" if name == "wigner" else "wigner", n)
    lam = np.linalg.eigvalsh(W)
    scale = float(np.max(np.abs(lam)))
    bound = 1e-12 * scale if scale > 0.0 else 1e-200
    run = lr.run(W, 0) if n > 16 else None
    worst = [0.0, 0.0]
    for steps in lr.STEPS:
        k = lr.steps_of(n, steps)
        t_ref, r_ref, d_ref = expected(name, n, lam, run, steps)
        th, rs, sd = gpu.lambda_min2_unit(W, None, steps)
        theta, resid, done = float(th[0]), float(rs[0]), int(sd[0])
        print("%s n = %d steps %d: theta %.17g (ref %.17g, lambda_1 %.17g), resid %.3g (ref %.3g), steps_done %d (ref %d); "
              "|theta - ref| / scale = %.3g, |resid - ref| / scale = %.3g" %
              (name, n, steps, theta, t_ref, lam[0], resid, r_ref, done, d_ref, abs(theta - t_ref) / max(scale, 1e-300),
               abs(resid - r_ref) / max(scale, 1e-300)))
        if scale > 0.0:
            worst = [max(worst[0], abs(theta - t_ref) / scale), max(worst[1], abs(resid - r_ref) / scale)]
        assert np.isfinite(theta) and np.isfinite(resid) and resid >= 0.0
        assert np.isnan(th[1]) and np.isnan(rs[1]) and sd[1] == -1                       # the slot of the matrix that was not given
        # against the reference
        assert abs(theta - t_ref) <= bound, (name, n, steps, theta, t_ref)
        assert abs(resid - r_ref) <= bound, (name, n, steps, resid, r_ref)
        # the theorems
        assert theta >= lam[0] - bound, (name, n, steps, theta, lam[0])
        assert np.min(np.abs(lam - theta)) <= resid + bound, (name, n, steps, theta, resid)
        if steps == 0 and n <= 250:
            assert abs(theta - lam[0]) <= bound and resid <= bound, (name, n, theta, lam[0], resid)
        if name == "zero":
            assert abs(theta) < 1e-200 and resid < 1e-200
        # the step count
        if n <= 16:
            assert done == n
        elif name in NO_BREAKDOWN:
            assert done == k == d_ref, (name, n, steps, done, k, d_ref)
        elif name in ONE_STEP:
            assert done == 1 == d_ref
        else:
            assert 1 <= done <= min(k, d_ref + 1), (name, n, steps, done, d_ref)       # (the device sums in another order)
        # two matrices per launch: the bits of the single call per matrix, in either slot
        th1, rs1, sd1 = gpu.lambda_min2_unit(other, None, steps)
        single0, single1 = bits(th[0], rs[0], sd[0]), bits(th1[0], rs1[0], sd1[0])
        tp, rp, sp = gpu.lambda_min2_unit(W, other, steps)
        assert bits(tp[0], rp[0], sp[0]) == single0 and bits(tp[1], rp[1], sp[1]) == single1, (name, n, steps)
        tp, rp, sp = gpu.lambda_min2_unit(other, W, steps)
        assert bits(tp[0], rp[0], sp[0]) == single1 and bits(tp[1], rp[1], sp[1]) == single0, (name, n, steps)
        tp, rp, sp = gpu.lambda_min2_unit(W, W, steps)
        assert bits(tp[0], rp[0], sp[0]) == single0 == bits(tp[1], rp[1], sp[1]), (name, n, steps)
        # two identical calls
        th2, rs2, sd2 = gpu.lambda_min2_unit(W, None, steps)
        assert bits(th2[0], rs2[0], sd2[0]) == single0
        # the entry of the older tests runs the same launches
        t_old, r_old = gpu.lambda_min(W, steps)
        assert bits(t_old, r_old) == single0[:2]
    print("%s n = %d: largest |theta - ref| / scale = %.3g, |resid - ref| / scale = %.3g" % (name, n, worst[0], worst[1]))


def test_the_launch_per_step_form_above_8192_rows(gpu):
    """n = 8193, 24 steps: hs_lanczos_lmin_unfused (k_lanczos_init, a product and k_lanczos_step per step, k_tridiag_min).  W = H diag(d) H
    with a reflector H is built in O(n^2) and has the spectrum d to rounding (n 2^-53 max |d| at the most, far below the bound), so the
    theorems are checked against d and no eigvalsh of this size is needed."""
    W, d = lr.reflected_diag(lr.BIG_N)
    scale = float(np.max(np.abs(d)))
    bound = 1e-12 * scale
    t_ref, r_ref, d_ref = lr.lanczos(W, lr.BIG_STEPS)
    th, rs, sd = gpu.lambda_min2_unit(W, None, lr.BIG_STEPS)
    theta, resid, done = float(th[0]), float(rs[0]), int(sd[0])
    print("n = %d steps %d: theta %.17g (ref %.17g, lambda_1 %.17g), resid %.3g (ref %.3g), steps_done %d; |theta - ref| / scale = %.3g, "
          "|resid - ref| / scale = %.3g" % (lr.BIG_N, lr.BIG_STEPS, theta, t_ref, d[0], resid, r_ref, done, abs(theta - t_ref) / scale,
                                             abs(resid - r_ref) / scale))
    assert done == lr.BIG_STEPS == d_ref
    assert abs(theta - t_ref) <= bound and abs(resid - r_ref) <= bound
    assert theta >= d[0] - bound
    assert np.min(np.abs(d - theta)) <= resid + bound
