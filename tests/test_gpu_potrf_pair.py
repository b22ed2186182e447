"""The Cholesky check of a step for blocks above 64 rows as one chain of launches (scip-sdp_amd/csrc/chol.hip: hs_potrf_pair,
kernels.hip: hs_trial_pair), through the unit entries hipsdp_potrf_pair_unit and hipsdp_trial_pair_unit.

  1 hs_potrf_pair against two hs_potrf calls on copies: L, all of dinv - the inverses of the diagonal blocks and the staging blocks of the
    block-column kernel (the last one is never written: zero on both sides) - and both flags, bit for bit.  Orders 65 (two blocks, the
    last of one row), 128 (exact blocks), 129 and 191 (ragged last blocks of 1 and 63 rows), 500 (the bench size).  The two matrices of
    a pair differ in condition, seed and row scaling, so that a job that read the other's matrix, inverses or staging blocks shows
  2 failure cases against hs_potrf: only the first matrix not positive definite, only the second, both - the failing pivot in block 0
    and in the last block, either way round.  Each flag carries its own first failing index (k + 1, LAPACK's info), the other stays 0,
    and what the factorization leaves behind after the failure has the bits of the single form as well
  3 hs_trial_pair against hs_copy / hs_scale_add / hs_copy: orders 65, 130, 500; alpha = 1, 0.37, 2^-20; first attempt (base X, Z,
    saved to Xs, Zs) and halved step (base Xs, Zs): X, Z, Xs, Zs, Lx, Lz bit for bit.  Every array starts from random values, so an
    array that one form writes and the other leaves alone differs.  (The kernel does not claim the upper triangle of Lx: the trailing
    update of the diagonal tiles writes there, hs_zero_upper stays in the X chain.)"""
import numpy as np
import pytest

import chol_cases as cc
from chol_cases import graded, indefinite_at, same_bits

pytestmark = pytest.mark.gpu

ORDERS = (65, 128, 129, 191, 500)
TRIAL_ORDERS = (65, 130, 500)
ALPHAS = (1.0, 0.37, 2.0 ** -20)


def _pair(n):
    """two positive definite matrices of order n that share nothing"""
    return graded(n, 1e2, seed=0), graded(n, 1e8, seed=1, rowscale=True)


def _both(gpu, A0, A1):
    A2 = np.stack([A0, A1])
    return gpu.potrf_pair_unit(A2, pair=False), gpu.potrf_pair_unit(A2, pair=True)


def _same(what, ref, got, bad):
    (L0, d0, f0), (L1, d1, f1) = ref, got
    for k in range(2):
        same_bits("%s: L of matrix %d" % (what, k), np.tril(L1[k]), np.tril(L0[k]), bad)
        same_bits("%s: stored array of matrix %d" % (what, k), L1[k], L0[k], bad)
        same_bits("%s: dinv with staging blocks of matrix %d" % (what, k), d1[k], d0[k], bad)
    if not np.array_equal(f0, f1):
        bad.append((what, "flags differ", f0.tolist(), f1.tolist()))


@pytest.mark.parametrize("n", ORDERS)
def test_pair_has_the_bits_of_two_single_factorizations(gpu, n):
    bad = []
    S0, S1 = _pair(n)
    ref, got = _both(gpu, S0, S1)
    _same("n=%d" % n, ref, got, bad)
    assert ref[2].tolist() == [0, 0] and got[2].tolist() == [0, 0]
    nblk = (n + 63) // 64
    assert ref[1].shape[1] == 2 * nblk * 4096
    # the staging blocks of all block columns but the last hold L_kk: defined, and not all zero
    for k in range(2):
        st = got[1][k, nblk * 4096:].reshape(nblk, 64, 64)
        assert all(np.any(st[b] != 0.0) for b in range(nblk - 1)) and not np.any(st[nblk - 1] != 0.0)
    # (that the single form is a Cholesky factorization is tests/test_gpu_chol.py's business; here only that nothing is trivially equal)
    Lref = np.linalg.cholesky(S0)
    err = np.linalg.norm(np.tril(got[0][0]) - Lref) / np.linalg.norm(Lref)
    print("n=%d: pair against numpy, well-conditioned matrix: %.3e" % (n, err))
    assert err <= 1e-12
    assert not bad, bad


@pytest.mark.parametrize("n", ORDERS)
def test_pair_failure_flags_stay_apart(gpu, n):
    bad = []
    S0, S1 = _pair(n)
    first, last = 5, n - 1                       # a pivot of block 0 and the last pivot (last block)
    cases = [("first only, block 0", first, None), ("first only, last block", last, None),
             ("second only, block 0", None, first), ("second only, last block", None, last),
             ("both, block 0 / last block", first, last), ("both, last block / block 0", last, first),
             ("both, block 0", first, 0), ("both, last block", last, last)]
    for name, k0, k1 in cases:
        T0 = S0 if k0 is None else indefinite_at(S0, k0)
        T1 = S1 if k1 is None else indefinite_at(S1, k1)
        ref, got = _both(gpu, T0, T1)
        want = [0 if k0 is None else k0 + 1, 0 if k1 is None else k1 + 1]
        print("n=%d %s: hs_potrf %s, hs_potrf_pair %s, expected %s" % (n, name, ref[2].tolist(), got[2].tolist(), want))
        if ref[2].tolist() != want or got[2].tolist() != want:
            bad.append((n, name, ref[2].tolist(), got[2].tolist(), want))
        _same("n=%d %s" % (n, name), ref, got, bad)
    assert not bad, bad


@pytest.mark.parametrize("first", (True, False), ids=("first_attempt", "halved_step"))
@pytest.mark.parametrize("n", TRIAL_ORDERS)
def test_trial_iterates_in_one_launch(gpu, n, first):
    bad = []
    rng = np.random.default_rng([n, int(first), 5])
    arrays = rng.standard_normal((8, n, n))
    arrays[2:4] *= 10.0 ** rng.integers(-6, 7, (2, n, n))          # directions of mixed magnitude: every rounding of a x + b y differs
    names = ("X", "Z", "dX", "dZ", "Xs", "Zs", "Lx", "Lz")
    for alpha in ALPHAS:
        ref = gpu.trial_pair_unit(arrays, alpha, fused=False, first=first)
        got = gpu.trial_pair_unit(arrays, alpha, fused=True, first=first)
        for k, nm in enumerate(names):
            same_bits("n=%d alpha=%g %s" % (n, alpha, nm), got[k], ref[k], bad)
        # what the sequence means, stated once more on the host: saved iterate, a x + 1.0 y with one rounding or two, the copy
        base = arrays[0:2] if first else arrays[4:6]
        assert np.array_equal(got[4:6], base) and np.array_equal(got[6:8], got[0:2]) and np.array_equal(got[2:4], arrays[2:4])
        assert np.all(np.abs(got[0:2] - (alpha * arrays[2:4] + base)) <= 2.0 * cc.EPS * (np.abs(alpha * arrays[2:4]) + np.abs(base)))
    assert not bad, bad
