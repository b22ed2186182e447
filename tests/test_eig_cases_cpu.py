"""CPU: the reference of tests/test_gpu_eig_structured.py meets the bounds that file asks of the device - numpy.linalg.eigh on every
case of eig_cases.structured(n) at the scales 2^0, 2^-100, 2^-40, 2^40, 2^100, checked by the same functions with the same no-floor
scale, the analytic spectra against eigvalsh, and the exactness of the scaling.

Measured with numpy on these matrices, worst figure over all sizes, cases and scales: eigenvalue error 4.4e-15, residual 7.1e-15,
orthogonality 8.1e-15, scaling relation 4.4e-15, analytic spectra 1.7e-15 (in units of scale) - two to three orders of magnitude
inside every bound, so no case is left out."""
import numpy as np
import pytest
from eig_cases import structured, scaled, check_all_pairs, check_pairs, check_zero, tridiagonals, ANALYTIC

SIZES = [3, 64, 65, 128, 129, 257, 512]
SCALES = [0, -100, -40, 40, 100]
NAMES = ("cycle", "complete", "ones", "kron_perm", "arrow", "tridiag_dense", "laplacian", "diag_minus_adj", "zero")


@pytest.mark.parametrize("n", SIZES)
def test_numpy_meets_the_relative_bounds(n):
    cases = structured(n)
    assert tuple(cases) == NAMES
    bad = []
    for name, case in cases.items():
        lam0 = np.linalg.eigvalsh(case[0])
        for k in SCALES:
            W, ev, scale = scaled(case, k)
            lam, Q = np.linalg.eigh(W)
            what = "%s 2^%d" % (name, k)
            if name == "zero":
                assert scale == 0.0
                check_zero(what, lam, Q.T, bad)
                continue
            assert scale > 0.0 and scale == np.abs(ev).max()
            bad += check_all_pairs(what, W, ev, scale, lam, Q.T)
            rel = np.abs(lam - 2.0 ** k * lam0).max() / scale
            print("%s: |eigvalsh(2^k W) - 2^k eigvalsh(W)| / scale %.2e" % (what, rel))
            if not rel <= 1e-13:
                bad.append((what, "scaling", rel))
    assert not bad, bad


@pytest.mark.parametrize("n", [2] + SIZES)
def test_analytic_spectra(n):
    bad = []
    for name in ANALYTIC:
        W, ev, scale = structured(n)[name]
        assert np.all(np.diff(ev) >= 0.0), name
        rel = np.abs(np.linalg.eigvalsh(W) - ev).max() / scale
        print("%s n=%d: |eigvalsh - analytic| / scale %.2e" % (name, n, rel))
        if not rel <= 1e-13:
            bad.append((name, n, rel))
    assert not bad, bad


@pytest.mark.parametrize("n", [3, 64, 129])
def test_structure_of_the_cases(n):
    """what the names promise: integer symmetric entries (asserted by the generator), hollow diagonals, zero row sums, exact
    multiplicities, read-only arrays shared between calls"""
    c = structured(n)
    assert structured(n) is c
    for name, (W, ev, scale) in c.items():
        assert not W.flags.writeable and not ev.flags.writeable, name
        assert W.shape == (n, n) and ev.shape == (n,), name
    assert not np.any(np.diag(c["cycle"][0])) and np.all(c["cycle"][0].sum(axis=1) == (2.0 if n > 2 else 1.0))
    assert not np.any(np.diag(c["complete"][0]))
    assert not np.any(c["laplacian"][0].sum(axis=1)) and np.any(c["laplacian"][0])
    if n >= 64:
        assert c["diag_minus_adj"][1][3] < -1.0 and c["diag_minus_adj"][1][-1] > 1.0          # indefinite, four cuts to find
    assert not np.any(c["zero"][0]) and c["zero"][2] == 0.0
    A = np.diag(np.diag(c["laplacian"][0])) - c["laplacian"][0]
    D = c["diag_minus_adj"][0]
    assert set(np.unique(A)) <= {0.0, 1.0} and np.array_equal(np.diag(np.diag(D)) - D, A) and set(np.diag(D)) <= {0.0, 1.0, 2.0}
    b = max(2, n // 8)
    k = n // b
    ev = c["kron_perm"][1]
    distinct = np.unique(np.round(ev, 9))
    assert len(distinct) <= b + 1, (len(distinct), b)
    if k > 1:
        assert np.sum(np.abs(ev - ev[-1]) <= 1e-9) >= k                 # the largest eigenvalue of B, once per copy


def test_selected_pairs_and_the_collecting_mode():
    """check_pairs with a list collects what check_pairs without one asserts; a wrong pair is caught under the no-floor scale where the
    floor at 1 hides it"""
    W, ev, scale = scaled(structured(64)["diag_minus_adj"], -40)
    lam, Q = np.linalg.eigh(W)
    bad = []
    check_pairs("ok", W, ev, scale, 3, lam[2:7], Q.T[2:7], bad)
    assert not bad
    wrong = lam[2:7] * (1.0 + 1e-9)
    check_pairs("wrong", W, ev, scale, 3, wrong, Q.T[2:7], bad)
    assert [b[3] for b in bad] == ["eigenvalues"]
    check_pairs("hidden by the floor", W, ev, max(1.0, scale), 3, wrong, Q.T[2:7])
    with pytest.raises(AssertionError):
        check_pairs("wrong", W, ev, scale, 3, wrong, Q.T[2:7])
    bad = []
    check_zero("not zero", np.array([0.0, 1e-150]), np.eye(2), bad)
    check_zero("nan", np.array([0.0, np.nan]), np.eye(2), bad)
    check_zero("not orthonormal", np.zeros(2), np.ones((2, 2)), bad)
    assert len(bad) == 3


def test_tridiagonals_are_shared_and_read_only():
    t = tridiagonals(33)
    assert tridiagonals(33) is t
    assert tuple(t) == ("toeplitz_121", "wilkinson", "wilkinson_glued", "diagonal_repeated", "ones_cut_every_7th", "graded")
    for name, (d, e, T, ev, scale) in t.items():
        assert len(d) == 33 and len(e) == 32 and not T.flags.writeable and scale >= 1.0
