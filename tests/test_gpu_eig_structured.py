"""GPU: every eigenvalue entry point on inputs that are not generic - the integer matrices with exact structure of
eig_cases.structured(n) (adjacency, Laplacian, Diag(d) - W, Kronecker blocks behind a permutation, the zero matrix) and the same
matrices times 2^k, k in {-100, -40, 40, 100}, the scale range include/hipsdp.h states for the eigen entries.

Reference: the analytic spectrum or numpy.linalg.eigvalsh (tests/test_eig_cases_cpu.py: numpy meets every bound below with two to
three orders of magnitude to spare).  scale = max|ev| WITHOUT a floor at 1, so all four bounds are relative to the matrix:
|lam - ev| <= 1e-12 scale and ascending, | ||v|| - 1 | <= 1e-12, residual <= 1e-9 scale, |V V^T - I| <= 1e-11.  The zero matrix: lam
finite and max|lam| < 1e-200, V finite and orthonormal to 1e-11.

Sizes are the class edges of the kernels: 3, 64 (matrix in registers), 65, 128 (matrix in LDS), 129, 257, 512 (tridiagonal
multi-launch paths); 130 and 300 for hipsdp_syev alone, which takes the block Jacobi above 128 rows.  Every figure is printed before
it is checked; a test collects what failed and asserts once.

Measured on an MI355X: the worst figure over all sizes and cases of each entry point and scale, eigenvalues and residuals in units of
scale, orthogonality absolute.  The device's figures at 2^-100, 2^-40, 2^40 and 2^100 agree among themselves to the two digits shown.
  entry point               scale          eigenvalues  residual  |V V^T - I|
  syevr                     2^0            5.4e-15      2.2e-14   7.0e-12
  syevr                     2^k, k != 0    5.4e-15      2.2e-14   7.0e-12
  syev                      2^0            5.6e-14      5.5e-14   7.0e-12
  syev                      2^k, k != 0    4.9e-14      4.9e-14   7.0e-12
  batched decomposition     2^0            2.3e-15      1.4e-14   7.0e-12
  syevx                     2^0            5.4e-15      1.3e-14   7.0e-12
  syevx                     2^k, k != 0    5.4e-15      4.7e-15   2.4e-13
  syevx_below               2^0            4.4e-16      6.4e-15   2.6e-13
  syevx_below               2^k, k != 0    3.4e-15      2.0e-15   8.4e-15
  syevi_small               2^0            2.5e-15      1.2e-14   -
  tvec_unit                 2^-100, 2^100  6.3e-15      6.1e-15   2.7e-13
  check_y                   2^0, 2^+-40    2.3e-15      -         -
  eigencuts_all             2^0, 2^+-40    3.3e-14      3.3e-14   3.7e-14
Every 7.0e-12 is one case, diag_minus_adj at 128 rows (pairs 64..71 inside its multiple eigenvalue, the one-launch kernel with the
matrix in LDS), 1.4 times inside the bound; the next largest orthogonality figure of any entry point is 2.7e-13.  The results for 2^k W
are 2^k times the results for W to the bit at every scale; the zero matrix returns at most 1e-300 in absolute value everywhere.
The bound on lhs = v^T A_0 v, which the issue states as 1e-11, is taken relative, 1e-11 scale: lhs scales with A_0."""
import ctypes as C
import numpy as np
import pytest
from eig_cases import structured, scaled, tridiagonals, check_pairs, check_all_pairs, check_zero

pytestmark = pytest.mark.gpu

SIZES = [3, 64, 65, 128, 129, 257, 512]
SCALED = ("cycle", "kron_perm", "diag_minus_adj")
SCALES = (-100, -40, 40, 100)


def _pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def all_pairs(what, case, lam, V, bad):
    W, ev, scale = case
    if scale == 0.0:
        check_zero(what, lam, V, bad)
    else:
        bad += check_all_pairs(what, W, ev, scale, lam, V)


def some_pairs(what, case, first, lam, V, bad):
    W, ev, scale = case
    if scale == 0.0:
        check_zero(what, lam, V, bad)
    else:
        check_pairs(what, W, ev, scale, first, lam, V, bad)


def against_unscaled(what, k, scale, lamk, lam0, bad):
    """the device's own two results: |lam(2^k W) - 2^k lam(W)| <= 1e-12 2^k scale"""
    dev = np.abs(lamk - 2.0 ** k * lam0).max()
    print("%s: |lam(2^k W) - 2^k lam(W)| %.2e (scale %.2e)" % (what, dev, 2.0 ** k * scale))
    if not dev <= 1e-12 * 2.0 ** k * scale:
        bad.append((what, "against the unscaled result", dev))


def gap_bound(case):
    """(bound, eigenvalues <= bound): the midpoint of the gap of the reference spectrum that holds zero or lies just above it"""
    ev = case[1]
    u = np.unique(np.round(ev, 9))
    j = max(0, np.searchsorted(u, 0.0, side="right") - 1)          # the largest distinct value <= 0 (the smallest if none is)
    j = min(j, len(u) - 2)
    b = 0.5 * (u[j] + u[j + 1])
    return float(b), int(np.sum(ev <= b))


# ---- all pairs ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_all_pairs_through_the_tridiagonal_form(gpu, n):
    bad = []
    for name, case in structured(n).items():
        lam, V = gpu.syevr(case[0])
        all_pairs("syevr " + name, case, lam, V, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", [3, 64, 65, 128, 130, 300])
def test_all_pairs_syev(gpu, n):
    bad = []
    for name, case in structured(n).items():
        lam, V = gpu.syev(case[0])
        all_pairs("syev " + name, case, lam, V, bad)
    assert not bad, bad


def test_many_form_on_structured_blocks(gpu):
    """the batched decomposition behind hipsdp_eigencuts_all on the nine cases of 64 and the nine of 128 rows in one call: the bits of
    hipsdp_syev_small per matrix, at most three launches, and the bounds"""
    cases = [("%s %d" % (name, n), c) for n in (64, 128) for name, c in structured(n).items()]
    ns = [c[0].shape[0] for _, c in cases]
    cat = np.concatenate([np.ascontiguousarray(c[0]).reshape(-1) for _, c in cases])
    lam, V = np.zeros(sum(ns)), np.zeros(sum(n * n for n in ns))
    nl = C.c_int(-1)
    rc = gpu.ulib().hipsdp_syev_many_unit(0, len(ns), (C.c_int * len(ns))(*ns), _pd(cat), _pd(lam), _pd(V), C.byref(nl))
    assert rc == 0, gpu.ulib().hipsdp_last_error()
    print("launches %d" % nl.value)
    bad = []
    if not 1 <= nl.value <= 3:
        bad.append(("launches", nl.value))
    lo = vo = 0
    for (what, case), n in zip(cases, ns):
        l1, V1 = np.zeros(n), np.zeros(n * n)
        W = np.ascontiguousarray(case[0])
        assert gpu.lib().hipsdp_syev_small(0, n, _pd(W), _pd(l1), _pd(V1)) == 0
        if not (np.array_equal(lam[lo:lo + n], l1, equal_nan=True) and np.array_equal(V[vo:vo + n * n], V1, equal_nan=True)):
            bad.append((what, "bits differ from hipsdp_syev_small"))
        all_pairs("many " + what, case, lam[lo:lo + n], V[vo:vo + n * n].reshape(n, n), bad)
        lo += n
        vo += n * n
    assert not bad, bad


# ---- selected pairs -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_index_ranges(gpu, n):
    """first, last and eight in the middle, as test_gpu_syevx.py::test_index_ranges chooses them"""
    bad = []
    for name, case in structured(n).items():
        for il, iu in ((1, 1), (n // 2, min(n, n // 2 + 7)), (n, n)):
            lam, V = gpu.syevx(case[0], il, iu)
            some_pairs("syevx " + name, case, il, lam, V, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", SIZES)
def test_below_a_bound_in_a_gap(gpu, n):
    """the bound lies in a gap of the exact spectrum, never on an eigenvalue: the count is exact"""
    c = structured(n)
    maxk = 5
    asked = [("complete", -0.5, n - 1), ("ones", 0.5 * n, n - 1), ("cycle",) + gap_bound(c["cycle"]), ("zero", -1.0, 0), ("zero", 1.0, n)]
    bad = []
    for name, bound, exact in asked:
        assert exact == int(np.sum(c[name][1] <= bound))
        lam, V, nbelow = gpu.syevx_below(c[name][0], bound, maxk)
        print("%s n=%d bound %g: nbelow %d (exact %d), returned %d" % (name, n, bound, nbelow, exact, len(lam)))
        if nbelow != exact:
            bad.append((name, n, bound, "nbelow", nbelow, exact))
        if len(lam) != min(maxk, nbelow):
            bad.append((name, n, bound, "count", len(lam), nbelow))
        if 0 < len(lam) <= exact:
            some_pairs("syevx_below " + name, c[name], 1, lam, V, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", [3, 64, 65, 128])
def test_ith_pair_in_one_launch(gpu, n):
    lib = gpu.lib()
    bad = []
    for name, case in structured(n).items():
        W = np.ascontiguousarray(case[0])
        for i in (1, n // 2, n):
            val, vec = C.c_double(np.nan), np.full(n, np.nan)
            assert lib.hipsdp_syevi_small(0, n, _pd(W), i, C.byref(val), _pd(vec)) == 0
            some_pairs("syevi_small " + name, case, i, np.array([val.value]), vec.reshape(1, n), bad)
    assert not bad, bad


# ---- scales ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_scaled_all_pairs_through_the_tridiagonal_form(gpu, n):
    bad = []
    for name in SCALED:
        case = structured(n)[name]
        lam0, _ = gpu.syevr(case[0])
        for k in SCALES:
            ck = scaled(case, k)
            lam, V = gpu.syevr(ck[0])
            what = "syevr %s 2^%d" % (name, k)
            all_pairs(what, ck, lam, V, bad)
            against_unscaled(what, k, case[2], lam, lam0, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", [64, 128, 300])
def test_scaled_all_pairs_syev(gpu, n):
    bad = []
    for name in SCALED:
        case = structured(n)[name]
        lam0, _ = gpu.syev(case[0])
        for k in SCALES:
            ck = scaled(case, k)
            lam, V = gpu.syev(ck[0])
            what = "syev %s 2^%d" % (name, k)
            all_pairs(what, ck, lam, V, bad)
            against_unscaled(what, k, case[2], lam, lam0, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", [129, 512])
def test_scaled_selected_pairs(gpu, n):
    """first five and last five; the counts below 2^k b are the counts below b of the unscaled matrix"""
    bad = []
    for name in SCALED:
        case = structured(n)[name]
        b, exact = gap_bound(case)
        _, _, nb0 = gpu.syevx_below(case[0], b, 5, vectors=False)
        if nb0 != exact:
            bad.append((name, n, "nbelow", nb0, exact))
        unscaled = {r: gpu.syevx(case[0], r[0], r[1], vectors=False)[0] for r in ((1, 5), (n - 4, n))}
        for k in SCALES:
            ck = scaled(case, k)
            what = "syevx %s 2^%d" % (name, k)
            for (il, iu), lam0 in unscaled.items():
                lam, V = gpu.syevx(ck[0], il, iu)
                some_pairs(what, ck, il, lam, V, bad)
                against_unscaled("%s %d..%d" % (what, il, iu), k, case[2], lam, lam0, bad)
            lam, V, nb = gpu.syevx_below(ck[0], 2.0 ** k * b, 5)
            print("%s: below %g: %d (unscaled %d, exact %d), returned %d" % (what, 2.0 ** k * b, nb, nb0, exact, len(lam)))
            if nb != nb0 or len(lam) != min(5, nb0):
                bad.append((what, "counts below the bound", nb, len(lam), nb0))
            elif len(lam):
                some_pairs(what + " below", ck, 1, lam, V, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", [33, 129, 512])
def test_scaled_tridiagonal_stages_alone(gpu, n):
    bad = []
    for name in ("toeplitz_121", "wilkinson_glued", "graded"):
        d, e, T, ev, _ = tridiagonals(n)[name]
        scale = float(np.abs(ev).max())
        for k in (-100, 100):
            f = 2.0 ** k
            lam, Z = gpu.tvec_unit(d * f, e * f)
            bad += check_all_pairs("tvec_unit %s 2^%d" % (name, k), T * f, ev * f, scale * f, lam, Z)
    assert not bad, bad


# ---- through a solver -----------------------------------------------------------------------------------------------------------

BLOCKS = [64, 128, 257]


def _solver(gpu, A0s, A1s):
    s = gpu.Solver(0)
    s.set_shape(1, [A.shape[0] for A in A0s], 0)
    s.set_obj(np.ones(1))
    for b, (A0, A1) in enumerate(zip(A0s, A1s)):
        s.set_block_dense(b, np.stack([A0, A1]))
    return s


@pytest.mark.parametrize("k", [0, -40, 40])
def test_feasibility_and_cuts_of_scaled_blocks(gpu, k):
    """one variable, A_1 = I, A_0 = -2^k (Diag(d) - W): Z(0) = 2^k (Diag(d) - W) in blocks of 64, 128 (the batched decomposition) and
    257 rows (the per-block route).  lambda_min from hipsdp_check_y, and from hipsdp_eigencuts_all with tol = 2^k 1e-6 the four
    smallest eigenvalues with lhs = v^T A_0 v and coefficient v^T A_1 v = 1"""
    f = 2.0 ** k
    cases = [scaled(structured(n)["diag_minus_adj"], k) for n in BLOCKS]
    s = _solver(gpu, [-c[0] for c in cases], [np.eye(n) for n in BLOCKS])
    y = np.zeros(1)
    lmin, _ = s.check_y(y)
    res = s.eigencuts_all(y, f * 1e-6, 4)
    s.close()
    bad = []
    for b, (W, ev, scale) in enumerate(cases):
        n = BLOCKS[b]
        assert ev[3] < -f * 1e-6
        e0 = abs(lmin[b] - ev[0])
        lm, evs, co, lh, ve = res[b]
        print("2^%d block %d (n = %d): check_y |lmin - ev_min| %.2e, eigencuts_all |lmin - ev_min| %.2e (scale %.2e), cuts %d"
              % (k, b, n, e0, abs(lm - ev[0]), scale, len(evs)))
        if not e0 <= 1e-12 * scale:
            bad.append((k, n, "check_y", e0))
        if not abs(lm - ev[0]) <= 1e-12 * scale:
            bad.append((k, n, "lmin of eigencuts_all", abs(lm - ev[0])))
        if len(evs) != 4:
            bad.append((k, n, "cuts", len(evs)))
            continue
        ee = np.abs(evs - ev[:4]).max()
        el = np.abs(lh - np.array([v @ (-W) @ v for v in ve])).max()
        ec = np.abs(co.reshape(-1) - 1.0).max()
        print("   cuts: |eigvals - ev| %.2e, |lhs - v^T A_0 v| %.2e, |coefs - 1| %.2e" % (ee, el, ec))
        if not ee <= 1e-12 * scale:
            bad.append((k, n, "eigvals", ee))
        if not el <= 1e-11 * scale:
            bad.append((k, n, "lhs", el))
        if not ec <= 1e-11:
            bad.append((k, n, "coefs", ec))
        check_pairs("2^%d cut vectors" % k, W, ev, scale, 1, evs, ve, bad)
    assert not bad, bad


def test_feasibility_and_cuts_of_the_zero_block(gpu):
    """Z(y) = 0: what a block looks like at y = 0 with A_0 = 0"""
    zeros = [np.zeros((n, n)) for n in BLOCKS]
    s = _solver(gpu, zeros, zeros)
    y = np.zeros(1)
    lmin, _ = s.check_y(y)
    res = s.eigencuts_all(y, 1e-6, 4)
    s.close()
    bad = []
    for b, n in enumerate(BLOCKS):
        print("zero block %d (n = %d): check_y lmin %.3e, eigencuts_all lmin %.3e, cuts %d" % (b, n, lmin[b], res[b][0], len(res[b][1])))
        for what, v in (("check_y", lmin[b]), ("eigencuts_all", res[b][0])):
            if not (np.isfinite(v) and abs(v) < 1e-200):
                bad.append((n, what, v))
        if len(res[b][1]) != 0:
            bad.append((n, "cuts", len(res[b][1])))
    assert not bad, bad
