"""GPU: all eigenpairs above 128 rows through the tridiagonal form (hipsdp_syevr, csrc/syevr.hip) and its stages 2 + 3 alone on a
caller's tridiagonal matrix (hipsdp_tvec_unit).

Reference: numpy.linalg.eigvalsh, scale = max(1, max|ev|).  Matrices and checks: tests/harness/eig_cases.py, shared with
test_gpu_syevx.py; the tolerances of check_pairs applied to all n
pairs at once - |lam - ev| <= 1e-12 scale and ascending, | ||v|| - 1 | <= 1e-12, residual <= 1e-9 scale, |V V^T - I| <= 1e-11 over the
whole n x n product.  numpy.linalg.eigh itself meets them on every matrix below.

Dense sizes: 129 (first size of the multi-launch path: four panels and one vector), 130, 193, 257, 512 (the cap); 5 and 128 are
served by the one-launch decomposition behind the same interface, bit for bit.  Tridiagonal sizes: the panel edges 31, 32, 33, 65, 129,
the smallest (2) and the cap."""
import ctypes as C
import threading
import numpy as np
import pytest
import eig_cases
from eig_cases import check_all_pairs, tridiagonals

pytestmark = pytest.mark.gpu

LARGE = [129, 130, 193, 257, 512]
TSIZES = [2, 31, 32, 33, 65, 129, 512]


def spectra(n):
    """the seven spectra of tests/harness/eig_cases.py and, above 50 rows, its two decoupled ones"""
    return eig_cases.spectra(n, decoupled=True)


@pytest.mark.parametrize("n", LARGE)
def test_dense_route(gpu, n):
    bad = []
    for name, (W, ev, scale) in spectra(n).items():
        lam, V = gpu.syevr(W)
        bad += check_all_pairs(name, W, ev, scale, lam, V)
    assert not bad, bad


@pytest.mark.parametrize("n", [5, 128])
def test_small_sizes_are_the_one_launch_decomposition(gpu, n):
    lib = gpu.lib()
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for name in ("random", "low_rank_shifted", "graded"):
        W = np.ascontiguousarray(spectra(n)[name][0])
        lam, V = gpu.syevr(W)
        lam0, V0 = np.zeros(n), np.zeros((n, n))
        assert lib.hipsdp_syev_small(0, n, pd(W), pd(lam0), pd(V0)) == 0
        assert lam.tobytes() == lam0.tobytes() and V.tobytes() == V0.tobytes(), name
        lamv, Vv = gpu.syevr(W, vectors=False)
        assert lib.hipsdp_syev_small(0, n, pd(W), pd(lam0), None) == 0
        assert Vv is None and lamv.tobytes() == lam0.tobytes(), name


@pytest.mark.parametrize("n", TSIZES)
def test_tridiagonal_stages_alone(gpu, n):
    bad = []
    for name, (d, e, T, ev, scale) in tridiagonals(n).items():
        lam, Z = gpu.tvec_unit(d, e)
        bad += check_all_pairs(name, T, ev, scale, lam, Z)
        if name == "toeplitz_121":
            exact = 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))
            err = np.abs(lam - exact).max()
            print("%s n=%d: against 2 - 2 cos(k pi / (n + 1)) %.2e" % (name, n, err))
            if not err <= 1e-12 * scale:
                bad.append((name, n, "analytic", err))
    assert not bad, bad


@pytest.mark.parametrize("n", [129, 512])
def test_values_only_second_call_and_triangle(gpu, n):
    """vectors=False returns None and the same eigenvalue bits; a second call returns the same bits; the triangle DSYEVR('L') reads
    from a column-major array (memory [j n + i], i >= j) is the one that is read"""
    rng = np.random.default_rng(n)
    for name in ("random", "low_rank_shifted", "graded"):
        W = spectra(n)[name][0]
        lam, V = gpu.syevr(W)
        lam0, V0 = gpu.syevr(W, vectors=False)
        assert V0 is None and lam0.tobytes() == lam.tobytes(), name
        lam2, V2 = gpu.syevr(W)
        assert lam2.tobytes() == lam.tobytes() and V2.tobytes() == V.tobytes(), name
        B = np.triu(W) + np.tril(rng.standard_normal((n, n)), -1)
        lamb, Vb = gpu.syevr(B)
        assert lamb.tobytes() == lam.tobytes() and Vb.tobytes() == V.tobytes(), name


def test_agrees_with_selected_pairs(gpu):
    n = 257
    for name in ("random", "graded"):
        W, ev, scale = spectra(n)[name]
        lam, _ = gpu.syevr(W, vectors=False)
        for il, iu in ((1, 1), (1, 32), (n // 2, n // 2 + 7), (n - 4, n)):
            lx, _ = gpu.syevx(W, il, iu, vectors=False)
            err = np.abs(lam[il - 1:iu] - lx).max()
            print("%s %d..%d: |syevr - syevx| %.2e (scale %.2e)" % (name, il, iu, err, scale))
            assert err <= 1e-12 * scale, (name, il, iu, err)


def test_arguments(gpu):
    lib = gpu.lib()
    n = 130
    A = np.ascontiguousarray(spectra(n)["random"][0])
    big = np.ascontiguousarray(spectra(512)["random"][0])
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lam, V = np.zeros(513), np.zeros((513, 513))
    bad = 3                                                  # HIPSDP_ERR_ARG
    assert lib.hipsdp_syevr(0, 0, pd(A), pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevr(0, -1, pd(A), pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevr(0, 513, pd(V), pd(lam), None) == bad
    assert lib.hipsdp_syevr(0, n, None, pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevr(0, n, pd(A), None, pd(V)) == bad
    # the cap itself is served, with and without vectors
    ev, scale = spectra(512)["random"][1:]
    assert lib.hipsdp_syevr(0, 512, pd(big), pd(lam), None) == 0
    assert np.abs(lam[:512] - ev).max() <= 1e-12 * scale
    lam2 = np.zeros(512)
    assert lib.hipsdp_syevr(0, 512, pd(big), pd(lam2), pd(V)) == 0
    assert lam2.tobytes() == lam[:512].tobytes()


def test_no_allocation_on_a_repeated_call(gpu):
    lib = gpu.lib()
    W = spectra(257)["random"][0]
    gpu.syevr(W)                                             # warm-up: the context grows here
    f0, f1, tot = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    assert lib.hipsdp_mem_info(0, C.byref(f0), C.byref(tot)) == 0
    for _ in range(5):
        gpu.syevr(W)
    assert lib.hipsdp_mem_info(0, C.byref(f1), C.byref(tot)) == 0
    assert f0.value == f1.value, (f0.value, f1.value)


def test_two_host_threads(gpu):
    """each host thread has its own context (stream, staging, pool): two threads, four calls each on different matrices, reproduce
    the single-thread bits"""
    names = [("random", "graded", "close_pairs", "tight_cluster"), ("low_rank_shifted", "two_clusters", "block_diagonal", "rank_one")]
    mats = [[spectra(193)[nm][0] for nm in row] for row in names]
    ref = [[gpu.syevr(W) for W in row] for row in mats]
    bad = []

    def work(t):
        for i, W in enumerate(mats[t]):
            lam, V = gpu.syevr(W)
            if lam.tobytes() != ref[t][i][0].tobytes() or V.tobytes() != ref[t][i][1].tobytes():
                bad.append((t, i))

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, bad
