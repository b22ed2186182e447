"""GPU: selected eigenpairs without a full decomposition (hipsdp_syevx / hipsdp_syevx_below, csrc/syevx.hip).

Sizes: 129 (first size of the multi-launch path), 130 (even), 193 (not divisible by the rows per workgroup), 257 (one past a power of
two), 512 (the cap); 5, 64, 128 are served by the one-launch kernels behind the same interface.  Matrices (the seven spectra),
reference and tolerances: tests/harness/eig_cases.py, shared with test_gpu_syevr.py."""
import ctypes as C
import threading
import numpy as np
import pytest
from eig_cases import spectra, check_pairs

pytestmark = pytest.mark.gpu

LARGE = [129, 130, 193, 257, 512]
SMALL = [5, 64, 128]


@pytest.mark.parametrize("n", [129, 193, 512])
def test_tridiagonalisation_alone(gpu, n):
    """stage 1 at its own scale: Q accumulated on the host from the reflectors; random, and the matrix with a decoupled row of the
    i-th-eigenpair test"""
    rng = np.random.default_rng(40 + n)
    G = rng.standard_normal((n, n))
    A = 0.5 * (G + G.T)
    Z = A.copy()
    Z[2, :] = Z[:, 2] = 0.0
    Z[2, 2] = Z[3, 3]
    for name, W in (("random", A), ("zeroed_row", Z)):
        d, e, Vr, tau = gpu.tridiag_unit(W)
        Q = np.eye(n)
        for j in range(n - 1):
            Q -= np.outer(Q @ Vr[j], tau[j] * Vr[j])
        T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
        ev = np.linalg.eigvalsh(W)
        scale = max(1.0, np.abs(ev).max())
        o, r, v = np.abs(Q.T @ Q - np.eye(n)).max(), np.abs(Q.T @ W @ Q - T).max(), np.abs(np.linalg.eigvalsh(T) - ev).max()
        print("%s n=%d: |Q^T Q - I| %.2e, |Q^T A Q - T| %.2e, eigenvalues %.2e (scale %.2e)" % (name, n, o, r, v, scale))
        assert o <= 1e-11, (name, o)
        assert r <= 1e-11 * scale, (name, r)
        assert v <= 1e-12 * scale, (name, v)


@pytest.mark.parametrize("n", LARGE + SMALL)
def test_index_ranges(gpu, n):
    """DSYEVR RANGE = 'I' on every spectrum: first, first five, last five, eight in the middle, last (ranges clipped to 1 .. n at
    n = 5), and the full 32 at n = 257; values-only call and a second call return the same bits"""
    ranges = [(1, 1), (1, 5), (n - 4, n), (n // 2, min(n, n // 2 + 7)), (n, n)] + ([(1, 32)] if n == 257 else [])
    for name, (W, ev, scale) in spectra(n).items():
        for il, iu in ranges:
            lam, V = gpu.syevx(W, il, iu)
            check_pairs(name, W, ev, scale, il, lam, V)
            lam0, V0 = gpu.syevx(W, il, iu, vectors=False)
            assert V0 is None and lam0.tobytes() == lam.tobytes(), (name, il, iu)
            lam2, V2 = gpu.syevx(W, il, iu)
            assert lam2.tobytes() == lam.tobytes() and V2.tobytes() == V.tobytes(), (name, il, iu)


@pytest.mark.parametrize("n", LARGE + SMALL)
def test_below_a_bound(gpu, n):
    """DSYEVR RANGE = 'V' with a cap: the n - n // 10 eigenvalues -0.01 of the shifted low-rank matrix, a bound inside and one below a
    random spectrum"""
    W, ev, scale = spectra(n)["low_rank_shifted"]
    lam, V, nbelow = gpu.syevx_below(W, -1e-6, 5)
    assert len(lam) == 5 and nbelow == n - n // 10, (len(lam), nbelow)
    check_pairs("low_rank_shifted", W, ev, scale, 1, lam, V)
    lam0, V0, nb0 = gpu.syevx_below(W, -1e-6, 0)
    assert len(lam0) == 0 and nb0 == n - n // 10
    lamv, Vv, nbv = gpu.syevx_below(W, -1e-6, 5, vectors=False)
    assert Vv is None and nbv == nbelow and lamv.tobytes() == lam.tobytes()
    W, ev, scale = spectra(n)["random"]
    lam, V, nbelow = gpu.syevx_below(W, 0.5 * (ev[2] + ev[3]), 32)
    assert len(lam) == 3 and nbelow == 3, (len(lam), nbelow)
    check_pairs("random", W, ev, scale, 1, lam, V)
    lam, V, nbelow = gpu.syevx_below(W, ev[0] - 1.0, 5)
    assert len(lam) == 0 and nbelow == 0


@pytest.mark.parametrize("n", [128, 129, 512])
def test_only_the_dsyevr_triangle_is_read(gpu, n):
    """the triangle DSYEVR('L') reads from a column-major array (memory [j n + i], i >= j): noise in the other one changes nothing"""
    W, ev, scale = spectra(n)["random"]
    rng = np.random.default_rng(n)
    B = np.triu(W) + np.tril(rng.standard_normal((n, n)), -1)
    for il, iu in ((1, 1), (1, 5)):
        lam, V = gpu.syevx(W, il, iu)
        lamb, Vb = gpu.syevx(B, il, iu)
        assert lamb.tobytes() == lam.tobytes() and Vb.tobytes() == V.tobytes(), (il, iu)
    lam, V, nb = gpu.syevx_below(W, 0.5 * (ev[2] + ev[3]), 5)
    lamb, Vb, nbb = gpu.syevx_below(B, 0.5 * (ev[2] + ev[3]), 5)
    assert nb == nbb == 3 and lamb.tobytes() == lam.tobytes() and Vb.tobytes() == V.tobytes()


def test_arguments(gpu):
    lib = gpu.lib()
    n = 130
    A = np.ascontiguousarray(spectra(n)["random"][0])
    big = np.ascontiguousarray(spectra(512)["random"][0])
    pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lam, V = np.zeros(40), np.zeros((40, 513))
    cnt, nb = C.c_int(0), C.c_int(0)
    bad = 3                                                  # HIPSDP_ERR_ARG
    assert lib.hipsdp_syevx(0, 0, pd(A), 1, 1, pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx(0, 513, pd(V), 1, 1, pd(lam), None) == bad
    assert lib.hipsdp_syevx(0, n, pd(A), 0, 1, pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx(0, n, pd(A), 1, n + 1, pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx(0, n, pd(A), 5, 4, pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx(0, n, pd(A), 1, 33, pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx(0, n, None, 1, 1, pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx(0, n, pd(A), 1, 1, None, pd(V)) == bad
    b = C.c_double(0.0)
    assert lib.hipsdp_syevx_below(0, 0, pd(A), b, 1, C.byref(cnt), C.byref(nb), pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx_below(0, 513, pd(V), b, 1, C.byref(cnt), C.byref(nb), pd(lam), None) == bad
    assert lib.hipsdp_syevx_below(0, n, pd(A), b, -1, C.byref(cnt), C.byref(nb), pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx_below(0, n, pd(A), b, 33, C.byref(cnt), C.byref(nb), pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx_below(0, n, None, b, 1, C.byref(cnt), C.byref(nb), pd(lam), pd(V)) == bad
    assert lib.hipsdp_syevx_below(0, n, pd(A), b, 1, C.byref(cnt), C.byref(nb), None, pd(V)) == bad
    assert lib.hipsdp_syevx_below(0, n, pd(A), b, 1, None, C.byref(nb), pd(lam), pd(V)) == bad
    # the cap itself is served: n = 512, 32 pairs; nbelow may be NULL
    assert lib.hipsdp_syevx(0, 512, pd(big), 1, 32, pd(lam), pd(V)) == 0
    assert lib.hipsdp_syevx_below(0, 512, pd(big), b, 32, C.byref(cnt), None, pd(lam), pd(V)) == 0 and cnt.value == 32


def test_no_allocation_on_a_repeated_call(gpu):
    lib = gpu.lib()
    W = spectra(257)["random"][0]
    gpu.syevx(W, 1, 5)                                       # warm-up: the context grows here
    f0, f1, tot = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    assert lib.hipsdp_mem_info(0, C.byref(f0), C.byref(tot)) == 0
    for _ in range(20):
        gpu.syevx(W, 1, 5)
    assert lib.hipsdp_mem_info(0, C.byref(f1), C.byref(tot)) == 0
    assert f0.value == f1.value, (f0.value, f1.value)


def test_two_host_threads(gpu):
    """each host thread has its own context (stream, staging, pool): two threads at once reproduce their single-thread bits"""
    mats = [spectra(193)["random"][0], spectra(193)["low_rank_shifted"][0]]
    ref = [gpu.syevx(W, 1, 5) for W in mats]
    bad = []

    def work(t):
        for _ in range(20):
            lam, V = gpu.syevx(mats[t], 1, 5)
            if lam.tobytes() != ref[t][0].tobytes() or V.tobytes() != ref[t][1].tobytes():
                bad.append(t)

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not bad, bad
