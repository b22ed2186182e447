"""Symmetric test matrices with known spectra and the accuracy checks of returned eigenpairs, shared by tests/test_gpu_syevx.py
(selected pairs) and tests/test_gpu_syevr.py (all pairs).

Reference: numpy.linalg.eigvalsh, scale = max(1, max|ev|).  Tolerances (those of test_gpu_units.py for the one-launch kernels):
|lam - ev| <= 1e-12 scale and ascending, | ||v|| - 1 | <= 1e-12, residual <= 1e-9 scale, |V V^T - I| <= 1e-11.  numpy.linalg.eigh itself
meets them on every matrix below."""
import numpy as np

_CACHE = {}
SEVEN = ("low_rank_shifted", "rank_one", "two_clusters", "identity", "random", "close_pairs", "graded")


def spectra(n, decoupled=False):
    """name -> (W, eigenvalues, scale), computed once, shared, read-only: the spectra of test_block_jacobi_on_clustered_spectra plus
    graded / close_pairs of test_mid_full_decomposition_in_one_launch (SEVEN); with decoupled=True and above 50 rows also two
    decoupled blocks that share an eigenvalue and a cluster of 40 eigenvalues 1e-10 apart"""
    if n not in _CACHE:
        rng = np.random.default_rng(300 + n)
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        cases = {"low_rank_shifted": (lambda B: B @ B.T - 0.01 * np.eye(n))(rng.standard_normal((n, n // 10))),
                 "rank_one": (lambda b: np.outer(b, b))(rng.standard_normal(n)),
                 "two_clusters": (Q * np.where(np.arange(n) < n // 2, -1.0, 2.0)) @ Q.T,
                 "identity": 3.5 * np.eye(n),
                 "random": (lambda G: G + G.T)(rng.standard_normal((n, n))),
                 "close_pairs": (Q * np.repeat(np.arange(1, n // 2 + 2, dtype=float), 2)[:n] * (1 + 1e-9 * np.arange(n))) @ Q.T,
                 "graded": (Q * 10.0 ** np.linspace(-6, 6, n)) @ Q.T}
        if n > 50:
            # (the dense sizes) two decoupled random blocks of 50 and n - 50 rows; the second one is built around an eigenvalue of the first
            G1 = rng.standard_normal((50, 50))
            B1 = 0.5 * (G1 + G1.T)
            mu = np.linalg.eigvalsh(B1)[20]
            Q2, _ = np.linalg.qr(rng.standard_normal((n - 50, n - 50)))
            ev2 = 3.0 * rng.standard_normal(n - 50)
            ev2[0] = mu
            B2 = (Q2 * ev2) @ Q2.T
            BD = np.zeros((n, n))
            BD[:50, :50] = B1
            BD[50:, 50:] = 0.5 * (B2 + B2.T)
            cases["block_diagonal"] = BD
            tc = 3.0 * rng.standard_normal(n)
            tc[:40] = 1.0 + 1e-10 * np.arange(40)
            cases["tight_cluster"] = (Q * tc) @ Q.T
        out = {}
        for name, W in cases.items():
            W = np.ascontiguousarray(0.5 * (W + W.T))
            ev = np.linalg.eigvalsh(W)
            W.setflags(write=False); ev.setflags(write=False)
            out[name] = (W, ev, max(1.0, np.abs(ev).max()))
        _CACHE[n] = out
    return {k: v for k, v in _CACHE[n].items() if decoupled or k in SEVEN}


def check_pairs(name, W, ev, scale, first, lam, V):
    """accuracy of returned pairs first .. first + len(lam) - 1 (1-based)"""
    k = len(lam)
    n = W.shape[0]
    err = np.abs(lam - ev[first - 1:first - 1 + k]).max()
    print("%s n=%d pairs %d..%d: |lam - ev| %.2e (scale %.2e)" % (name, n, first, first + k - 1, err, scale), end="")
    assert err <= 1e-12 * scale, (name, first, err)
    assert np.all(np.diff(lam) >= 0.0), (name, first)
    if V is not None:
        nrm = np.abs(np.linalg.norm(V, axis=1) - 1.0).max()
        res = np.linalg.norm(W @ V.T - V.T * lam, axis=0).max()
        orth = np.abs(V @ V.T - np.eye(k)).max()
        print(", |norm - 1| %.2e, residual %.2e, |VV^T - I| %.2e" % (nrm, res, orth), end="")
        assert nrm <= 1e-12, (name, first, nrm)
        assert res <= 1e-9 * scale, (name, first, res)
        assert orth <= 1e-11, (name, first, orth)
    print()


def check_all_pairs(name, W, ev, scale, lam, V):
    """the four checks of check_pairs on all n pairs, |V V^T - I| over the whole n x n product; every figure is printed before it is
    asserted; returns the list of what failed"""
    n = W.shape[0]
    err = np.abs(lam - ev).max()
    nrm = np.abs(np.linalg.norm(V, axis=1) - 1.0).max()
    res = np.linalg.norm(W @ V.T - V.T * lam, axis=0).max()
    orth = np.abs(V @ V.T - np.eye(n)).max()
    print("%s n=%d: |lam - ev| %.2e (scale %.2e), |norm - 1| %.2e, residual %.2e, |VV^T - I| %.2e" % (name, n, err, scale, nrm, res, orth))
    bad = []
    if not err <= 1e-12 * scale:
        bad.append(("eigenvalues", err))
    if not np.all(np.diff(lam) >= 0.0):
        bad.append(("not ascending", float(np.diff(lam).min())))
    if not nrm <= 1e-12:
        bad.append(("norm", nrm))
    if not res <= 1e-9 * scale:
        bad.append(("residual", res))
    if not orth <= 1e-11:
        bad.append(("orthogonality", orth))
    return [(name, n) + b for b in bad]
