"""Symmetric test matrices with known spectra and the accuracy checks of returned eigenpairs, shared by tests/test_gpu_syevx.py
(selected pairs), tests/test_gpu_syevr.py (all pairs) and tests/test_gpu_eig_structured.py (structured and scaled inputs).

Reference: numpy.linalg.eigvalsh, scale = max(1, max|ev|).  Tolerances (those of test_gpu_units.py for the one-launch kernels):
|lam - ev| <= 1e-12 scale and ascending, | ||v|| - 1 | <= 1e-12, residual <= 1e-9 scale, |V V^T - I| <= 1e-11.  numpy.linalg.eigh itself
meets them on every matrix below.

structured(n) and scaled(case, k) carry scale = max|ev| WITHOUT the floor at 1: handed to the same checks, all four bounds are
relative to the matrix (tests/test_eig_cases_cpu.py shows that the reference itself meets them at 2^-100 .. 2^100)."""
import numpy as np

_CACHE = {}
_SCACHE = {}
_TCACHE = {}
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


def check_pairs(name, W, ev, scale, first, lam, V, bad=None):
    """accuracy of returned pairs first .. first + len(lam) - 1 (1-based); every figure is printed before it is checked.  bad = None:
    asserts; bad = a list: what failed is appended to it instead, for one assertion at the end of a test"""
    k = len(lam)
    n = W.shape[0]
    fails = []
    err = np.abs(lam - ev[first - 1:first - 1 + k]).max()
    print("%s n=%d pairs %d..%d: |lam - ev| %.2e (scale %.2e)" % (name, n, first, first + k - 1, err, scale), end="")
    if not err <= 1e-12 * scale:
        fails.append((name, n, first, "eigenvalues", err))
    if not np.all(np.diff(lam) >= 0.0):
        fails.append((name, n, first, "not ascending"))
    if V is not None:
        nrm = np.abs(np.linalg.norm(V, axis=1) - 1.0).max()
        res = np.linalg.norm(W @ V.T - V.T * lam, axis=0).max()
        orth = np.abs(V @ V.T - np.eye(k)).max()
        print(", |norm - 1| %.2e, residual %.2e, |VV^T - I| %.2e" % (nrm, res, orth), end="")
        if not nrm <= 1e-12:
            fails.append((name, n, first, "norm", nrm))
        if not res <= 1e-9 * scale:
            fails.append((name, n, first, "residual", res))
        if not orth <= 1e-11:
            fails.append((name, n, first, "orthogonality", orth))
    print()
    if bad is None:
        assert not fails, fails
    else:
        bad += fails


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


def _adjacency(n, rng):
    """0/1 adjacency of density 0.1, hollow; the edge (0, 1) is always there so that no size gives the empty graph (whose Laplacian
    would be a second zero matrix)"""
    U = np.triu((rng.random((n, n)) < 0.1).astype(float), 1)
    U[0, 1] = 1.0
    return U + U.T


def structured(n):
    """name -> (W, eigenvalues, scale = max|ev|, no floor), computed once, shared, read-only; n >= 2.  Every entry is a small integer:
    the matrices carry no rounding, have exact multiplicities, hollow diagonals and couplings that vanish exactly or at rounding
    level during the tridiagonalisation - adjacency / Laplacian / Diag(y) - W shaped blocks.  Reference: the analytic spectrum for
    cycle, complete, ones and tridiag_dense, numpy.linalg.eigvalsh for the rest."""
    if n not in _SCACHE:
        rng = np.random.default_rng(7100 + n)
        idx = np.arange(n)
        J = np.ones((n, n))
        cyc = np.zeros((n, n))
        cyc[idx, (idx + 1) % n] = 1.0
        cyc[(idx + 1) % n, idx] = 1.0                     # (n = 2: the single edge, not a double one)
        cyc_ev = np.array([-1.0, 1.0]) if n == 2 else np.sort(2.0 * np.cos(2.0 * np.pi * idx / n))
        b = max(2, n // 8)
        k = n // b
        B = np.triu(rng.integers(-3, 4, (b, b)).astype(float))
        B = B + np.triu(B, 1).T
        K = np.zeros((n, n))
        K[:k * b, :k * b] = np.kron(np.eye(k), B)
        perm = rng.permutation(n)
        K = K[np.ix_(perm, perm)]
        arrow = np.diag(np.arange(1.0, n + 1.0))
        arrow[0, 1:] = arrow[1:, 0] = 1.0
        tri = 2.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)
        adj = _adjacency(n, rng)
        cases = {"cycle": (cyc, cyc_ev),
                 "complete": (J - np.eye(n), np.array([-1.0] * (n - 1) + [n - 1.0])),
                 "ones": (J, np.array([0.0] * (n - 1) + [float(n)])),
                 "kron_perm": (K, None),
                 "arrow": (arrow, None),
                 "tridiag_dense": (tri, 2.0 - 2.0 * np.cos(np.arange(1, n + 1) * np.pi / (n + 1))),
                 "laplacian": (np.diag(adj.sum(axis=1)) - adj, None),
                 "diag_minus_adj": (np.diag(rng.integers(0, 3, n).astype(float)) - adj, None),
                 "zero": (np.zeros((n, n)), np.zeros(n))}
        out = {}
        for name, (W, ev) in cases.items():
            W = np.ascontiguousarray(W)
            assert np.array_equal(W, W.T) and np.array_equal(W, np.round(W))
            if ev is None:
                ev = np.linalg.eigvalsh(W)
            W.setflags(write=False); ev.setflags(write=False)
            out[name] = (W, ev, float(np.abs(ev).max()))
        _SCACHE[n] = out
    return _SCACHE[n]


ANALYTIC = ("cycle", "complete", "ones", "tridiag_dense")


def scaled(case, k):
    """(W, ev, scale) times 2^k: the products are exact in binary floating point"""
    W, ev, scale = case
    f = 2.0 ** k
    Wk, evk = W * f, ev * f
    Wk.setflags(write=False); evk.setflags(write=False)
    return Wk, evk, scale * f


def tridiagonals(n):
    """name -> (d, e, T, eigenvalues of T, scale = max(1, max|ev|)); n >= 2"""
    if n not in _TCACHE:
        i = np.arange(n, dtype=float)
        m1 = n // 2
        m2 = n - m1
        glued_d = np.concatenate([np.abs(np.arange(m1) - m1 // 2), np.abs(np.arange(m2) - m2 // 2)]).astype(float)
        glued_e = np.ones(n - 1)
        glued_e[m1 - 1] = 1e-14
        cut = np.full(n - 1, 0.5)
        cut[6::7] = 0.0
        gd = 10.0 ** np.linspace(-6, 6, n)
        cases = {"toeplitz_121": (np.full(n, 2.0), np.ones(n - 1)),
                 "wilkinson": (np.abs(i - n // 2), np.ones(n - 1)),
                 "wilkinson_glued": (glued_d, glued_e),
                 "diagonal_repeated": (np.mod(i, 5.0) - 1.0, np.zeros(n - 1)),
                 "ones_cut_every_7th": (np.ones(n), cut),
                 "graded": (gd, 1e-3 * np.sqrt(gd[:-1] * gd[1:]))}
        out = {}
        for name, (d, e) in cases.items():
            T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
            ev = np.linalg.eigvalsh(T)
            for a in (d, e, T, ev):
                a.setflags(write=False)
            out[name] = (d, e, T, ev, max(1.0, np.abs(ev).max()))
        _TCACHE[n] = out
    return _TCACHE[n]


def check_zero(name, lam, V, bad):
    """the zero matrix: eigenvalues finite and far below anything a caller can tell from zero or turn into a cut, the vectors any
    orthonormal set; figures printed, failures appended to bad"""
    k = len(lam)
    fin = bool(np.all(np.isfinite(lam)))
    big = float(np.abs(lam).max()) if fin else float("inf")
    print("%s n=%s, %d pairs: max|lam| %.2e" % (name, "?" if V is None else V.shape[1], k, big), end="")
    if not (fin and big < 1e-200):
        bad.append((name, "eigenvalues of the zero matrix", big))
    if V is not None:
        vfin = bool(np.all(np.isfinite(V)))
        orth = float(np.abs(V @ V.T - np.eye(k)).max()) if vfin else float("inf")
        print(", |VV^T - I| %.2e" % orth, end="")
        if not (vfin and orth <= 1e-11):
            bad.append((name, "vectors of the zero matrix", orth))
    print()
