"""sparsecuts_variants_ref.py - TEST INFRASTRUCTURE.  Numpy restatement of the loop of addMultipleSparseCuts (cons_sdp.c:1440-1589)
with its three switches recomputesparseev, recomputeinitial and exacttrans (:1460-1514, :1532-1550, :1552-1568) as the bit mask of
hipsdp_sparsecuts_all_ex; TPower and the margins of its decisions are those of sparsecuts_ref.py, variant 0 is its loop.

Besides those margins a run reports how well the eigenpairs it takes from a decomposition are defined - the relative gap between the
two smallest eigenvalues of every Z_S and of every deflated Z that supplied a start vector - and how far every lambda was from -tol.
stable() re-runs a case with every eigenvalue and eigenvector taken from a decomposition perturbed by 1e-9 of the matrix' norm (the
residual bound of the eigen contract in include/hipsdp.h): a case is stable when the cut count, every support and every run's
iteration number come out unchanged.  Only a stable case can be compared with another implementation count for count."""
import numpy as np
from sparsecuts_ref import tpower, Margins, MAXIT

SPARSEEV, INITIAL, EXACTTRANS = 1, 2, 4
PERTURB = 1e-9


class VariantMargins(Margins):
    def __init__(self):
        super().__init__()
        self.sub_gap = np.inf       # (lam_1 - lam_0) / max |lam| of a Z_S (size >= 2)
        self.defl_gap = np.inf      # the same of a deflated Z whose first eigenvector became a start vector
        self.tol = np.inf           # |lambda + tol|


def _eigh(W, rng):
    """eigenvalues ascending and eigenvectors (columns); with rng: each moved by PERTURB relative to the norm of W"""
    lam, V = np.linalg.eigh(W)
    if rng is not None:
        scale = max(float(np.max(np.abs(lam))), np.finfo(float).tiny)
        lam = lam + PERTURB * scale * rng.uniform(-1.0, 1.0, len(lam))
        V = V + PERTURB * rng.standard_normal(V.shape) / np.sqrt(len(lam))
        V = V / np.linalg.norm(V, axis=0)
    return lam, V


def _rel_gap(lam):
    return float(lam[1] - lam[0]) / max(float(np.max(np.abs(lam))), np.finfo(float).tiny) if len(lam) > 1 else np.inf


def sparse_cuts_matrix_ex(Z, v0, maxeig, size, tol, feastol, maxcuts, variant, convtol=1e-6, maxit=MAXIT, rng=None):
    """the loop on a given matrix, start vector and largest eigenvalue.  Returns (eigvals[k], vecs[k, n], supports [k arrays], iters,
    flags, VariantMargins, runs) - eigvals: the value the cut and the deflation used; flags bit 2: the loop ended at lambda >= -tol;
    runs: the iteration number of every TPower run."""
    n = Z.shape[0]
    Z = np.array(Z, dtype=np.float64)
    v0 = np.array(v0, dtype=np.float64)
    mg = VariantMargins()
    vals, vecs, sups, runs = [], [], [], []
    iters, flags = 0, 0
    start = v0
    while True:
        M = maxeig * np.eye(n) - Z
        x, sup, theta, it, fl = tpower(M, start, size, convtol, maxit, mg)
        iters += it
        runs.append(it)
        flags |= fl
        if fl & 2 or it == 0:
            break
        scalar = maxeig - theta
        mg.feas = min(mg.feas, abs(scalar + feastol))
        if not scalar < -feastol or len(vals) >= maxcuts:
            break
        value = scalar
        if variant & SPARSEEV:
            lam, W = _eigh(Z[np.ix_(sup, sup)], rng)
            mg.sub_gap = min(mg.sub_gap, _rel_gap(lam))
            mg.tol = min(mg.tol, abs(float(lam[0]) + tol))
            if lam[0] >= -tol:                       # :1487
                flags |= 4
                break
            w = W[:, 0] / np.linalg.norm(W[:, 0])
            x = np.zeros(n)
            x[sup] = w
            value = float(lam[0])
        vals.append(value)
        vecs.append(x)
        sups.append(sup)
        Z = Z - value * np.outer(x, x)
        if variant & (INITIAL | EXACTTRANS):
            lam, V = _eigh(Z, rng)
            if variant & INITIAL:
                mg.defl_gap = min(mg.defl_gap, _rel_gap(lam))
                start = V[:, 0]
        maxeig = float(lam[-1]) if variant & EXACTTRANS else maxeig - value
    return np.array(vals), np.array(vecs).reshape(len(vals), n), sups, iters, flags, mg, runs


def sparse_cuts_dense_ex(A, y, size, tol, feastol, maxcuts, variant, convtol=1e-6, maxit=MAXIT, rng=None):
    """A[m + 1, n, n] with A[0] the constant matrix.  Returns (ncuts, lmin, eigvals[k], coefs[k, m], lhs[k], vecs[k, n], supports,
    iters, flags, margins, runs) of block Z(y) = sum_i A[i] y_i - A[0]: the tuple of sparsecuts_ref.sparse_cuts_dense, and the runs"""
    m, n = A.shape[0] - 1, A.shape[1]
    Z = np.tensordot(y, A[1:], axes=(0, 0)) - A[0] if m > 0 else -A[0]
    lam, V = _eigh(Z, rng)
    lmin = float(lam[0])
    if not lmin < -tol or size > n or maxcuts == 0:
        return 0, lmin, np.zeros(0), np.zeros((0, m)), np.zeros(0), np.zeros((0, n)), [], 0, 0, VariantMargins(), []
    vals, vecs, sups, iters, flags, mg, runs = sparse_cuts_matrix_ex(Z, V[:, 0], float(lam[-1]), size, tol, feastol, maxcuts, variant,
                                                                     convtol, maxit, rng)
    coefs = np.array([[float(v @ A[1 + i] @ v) for i in range(m)] for v in vecs]).reshape(len(vals), m)
    lhs = np.array([float(v @ A[0] @ v) for v in vecs])
    return len(vals), lmin, vals, coefs, lhs, vecs, sups, iters, flags, mg, runs


def stable(A, y, size, tol, feastol, maxcuts, variant, base=None, convtol=1e-6, maxit=MAXIT, reruns=3, seed=1):
    """True when three perturbed re-runs of the case give the cut count, the supports and the iteration number of every run that the
    unperturbed run (base, computed here when None) gives"""
    if base is None:
        base = sparse_cuts_dense_ex(A, y, size, tol, feastol, maxcuts, variant, convtol, maxit)
    for k in range(reruns):
        r = sparse_cuts_dense_ex(A, y, size, tol, feastol, maxcuts, variant, convtol, maxit, rng=np.random.default_rng(seed + k))
        if r[0] != base[0] or r[10] != base[10] or r[8] != base[8]:
            return False
        if any(list(a) != list(b) for a, b in zip(r[6], base[6])):
            return False
    return True
