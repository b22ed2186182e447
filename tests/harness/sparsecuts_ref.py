"""sparsecuts_ref.py - TEST INFRASTRUCTURE.  Numpy restatement of the reference's separation mode `multiplesparsecuts` in its
default configuration (recomputesparseev, recomputeinitial, exacttrans FALSE): cons_sdp.c:1140-1234 (truncatedPowerMethod) and
:1340-1607 (addMultipleSparseCuts), with the coefficients of :826-952 (lhs = x^T A_0 x, coefficients x^T A_j x).

M = maxeig I - Z is formed explicitly, as the reference does.  The reference sorts |w| with an unstable sort; here the order is a
stable descending argsort - of two equal absolute values the smaller index is kept, which is the project's rule.  Every run also
reports how far its decisions were from flipping (the margins): a test that compares counts and supports asserts them first."""
import numpy as np

MAXIT = 10000            # HIPSDP_SPARSECUTS_MAXIT


class Margins:
    """smallest distances of the data-dependent decisions of a run from their thresholds"""

    def __init__(self):
        self.select = np.inf     # relative gap between the size-th and the next |w| (size < n only)
        self.conv = np.inf       # |(new - old) - convtol|
        self.feas = np.inf       # |scalar + feastol|
        self.longest = 0         # iterations of the longest single TPower run


def tpower(M, v0, size, convtol=1e-6, maxit=MAXIT, margins=None):
    """cons_sdp.c:1140-1234 with a cap on the iterations.  Returns (x, support (ascending indices), value, iterations, flags):
    flags bit 0 - stopped at maxit, bit 1 - a truncated iterate had norm 0 (x is then the zero vector)."""
    n = len(v0)
    x = np.array(v0, dtype=np.float64)
    new, old = -1.0, -2.0
    it, flags = 0, 0
    support = np.arange(n)
    while new - old > convtol and it < maxit:
        old = new
        w = M @ x
        aw = np.abs(w)
        order = np.argsort(-aw, kind="stable")
        if margins is not None and size < n:
            big, nxt = aw[order[size - 1]], aw[order[size]]
            margins.select = min(margins.select, (big - nxt) / big if big > 0.0 else 0.0)
        support = np.sort(order[:size])
        t = np.zeros(n)
        t[support] = w[support]
        nrm = np.sqrt(float(t @ t))
        if nrm == 0.0:
            return np.zeros(n), support, new, it, flags | 2
        x = t / nrm
        new = float(x @ (M @ x))
        it += 1
        if margins is not None:
            margins.conv = min(margins.conv, abs((new - old) - convtol))
    if it >= maxit and new - old > convtol:
        flags |= 1
    if margins is not None:
        margins.longest = max(margins.longest, it)
    return x, support, new, it, flags


def sparse_cuts_matrix(Z, v0, maxeig, size, feastol, maxcuts, convtol=1e-6, maxit=MAXIT):
    """the loop of cons_sdp.c:1440-1589 on a given matrix, start vector and largest eigenvalue.  Returns (eigvals[k], vecs[k, n],
    supports [k arrays], iters, flags, Margins)."""
    n = Z.shape[0]
    Z = np.array(Z, dtype=np.float64)
    mg = Margins()
    vals, vecs, sups = [], [], []
    iters, flags = 0, 0
    while True:
        M = maxeig * np.eye(n) - Z
        x, sup, theta, it, fl = tpower(M, v0, size, convtol, maxit, mg)
        iters += it
        flags |= fl
        if fl & 2 or it == 0:
            break
        scalar = maxeig - theta
        mg.feas = min(mg.feas, abs(scalar + feastol))
        if not scalar < -feastol or len(vals) >= maxcuts:
            break
        vals.append(scalar)
        vecs.append(x)
        sups.append(sup)
        Z = Z - scalar * np.outer(x, x)
        maxeig = maxeig - scalar
    return np.array(vals), np.array(vecs).reshape(len(vals), n), sups, iters, flags, mg


def sparse_cuts_dense(A, y, size, tol, feastol, maxcuts, convtol=1e-6, maxit=MAXIT):
    """A[m + 1, n, n] with A[0] the constant matrix.  Returns (ncuts, lmin, eigvals[k], coefs[k, m], lhs[k], vecs[k, n], supports,
    iters, flags, Margins) of block Z(y) = sum_i A[i] y_i - A[0]; cut: coefs @ y >= lhs."""
    m, n = A.shape[0] - 1, A.shape[1]
    Z = np.tensordot(y, A[1:], axes=(0, 0)) - A[0] if m > 0 else -A[0]
    lam, V = np.linalg.eigh(Z)
    lmin = float(lam[0])
    if not lmin < -tol or size > n or maxcuts == 0:
        return 0, lmin, np.zeros(0), np.zeros((0, m)), np.zeros(0), np.zeros((0, n)), [], 0, 0, Margins()
    vals, vecs, sups, iters, flags, mg = sparse_cuts_matrix(Z, V[:, 0], float(lam[-1]), size, feastol, maxcuts, convtol, maxit)
    coefs = np.array([[float(v @ A[1 + i] @ v) for i in range(m)] for v in vecs]).reshape(len(vals), m)
    lhs = np.array([float(v @ A[0] @ v) for v in vecs])
    return len(vals), lmin, vals, coefs, lhs, vecs, sups, iters, flags, mg
