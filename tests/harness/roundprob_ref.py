"""roundprob_ref.py - TEST INFRASTRUCTURE.  A numpy restatement of the device work of the reference's primal rounding problem
(solvePrimalRoundingProblem, relax_sdp.c:1551-2640), loop for loop and in the reference's index conventions, so that
hipsdp_rounding_frame / hipsdp_rounding_recombine can be compared with what the host code computes:

    decompose      :1875-1877  SCIPlapackComputeEigenvectorDecomposition of the expanded X_b: eigenvalues ascending, row j of V = v_j
    coefficients   :1906-1923  obj[j]    = sum over the lower-triangular nonzeros (r, c, a) of A_0:  a v_j[r] v_j[c], doubled off the diagonal
                   :1926-1947  val[j][i] = the same over A_i  (val[evind * nvars + varind])
    recombine      :2164-2207 (X) and :2550-2591 (Z): scaleTransposedMatrix(V, lambda) followed by
                   SCIPlapackMatrixMatrixMult(V, TRUE, S, FALSE): R[i][j] = sum_c V[i][c] lambda_c V[j][c]  (mode 0, the literal chain)
                   mode 1: the spectral form R = sum_k lambda_k v_k v_k^T

Matrices are dense [m + 1, n, n] arrays with row 0 the constant matrix.  `dtype` picks the arithmetic (np.longdouble for references)."""
import numpy as np


def expand(n, row, col, val):
    """expandSparseMatrix (relax_sdp.c:243-277): both triangles are filled"""
    M = np.zeros((n, n))
    for r, c, v in zip(row, col, val):
        M[r, c] = v
        M[c, r] = v
    return M


def decompose(X):
    """eigenvalues ascending, row j of V = j-th eigenvector"""
    lam, U = np.linalg.eigh(np.asarray(X, dtype=np.float64))
    return lam, U.T.copy()


def coefficients(V, A, dtype=np.float64):
    """table[j, i] = v_j^T A_i v_j by the reference's loop over the lower-triangular nonzeros of A_i, an off-diagonal one counted twice;
    column 0 is obj, the columns 1 .. m are val"""
    V = np.asarray(V, dtype=dtype)
    n = V.shape[0]
    m1 = A.shape[0]
    out = np.zeros((n, m1), dtype=dtype)
    for i in range(m1):
        r, c = np.nonzero(np.tril(A[i]))
        a = np.asarray(A[i][r, c], dtype=dtype) * np.where(r == c, 1, 2).astype(dtype)
        for j in range(n):
            out[j, i] = np.sum(a * V[j, r] * V[j, c])
    return out


def coefficients_einsum(V, A, dtype=np.longdouble):
    """the same table as one contraction over the full symmetric matrices"""
    V = np.asarray(V, dtype=dtype)
    return np.einsum("jr,irc,jc->ji", V, np.asarray(A, dtype=dtype), V)


def coefficient_bound(V, A, entries):
    """(L + 4) 2^-53 sum_p |w_p A_p v_r v_c| per (j, i): the first-order rounding bound of a sum of L = `entries` products of three rounded
    factors, whatever the order of the sum"""
    Va = np.abs(np.asarray(V, dtype=np.longdouble))
    mag = np.einsum("jr,irc,jc->ji", Va, np.abs(np.asarray(A, dtype=np.longdouble)), Va)
    return np.asarray((entries + 4) * 2.0 ** -53 * mag, dtype=np.float64)


def recombine(V, lam, mode, dtype=np.float64):
    """mode 0: R[i][j] = sum_c V[i][c] lam_c V[j][c]; mode 1: R = sum_k lam_k v_k v_k^T"""
    V = np.asarray(V, dtype=dtype)
    lam = np.asarray(lam, dtype=dtype)
    if mode == 0:
        return (V * lam[None, :]) @ V.T
    return V.T @ (lam[:, None] * V)


def recombine_bound(V, lam, mode):
    """(n + 4) 2^-53 sum_k |lam_k v_k[i] v_k[j]| (mode 1; mode 0 with the roles of the two indices of V exchanged)"""
    Va = np.abs(np.asarray(V, dtype=np.longdouble))
    la = np.abs(np.asarray(lam, dtype=np.longdouble))
    n = Va.shape[0]
    mag = (Va * la[None, :]) @ Va.T if mode == 0 else Va.T @ (la[:, None] * Va)
    return np.asarray((n + 4) * 2.0 ** -53 * mag, dtype=np.float64)


def kept(R, epsilon):
    """the entries with row <= col and |value| > epsilon in row-major order: (row, col, val)"""
    n = R.shape[0]
    r, c = np.triu_indices(n)
    v = R[r, c]
    keep = np.abs(v) > epsilon
    return r[keep].astype(np.int32), c[keep].astype(np.int32), v[keep]
