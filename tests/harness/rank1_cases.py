"""Rank-1 constraints on the host, for the tests of hipsdp_rank1_check_many (tests/test_rank1_cpu.py, tests/test_gpu_rank1.py): numpy
restatements of the two scans over the principal 2 x 2 minors (cons_sdp.c:788-806 and :3756-3780) and of the right-hand side of the
rank-1 approximation heuristic (:8058-8092), matrix families with a planted answer, solvers whose Z(y) is exactly rank one, and the
rank-1 part of CONSCHECK written once over the call's outputs and once point by point in numpy."""
import numpy as np
from check_y_cases import load, zmat, family  # noqa: F401 - re-exported for the tests

NONE = (-1, -1)


def pairs(n):
    """the pairs (i, k), k < i, in the reference's order: i ascending, then k ascending"""
    return np.tril_indices(n, -1)


def minor_ev(a, b, c):
    """smaller eigenvalue of [[a, b], [b, c]] by the header's closed form, every operation rounded on its own"""
    h, g = 0.5 * (a + c), 0.5 * (a - c)
    return h - np.sqrt(g * g + b * b)


def scan_ev(Z):
    """(minorev, (i, k)): the largest smaller eigenvalue that is > 0 and the FIRST pair that has it; 0.0 and (-1, -1) without one"""
    n = Z.shape[0]
    i, k = pairs(n)
    if len(i) == 0:
        return 0.0, NONE
    ev = minor_ev(Z[i, i], Z[i, k], Z[k, k])
    ev = np.where(np.isnan(ev), -np.inf, ev)
    p = int(np.argmax(ev))                           # (the first of equal values)
    if not ev[p] > 0.0:
        return 0.0, NONE
    return float(ev[p]), (int(i[p]), int(k[p]))


def minors(Z):
    n = Z.shape[0]
    i, k = pairs(n)
    return Z[i, i] * Z[k, k] - Z[i, k] * Z[i, k]     # (numpy rounds both products, then the difference)


def scan_det(Z, feastol):
    """(minordet, (i, k)): the largest |minor| and the FIRST pair with minor < -feastol or minor > feastol, else (-1, -1)"""
    n = Z.shape[0]
    i, k = pairs(n)
    if len(i) == 0:
        return 0.0, NONE
    mn = minors(Z)
    bad = np.nonzero((mn < -feastol) | (mn > feastol))[0]
    return float(np.max(np.abs(mn))), (NONE if len(bad) == 0 else (int(i[bad[0]]), int(k[bad[0]])))


def ev_reference(Z):
    """numpy.linalg.eigvalsh of every 2 x 2 minor: the smaller eigenvalues in the reference's order"""
    n = Z.shape[0]
    i, k = pairs(n)
    M = np.empty((len(i), 2, 2))
    M[:, 0, 0], M[:, 0, 1], M[:, 1, 0], M[:, 1, 1] = Z[i, i], Z[i, k], Z[i, k], Z[k, k]
    return np.linalg.eigvalsh(M)[:, 0], i, k


def rhs(A0, lam, v):
    """packed lower triangle, row order: rhs[i (i + 1) / 2 + k] = A_0[i][k] + (lam v_i) v_k, every operation rounded"""
    n = len(v)
    i, k = np.tril_indices(n)
    return A0[i, k] + (lam * v[i]) * v[k]


# ---- matrix families ------------------------------------------------------------------------------------------------------------------------

def planted_pair(n, p, q, seed=0):
    """Z_pp = Z_qq = 10, the other diagonal entries in [0.5, 1.2], |off-diagonal| <= 0.1: the smaller eigenvalue of a minor cannot exceed
    its smaller diagonal entry, so (max(p, q), min(p, q)) is the unique maximum by a margin of more than 8"""
    rng = np.random.default_rng([seed, n, p, q])
    R = rng.uniform(-0.1, 0.1, (n, n))
    Z = np.tril(R, -1) + np.tril(R, -1).T + np.diag(rng.uniform(0.5, 1.2, n))
    Z[p, p] = Z[q, q] = 10.0
    return Z, (max(p, q), min(p, q))


def constant(n):
    """diagonal 2, off-diagonal 1: every minor has the same bits, the first pair (1, 0) wins"""
    return np.ones((n, n)) + np.eye(n)


def negative_definite(n, seed=0):
    rng = np.random.default_rng([seed, n])
    R = rng.uniform(-0.1, 0.1, (n, n))
    return np.tril(R, -1) + np.tril(R, -1).T - np.diag(rng.uniform(1.0, 2.0, n))


def rank_one_blocks(ns, m, count, seed=0):
    """A_i = c_i u u^T with u in {+-1}^n and integer c_i, A_0 = 0, points with sum_i c_i y_i > 0: every entry of Z(y) is +- the same sum
    (the points are multiples of 1 / 8, so that sum is exact in every order of the additions)"""
    rng = np.random.default_rng([seed, m, len(ns), count])
    blocks = []
    cs = []
    for n in ns:
        u = rng.choice([-1.0, 1.0], n)
        c = rng.integers(1, 5, m).astype(np.float64)
        A = np.zeros((m + 1, n, n))
        for i in range(m):
            A[i + 1] = c[i] * np.outer(u, u)
        blocks.append(A)
        cs.append(c)
    Y = rng.integers(2, 13, (count, m)) / 8.0          # (multiples of 1 / 8: every product and every partial sum is exact)
    return blocks, Y, cs


def planted_top(ns, m, seed=0):
    """blocks [m + 1, n, n] and ONE point y with Z_b(y) = s u u^T + E, u a unit vector, ||E||_2 <= s / 10: variable 1 carries u u^T, the
    others and A_0 random symmetric matrices; y_1 = s is set from the norm of the rest, the largest over the blocks.  By Weyl's
    inequalities the gap above eigenvalue n - 1 is at least 0.8 s"""
    rng = np.random.default_rng([seed, m, len(ns)])
    y = rng.uniform(-1.0, 1.0, m)
    blocks, norms = [], []
    for n in ns:
        A = np.zeros((m + 1, n, n))
        u = rng.standard_normal(n)
        A[1] = np.outer(u, u) / (u @ u)
        for i in [0] + list(range(2, m + 1)):
            R = rng.standard_normal((n, n))
            A[i] = (R + R.T) / (2.0 * np.sqrt(n))
        E = (np.tensordot(y[1:], A[2:], axes=(0, 0)) if m > 1 else 0.0) - A[0]
        norms.append(float(np.linalg.norm(E, 2)))
        blocks.append(A)
    y[0] = 10.5 * max(norms)
    return blocks, y


# ---- the rank-1 part of CONSCHECK -----------------------------------------------------------------------------------------------------------

def feas_eq0(x, feastol):
    """SCIPisFeasEQ(x, 0.0): relative difference within feastol, which against 0 is |x| <= feastol"""
    return abs(x) <= feastol


def conscheck_from_call(lam, minorev, minorind, feastol):
    """isMatrixRankOne (cons_sdp.c:733-823) over the outputs of hipsdp_rank1_check_many: per (point, block) the verdict isrankone, the
    violation (largestminev) and maxevsubmat - (-1, -1) where the reference does not scan"""
    count, nb = lam.shape[:2]
    rank1 = np.zeros((count, nb), dtype=bool)
    viol = np.zeros((count, nb))
    sub = np.full((count, nb, 2), -1, dtype=np.int64)
    for j in range(count):
        for b in range(nb):
            rank1[j, b] = feas_eq0(lam[j, b, 1], feastol)
            if not rank1[j, b]:
                viol[j, b] = minorev[j, b]
                sub[j, b] = minorind[j, b]
    return rank1, viol, sub


def conscheck_numpy(blocks, Y, feastol):
    """the same loop point by point in numpy: eigvalsh for eigenvalue n - 1, the restated scan for the minors"""
    count, nb = len(Y), len(blocks)
    rank1 = np.zeros((count, nb), dtype=bool)
    viol = np.zeros((count, nb))
    sub = np.full((count, nb, 2), -1, dtype=np.int64)
    for j, y in enumerate(Y):
        for b, A in enumerate(blocks):
            Z = zmat(A, y)
            n = Z.shape[0]
            w = np.linalg.eigvalsh(Z)
            second = 0.0 if n == 1 else (w[0] if n == 2 else w[n - 2])
            rank1[j, b] = feas_eq0(second, feastol)
            if not rank1[j, b]:
                viol[j, b], sub[j, b] = scan_ev(Z)
    return rank1, viol, sub
