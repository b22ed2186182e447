"""Seeded input families, the oracle's semidefinite pivot loop with its pivots laid open, and the error figures of
tests/test_gpu_chol.py (Cholesky kernels of scip-sdp_amd/csrc/chol.hip against LAPACK and ipm_ref.chol_psd).
tests/test_chol_cases_cpu.py holds LAPACK and the oracle alone to everything the GPU tests assume of them.

Every matrix is computed once, shared and read-only.  Products that measure an error are formed in numpy.longdouble (64-bit mantissa
on x86): a residual of the order n eps |L||L^T| formed in double would carry a rounding error of its own size.

Figures go through check(): printed before they are judged, the worst of every group kept in LEVELS (tests/devtools/chol_levels.py
writes that table down), a miss appended to the caller's list for one assertion at the end of a test."""
import hashlib
import numpy as np
import scipy.linalg as sla

EPS = float(np.finfo(np.float64).eps)           # 2^-52, the eps of 1.78e-15 = 8 eps in the pivot rule
XD = np.longdouble
REGTOL = 1e-13                                   # forcing threshold of the pivot rule, relative to M_kk
NOISE = 1.78e-15                                 # zeroing threshold (rule 3), times (k + 1) M_kk

SINGLE = (1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)                    # panel edges of the single-block kernel
BLOCKED = (65, 80, 81, 96, 97, 128, 129, 150, 200, 321)                        # last blocks of 1, 16, 17, 32, 33, 64, 1, 22, 8, 1 rows
PSD_SIZES = (3, 9, 16, 17, 33, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 200, 260)
CONDS = (1e2, 1e8, 1e12)
FAIL_SIZES = (130, 200)
FAIL_AT = (0, 15, 16, 63, 64, 65, 79, 80, 127, 128, -1)                        # -1: the last pivot
SMALL_FAIL_AT = (0, 15, 16, 31, 47, 48, -1)
SEQ_SIZES = (1, 2, 17, 63, 64, 65, 127, 128, 129, 192, 200, 321)               # up to 128: one workgroup; above: chains of workgroups

_CACHE = {}


def _keep(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def graded(n, cond, seed=0, rowscale=False):
    """Q diag(10^(-log10(cond) i / (n - 1))) Q^T, symmetrised; rowscale: rows and columns times 2^k, k uniform in -10 .. 10 (exact)"""
    def make():
        rng = np.random.default_rng([seed, n, int(round(np.log10(cond))), int(rowscale)])
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = 10.0 ** (-np.log10(cond) * np.arange(n) / max(n - 1, 1))
        S = (Q * lam) @ Q.T
        S = 0.5 * (S + S.T)
        if rowscale:
            s = 2.0 ** rng.integers(-10, 11, n)
            S = S * s[:, None] * s[None, :]
        return np.ascontiguousarray(S)
    return _keep(("graded", n, cond, seed, rowscale), make)


def graded_all(n, seed=0):
    """[(name, S)]: the three conditions, each without and with the row scaling"""
    return [("graded n=%d cond=%.0e%s" % (n, c, " rowscale" if rs else ""), graded(n, c, seed, rs)) for c in CONDS for rs in (False, True)]


def indefinite_at(S, k):
    """a copy of S with S[k, k] = l.l - 1, l = row k of the factor of the leading k x k block: pivot k is -1 up to rounding and the
    pivots before it are those of S"""
    T = np.array(S, dtype=np.float64, copy=True)
    if k == 0:
        T[0, 0] = -1.0
        return T
    Lk = np.linalg.cholesky(T[:k, :k])
    l = sla.solve_triangular(Lk, T[k, :k], lower=True, check_finite=False)
    T[k, k] = l @ l - 1.0
    return T


KEPT_SIZES = (33, 64, 130)
KEPT_AT = (1, 5, 15, 16, 31)


def forced_kept_at(S, k):
    """a copy of S whose pivot k is c S_kk with c = sqrt(1e-13 * 1.78e-15 (k + 1)), the geometric mean of the two thresholds of the
    rule: the pivot is forced and its column KEPT.  k + 1 < 56 keeps the two thresholds apart; the pivot sits a factor
    sqrt(56 / (k + 1)) >= 1.3 from either, and - unlike a pivot that is the noise of an elimination - it is made by one subtraction
    from a well-conditioned leading block, good to a few eps S_kk, a hundredth of c: every implementation decides it alike"""
    T = np.array(S, dtype=np.float64, copy=True)
    Lk = np.linalg.cholesky(T[:k, :k])
    l = sla.solve_triangular(Lk, T[k, :k], lower=True, check_finite=False)
    c = np.sqrt(REGTOL * NOISE * (k + 1))
    T[k, k] = (l @ l) / (1.0 - c)
    return T


def fail_columns(n, at):
    """the pivots of `at` that exist in n rows (-1 = the last)"""
    return sorted({n - 1 if k < 0 else k for k in at if k < n})


def psd_ranks(m):
    """ranks of lead(m, .): floor(m / 4), floor(m / 2), floor(0.9 m), at least 1 (rank 0 is the zero matrix, which has no
    reference diagonal to scale the rule with), without repeats"""
    return sorted({max(1, m // 4), max(1, m // 2), max(1, (9 * m) // 10)})


def spread_shapes(m):
    """(rank, decades) of spread(m, ., .)"""
    return [(max(1, m // 2), 0), (max(1, (3 * m) // 4), 4), (max(1, m // 2), 8), (m, 12)]


def lead(m, r, seed=0):
    """M = B B^T, B = [Q_r ; C] with Q_r r x r orthogonal, C uniform in (-1, 1) / sqrt(r): rank exactly r, the leading r x r block
    perfectly conditioned, every later pivot rounding noise of an exact zero"""
    def make():
        rng = np.random.default_rng([seed, m, r, 1])
        Q, _ = np.linalg.qr(rng.standard_normal((r, r)))
        Cm = rng.uniform(-1.0, 1.0, (m - r, r)) / np.sqrt(r)
        B = np.vstack([Q, Cm])
        M = B @ B.T
        return np.ascontiguousarray(0.5 * (M + M.T))
    return _keep(("lead", m, r, seed), make)


def spread(m, r, s, seed=0):
    """B = randn(m, r) with column j times 10^(-s U(0, 1)), M = B B^T (the family of tests/devtools/psd_chol_cmp.py): forced pivots that
    keep their column, pivots near either threshold, long runs of dependent columns"""
    def make():
        rng = np.random.default_rng([seed, m, r, s, 2])
        B = rng.standard_normal((m, r)) * (10.0 ** (-s * rng.random(r)))[None, :]
        M = B @ B.T
        return np.ascontiguousarray(0.5 * (M + M.T))
    return _keep(("spread", m, r, s, seed), make)


# seeds of spread(m, r, s): 0, except where seed 0 puts more than 30 % of the columns within a factor 8 of a threshold in the ORACLE's
# own pivots (31 - 41 % in these twelve; clear_columns is a property of the matrix and the oracle, no device result enters): there the
# first seed that does not
SPREAD_SEEDS = {(16, 8, 8): 2, (16, 16, 12): 1, (17, 17, 12): 2, (33, 16, 0): 1, (64, 32, 8): 1, (81, 40, 8): 1, (128, 64, 8): 1,
                (129, 64, 0): 1, (129, 129, 12): 1, (200, 100, 8): 2, (260, 130, 8): 2, (260, 260, 12): 1}


def spread_seed(m, r, s):
    return SPREAD_SEEDS.get((m, r, s), 0)


def psd_all(m):
    """[(family, name, M)] of the semidefinite tests"""
    out = [("lead", "lead m=%d r=%d" % (m, r), lead(m, r)) for r in psd_ranks(m)]
    out += [("spread", "spread m=%d r=%d s=%d" % (m, r, s), spread(m, r, s, spread_seed(m, r, s))) for r, s in spread_shapes(m)]
    return out


def chol_psd_pivots(M):
    """the loop of ipm_ref.chol_psd under pivot rule 3, operation for operation -> (L, pivots as met, forced, zeroed)"""
    n = M.shape[0]
    L = np.tril(M).astype(np.float64).copy()
    piv = np.zeros(n)
    forced = np.zeros(n, dtype=bool)
    zeroed = np.zeros(n, dtype=bool)
    for k in range(n):
        d = L[k, k]
        piv[k] = d
        if not (d > REGTOL * M[k, k]) or not (d > 1e-300):
            forced[k] = True
            zero = not (d > NOISE * (k + 1) * M[k, k])
            d = REGTOL * M[k, k] if M[k, k] > 1e-280 else 1.0
            if zero:
                zeroed[k] = True
                L[k, k] = np.sqrt(d)
                L[k + 1:, k] = 0.0
                continue
        L[k, k] = np.sqrt(d)
        L[k + 1:, k] /= L[k, k]
        L[k + 1:, k + 1:] -= np.tril(np.outer(L[k + 1:, k], L[k + 1:, k]))
    return L, piv, forced, zeroed


def psd_oracle(M):
    """chol_psd_pivots(M), computed once per matrix, read-only"""
    return _keep(("oracle", M.shape[0], hashlib.sha1(np.ascontiguousarray(M).tobytes()).hexdigest()), lambda: chol_psd_pivots(M))


def clear_columns(M, band=8.0):
    """true where two implementations of the rule must decide alike: the pivot is not within a factor `band` of the forcing threshold
    1e-13 M_kk and, when forced, its absolute value not within that factor of the zeroing threshold 1.78e-15 (k + 1) M_kk"""
    _, piv, forced, _ = psd_oracle(M)
    dd = np.diag(M)
    k1 = np.arange(1, M.shape[0] + 1)
    t1 = REGTOL * dd
    t2 = NOISE * k1 * dd
    near1 = (piv >= t1 / band) & (piv <= t1 * band)
    near2 = forced & (np.abs(piv) >= t2 / band) & (np.abs(piv) <= t2 * band)
    return ~(near1 | near2)


# ---- figures ------------------------------------------------------------------------------------------------------------

def xmul(A, B):
    return np.asarray(A, dtype=XD) @ np.asarray(B, dtype=XD)


def lapack_chol(S):
    """(lower factor, info) of LAPACK's dpotrf"""
    c, info = sla.lapack.dpotrf(np.asarray(S), lower=1, clean=1)
    return np.tril(c), int(info)


def backward_figures(L, S):
    """(componentwise, norm-wise) backward error of a factor: max_ij |L L^T - S|_ij / ((n + 1) eps (|L||L^T|)_ij) - Higham's bound
    gamma_{n+1} holds this at 1 / 2 for any order of summation with correctly rounded operations of unit roundoff eps / 2 - and
    ||L L^T - S||_F / ||S||_F.  The residual is formed in extended precision, the denominator (a scale) in double"""
    n = S.shape[0]
    R = np.abs(xmul(L, L.T) - np.asarray(S, dtype=XD)).astype(np.float64)
    D = (np.abs(L) @ np.abs(L.T)) * ((n + 1) * EPS)
    ok = D > 0
    if not np.all(np.isfinite(R)) or np.any(R[~ok] != 0):
        comp = float("inf")
    else:
        comp = float(np.max(R[ok] / D[ok])) if np.any(ok) else 0.0
    return comp, float(np.linalg.norm(R) / np.linalg.norm(S))


def comp_backward(L, S):
    return backward_figures(L, S)[0]


def recon(L, M):
    """||L L^T - M||_F / ||M||_F"""
    return backward_figures(L, M)[1]


def lapack_figures(S):
    """(factor, info, componentwise, norm-wise, kappa of the diagonal blocks) of LAPACK on a shared matrix, computed once"""
    def make():
        L, info = lapack_chol(S)
        return (L, info) + backward_figures(L, S) + (block_kappa(L),)
    return _keep(("lapack", S.shape[0], hashlib.sha1(np.ascontiguousarray(S).tobytes()).hexdigest()), make)


def residual(M, x, b):
    """||M x - b|| / ||b||, right-hand sides as ROWS of x and b"""
    r = (xmul(M, np.atleast_2d(x).T) - np.asarray(np.atleast_2d(b).T, dtype=XD)).astype(np.float64)
    return float(np.linalg.norm(r) / np.linalg.norm(b))


def inverse_defect(Xi, A):
    """max |Xi A - I|"""
    return float(np.max(np.abs(xmul(Xi, A) - np.eye(A.shape[0], dtype=XD))))


def block_kappa(L, nb=64):
    """largest 2-norm condition number of the nb x nb diagonal blocks of a factor"""
    n = L.shape[0]
    return max(float(np.linalg.cond(L[j:min(j + nb, n), j:min(j + nb, n)])) for j in range(0, n, nb))


LEVELS = {}          # group -> (value / bound, value, reference's figure or None, bound, what): the worst case seen


def check(group, what, value, bound, ref=None, bad=None, asserted=True):
    """one figure against its bound: printed, kept in LEVELS when it is the worst of its group (by value / bound), and - when it
    misses - appended to bad (bad = None: asserted on the spot).  asserted = False: recorded only"""
    value = float(value)
    bound = float(bound)
    ratio = value / bound if bound > 0 else (0.0 if value == 0 else float("inf"))
    if not np.isfinite(value):
        ratio = float("inf")
    print("%-34s %-44s %.3e%s  bound %.3e%s" % (group, what, value, "" if ref is None else "  (reference %.3e)" % ref, bound,
                                                 "" if asserted else "  [recorded]"))
    if group not in LEVELS or not ratio <= LEVELS[group][0]:
        LEVELS[group] = (ratio, value, ref, bound, what)
    if asserted and not value <= bound:
        if bad is None:
            raise AssertionError((group, what, value, bound))
        bad.append((group, what, value, bound))


def same_bits(what, a, b, bad):
    """two arrays equal bit for bit (signed zeros told apart, NaN equal to itself)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
        nd = int(np.sum(a.view(np.uint64) != b.view(np.uint64))) if a.shape == b.shape else -1
        print("%s: %d entries differ" % (what, nd))
        bad.append((what, "bits differ", nd))
