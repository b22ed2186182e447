"""Host reference of the Lanczos kernels of csrc/eig.hip (k_lanczos_fused, k_lanczos_step) and the matrices their tests use.

The reference follows the device step by step - the same start vector (the 64-bit hash of k_lanczos_init, reproduced with Python
integers), classical Gram-Schmidt applied twice against the whole basis, scale = max (|alpha| + beta), a breakdown when
not (b > 1e-13 scale) or not (b > 1e-300), k = min(steps, n, 250) - in numpy, in float64 or in longdouble.  The smallest eigenvalue of
the tridiagonal matrix and its vector come from numpy.linalg.eigh (LAPACK has no extended precision: a longdouble run hands its
tridiagonal matrix over rounded to float64), resid = |beta_last s_last|, 0 after a breakdown.

A run of k steps is the first k steps of a longer run (the breakdown rule looks at the past only), so `run` makes the recurrence once
and `ritz` reads the result of every step count off it.

No device code is involved: tests/test_lanczos_ref_cpu.py shows on the CPU that the two precisions agree on the matrices below, i.e.
that what the GPU tests compare a kernel with is a property of the matrix and not of this file's rounding."""
import numpy as np

MAXSTEPS = 250
_M64 = (1 << 64) - 1


def start_vector(n):
    """the unnormalised start vector of k_lanczos_init, float64: entry i is 0.5 + (h >> 11) 2^-53 of the hash h of i + 1"""
    v = np.empty(n)
    for i in range(n):
        h = ((i + 1) * 0x9E3779B97F4A7C15) & _M64
        h ^= h >> 29
        h = (h * 0xBF58476D1CE4E5B9) & _M64
        h ^= h >> 32
        v[i] = 0.5 + float(h >> 11) * (1.0 / 9007199254740992.0)          # (h >> 11 < 2^53: every operation but the sum is exact)
    return v


def steps_of(n, steps):
    """the device's step count: steps <= 0 asks for min(n, 250)"""
    k = min(n, MAXSTEPS) if steps <= 0 else steps
    return min(k, n, MAXSTEPS)


class Run:
    """alpha[0 .. done), beta[0 .. done) (beta of a breakdown step is 0), broke: the step that broke down or -1"""

    def __init__(self, alpha, beta, broke):
        self.alpha, self.beta, self.broke = alpha, beta, broke


def run(W, steps=0, dtype=np.float64, matvec=None):
    """the recurrence for steps_of(n, steps) steps, or up to the breakdown.  W: the matrix (cast to dtype), or with matvec - a function
    of a dtype vector - only its order n"""
    n = int(W) if matvec is not None else W.shape[0]
    k = steps_of(n, steps)
    if matvec is None:
        Wd = np.asarray(W, dtype=dtype)
        matvec = lambda q: Wd @ q
    v = start_vector(n).astype(dtype)
    Q = np.zeros((k + 1, n), dtype=dtype)
    Q[0] = v / np.sqrt(v @ v)
    alpha, beta = np.zeros(k, dtype=dtype), np.zeros(k, dtype=dtype)
    scale = dtype(0.0)
    for j in range(k):
        v = matvec(Q[j])
        for sweep in range(2):
            c = Q[:j + 1] @ v
            if sweep == 0:
                alpha[j] = c[j]
            v = v - c @ Q[:j + 1]
        b = np.sqrt(v @ v)
        scale = max(scale, abs(alpha[j]) + b)
        if not (b > dtype(1e-13) * scale) or not (b > dtype(1e-300)):
            return Run(alpha[:j + 1], beta[:j + 1], j)
        beta[j] = b
        Q[j + 1] = v / b
    return Run(alpha, beta, -1)


def ritz(r, k):
    """(theta, resid, steps_done) of the run of k steps read off the longer run r"""
    broke = r.broke >= 0 and r.broke < k
    size = r.broke + 1 if broke else k
    assert size <= len(r.alpha)
    a = np.asarray(r.alpha[:size], dtype=np.float64)
    b = np.asarray(r.beta[:size], dtype=np.float64)
    T = np.diag(a) + np.diag(b[:size - 1], 1) + np.diag(b[:size - 1], -1)
    lam, S = np.linalg.eigh(T)
    resid = 0.0 if broke else abs(float(b[size - 1]) * float(S[size - 1, 0]))
    return float(lam[0]), resid, size


def lanczos(W, steps=0, dtype=np.float64):
    """(theta, resid, steps_done) as the device reports them in res[0 .. 2]"""
    return ritz(run(W, steps, dtype), steps_of(W.shape[0], steps))


# ---- the matrices ------------------------------------------------------------------------------------------------------------------------

def spectrum(n, lam, rng):
    """Q diag(lam) Q^T with Q from the QR factorization of a normal matrix, symmetrised"""
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    W = (Q * np.asarray(lam, dtype=np.float64)) @ Q.T
    return 0.5 * (W + W.T)


def adversarial(n, rng):
    """I - 2 u u^T with the unit vector u orthogonal to the start vector: eigenvalues 1 (n - 1 times, the start vector among its
    vectors) and -1 (u).  The first step already finds beta = 0: the run stops with theta = 1 and resid = 0."""
    q = start_vector(n)
    q /= np.linalg.norm(q)
    u = rng.standard_normal(n)
    for _ in range(2):
        u -= (q @ u) * q
    u /= np.linalg.norm(u)
    W = np.eye(n) - 2.0 * np.outer(u, u)
    return 0.5 * (W + W.T)


FAMILIES = ["wigner", "optlike", "neg1", "graded", "neg1_up", "neg1_down", "identity", "zero", "diag"]
TOL_FAMILIES = ["inside", "outside"]            # around tol = 1e-5 at unit norm (the check_y tests)


def _neg1(n, rng, first=-1e-3, lo=1.0, hi=2.0):
    lam = rng.uniform(lo, hi, n)
    lam[0] = first
    return lam


def matrix(name, n, seed=0):
    """the matrix of a family at n rows: wigner G + G^T; optlike n // 4 zeros, the rest in [1, 2]; neg1 lambda_1 = -1e-3, the rest in
    [1, 2]; graded logspace(-8, 0, n); neg1_up / neg1_down: neg1 times 2^40 / 2^-40 (exact: the same bits at another exponent);
    identity, zero, diag(1 .. n); inside / outside: lambda_1 = -0.5e-5 / -2e-5, the rest in [0.5, 1]"""
    rng = np.random.default_rng([seed, n, (FAMILIES + TOL_FAMILIES).index(name)])
    if name == "wigner":
        G = rng.standard_normal((n, n))
        return G + G.T
    if name == "optlike":
        return spectrum(n, np.concatenate([np.zeros(n // 4), rng.uniform(1.0, 2.0, n - n // 4)]), rng)
    if name == "neg1":
        return spectrum(n, _neg1(n, rng), rng)
    if name == "graded":
        return spectrum(n, np.logspace(-8.0, 0.0, n), rng)
    if name in ("neg1_up", "neg1_down"):
        return matrix("neg1", n, seed) * (2.0 ** 40 if name == "neg1_up" else 2.0 ** -40)
    if name == "identity":
        return np.eye(n)
    if name == "zero":
        return np.zeros((n, n))
    if name == "diag":
        return np.diag(np.arange(1.0, n + 1.0))
    if name == "inside":
        return spectrum(n, _neg1(n, rng, -0.5e-5, 0.5, 1.0), rng)
    if name == "outside":
        return spectrum(n, _neg1(n, rng, -2e-5, 0.5, 1.0), rng)
    raise ValueError(name)


# ---- what the GPU tests run: shared with the CPU test of this file -----------------------------------------------------------------------

# the smallest sizes that meet each edge of the kernels: the exact kernel's last size and the first Lanczos one, a 64-wide tail (63, 64,
# 65, 127), the check's 200, the step cap (250, 251), a second trip of the i += 1024 loops (1025), the cap of 128 workgroups with 17
# rows each and trailing workgroups without rows (2050)
SIZES = [16, 17, 63, 64, 65, 127, 200, 250, 251, 1025, 2050]
STEPS = [24, 16, 4, 0]
BIG_N = 8193                                    # the launch-per-step form (above 8192 rows)
BIG_STEPS = 24


def reflected_diag(n, seed=0):
    """W = H diag(d) H with H = I - 2 u u^T, built in O(n^2): W = D - 2 (u w^T + w u^T) + 4 (u^T w) u u^T, w = D u.  The spectrum is d
    to rounding.  Returns (W, d ascending)"""
    rng = np.random.default_rng([seed, n, 77])
    d = np.sort(np.concatenate([[-1e-3], rng.uniform(1.0, 2.0, n - 1)]))
    u = rng.standard_normal(n)
    u /= np.linalg.norm(u)
    w = d * u
    W = -2.0 * np.outer(u, w)
    W += W.T
    W += (4.0 * (u @ w)) * np.outer(u, u)
    W[np.diag_indices(n)] += d
    return W, d
