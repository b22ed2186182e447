"""Inputs of the hipsdp_psd_project_many_large tests: matrices of 129 .. 512 rows.  random_sparse_sym, block_permuted and Job are those of
psd_many_cases.py; added here are the sizes at which the large path changes (129: smallest served, the last panel of 32 vectors
holds one; 160: a multiple of 32; 200; 257: crosses 256, nine panels; 512: once), low-rank matrices plus a shift (n - r equal
eigenvalues: one cluster of hundreds of vectors, and the tridiagonal form splits), block matrices whose projection is sparse, and
three edge cases at 129 rows.  Inputs only: nothing here touches the library or the oracle."""
import numpy as np

from psd_many_cases import Job, random_sparse_sym, block_permuted, band_is_empty, EPSILON, BAND     # noqa: F401 (re-exported)

SIZES = (129, 160, 200, 257)          # the sizes of the mixed call; 512 comes once, on its own
DENSITIES = (1.0, 0.05)
MINEVS = (1e-4, 0.5)
LOW_RANK = ((129, 12, 0.0), (200, 20, 0.25), (257, 30, -0.01))       # (n, r, shift)
BLOCKS = ((150, 107, 920), (100, 29, 930))                           # (n1, n2, seed): 257 and 129 rows


def random_job(n, density, minev):
    row, col, val, M = random_sparse_sym(n, 700 + n, density)
    return Job("random_n%d_d%g_m%g" % (n, density, minev), n, row, col, val, M, minev)


def random_jobs(sizes=SIZES):
    return [random_job(n, density, minev) for n in sizes for density in DENSITIES for minev in MINEVS]


def low_rank_shifted(n, r, shift, minev=1e-4, seed=None):
    """Q diag(linspace(1, 3, r)) Q^T + shift I with Q of r orthonormal columns: n - r eigenvalues equal to shift"""
    rng = np.random.default_rng(800 + n if seed is None else seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, r)))
    M = (Q * np.linspace(1.0, 3.0, r)) @ Q.T
    M = 0.5 * (M + M.T) + shift * np.eye(n)
    rr, cc = np.nonzero(np.tril(np.ones((n, n), dtype=bool)))
    return Job("low_rank_n%d_r%d_s%g" % (n, r, shift), n, rr.astype(np.int32), cc.astype(np.int32), M[rr, cc].copy(), M, minev)


def low_rank_jobs():
    return [low_rank_shifted(n, r, shift) for n, r, shift in LOW_RANK]


def blocks_jobs():
    return [block_permuted(n1, n2, seed) for n1, n2, seed in BLOCKS]


def edge_jobs():
    """at 129 rows: no triplets (minev 0.5), a diagonal matrix (T is all 1 x 1 blocks), a matrix that is already >= minev"""
    n = 129
    none_i, none_d = np.zeros(0, np.int32), np.zeros(0)
    idx = np.arange(n, dtype=np.int32)
    d = np.linspace(-1.0, 2.2, n)                   # (steps of 0.025: the entries next to minev = 0.26 are 0.25 and 0.275)
    empty = Job("edge_empty", n, none_i, none_i, none_d, np.zeros((n, n)), 0.5)
    diag = Job("edge_diag", n, idx, idx, d, np.diag(d), 0.26)
    M = random_sparse_sym(n, 940, 1.0)[3]
    M = M @ M.T / n + 0.5 * np.eye(n)               # eigenvalues >= 0.5
    r, c = np.nonzero(np.tril(np.ones((n, n), dtype=bool)))
    psd = Job("edge_psd", n, r.astype(np.int32), c.astype(np.int32), M[r, c].copy(), M, 1e-4)
    return [empty, diag, psd]


def job_512():
    return random_job(512, 1.0, 1e-4)


def mixed_jobs():
    """all random, low_rank_shifted and blocks cases up to 257 rows, in a fixed shuffled order"""
    jobs = random_jobs() + low_rank_jobs() + blocks_jobs()
    order = np.random.default_rng(4712).permutation(len(jobs))
    return [jobs[i] for i in order]


def all_jobs():
    """every case of this file (the CPU test checks the two preconditions on each of them)"""
    return random_jobs() + low_rank_jobs() + blocks_jobs() + edge_jobs() + [job_512()]


def decomposition_table():
    """the dense matrices of the batched-decomposition test: 129 random, 160 random, 200 low rank, 257 blocks, 129 diagonal"""
    return [random_job(129, 1.0, 1e-4).M, random_job(160, 1.0, 1e-4).M, low_rank_shifted(200, 20, 0.25).M, block_permuted(150, 107, 920).M,
            edge_jobs()[1].M]
