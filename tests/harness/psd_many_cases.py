"""Inputs of the hipsdp_psd_project_many tests: the generator of tests/test_gpu_psd_project.py restated, the sizes at which the batched
path changes (class boundaries of the batched decomposition at 10 and 65 rows, the 64-column compaction boundary, the LDS limit at
128 rows), and matrices whose projection is sparse.  Inputs only: nothing here touches the library or the oracle."""
import numpy as np

SIZES = (1, 2, 9, 10, 16, 17, 33, 63, 64, 65, 127, 128)
DENSITIES = (1.0, 0.3)
MINEVS = (1e-4, 0.5)
EPSILON = 1e-9
BAND = (1e-10, 1e-8)          # no upper-triangle entry of an oracle result may lie here: kept / dropped is then decided by far more than rounding


def random_sparse_sym(n, seed, density):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, n))
    M = 0.5 * (M + M.T)
    mask = rng.random((n, n)) < density
    mask = np.triu(mask) | np.triu(mask).T | np.eye(n, dtype=bool)
    M = M * mask
    r, c = np.nonzero(np.tril(M))
    return r.astype(np.int32), c.astype(np.int32), M[r, c].copy(), M


class Job:
    def __init__(self, name, n, row, col, val, M, minev):
        self.name, self.n, self.row, self.col, self.val, self.M, self.minev = name, n, row, col, val, M, minev
        self.scale = max(1.0, np.abs(M).max() * n ** 0.5) if M.size else 1.0

    def args(self):
        return (self.n, self.row, self.col, self.val, self.minev)


def mixed_jobs():
    """every size x density x minev, in a fixed shuffled order"""
    jobs = []
    for n in SIZES:
        for density in DENSITIES:
            row, col, val, M = random_sparse_sym(n, 700 + n, density)
            for minev in MINEVS:
                jobs.append(Job("n%d_d%g_m%g" % (n, density, minev), n, row, col, val, M, minev))
    order = np.random.default_rng(4711).permutation(len(jobs))
    return [jobs[i] for i in order]


def block_permuted(n1, n2, seed, minev=1e-4):
    """a symmetric permutation of diag(B1, B2), B1 and B2 dense random symmetric: the projection has the same two blocks, so most of
    every row is dropped and the kept columns are scattered over the whole row"""
    n = n1 + n2
    M = np.zeros((n, n))
    M[:n1, :n1] = random_sparse_sym(n1, seed, 1.0)[3]
    M[n1:, n1:] = random_sparse_sym(n2, seed + 1, 1.0)[3]
    p = np.random.default_rng(seed + 2).permutation(n)
    M = M[np.ix_(p, p)]
    r, c = np.nonzero(np.tril(M))
    return Job("blocks_%d_%d" % (n1, n2), n, r.astype(np.int32), c.astype(np.int32), M[r, c].copy(), M, minev)


def sparse_result_jobs():
    return [block_permuted(40, 25, 900), block_permuted(70, 58, 910)]


def band_is_empty(dense_result):
    """the precondition on an oracle result (dense n x n): no upper-triangle entry with BAND[0] < |v| < BAND[1]"""
    a = np.abs(np.triu(dense_result))
    return not np.any((a > BAND[0]) & (a < BAND[1]))
