"""sparsecuts_variants_cases.py - TEST INFRASTRUCTURE.  The cases on which hipsdp_sparsecuts_all_ex is compared with the numpy
restatement (sparsecuts_variants_ref.py), shared by the CPU test of their stability, the GPU tests and tests/devtools/
sparsecuts_variants_rate.py.

The families are built as tests/test_gpu_sparsecuts_all.py builds its own (block k of sizes ns is instances.planted_dense(n_k, m,
seed = 20240 + 1000 k) with the constant matrix rebuilt around the common ys of block 0, minus 10 I for the quiet blocks; the point
is ys + 0.7 N(0, 1)):
  "f0"  : its family 0 - blocks of 3, 9, 10, 17, 33, 64, 65, 100, 128 rows, m = 20, blocks 2 and 5 quiet;
  "b12" : eight blocks of 12 rows, m = 15 (the first eight of its family 1);
  "b40" : four blocks of 40 rows, m = 15 (its family 2);
  "r12" : the 32 blocks of 12 rows of its family 1 (the rate tool only);
  "f3"  : its family 3 - blocks of 16, 150, 48, 200, 10 rows, m = 25: two blocks above the 128 rows a call with a switch serves;
  "f4"  : blocks of 130, 12, 129, 131 rows, m = 25, none quiet: three blocks above 128 rows whose index order is not their size order
          (the chunk tests of the _large calls: a chunk of several blocks that is not the whole call).
CASES: (family, target size, variant) - variants 1, 2, 4 and 7 everywhere, 3, 5 and 6 on the 12-row family, so that every combination
of the three switches runs."""
import numpy as np
import instances
import sparsecuts_variants_ref as V

TOL, FEASTOL, MAXCUTS = 1e-6, 1e-6, 5
#           sizes                                   m   quiet   seed
FAMILIES = {"f0": ([3, 9, 10, 17, 33, 64, 65, 100, 128], 20, (2, 5), 0),
            "b12": ([12] * 8, 15, (), 1),
            "b40": ([40] * 4, 15, (), 1),
            "r12": ([12] * 32, 15, (), 1),
            "f3": ([16, 150, 48, 200, 10], 25, (2,), 2),
            "f4": ([130, 12, 129, 131], 25, (), 5)}
SIZES = [("f0", 2), ("f0", 4), ("f0", 10), ("b12", 4), ("b40", 4), ("b40", 10)]
CASES = [(f, sz, v) for f, sz in SIZES for v in (1, 2, 4, 7)] + [("b12", 4, v) for v in (3, 5, 6)]

_fam, _ref, _mg = {}, {}, {}

# The hand example of recomputesparseev: 3 rows, size 2, convtol = 0.5.  TPower stops after its second iteration, far from
# convergence (the two eigenvalues of M on the support {0, 1} are close), so its vector is NOT the eigenvector of the 2 x 2 submatrix:
# the default loop cuts with x^T Z x = -1.8402.., the switch with the smallest eigenvalue of Z_S, -2.0618.. = -1.95 - sqrt(0.0125).
# The selection of the support is clear (relative gap 0.15).
HAND_Z = np.array([[-2.0, 0.1, 0.5], [0.1, -1.9, 0.75], [0.5, 0.75, 0.0]])
HAND_SIZE, HAND_CONVTOL = 2, 0.5


def hand_block():
    """(A[2, 3, 3], y) with Z(y) = HAND_Z: one variable whose matrix is the identity, y = 0"""
    return np.array([-HAND_Z, np.eye(3)]), np.zeros(1)


def family(name):
    """(blocks [A_k (m + 1, n_k, n_k)], ys, y, b)"""
    if name not in _fam:
        ns, m, quiet, seed = FAMILIES[name]
        blocks, ys, b = [], None, np.zeros(m)
        for k, n in enumerate(ns):
            _, A, ysk, Xs, Zs = instances.planted_dense(n, m, seed=20240 + 1000 * k)
            if k == 0:
                ys = ysk
            A = A.copy()
            A0 = (np.tensordot(ys, A[1:], axes=(0, 0)) if m > 0 else np.zeros((n, n))) - Zs
            A[0] = 0.5 * (A0 + A0.T)
            if k in quiet:
                A[0] -= 10.0 * np.eye(n)
            b += A[1:].reshape(m, -1) @ Xs.reshape(-1)
            blocks.append(A)
        y = ys + 0.7 * np.random.default_rng(seed).standard_normal(m)
        _fam[name] = (blocks, ys, y, b)
    return _fam[name]


def reference(name, size, variant):
    """the restatement of every block of a case, computed once and left unchanged"""
    key = (name, size, variant)
    if key not in _ref:
        blocks, ys, y, b = family(name)
        _ref[key] = [V.sparse_cuts_dense_ex(A, y, size, TOL, FEASTOL, MAXCUTS, variant) for A in blocks]
    return _ref[key]


def check_margins(name, size, variant):
    """what has to hold before counts, supports and iteration numbers of a case are compared with another implementation: no decision
    of the restatement was close, the eigenvectors it took were well defined, and three perturbed re-runs change nothing.  Returns the
    worst margins (select, conv, feas, sub_gap, defl_gap, tol) over the blocks."""
    if (name, size, variant) in _mg:
        return _mg[(name, size, variant)]
    blocks, ys, y, b = family(name)
    worst = [np.inf] * 6
    for k, (A, r) in enumerate(zip(blocks, reference(name, size, variant))):
        mg = r[9]
        got = (mg.select, mg.conv, mg.feas, mg.sub_gap, mg.defl_gap, mg.tol)
        worst = [min(a, b_) for a, b_ in zip(worst, got)]
        what = (name, size, variant, k)
        assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11, (what, got)
        assert mg.sub_gap >= 1e-4 and mg.defl_gap >= 1e-4, (what, got)
        assert mg.longest <= V.MAXIT // 10 and r[8] & 3 == 0, what
        assert V.stable(A, y, size, TOL, FEASTOL, MAXCUTS, variant, base=r), what
    _mg[(name, size, variant)] = worst
    return worst
