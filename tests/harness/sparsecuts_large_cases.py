"""sparsecuts_large_cases.py - TEST INFRASTRUCTURE.  The blocks of 129 .. 512 rows on which hipsdp_sparsecuts is compared with the
numpy restatement (sparsecuts_ref.py), shared by the CPU test of the fixture, the GPU tests and tests/devtools/
sparsecuts_large_rate.py.

Two kinds of block, both instances.planted_dense with the constant matrix rebuilt as sym(sum_i ys_i A_i - Zs):
  "f4"  : family 4 of tests/test_gpu_sparsecuts_all.py (blocks of 16, 150, 48, 200, 10 rows, m = 25, block k from seed 20240 +
          1000 k, the common ys of block 0, block 2 quiet, y = ys + 0.7 N(0, 1) from seed 2) - its blocks 1 and 3 are the ones
          hipsdp_sparsecuts_all turns away;
  "own" : one block (n, m, seed) around its own ys, y = ys + amp N(0, 1) from default_rng(seed).

TABLE holds, per case, the cuts and the TPower iterations of the restatement.  On all of them the restatement's margins are:
selection >= 3.8e-5, convergence >= 2.4e-10, feasibility >= 1.0e-6, flags 0; perturbing v0 by 1e-12 .. 1e-8 and maxeig relatively by
the same moved no count, support or iteration number and the cut values by at most 1.8e-10."""
import numpy as np
import instances
import sparsecuts_ref as R

TOL, FEASTOL, MAXCUTS = 1e-6, 1e-6, 5
F4_NS, F4_M, F4_QUIET, F4_SEED = [16, 150, 48, 200, 10], 25, (2,), 2

#        name      block                          size  cuts  iterations
TABLE = [("f4b1",  ("f4", 1),                      4,    2,    104),
         ("f4b1",  ("f4", 1),                      10,   5,    425),
         ("f4b3",  ("f4", 3),                      4,    0,    73),
         ("f4b3",  ("f4", 3),                      10,   3,    262),
         ("n129",  ("own", 129, 6, 31129, 2.0),    10,   5,    512),
         ("n129",  ("own", 129, 6, 31129, 2.0),    48,   5,    705),
         ("n129s", ("own", 129, 6, 31129, 0.7),    129,  1,    4),
         ("n257",  ("own", 257, 6, 31257, 2.0),    10,   5,    554),
         ("n257",  ("own", 257, 6, 31257, 2.0),    24,   5,    552),
         ("n512",  ("own", 512, 4, 31512, 2.0),    10,   0,    60),
         ("n512",  ("own", 512, 4, 31512, 2.0),    24,   5,    558)]

_f4, _blk, _ref = [], {}, {}


def rebuilt(A, ys, Zs):
    """the block with its constant matrix formed around ys"""
    A = A.copy()
    n, m = A.shape[1], A.shape[0] - 1
    A0 = (np.tensordot(ys, A[1:], axes=(0, 0)) if m > 0 else np.zeros((n, n))) - Zs
    A[0] = 0.5 * (A0 + A0.T)
    return A


def family4():
    """(blocks, ys, y, b) of family 4, built as tests/test_gpu_sparsecuts_all.py builds it"""
    if not _f4:
        blocks, ys, b = [], None, np.zeros(F4_M)
        for k, n in enumerate(F4_NS):
            _, A, ysk, Xs, Zs = instances.planted_dense(n, F4_M, seed=20240 + 1000 * k)
            if k == 0:
                ys = ysk
            A = rebuilt(A, ys, Zs)
            if k in F4_QUIET:
                A[0] -= 10.0 * np.eye(n)
            b += A[1:].reshape(F4_M, -1) @ Xs.reshape(-1)
            blocks.append(A)
        y = ys + 0.7 * np.random.default_rng(F4_SEED).standard_normal(F4_M)
        _f4.append((blocks, ys, y, b))
    return _f4[0]


def block(spec):
    """(A[m + 1, n, n], ys, y, b) of a block of TABLE"""
    if spec not in _blk:
        if spec[0] == "f4":
            blocks, ys, y, b = family4()
            A = blocks[spec[1]]
            _blk[spec] = (A, ys, y, b)
        else:
            _, n, m, seed, amp = spec
            b, A, ys, Xs, Zs = instances.planted_dense(n, m, seed=seed)
            y = ys + amp * np.random.default_rng(seed).standard_normal(m)
            _blk[spec] = (rebuilt(A, ys, Zs), ys, y, b)
    return _blk[spec]


def reference(spec, size):
    """the restatement of a case, computed once; its margins are asserted here, before anything is compared with it"""
    if (spec, size) not in _ref:
        A, ys, y, b = block(spec)
        r = R.sparse_cuts_dense(A, y, size, TOL, FEASTOL, MAXCUTS)
        mg = r[9]
        print("restatement %s size %d: %d cuts, %d iterations, longest run %d, margins %.2e %.2e %.2e"
              % (spec, size, r[0], r[7], mg.longest, mg.select, mg.conv, mg.feas))
        assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11, (spec, size)
        assert mg.longest <= R.MAXIT // 10, (spec, size)
        assert r[8] == 0
        _ref[(spec, size)] = r
    return _ref[(spec, size)]


def matrix_inputs(spec):
    """(Z, v0, maxeig) of a block by numpy: what the unit entry of the TPower kernel takes"""
    A, ys, y, b = block(spec)
    Z = np.tensordot(y, A[1:], axes=(0, 0)) - A[0]
    lam, V = np.linalg.eigh(Z)
    return Z, V[:, 0].copy(), float(lam[-1])
