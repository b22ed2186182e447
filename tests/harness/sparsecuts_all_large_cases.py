"""sparsecuts_all_large_cases.py - TEST INFRASTRUCTURE.  The cases on which hipsdp_sparsecuts_all_large is compared with the numpy
restatement (sparsecuts_variants_ref.py), shared by the CPU test of their stability, the GPU tests and tests/devtools/
sparsecuts_all_large_rate.py.

  "f3"   : family "f3" of sparsecuts_variants_cases.py - blocks of 16, 150, 48, 200, 10 rows, m = 25; the call serves blocks 1 and 3;
  "f4"   : its family "f4" - blocks of 130, 12, 129, 131 rows, m = 25; the call serves blocks 0, 2 and 3, by descending rows 3, 0, 2.  It
           is compared with nothing but itself: the same call in one, two and three chunks (CHUNKED).  What that needs: every large block
           cuts at size 4 under masks 0 and 7, and has at least 5 eigenvalues <= -tol.  Seeds 3 and 4 leave a block without a cut at
           size 4; seed 5 holds;
  "n129", "n257", "n512": one block each, at the edges of the 512-thread workgroup of the TPower kernel - 129 rows are two wavefronts
           and one row, 257 four and one, 512 all eight full: instances.planted_dense(n, 25, seed) with the constant matrix rebuilt as
           sym(sum_i ys_i A_i - Zs), y = ys + 0.7 default_rng(seed).standard_normal(25).
ROWS: (family, block, target size) - every block that is compared count for count; MASKS: the variants of a row.  Expected values
come from the restatement at run time."""
import numpy as np
import instances
import sparsecuts_variants_ref as V
import sparsecuts_variants_cases as K

TOL, FEASTOL, MAXCUTS = 1e-6, 1e-6, 5
M = 25
SINGLES = {"n129": (129, 41), "n257": (257, 43), "n512": (512, 45)}
#        family  block  size
ROWS = [("f3", 1, 4), ("f3", 1, 10), ("f3", 3, 10),
        ("n129", 0, 4), ("n129", 0, 10), ("n129", 0, 24),
        ("n257", 0, 4), ("n257", 0, 10),
        ("n512", 0, 24)]
SWITCHED = (1, 2, 4, 7)
# (family, block, size, variant): the restatement cases; variant 0 only on the single blocks (f3 at variant 0 is compared with hipsdp_sparsecuts)
CASES = [(f, k, sz, v) for f, k, sz in ROWS for v in SWITCHED] + [("n129", 0, 4, v) for v in (3, 5, 6)]
CASES0 = [(f, k, sz, 0) for f, k, sz in ROWS if f != "f3"]
# the 200-row block of f3 at size 4: no cut under any mask, the loop ends at once
QUIET = ("f3", 3, 4)
# the family, target size and masks of the chunk tests: three large blocks, so that a chunk of two is neither one block nor the call
CHUNKED, CHUNKED_SIZE, CHUNKED_MASKS = "f4", 4, (0, 7)

_fam, _ref, _mg = {}, {}, {}


def family(name):
    """(blocks [A_k (m + 1, n_k, n_k)], ys, y, b)"""
    if name in ("f3", "f4"):
        return K.family(name)
    if name not in _fam:
        n, seed = SINGLES[name]
        b, A, ys, Xs, Zs = instances.planted_dense(n, M, seed)
        A = A.copy()
        A0 = np.tensordot(ys, A[1:], axes=(0, 0)) - Zs
        A[0] = 0.5 * (A0 + A0.T)
        y = ys + 0.7 * np.random.default_rng(seed).standard_normal(M)
        _fam[name] = ([A], ys, y, np.array(b, dtype=np.float64))
    return _fam[name]


def large_blocks(name):
    """the indices of the blocks of a family that the call serves"""
    return [k for k, A in enumerate(family(name)[0]) if 128 < A.shape[1] <= 512]


def reference(name, k, size, variant):
    """the restatement of block k of a case, computed once and left unchanged"""
    key = (name, k, size, variant)
    if key not in _ref:
        blocks, ys, y, b = family(name)
        _ref[key] = V.sparse_cuts_dense_ex(blocks[k], y, size, TOL, FEASTOL, MAXCUTS, variant)
    return _ref[key]


def check_margins(name, k, size, variant):
    """the thresholds of sparsecuts_variants_cases.check_margins for one block: no decision of the restatement was close, the
    eigenvectors it took were well defined, three perturbed re-runs change nothing.  Returns (select, conv, feas, sub_gap, defl_gap,
    tol)."""
    key = (name, k, size, variant)
    if key in _mg:
        return _mg[key]
    blocks, ys, y, b = family(name)
    r = reference(name, k, size, variant)
    mg = r[9]
    got = (mg.select, mg.conv, mg.feas, mg.sub_gap, mg.defl_gap, mg.tol)
    assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11, (key, got)
    assert mg.sub_gap >= 1e-4 and mg.defl_gap >= 1e-4, (key, got)
    assert mg.longest <= V.MAXIT // 10 and r[8] & 3 == 0, key
    assert V.stable(blocks[k], y, size, TOL, FEASTOL, MAXCUTS, variant, base=r), key
    _mg[key] = got
    return got
