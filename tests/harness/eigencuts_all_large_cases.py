"""eigencuts_all_large_cases.py - TEST INFRASTRUCTURE.  The cases on which hipsdp_eigencuts_all_large is compared with the numpy
restatement oracle/eigcuts_ref.cuts_dense, shared by the CPU test of their margins, the GPU tests and tests/devtools/
eigencuts_all_large_rate.py.  The families are those of sparsecuts_all_large_cases.py:

  "f3"   : blocks of 16, 150, 48, 200, 10 rows, m = 25; the call serves blocks 1 and 3;
  "f4"   : blocks of 130, 12, 129, 131 rows, m = 25 (CHUNKED): the call serves blocks 0, 2 and 3; compared with nothing but itself, the
           same call in one, two and three chunks, so it has no ROWS;
  "n129", "n257", "n512": one block each at the point y of that file - 129 rows is the first size of the path (two wavefronts and one
           row), 257 is one past a power of two, 512 is the cap.

At tol 1e-6 every served block has more than 32 eigenvalues <= -tol, so with maxcuts 5 and 32 it returns exactly maxcuts cuts; margins()
recomputes from the oracle what makes the comparison safe: counts immune to rounding (no eigenvalue near -tol), vectors defined up to
sign (relative gaps among the selected values and the next one).  At ys every block has lmin ~ -1e-15: nothing to cut.  Expected values
come from the oracle at run time, computed once per (case, block, maxcuts) and left unchanged."""
import numpy as np
import eigcuts_ref
import sparsecuts_all_large_cases as S

TOL, MAXCUTS, WIDE = 1e-6, 5, 32
M = S.M
FAMILIES = ("f3", "n129", "n257", "n512")
#        family  block  rows
ROWS = [("f3", 1, 150), ("f3", 3, 200), ("n129", 0, 129), ("n257", 0, 257), ("n512", 0, 512)]
# the margins every compared row has to keep (measured: smallest relative gap 1.4e-3, nearest eigenvalue to -tol 3.2e-3)
MIN_GAP, MIN_TOL_DIST = 1e-3, 1e-3

CHUNKED = S.CHUNKED
family = S.family
large_blocks = S.large_blocks
_ref, _spec = {}, {}


def zmat(name, k, at_ys=False):
    blocks, ys, y, b = family(name)
    A = blocks[k]
    return np.tensordot(ys if at_ys else y, A[1:], axes=(0, 0)) - A[0]


def spectrum(name, k):
    """all eigenvalues of Z_k(y), ascending, computed once"""
    if (name, k) not in _spec:
        w = np.linalg.eigvalsh(zmat(name, k))
        w.setflags(write=False)
        _spec[(name, k)] = w
    return _spec[(name, k)]


def reference(name, k, maxcuts):
    """(lmin, eigvals, coefs, lhs, vecs) of block k from the oracle, computed once and left unchanged"""
    key = (name, k, maxcuts)
    if key not in _ref:
        blocks, ys, y, b = family(name)
        ev, co, lh, ve = eigcuts_ref.cuts_dense(blocks[k], y, TOL, maxcuts)
        for a in (ev, co, lh, ve):
            a.setflags(write=False)
        _ref[key] = (float(ev[0]) if len(ev) else float(spectrum(name, k)[0]), ev, co, lh, ve)
    return _ref[key]


def margins(name, k, maxcuts):
    """(eigenvalues <= -tol, smallest gap among the first maxcuts + 1 eigenvalues relative to max(1, |lambda|_max), distance of the
    nearest eigenvalue to -tol) - the figures of the table the cases were chosen by"""
    w = spectrum(name, k)
    below = int(np.sum(w <= -TOL))
    sel = w[:maxcuts + 1]
    scale = max(1.0, float(np.abs(w).max()))
    gap = float(np.min(np.diff(sel)) / scale)
    dist = float(np.min(np.abs(w + TOL)))
    return below, gap, dist


def multiple_case():
    """one block of 129 rows, m = 1, A_0 = -W with W the low_rank_shifted matrix of eig_cases (117 eigenvalues -0.01), A_1 a fixed
    symmetric matrix, y = 0: Z(y) = W.  Returns (blocks, y, b, W, eigenvalues of W)"""
    import eig_cases
    n = 129
    W, ev, scale = eig_cases.spectra(n)["low_rank_shifted"]
    G = np.random.default_rng(129).standard_normal((n, n))
    A = np.stack([-np.array(W), 0.5 * (G + G.T)])
    return [A], np.zeros(1), np.ones(1), np.array(W), np.array(ev)
