"""sparse_kernel_cases.py - TEST INFRASTRUCTURE: inputs, extended-precision references and derived error bounds for the kernels of
scip-sdp_amd/csrc/sparse.hip (k_sp_trows + k_sp_schur / k_sp_schur_t, k_sp_apply, k_sp_apply_t).  A plain module, imported by
tests/test_sparse_kernel_cases_cpu.py (which checks inputs and bounds on float64 restatements of the kernels) and
tests/test_gpu_sparse_kernels.py (which checks the kernels).

A case is (n, m, coo): coo = (var 1 .. m, row, col, val) as a caller may hand it over - either triangle, and of several entries with
the same (var, row, col) the last one counts (hs_sp_build; the rule of the dense scatter).  clean() is that list as hs_sp_build keeps
it.

The bound.  Every result r of the three operations is a sum of products.  With S the same sum over absolute values and K the number
of additions that can lie on the path from one product to r, recursive summation IN ANY ORDER satisfies |fl(r) - r| <= K u S to
first order (u = 2^-53; Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The tests demand
|device - ref| <= 2 K u S: the factor 2 covers the nested levels (the sum T_j = A_j Zinv inside the sum over the rows of A_j inside
the sum over the entries of A_i), the roundings of the products and the terms of higher order.  K is
    Schur entry (i, j):   nfull_i + nfull_j + 6     (entries of A_i; rows of A_j and entries of a row; six shuffle steps)
    <A_v, V>:             nnz_v + 7                 (lower entries of A_v, the addition V_rc + V_cr, six shuffle steps)
    A^T at position p:    len_p + 1                 (variables with an entry at p, the addition to base)
Nothing here is measured on a device.  The references are numpy.longdouble (64-bit significand on x86-64: 2^11 below the bound)."""
import functools
import numpy as np

import instances

U = 2.0 ** -53
LD = np.longdouble


def _coo(var, row, col, val):
    return (np.asarray(var, dtype=np.int32), np.asarray(row, dtype=np.int32), np.asarray(col, dtype=np.int32),
            np.asarray(val, dtype=np.float64))


def _from_lists(n, m, per_var, rng):
    """per_var[v - 1]: list of lower positions (r, c) of variable v; values N(0, 1)"""
    var, row, col = [], [], []
    for v, pos in enumerate(per_var, start=1):
        for (r, c) in sorted(pos):
            assert 0 <= c <= r < n
            var.append(v); row.append(r); col.append(c)
    return n, m, _coo(var, row, col, rng.standard_normal(len(var)))


def draw_positions(rng, n, ndiag, noff):
    """ndiag distinct diagonal and noff distinct strictly lower positions of an n x n matrix"""
    d = rng.choice(n, size=ndiag, replace=False) if ndiag else []
    pos = [(int(r), int(r)) for r in d]
    if noff:
        ii, jj = np.tril_indices(n, -1)
        pick = rng.choice(len(ii), size=noff, replace=False)
        pos += [(int(ii[p]), int(jj[p])) for p in pick]
    return pos


# ---- the families ------------------------------------------------------------------------------------------------------------------

def uniform(n, m, k, seed=9):
    """what instances.planted_sparse draws: k lower entries per matrix, one of them on the diagonal"""
    return n, m, instances.planted_sparse(n, m, k, seed=seed)[1]


def lane_edges():
    """matrices of exactly 63, 64, 65, 128 and 129 full entries: the lane loop of k_sp_schur takes one, exactly one, two, two and three
    trips (the one of k_sp_apply over 32, 32, 33, 64 and 65 lower entries one, one, one, exactly one and two)"""
    rng = np.random.default_rng(41)
    n = 70
    per = [draw_positions(rng, n, 1, 31), draw_positions(rng, n, 0, 32), draw_positions(rng, n, 1, 32),
           draw_positions(rng, n, 0, 64), draw_positions(rng, n, 1, 64)]
    return _from_lists(n, 5, per, rng)


def with_empty(m, ndiag, noff, seed):
    """every third variable (the first and the last among them) occurs nowhere in the block"""
    assert m % 3 == 1
    rng = np.random.default_rng(seed)
    n = 70
    per = [[] if v % 3 == 0 else draw_positions(rng, n, ndiag, noff) for v in range(m)]
    return _from_lists(n, m, per, rng)


def single(empty):
    """m = 1: the only matrix empty, or with 30 lower entries"""
    rng = np.random.default_rng(43)
    n = 66
    return _from_lists(n, 1, [[] if empty else draw_positions(rng, n, 2, 28)], rng)


def skewed():
    """one matrix of 600 lower entries among 59 of one entry each: the average stays below 24, one thread walks the long row"""
    rng = np.random.default_rng(44)
    n, m = 70, 60
    per = [draw_positions(rng, n, *((1, 0) if rng.random() < 0.5 else (0, 1))) for _ in range(m)]
    per[37] = draw_positions(rng, n, 20, 580)
    return _from_lists(n, m, per, rng)


def diagonal_only():
    rng = np.random.default_rng(45)
    n, m = 70, 40
    return _from_lists(n, m, [draw_positions(rng, n, int(rng.integers(1, 6)), 0) for _ in range(m)], rng)


def offdiag_only():
    rng = np.random.default_rng(46)
    n, m = 90, 40
    return _from_lists(n, m, [draw_positions(rng, n, 0, int(rng.integers(1, 6))) for _ in range(m)], rng)


def tiny(n):
    """n = 1 and n = 2: every variable uses every position"""
    rng = np.random.default_rng(47 + n)
    m = 3 if n == 1 else 4
    ii, jj = np.tril_indices(n)
    return _from_lists(n, m, [list(zip(ii.tolist(), jj.tolist())) for _ in range(m)], rng)


def shared_positions():
    """all variables on the same four positions: every segment of the by-position order (poff) is m long"""
    rng = np.random.default_rng(49)
    n, m = 70, 50
    pos = [(3, 3), (69, 69), (40, 7), (69, 0)]
    return _from_lists(n, m, [pos for _ in range(m)], rng)


def messy_input():
    """a clean list of five entries per matrix, then: a fifth of the entries a second time with another value, everything shuffled,
    a third of the entries (repeated ones included, so some positions are named once in either triangle) given as row < col"""
    rng = np.random.default_rng(50)
    n, m, (var, row, col, val) = uniform(70, 40, 5, seed=50)
    dup = rng.choice(len(val), size=len(val) // 5, replace=False)
    var = np.concatenate([var, var[dup]]); row = np.concatenate([row, row[dup]]); col = np.concatenate([col, col[dup]])
    val = np.concatenate([val, rng.standard_normal(len(dup))])
    p = rng.permutation(len(val))
    var, row, col, val = var[p], row[p], col[p], val[p]
    flip = rng.random(len(val)) < 1.0 / 3.0
    row, col = np.where(flip, col, row), np.where(flip, row, col)
    return n, m, _coo(var, row, col, val)


# name -> (builder, the kernel hs_sp_schur's rule is meant to pick: 0 k_sp_schur_t (nfull / m < 24), 1 k_sp_schur)
FAMILIES = {
    "uniform_k4": (lambda: uniform(70, 40, 4), 0),
    "uniform_k3": (lambda: uniform(96, 60, 3), 0),
    "uniform_k9": (lambda: uniform(130, 60, 9), 0),
    "lane_edges": (lane_edges, 1),
    "with_empty_below_24": (lambda: with_empty(40, 1, 2, 42), 0),
    "with_empty_above_24": (lambda: with_empty(25, 1, 24, 142), 1),
    "single_empty": (lambda: single(True), 0),
    "single_nonempty": (lambda: single(False), 1),
    "skewed": (skewed, 0),
    "diagonal_only": (diagonal_only, 0),
    "offdiag_only": (offdiag_only, 0),
    "tiny_n1": (lambda: tiny(1), 0),
    "tiny_n2": (lambda: tiny(2), 0),
    "shared_positions": (shared_positions, 0),
    "messy_input": (messy_input, 0),
}
NAMES = list(FAMILIES)


def _freeze(*arrs):
    for a in arrs:
        a.flags.writeable = False
    return arrs


@functools.lru_cache(maxsize=None)
def case(name):
    n, m, coo = FAMILIES[name][0]()
    return n, m, _freeze(*_coo(*coo))


def intended_kernel(name):
    return FAMILIES[name][1]


# ---- what hs_sp_build makes of a list ----------------------------------------------------------------------------------------------

def clean(n, m, coo):
    """lower triangle, the last of equal (var, row, col) wins, sorted by (var, row, col)"""
    var, row, col, val = coo
    last = {}
    for v, r, c, x in zip(var.tolist(), row.tolist(), col.tolist(), val.tolist()):
        assert 1 <= v <= m and 0 <= r < n and 0 <= c < n
        last[(v, max(r, c), min(r, c))] = x
    keys = sorted(last)
    return _coo([k[0] for k in keys], [k[1] for k in keys], [k[2] for k in keys], [last[k] for k in keys])


def counts(n, m, coo):
    """(nnz_v[m], nfull_v[m]) of the cleaned list: lower entries and entries of both triangles per variable"""
    var, row, col, _ = clean(n, m, coo)
    nnz = np.bincount(var - 1, minlength=m)
    nfull = np.bincount(var - 1, weights=np.where(row != col, 2, 1), minlength=m).astype(np.int64)
    return nnz, nfull


def rule_kernel(n, m, coo):
    """hs_sp_schur's rule: one thread per pair (0) when a matrix has fewer than 24 full entries on average, else one wavefront (1)"""
    return 0 if float(counts(n, m, coo)[1].sum()) / float(m) < 24.0 else 1


def expand(n, m, coo, dtype=LD):
    """dense [m, n, n] (variables 1 .. m), written in list order: the last duplicate wins"""
    var, row, col, val = coo
    A = np.zeros((m, n, n), dtype=dtype)
    for v, r, c, x in zip(var.tolist(), row.tolist(), col.tolist(), val.tolist()):
        A[v - 1, r, c] = x
        A[v - 1, c, r] = x
    return A


def shuffled(coo, seed=7):
    p = np.random.default_rng(seed).permutation(len(coo[3]))
    return tuple(a[p] for a in coo)


# ---- operands ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def schur_operands(n, kind):
    """(X, Zinv) in float64.  'well': as tests/test_gpu_sparse.py makes them.  'ill': the end of a solve - the eigenvalues of Z spread
    over 1e8, X = mu Z^-1 up to 10 per cent, so the terms of a Schur entry cancel and S is far above |ref|"""
    rng = np.random.default_rng(1)
    if kind == "well":
        X = rng.standard_normal((n, n)); X = X @ X.T + n * np.eye(n)
        Z = rng.standard_normal((n, n)); Z = Z @ Z.T + n * np.eye(n)
        Zi = np.linalg.inv(Z); Zi = 0.5 * (Zi + Zi.T)
    else:
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lz = np.logspace(-4.0, 4.0, n) if n > 1 else np.ones(1)
        Zi = (Q / lz) @ Q.T; Zi = 0.5 * (Zi + Zi.T)
        X = (Q * (1e-3 / lz * (1.0 + 0.1 * rng.random(n)))) @ Q.T; X = 0.5 * (X + X.T)
    return _freeze(np.ascontiguousarray(X), np.ascontiguousarray(Zi))


@functools.lru_cache(maxsize=None)
def pass_operands(n, m):
    """V symmetric / not, coef with zeros and a nonzero coef[0], base random / zero"""
    rng = np.random.default_rng(2)
    Vn = rng.standard_normal((n, n))
    Vs = 0.5 * (Vn + Vn.T)
    coef = rng.standard_normal(m + 1)
    coef[1:][rng.random(m) < 0.25] = 0.0
    coef[0] = 3.25
    base = rng.standard_normal((n, n))
    return _freeze(Vs, Vn, coef, base, np.zeros((n, n)))


# ---- references in extended precision ----------------------------------------------------------------------------------------------

def _schur_ld(A, X, Zinv):
    """M[i, j] = tr(A_i X A_j Zinv) from the dense A[m, n, n]; the zero rows of A_j and the zero entries of A_i are left out of the
    products (they contribute exact zeros)"""
    m, n, _ = A.shape
    M = np.zeros((m, m), dtype=LD)
    vi, ra, cb = np.nonzero(A)
    av = A[vi, ra, cb]
    for j in range(m):
        rows = np.flatnonzero(A[j].any(axis=1))
        if len(rows) == 0:
            continue
        W = X[:, rows] @ (A[j][rows] @ Zinv)                  # X A_j Zinv
        np.add.at(M[:, j], vi, av * W[cb, ra])                # sum over (a, b) of A_i[a][b] W[b][a]
    return M


def schur_ref(n, m, coo, X, Zinv):
    """(M, S): M[i, j] = tr(A_i X A_j Zinv) and its magnitude S[i, j] = the same sum over |A_i|, |X|, |A_j|, |Zinv|; m x m, longdouble"""
    A = expand(n, m, coo)
    Xl, Zl = X.astype(LD), Zinv.astype(LD)
    return _schur_ld(A, Xl, Zl), _schur_ld(np.abs(A), np.abs(Xl), np.abs(Zl))


def schur_ref_pairs(n, m, coo, X, Zinv, pairs):
    """(M, S) of the listed pairs (i, j), 0-based, alone: sum over the entries (a, b) of A_i and (p, q) of A_j (both triangles) of
    A_i[a][b] X[b][p] A_j[p][q] Zinv[q][a]"""
    var, row, col, val = clean(n, m, coo)
    off = row != col
    fv = np.concatenate([var, var[off]]); fr = np.concatenate([row, col[off]]); fc = np.concatenate([col, row[off]])
    fx = np.concatenate([val, val[off]]).astype(LD)
    order = np.argsort(fv, kind="stable")
    fv, fr, fc, fx = fv[order], fr[order], fc[order], fx[order]
    start = np.searchsorted(fv, np.arange(1, m + 2))
    Xl, Zl = X.astype(LD), Zinv.astype(LD)
    M = np.zeros(len(pairs), dtype=LD)
    S = np.zeros(len(pairs), dtype=LD)
    for t, (i, j) in enumerate(pairs):
        ei = slice(start[i], start[i + 1]); ej = slice(start[j], start[j + 1])
        a, b, xi = fr[ei], fc[ei], fx[ei]
        p, q, xj = fr[ej], fc[ej], fx[ej]
        terms = (xi[:, None] * xj[None, :]) * Xl[b[:, None], p[None, :]] * Zl[q[None, :], a[:, None]]
        M[t] = terms.sum()
        S[t] = np.abs(terms).sum()
    return M, S


def schur_K(n, m, coo):
    nfull = counts(n, m, coo)[1]
    return nfull[:, None] + nfull[None, :] + 6


def schur_bound(n, m, coo, S):
    return 2.0 * schur_K(n, m, coo) * U * S.astype(np.float64) * (1.0 + 2.0 ** -40)      # (S rounded to float64)


def schur_structural_zero(n, m, coo):
    """[m, m] bool: A_i or A_j has no entry - the device value must be exactly 0.0"""
    e = counts(n, m, coo)[0] == 0
    return e[:, None] | e[None, :]


def apply_ref(n, m, coo, V):
    """(out, S): out[v] = <A_v, V> over both triangles, S[v] = sum |val| (|V_rc| + |V_cr|)"""
    A = expand(n, m, coo)
    Vl = V.astype(LD)
    return np.einsum("vab,ab->v", A, Vl), np.einsum("vab,ab->v", np.abs(A), np.abs(Vl))


def apply_bound(n, m, coo, S):
    return 2.0 * (counts(n, m, coo)[0] + 7) * U * S.astype(np.float64) * (1.0 + 2.0 ** -40)


def position_counts(n, m, coo):
    """[n, n] int: the number of variables with an entry at the position (both triangles)"""
    var, row, col, _ = clean(n, m, coo)
    cnt = np.zeros((n, n), dtype=np.int64)
    np.add.at(cnt, (row, col), 1)
    off = row != col
    np.add.at(cnt, (col[off], row[off]), 1)
    return cnt


def apply_t_ref(n, m, coo, coef, base):
    """(out, S): out = base + sum_{v >= 1} coef[v] A_v, S = |base| + sum |coef[v] A_v|; coef[0] takes no part"""
    A = expand(n, m, coo)
    c = coef[1:].astype(LD)
    return base.astype(LD) + np.einsum("v,vab->ab", c, A), np.abs(base).astype(LD) + np.einsum("v,vab->ab", np.abs(c), np.abs(A))


def apply_t_bound(n, m, coo, S):
    return 2.0 * (position_counts(n, m, coo) + 1) * U * S.astype(np.float64) * (1.0 + 2.0 ** -40)


# ---- float64 restatements of the two passes, in the kernels' order (the Schur matrix: ipm_ref.schur_rows_sparse) -------------------

def apply_f64(n, m, coo, V):
    """k_sp_apply: lane l of a wavefront sums the lower entries l, l + 64, ... of the variable, then six butterfly steps"""
    var, row, col, val = clean(n, m, coo)
    out = np.zeros(m)
    lanes = np.arange(64)
    for v in range(1, m + 1):
        acc = np.zeros(64)
        for k, e in enumerate(np.flatnonzero(var == v)):
            r, c = row[e], col[e]
            x = V[r, c]
            acc[k % 64] += val[e] * (x + V[c, r] if r != c else x)
        for o in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lanes ^ o]
        out[v - 1] = acc[0]
    return out


def apply_t_f64(n, m, coo, coef, base):
    """k_sp_apply_t: one thread per position sums coef[var] val over the variables in ascending order and adds to both triangles"""
    var, row, col, val = clean(n, m, coo)
    out = np.array(base, dtype=np.float64)
    pos = {}
    for v, r, c, x in zip(var.tolist(), row.tolist(), col.tolist(), val.tolist()):
        pos.setdefault((r, c), []).append((v, x))
    for (r, c), ents in sorted(pos.items()):
        acc = 0.0
        for v, x in sorted(ents):
            acc += coef[v] * x
        out[r, c] += acc
        if r != c:
            out[c, r] += acc
    return out
