"""Seeded input families, references and figures of tests/test_gpu_schur_forms.py: every form of the Schur assembly
M_ij = tr(A_i X A_j Z^-1) of scip-sdp_amd/csrc/schur.hip at the matrix level.  tests/test_schur_cases_cpu.py holds the references alone
to everything the GPU tests assume of them.

Forms (hipsdp_schur_form_unit): 0 hs_schur_W, 1 hs_schur_Wcols, 2 hs_schur_Urows, 3 hs_schur_U, 4 hs_schur_Wvar.  The W forms (0, 1, 4)
take R and G with X = R R^T, Z^-1 = G^T G and form W_j = G (A_j R), M = W W^T; the U forms (2, 3) and hs_schur_small take X and Zinv and form
U_j = X (A_j Zinv), M_ij = <A_i, U_j>.

Families
  exact    A_i symmetric and R, G lower triangular with entries in {-1, 0, 1} (nonzero diagonals), X = R R^T and Zinv = G^T G formed
           exactly; LP data integer with z a power of two.  Every product and partial sum of every form is an integer below 2^53
           (exact_premise proves it per case from the abs-value chains), so every summation order gives the same bits: the device must
           EQUAL float64 numpy, and every form every other.
  iterate  X = Q diag(lam) Q^T, Z = Q diag(mu / lam) Q^T, lam graded from 1 to 1 / cond, mu = cond^-1/2: the near-complementary pair an
           interior-point iteration produces.  R = chol(X), G = chol(Z)^-1 on the host, rounded to double; A_i Gaussian symmetric.  The
           reference is the same formula in numpy.longdouble ON THOSE ROUNDED OPERANDS (the U forms: on the double matrices R R^T and
           G^T G that are handed to the device), so no conditioning enters the comparison.  Figure: F = max_ij |M - M_ref|_ij /
           (eps B_ij), B the abs-value chain of the form, eps = 2^-52: component-wise over entries that span twelve decades.
  scaled   an iterate case with A_i times 2^k_i, k_i in -10 .. 10: M scales by 2^(k_i + k_j) bit for bit.

Every array is computed once, shared and read-only.  Figures go through check(): printed before they are judged, the worst of every
group kept in LEVELS (tests/devtools/schur_levels.py writes that table down)."""
import numpy as np
import scipy.linalg as sla

import shard_ref

EPS = float(np.finfo(np.float64).eps)           # 2^-52
XD = np.longdouble
W_FORMS = (0, 1, 4)
U_FORMS = (2, 3)
FORM_NAMES = {0: "hs_schur_W", 1: "hs_schur_Wcols", 2: "hs_schur_Urows", 3: "hs_schur_U", 4: "hs_schur_Wvar", "small": "hs_schur_small"}
MARGIN = 10.0                                   # device against numpy on the same terms in another order (the Cholesky tests' margin)

# (m1, n): the smallest shapes at which each rung of the product ladder can go wrong (dispatch rules: dgemm.hip hs_dgemm, dgemm2.hip
# hs_dgemm2_try, gram.hip hs_gram_try; predict_used() restates them and the GPU test holds the counters of the call to it)
LADDER = [(20, 24),          # the 32 x 32 kernel (stack and Gram products) and 64-wide tiles (the batch: HS_GEMM_REMAP)
          (9, 17),           # the same with odd n and K = 17: one K step and a tail
          (192, 131),        # odd n: the persistent kernels refuse it, the 128-wide tile kernel clips the triangles
          (192, 130),        # 195 x 2 = 390 >= 384 tiles: both triangular products on the paired-band kernel, second column tile 2 wide
          (300, 140),        # m1 >= 256, n^2 = 19600 >= 16384: the Gram kernel (it has a plan: measured), 3 x 3 tiles
          (401, 300)]        # n^2 = 90000: the Gram kernel (it has a plan), without one the XCD-walked slices
FORM1 = [(60, 150, 8),       # uneven narrow slices
         (60, 40, 3),        # empty slices
         (120, 300, 2)]      # slices above 64 columns: 128-wide tiles
FORM2 = [(101, 50, 3), (150, 64, 2), (33, 130, 2)]
FORM3 = [(4, 3), (9, 5), (41, 20), (101, 50), (150, 64), (33, 130)]            # test_gpu_units.py::test_schur_assembly, plain and chunked
FORM4 = [(70, 80, 48), (40, 150, 64)]
# (m1, block sizes, LP rows) of hs_schur_small
SMALL = [(1, (3,), 0), (13, (4, 9), 29), (38, (10,), 85), (106, (15,), 240), (5, (48,), 0), (9, (2, 3, 4, 5, 6, 7, 8, 9), 4),
         (300, (5,), 10)]    # the i += 256 loops
# refused: just above the work bound 0.5 m1^2 n^2 <= 1.5e6 (36^2 48^2 / 2 = 1 492 992 is taken, 37: 1 577 088), and n = 49
SMALL_REFUSED = [(37, (48,), 0), (3, (49,), 2)]
SMALL_EDGE_TAKEN = (36, (48,), 0)
ITERATE = [(9, 17), (16, 33), (20, 48), (12, 65), (33, 130)]
CONDS = (1e4, 1e8, 1e12)
SMALL_NMAX, SMALL_WORK = 48, 1.5e6


def chunk_gbytes(n):
    """the workspace budget with which test_schur_assembly chunks the U form: three matrices per chunk"""
    return 16.0 * n * n * 3 / 1e9


_CACHE = {}


def _keep(key, make):
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


# ---- inputs -------------------------------------------------------------------------------------------------------------

def _tri_int(rng, n):
    L = np.tril(rng.integers(-1, 2, (n, n))).astype(np.float64)
    L[np.arange(n), np.arange(n)] = rng.choice([-1.0, 1.0], n)
    return L


def _sym_int(rng, m1, n):
    T = np.tril(rng.integers(-1, 2, (m1, n, n))).astype(np.float64)
    return np.ascontiguousarray(T + np.tril(T, -1).transpose(0, 2, 1))


def exact(m1, n, seed=0):
    """(A, R, G, X, Zinv) of the exact family"""
    def make():
        rng = np.random.default_rng([seed, m1, n, 53])
        R, G = _tri_int(rng, n), _tri_int(rng, n)
        return _sym_int(rng, m1, n), R, G, R @ R.T, G.T @ G
    return _keep(("exact", m1, n, seed), make)


def exact_small(m1, ns, q, seed=0):
    """(As, Xs, Zinvs, Dext, x, z) of the exact family for hs_schur_small; Dext, x, z = None for q = 0"""
    def make():
        rng = np.random.default_rng([seed, m1, q, 54] + list(ns))
        As, Xs, Zs = [], [], []
        for n in ns:
            R, G = _tri_int(rng, n), _tri_int(rng, n)
            As.append(_sym_int(rng, m1, n)); Xs.append(R @ R.T); Zs.append(G.T @ G)
        if q == 0:
            return tuple(As), tuple(Xs), tuple(Zs), None, None, None
        D = rng.integers(-3, 4, (q, m1)).astype(np.float64)
        x = rng.integers(1, 8, q).astype(np.float64)
        z = 2.0 ** rng.integers(-3, 1, q)               # x / z = x 2^k, k in 0 .. 3: an exact integer
        return tuple(As), tuple(Xs), tuple(Zs), D, x, z
    return _keep(("exact_small", m1, tuple(ns), q, seed), make)


def iterate(m1, n, cond, seed=0):
    """(A, R, G, X, Zinv) of the iterate family: X = fl(R R^T) and Zinv = fl(G^T G) are the double matrices the U forms are handed"""
    def make():
        rng = np.random.default_rng([seed, m1, n, int(round(np.log10(cond))), 55])
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        lam = cond ** (-np.arange(n) / max(n - 1, 1))
        mu = cond ** -0.5
        X = (Q * lam) @ Q.T
        Z = (Q * (mu / lam)) @ Q.T
        R = np.tril(np.linalg.cholesky(0.5 * (X + X.T)))
        Lz = np.linalg.cholesky(0.5 * (Z + Z.T))
        G = np.tril(sla.solve_triangular(Lz, np.eye(n), lower=True, check_finite=False))
        A = rng.standard_normal((m1, n, n))
        A = np.ascontiguousarray(A + A.transpose(0, 2, 1))
        Xd = R @ R.T
        Zd = G.T @ G
        return A, np.ascontiguousarray(R), np.ascontiguousarray(G), 0.5 * (Xd + Xd.T), 0.5 * (Zd + Zd.T)
    return _keep(("iterate", m1, n, cond, seed), make)


def scaling(m1, seed=0):
    """k_i in -10 .. 10 and the factors 2^k_i of the scaled family"""
    def make():
        k = np.random.default_rng([seed, m1, 56]).integers(-10, 11, m1)
        return k, 2.0 ** k
    return _keep(("scaling", m1, seed), make)


# ---- the two formulations -----------------------------------------------------------------------------------------------

def w_matrix(A, R, G, dtype=np.float64):
    """M = W W^T, W_j = G (A_j R), in the given precision"""
    A, R, G = (np.asarray(a, dtype=dtype) for a in (A, R, G))
    m1, n = A.shape[0], A.shape[1]
    T = (A.reshape(m1 * n, n) @ R).reshape(m1, n, n)
    W = np.matmul(G, T).reshape(m1, n * n)
    return W @ W.T


def u_matrix(A, X, Zinv, dtype=np.float64):
    """M_ij = <A_i, U_j>, U_j = X (A_j Zinv), in the given precision"""
    A, X, Zinv = (np.asarray(a, dtype=dtype) for a in (A, X, Zinv))
    m1, n = A.shape[0], A.shape[1]
    T = (A.reshape(m1 * n, n) @ Zinv).reshape(m1, n, n)
    U = np.matmul(X, T).reshape(m1, n * n)
    return A.reshape(m1, n * n) @ U.T


def w_chain(A, R, G):
    """B_ij = <|G||A_i||R|, |G||A_j||R|>: bounds every partial sum of the W forms"""
    return w_matrix(np.abs(A), np.abs(R), np.abs(G))


def u_chain(A, X, Zinv):
    """B_ij = <|A_i|, |X||A_j||Zinv|>: bounds every partial sum of the U forms"""
    return u_matrix(np.abs(A), np.abs(X), np.abs(Zinv))


def lp_term(Dext, x, z, dtype=np.float64):
    D = np.asarray(Dext, dtype=dtype)
    return D.T @ ((np.asarray(x, dtype=dtype) / np.asarray(z, dtype=dtype))[:, None] * D)


def small_matrix(As, Xs, Zinvs, Dext=None, x=None, z=None, dtype=np.float64):
    """sum_k tr(A_i X_k A_j Zinv_k) + Dext^T diag(x / z) Dext"""
    M = sum(u_matrix(a, b, c, dtype) for a, b, c in zip(As, Xs, Zinvs))
    return M if Dext is None else M + lp_term(Dext, x, z, dtype)


def small_chain(As, Xs, Zinvs, Dext=None, x=None, z=None):
    B = sum(u_chain(a, b, c) for a, b, c in zip(As, Xs, Zinvs))
    return B if Dext is None else B + lp_term(np.abs(Dext), x, z)


def exact_ref(m1, n, seed=0):
    """float64 numpy on an exact case (the W formulation; the U formulation gives the same integers)"""
    return _keep(("exact_ref", m1, n, seed), lambda: w_matrix(*exact(m1, n, seed)[:3]))


def exact_premise(m1, n, seed=0):
    """the largest entry of the two abs-value chains of an exact case: below 2^53 every partial sum of every form is an exactly
    represented integer"""
    def make():
        A, R, G, X, Zi = exact(m1, n, seed)
        return float(max(np.max(w_chain(A, R, G)), np.max(u_chain(A, X, Zi))))
    return _keep(("exact_premise", m1, n, seed), make)


def exact_small_premise(m1, ns, q, seed=0):
    return float(np.max(small_chain(*exact_small(m1, ns, q, seed))))


def longdouble_ok():
    """the references need a 64-bit mantissa"""
    return float(np.finfo(XD).eps) <= 2.0 ** -63


def iterate_ref(m1, n, cond, seed=0):
    """(M_ref of the W forms, its chain B, M_ref of the U forms, its chain B) in extended precision on the rounded operands"""
    def make():
        A, R, G, X, Zi = iterate(m1, n, cond, seed)
        return (w_matrix(A, R, G, XD), w_chain(A, R, G), u_matrix(A, X, Zi, XD), u_chain(A, X, Zi))
    return _keep(("iterate_ref", m1, n, cond, seed), make)


def figure(M, Mref, B):
    """F = max_ij |M - M_ref|_ij / (eps B_ij); nothing is excluded: an entry with B = 0 must be reproduced exactly"""
    D = np.abs(np.asarray(M, dtype=XD) - Mref).astype(np.float64)
    if not np.all(np.isfinite(D)):
        return float("inf")
    ok = B > 0
    if np.any(D[~ok] != 0):
        return float("inf")
    return float(np.max(D[ok] / (EPS * B[ok]))) if np.any(ok) else 0.0


def cap(n):
    """Higham's first-order constant of the three chained sums (n, n and n^2 terms) in any order"""
    return float(n * n + 2 * n + 2)


def numpy_figures(m1, n, cond, seed=0):
    """(F of float64 numpy in the W formulation, in the U formulation) on an iterate case"""
    def make():
        A, R, G, X, Zi = iterate(m1, n, cond, seed)
        Mw, Bw, Mu, Bu = iterate_ref(m1, n, cond, seed)
        return figure(w_matrix(A, R, G), Mw, Bw), figure(u_matrix(A, X, Zi), Mu, Bu)
    return _keep(("numpy_figures", m1, n, cond, seed), make)


def seq_matmul(P, Qm):
    """P @ Qm (leading batch dimensions allowed) accumulated strictly in the order k = 0, 1, 2, ... in float64"""
    out = np.zeros(np.broadcast_shapes(P.shape[:-2], Qm.shape[:-2]) + (P.shape[-2], Qm.shape[-1]))
    for k in range(P.shape[-1]):
        out += P[..., :, k, None] * Qm[..., k, None, :]
    return out


def w_matrix_seq(A, R, G):
    m1, n = A.shape[0], A.shape[1]
    W = seq_matmul(G, seq_matmul(A, R)).reshape(m1, n * n)
    return seq_matmul(W, np.ascontiguousarray(W.T))


def u_matrix_seq(A, X, Zinv):
    m1, n = A.shape[0], A.shape[1]
    U = seq_matmul(X, seq_matmul(A, Zinv)).reshape(m1, n * n)
    return seq_matmul(A.reshape(m1, n * n), np.ascontiguousarray(U.T))


# ---- the sharding and the dispatch, restated ----------------------------------------------------------------------------------

def col_slices(m1, n, parts):
    """[(c0, cw)] of hs_shard_cols for every rank of `parts` (oracle/shard_ref.py restates the partition)"""
    b = shard_ref.shard_cols(m1, n, min(parts, 64))
    return [(b[g], b[g + 1] - b[g]) for g in range(min(parts, 64))]


def row_chunks(m1, parts):
    """[(r0, r1)] of the 2 * parts calls of hs_schur_Urows in the order the unit entry issues them, clipped as the function clips"""
    out = []
    for g in range(parts):
        c, b1, b2 = shard_ref.shard_rows(m1, parts, g)
        out += [(b1, min(b1 + c, m1)), (b2, min(b2 + c, m1))]
    return out


LOWER, A_LOWTRI, B_LOWTRI, XCD, REMAP, UPPER, NOFAST, TILE64 = 1, 2, 4, 8, 16, 32, 64, 128
KC, MC = 0, 1


def _cdiv(a, b):
    return -(-a // b)


def pick_splitk(M, N, K, lower):
    tm, tn = _cdiv(M, 128), _cdiv(N, 128)
    tiles = tm * (tm + 1) // 2 if lower else tm * tn
    if tiles >= 512 or K < 1024:
        return 1
    return max(1, min(_cdiv(1024, tiles), K // 256, 64))


def pick_xcd_slices(ntile, K):
    best, widest, bestscore = 2, 2, -1.0
    for s in range(2, 129):
        if K // s < 1024 and s > 2:
            break
        widest = s
        total = ntile * s
        rounds = _cdiv(total, 512)
        score = total / (rounds * 512.0) - 0.02 * (rounds - 1)
        if total >= 256 and score > bestscore:
            bestscore, best = score, s
    return widest if bestscore < 0.0 else best


def gemm_rung(M, N, K, layB, batch, splitk, flags, lda, ldb, strideB=0, offA=0, offB=0):
    """(1 if a persistent kernel of dgemm2.hip takes the product, 1 if that is the paired-band kernel): hs_dgemm and hs_dgemm2_try with
    A K-contiguous; offA, offB: operand offsets in doubles from a 16-byte aligned allocation"""
    if M <= 0 or N <= 0:
        return 0, 0
    if splitk <= 1 and K >= 16 and M >= 2 and N >= 2 and not flags & (XCD | REMAP | TILE64):
        t64 = _cdiv(M, 64) * _cdiv(N, 64) * batch
        t32 = _cdiv(M, 32) * _cdiv(N, 32) * batch
        if t64 <= 160 and t32 <= 4096 and batch <= 65535:
            return 0, 0                                                  # the 32 x 32 kernel
    big = _cdiv(M, 128) * _cdiv(N, 128) * (splitk if splitk > 1 else batch)
    if not ((big >= 192 or flags & XCD) and not flags & TILE64):
        return 0, 0                                                      # 64-wide tiles
    if splitk > 1:
        kchunk = _cdiv(_cdiv(K, splitk), 16) * 16
        splitk = max(1, _cdiv(K, kchunk))
    if flags & UPPER or (lda | ldb | strideB | K | offA | offB) & 1 or K < 16:
        return 0, 0
    if layB == MC and (N & 1 or N < 2):
        return 0, 0
    if flags & LOWER and M != N:
        return 0, 0
    tm, tn = _cdiv(M, 128), _cdiv(N, 128)
    ntile = tm * (tm + 1) // 2 if flags & LOWER else tm * tn
    if ntile * (splitk if splitk > 1 else batch) < 384:
        return 0, 0
    triA, triB = bool(flags & A_LOWTRI), bool(flags & B_LOWTRI)
    paired = triA != triB and splitk <= 1 and not flags & (LOWER | UPPER) and not (triB and layB != MC)
    return 1, int(paired)


def _ws_slabs(m1, cols, n2max, full):
    """split-K slabs hs_schur_ws_alloc provides, in units of m1 x cols doubles"""
    sk = max(16, pick_splitk(m1, cols, n2max, 1))
    if full:
        tm = _cdiv(m1, 128)
        sk = max(sk, pick_xcd_slices(tm * (tm + 1) // 2, n2max), 64)
    return sk


def _gram_product(m1, K, slabs, xcd, has_plan, used):
    """Mx += V V^T over K: the Gram kernel when it has a plan (64 slabs of m1^2 are there in every full workspace), else the tile
    kernels in the slabs schur_syrk_shape / hs_schur_W choose"""
    if slabs >= 2 and m1 >= 256 and K >= 16384 and not K & 1 and has_plan(m1, K):
        used[2] += 1
        return
    tm = _cdiv(m1, 128)
    if xcd and slabs >= 2:
        sk, flags = min(max(pick_xcd_slices(tm * (tm + 1) // 2, K), 2), slabs), LOWER | XCD | NOFAST
    else:
        sk, flags = min(pick_splitk(m1, m1, K, 1), slabs), LOWER
    t2, t5 = gemm_rung(m1, m1, K, KC, 1, sk, flags, K, K)
    used[0] += t2; used[1] += t5


def predict_used(form, m1, n, parts=1, ws_gbytes=0.0, has_plan=lambda M, K: False):
    """used[3] of hipsdp_schur_form_unit: the products of the call the persistent kernels take, of these the paired-band kernel's, and the
    Gram kernel's.  has_plan(M, K): whether gram.hip has a plan for the shape (hipsdp_gram_plan_info with 64 slabs; device code decides)"""
    used = [0, 0, 0]
    n2 = n * n

    def add(*a, **k):
        t2, t5 = gemm_rung(*a, **k)
        used[0] += t2; used[1] += t5

    if form == 0:
        add(m1 * n, n, n, MC, 1, 1, B_LOWTRI, n, n)
        add(n, n, n, MC, m1, 1, A_LOWTRI | REMAP, n, n, strideB=n2)
        _gram_product(m1, n2, _ws_slabs(m1, m1, n2, True), m1 >= 256 and n2 >= 16384 and (n2 >= 50000 or m1 >= 900), has_plan, used)
    elif form == 1:
        sl = col_slices(m1, n, parts)
        slabs = _ws_slabs(m1, m1, max([n * cw for _, cw in sl] + [1]), True)
        for c0, cw in sl:
            if cw <= 0:
                continue
            nk, narrow = n * cw, (TILE64 if cw <= 64 else 0)
            add(m1 * n, cw, n - c0, MC, 1, 1, B_LOWTRI | narrow, n, n, offA=c0, offB=c0 * n + c0)
            add(n, cw, n, MC, m1, 1, A_LOWTRI | REMAP | narrow, n, cw, strideB=nk)
            _gram_product(m1, nk, slabs, m1 >= 256 and nk >= 16384, has_plan, used)
    elif form in (2, 3):
        full = not (form == 3 and ws_gbytes > 0.0 and 16.0 * m1 * n2 > ws_gbytes * 1e9)
        cols = m1
        chunk = m1
        if not full:
            cols = min(m1, max(128, int(ws_gbytes * 1e9 / (16.0 * n2)) // 128 * 128))
            chunk = min(cols, max(1, int(ws_gbytes * 1e9 / (16.0 * n2))))
        kws = _ws_slabs(m1, cols, n2, full) * m1 * cols
        if form == 2:
            pieces = [(r0, r1 - r0) for r0, r1 in row_chunks(m1, parts) if r1 > r0]
        else:
            pieces = [(j0, min(chunk, m1 - j0)) for j0 in range(0, m1, chunk)]
        for r0, cj in pieces:
            add(cj * n, n, n, MC, 1, 1, REMAP, n, n, offA=r0 * n2)
            add(n, n, n, MC, cj, 1, REMAP, n, n, strideB=n2)
            if form == 2:
                continue                                                 # HS_GEMM_UPPER: never a persistent kernel
            rows = m1 - r0
            sk = pick_splitk(rows, cj, n2, 1)
            while sk > 1 and sk * rows * cj > kws:
                sk -= 1
            add(rows, cj, n2, KC, 1, sk, LOWER, n2, n2, offA=r0 * n2)
    else:
        cwmax = min(parts, n)
        tm = _cdiv(m1, 128)
        slabs = max(16, pick_splitk(m1, m1, n * cwmax, 1), pick_xcd_slices(tm * (tm + 1) // 2, n * cwmax), 64)
        for c0 in range(0, n, cwmax):
            cw = min(cwmax, n - c0)
            nk = n * cw
            add(m1 * n, cw, n - c0, MC, 1, 1, B_LOWTRI, n, n, offA=c0, offB=c0 * n + c0)
            add(n, cw, n, MC, m1, 1, REMAP, n, cw, strideB=nk)
            _gram_product(m1, nk, slabs, m1 >= 256 and nk >= 16384, has_plan, used)
    return tuple(used)


def small_admitted(m1, ns, q):
    """hs_schur_small's admission rule"""
    return (len(ns) <= 8 and 1 <= m1 <= 1024 and q * m1 <= 2000000 and sum(0.5 * m1 * m1 * n * n for n in ns) <= SMALL_WORK
            and all(1 <= n <= SMALL_NMAX for n in ns))


# ---- figures ------------------------------------------------------------------------------------------------------------

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


def first_difference(M, ref):
    """None when the two matrices hold the same bits, else (differing entries, first (i, j), the two values) and where that entry
    lies: its 128-, 64- and 32-wide tile"""
    a = np.ascontiguousarray(M, dtype=np.float64)
    b = np.ascontiguousarray(ref, dtype=np.float64)
    d = a.view(np.uint64) != b.view(np.uint64)
    if not np.any(d):
        return None
    i, j = (int(v[0]) for v in np.nonzero(d))
    return "%d entries differ, first (%d, %d): %r against %r; tiles 128: (%d, %d), 64: (%d, %d), 32: (%d, %d)" % (
        int(np.sum(d)), i, j, float(a[i, j]), float(b[i, j]), i // 128, j // 128, i // 64, j // 64, i // 32, j // 32)
