"""GPU: hipsdp_rounding_frame / hipsdp_rounding_recombine - the two device stages of the primal rounding problem (csrc/rounding.hip, the
expand / recombine / write launches of csrc/psd_many.hip and csrc/psd_large.hip, host side in csrc/cut_calls.hip) - against the
numpy restatement tests/harness/roundprob_ref.py, against the eigen entries that serve one matrix, and for what makes it a batch.

Bounds (all derived, none measured).
  eigenpairs       the header's contract: eigenvalues within 1e-12 max |lambda| of numpy's eigvalsh, residuals within 1e-9 max |lambda|,
                   orthonormality within 1e-11; bit-equal to hipsdp_syev_small (up to 128 rows) / hipsdp_syevr (above) on the expanded X.
  coefficients     against an np.longdouble evaluation on the RETURNED vectors: (L + 4) 2^-53 sum_p |w_p A_p v_r v_c| per entry, L = the
                   stored entries summed (n^2 dense rows, n (n + 1) / 2 packed, the nonzero count) - the first-order rounding bound of a
                   sum of L products of three rounded factors in any order, so it covers the matrix-core accumulation and the K slices.
  against X        |sum_j lambda_j coefs[j][i] - <A_i, X>| <= 2 (sqrt(n) 1e-9 + n 1e-11) max |lambda| ||A_i||_F + sum_j |lambda_j| bound[j][i]
                   |sum_j coefs[j][i] - tr A_i| <= 2 n 1e-11 ||A_i||_F + sum_j bound[j][i]
  stage 2          (n + 4) 2^-53 sum_k |lambda_k v_k[i] v_k[j]| against the longdouble restatement on the returned vectors; the kept
                   entries are compared as lists after asserting that no restatement value lies between 1e-11 and 1e-7 (epsilon = 1e-9).

Storage forms as tests/test_gpu_check_y_many.py makes them: dense-loaded (dense rows up to 64 rows, packed triangles above) and triplets
under sparse_policy(2) (nonzeros)."""
import ctypes as C
import threading
import numpy as np
import pytest
import ipm_ref
import roundprob_ref as ref

pytestmark = pytest.mark.gpu

ERR_ARG = 3
EDGES = [1, 3, 17, 64, 65, 128, 129, 130]
MS = [1, 5, 64, 70]
KINDS = ["random", "lowrank", "zero", "diag"]
U = 2.0 ** -53
EPS = 1e-9


def sym(rng, n):
    R = rng.standard_normal((n, n))
    return (R + R.T) / 2.0


def matrices(ns, m, seed=0):
    rng = np.random.default_rng([seed, m, len(ns)])
    return [np.stack([sym(rng, n) / np.sqrt(n) for _ in range(m + 1)]) for n in ns]


def xmat(kind, n, rng):
    if kind == "random":
        return sym(rng, n) / np.sqrt(n)
    if kind == "lowrank":
        r = max(1, n // 3)
        Uu = rng.standard_normal((n, r)) / np.sqrt(n)
        return Uu @ Uu.T + 0.25 * np.eye(n)
    if kind == "zero":
        return None
    return np.diag(rng.uniform(-1.0, 1.0, n))


def xlist(kind, ns, seed=0):
    rng = np.random.default_rng([seed, KINDS.index(kind), len(ns)])
    return [xmat(kind, n, rng) for n in ns]


def dense(X, n):
    return np.zeros((n, n)) if X is None else X


def load(hb, blocks, m, form, units=False):
    """form 'dense': dense input (dense rows up to 64 rows, packed triangles above); 'sparse': triplets, every block kept as nonzeros"""
    s = hb.Solver(0, units=units)
    if form == "dense":
        s.load_core(ipm_ref.CoreProblem(np.zeros(m), blocks, None, None))
        for k in range(len(blocks)):
            assert not s.is_sparse(k), k
        return s
    s.sparse_policy(2)
    trip = []
    for A in blocks:
        n = A.shape[1]
        il = np.tril_indices(n)
        var = np.repeat(np.arange(m + 1, dtype=np.int32), len(il[0]))
        row = np.tile(il[0].astype(np.int32), m + 1)
        col = np.tile(il[1].astype(np.int32), m + 1)
        val = np.concatenate([A[i][il] for i in range(m + 1)])
        keep = val != 0.0
        trip.append((var[keep], row[keep], col[keep], val[keep]))
    s.set_shape(m, [A.shape[1] for A in blocks], 0, nnz=[len(t[3]) for t in trip])
    s.set_obj(np.zeros(m))
    for k, t in enumerate(trip):
        s.add_entries(k, *t)
    for k in range(len(blocks)):
        assert s.is_sparse(k), k
    return s


def entries(form, A, i):
    """stored entries summed for matrix i of a block in the form the engine holds it in"""
    n = A.shape[1]
    if form == "dense":
        return n * n if n <= 64 else n * (n + 1) // 2
    return n * n if i == 0 else int(np.count_nonzero(np.tril(A[i])))


def bound2(form, V, A):
    L = np.array([entries(form, A, i) for i in range(A.shape[0])], dtype=np.float64)
    Va = np.abs(V).astype(np.longdouble)
    mag = np.einsum("jr,irc,jc->ji", Va, np.abs(A).astype(np.longdouble), Va)
    return np.asarray((L[None, :] + 4) * U * mag, dtype=np.float64)


def split(ns, eig, obj, coefs, vecs):
    """per block (lam[n], table[n, m + 1], V[n, n])"""
    out, o, vo = [], 0, 0
    for n in ns:
        V = vecs[vo:vo + n * n].reshape(n, n) if vecs is not None else None
        out.append((eig[o:o + n], np.concatenate([obj[o:o + n, None], coefs[o:o + n]], axis=1), V))
        o += n
        vo += n * n
    return out


def hexes(a):
    return [float(v).hex() for v in np.asarray(a).reshape(-1)]


_CASES = {}


def case(gpu, form, m, kind, ns=tuple(EDGES)):
    """ONE call per (form, m, kind), shared by the tests that look at it; nothing of it is changed afterwards"""
    key = (form, m, kind, ns)
    if key not in _CASES:
        blocks = matrices(ns, m)
        X = xlist(kind, ns)
        s = load(gpu, blocks, m, form)
        eig, obj, coefs, vecs, served = s.rounding_frame(X)
        s.close()
        assert list(served) == [0] * len(ns)
        _CASES[key] = (blocks, X, split(ns, eig, obj, coefs, vecs))
    return _CASES[key]


def one_matrix_pairs(gpu, M):
    """hipsdp_syev_small up to 128 rows, hipsdp_syevr above, on the expanded matrix alone"""
    n = M.shape[0]
    M = np.ascontiguousarray(M, dtype=np.float64)
    lam, V = np.zeros(n), np.zeros((n, n))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    f = gpu.lib().hipsdp_syev_small if n <= 128 else gpu.lib().hipsdp_syevr
    assert f(0, n, dp(M), dp(lam), dp(V)) == 0
    return lam, V


def check_pairs(lam, V, M, what):
    n = M.shape[0]
    w = np.linalg.eigvalsh(M)
    top = max(abs(w[0]), abs(w[-1]))
    if top == 0.0:
        assert np.all(np.abs(lam) < 1e-200), what
    else:
        e1 = np.max(np.abs(lam - w)) / top
        e2 = np.max(np.linalg.norm(V @ M - lam[:, None] * V, axis=1)) / top
        print("%s n = %3d: eigenvalues %.3g, residuals %.3g of max |lambda|" % (what, n, e1, e2))
        assert e1 <= 1e-12 and e2 <= 1e-9, (what, n, e1, e2)
    assert np.all(np.diff(lam) >= 0.0), what
    e3 = np.max(np.abs(V @ V.T - np.eye(n)))
    assert e3 <= 1e-11, (what, n, e3)


# ---- 1. eigenpairs ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
def test_eigenpairs_are_those_of_the_one_matrix_entries_and_meet_the_contract(gpu, kind):
    blocks, X, got = case(gpu, "dense", 1, kind)
    for n, Xb, (lam, _, V) in zip(EDGES, X, got):
        M = dense(Xb, n)
        l1, V1 = one_matrix_pairs(gpu, M)
        assert hexes(lam) == hexes(l1) and hexes(V) == hexes(V1), (kind, n)
        check_pairs(lam, V, M, kind)


# ---- 2. coefficients against the returned vectors -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("m", MS)
def test_coefficients_match_longdouble_on_the_returned_vectors(gpu, m, form):
    blocks, X, got = case(gpu, form, m, "random")
    for n, A, (lam, tab, V) in zip(EDGES, blocks, got):
        want = ref.coefficients_einsum(V, A)
        b = bound2(form, V, A)
        err = np.abs(np.asarray(tab, dtype=np.longdouble) - want).astype(np.float64)
        print("%s m = %d n = %3d: largest error / bound = %.3g" % (form, m, n, float(np.max(err / np.maximum(b, 1e-300)))))
        assert np.all(err <= b), (form, m, n, float(np.max(err / np.maximum(b, 1e-300))))


@pytest.mark.parametrize("m", [3, 70])
def test_a_single_block_of_512_rows(gpu, m):
    """all entries against a float64 evaluation (whose own rounding bound, (2 n + 8) 2^-53 of the same magnitudes, is added), 16 vectors
    against np.longdouble with the bound alone; the eigenpairs are hipsdp_syevr's, bit for bit"""
    n = 512
    blocks, X, got = case(gpu, "dense", m, "random", ns=(n,))
    lam, tab, V = got[0]
    A = blocks[0]
    l1, V1 = one_matrix_pairs(gpu, X[0])
    assert hexes(lam) == hexes(l1) and np.array_equal(V, V1)
    check_pairs(lam, V, X[0], "512 rows")
    L = n * (n + 1) // 2
    Va = np.abs(V)
    mag = np.stack([np.sum((Va @ np.abs(A[i])) * Va, axis=1) for i in range(m + 1)], axis=1)
    f64 = np.stack([np.sum((V @ A[i]) * V, axis=1) for i in range(m + 1)], axis=1)
    assert np.all(np.abs(tab - f64) <= ((L + 4) + (2 * n + 8)) * U * mag)
    rows = np.unique(np.concatenate([[0, n - 1], np.random.default_rng(m).integers(0, n, 14)]))
    want = ref.coefficients_einsum(V[rows], A)
    err = np.abs(np.asarray(tab[rows], dtype=np.longdouble) - want).astype(np.float64)
    print("512 rows, m = %d: largest error / bound on %d vectors = %.3g" % (m, len(rows), float(np.max(err / ((L + 4) * U * mag[rows])))))
    assert np.all(err <= (L + 4) * U * mag[rows])


# ---- 3. basis-free checks against X itself ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("kind", ["random", "lowrank"])
def test_sums_over_the_vectors_give_trace_and_inner_product(gpu, kind, form):
    m = 5
    blocks, X, got = case(gpu, form, m, kind)
    for n, A, Xb, (lam, tab, V) in zip(EDGES, blocks, X, got):
        b = bound2(form, V, A)
        top = float(np.max(np.abs(lam)))
        fro = np.array([np.linalg.norm(A[i]) for i in range(m + 1)])
        inner = np.array([float(np.sum(A[i].astype(np.longdouble) * Xb.astype(np.longdouble))) for i in range(m + 1)])
        tr = np.array([float(np.sum(np.diag(A[i]).astype(np.longdouble))) for i in range(m + 1)])
        t = np.asarray(tab, dtype=np.longdouble)
        e1 = np.abs(np.asarray(np.sum(np.asarray(lam, dtype=np.longdouble)[:, None] * t, axis=0), dtype=np.float64) - inner)
        e2 = np.abs(np.asarray(np.sum(t, axis=0), dtype=np.float64) - tr)
        assert np.all(e1 <= 2 * (np.sqrt(n) * 1e-9 + n * 1e-11) * top * fro + np.abs(lam) @ b), (kind, form, n)
        assert np.all(e2 <= 2 * n * 1e-11 * fro + np.sum(b, axis=0)), (kind, form, n)


# ---- 4. the unit entry: the coefficient launches alone ------------------------------------------------------------------------------------

def int_matrices(n, m, rng, lo=-3, hi=4):
    A = rng.integers(lo, hi, (m + 1, n, n)).astype(np.float64)
    return np.tril(A) + np.transpose(np.tril(A, -1), (0, 2, 1))


def signed_permutation(n, rng):
    pi = rng.permutation(n)
    V = np.zeros((n, n))
    V[np.arange(n), pi] = rng.choice([-1.0, 1.0], n)
    return V, pi


def unit(gpu, V, A, form):
    """form 0 dense rows, 1 packed, 2 nonzeros; returns (table, route, slices)"""
    if form < 2:
        return gpu.rounding_coefs_unit(V, A, form)
    n, m = A.shape[1], A.shape[0] - 1
    var, row, col, val = [], [], [], []
    for i in range(1, m + 1):
        r, c = np.nonzero(np.tril(A[i]))
        var += [i] * len(r); row += list(r); col += list(c); val += list(A[i][r, c])
    return gpu.rounding_coefs_unit(V, A[0], 2, nonzeros=(m, np.array(var, dtype=np.int32), np.array(row, dtype=np.int32),
                                                         np.array(col, dtype=np.int32), np.array(val, dtype=np.float64)))


@pytest.mark.parametrize("n,form,route", [(65, 0, 1), (65, 1, 1), (129, 0, 1), (129, 1, 1), (130, 0, 1), (130, 1, 1),
                                          (3, 0, 0), (3, 1, 0), (3, 2, 0), (17, 0, 0), (17, 1, 0), (17, 2, 0), (64, 0, 0), (64, 1, 0),
                                          (64, 2, 0), (130, 2, 0)])
@pytest.mark.parametrize("m", [1, 70])
def test_unit_identity_and_signed_permutation_are_exact(gpu, n, form, route, m):
    rng = np.random.default_rng([n, form, m])
    A = int_matrices(n, m, rng)
    tab, rt, slices = unit(gpu, np.eye(n), A, form)
    assert rt == route and (slices == 1 or route == 1)
    assert np.array_equal(tab, np.stack([np.diag(A[i]) for i in range(m + 1)], axis=1)), (n, form, m)
    V, pi = signed_permutation(n, rng)
    tab, rt, _ = unit(gpu, V, A, form)
    assert rt == route
    assert np.array_equal(tab, np.stack([np.diag(A[i])[pi] for i in range(m + 1)], axis=1)), (n, form, m)


def hadamard(n):
    H = np.array([[1.0]])
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


@pytest.mark.parametrize("n,forms", [(64, (0, 1, 2)), (128, (0, 1, 2)), (256, (0, 1))])
def test_unit_vectors_of_plus_minus_one_over_sqrt_n(gpu, n, forms):
    """V = H / sqrt(n), H a Sylvester matrix (orthogonal rows of +-1), matrices with entries 0 / +-1: every term of a sum is +-w t with
    t = fl(fl(1 / sqrt(n))^2).  For n = 64 and 256 (1 / sqrt(n) a power of two) t = 1 / n and every partial sum is a multiple of 1 / n
    far below 2^53 / n: the coefficients are EXACTLY the integer sums over n, whatever the order.  For n = 128, 1 / sqrt(128) is not a
    binary64 number and fl(.)^2 = (1 + 2^-52) / 128, so exactness in k / n cannot hold for any kernel; there the table must lie within
    the bound of test 2 of the longdouble evaluation on the rounded V, and n = 256 takes its place on the matrix-core route."""
    m = 5
    rng = np.random.default_rng(n)
    A = int_matrices(n, m, rng, -1, 2)
    s = 1.0 / np.sqrt(n)
    V = hadamard(n) * s
    H = hadamard(n)
    exact = np.stack([np.sum((H @ A[i]) * H, axis=1) for i in range(m + 1)], axis=1)          # integers, exact in float64
    for form in forms:
        tab, route, _ = unit(gpu, V, A, form)
        assert route == (1 if n > 64 and form < 2 else 0)
        if n != 128:
            assert np.array_equal(tab * n, exact), (n, form)
            assert np.array_equal(tab, exact / n), (n, form)
        else:
            L = {0: n * n, 1: n * (n + 1) // 2}.get(form)
            Ls = np.array([n * n] + [int(np.count_nonzero(np.tril(A[i]))) for i in range(1, m + 1)]) if form == 2 else np.full(m + 1, L)
            Va = np.abs(V).astype(np.longdouble)
            mag = np.einsum("jr,irc,jc->ji", Va, np.abs(A).astype(np.longdouble), Va)
            err = np.abs(np.asarray(tab, dtype=np.longdouble) - ref.coefficients_einsum(V, A))
            assert np.all(np.asarray(err, dtype=np.float64) <= np.asarray((Ls[None, :] + 4) * U * mag, dtype=np.float64)), (n, form)


# ---- 5. the forms agree -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [5, 70])
def test_dense_loaded_and_triplet_loaded_blocks_agree(gpu, m):
    _, _, gd = case(gpu, "dense", m, "random")
    blocks, _, gs = case(gpu, "sparse", m, "random")
    for n, A, (ld, td, Vd), (ls, ts, Vs) in zip(EDGES, blocks, gd, gs):
        assert hexes(ld) == hexes(ls) and hexes(Vd) == hexes(Vs), n                    # the same X: the same pairs
        assert np.all(np.abs(td - ts) <= bound2("dense", Vd, A) + bound2("sparse", Vd, A)), n


# ---- 6. independence, bit for bit ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_the_bits_of_a_block_do_not_depend_on_the_other_blocks_their_order_or_the_chunks(gpu, form, monkeypatch):
    """m = 1: the block of 130 rows runs in K slices"""
    monkeypatch.delenv("HIPSDP_ROUNDING_CHUNK", raising=False)
    m = 1
    blocks, X = matrices(EDGES, m, seed=3), xlist("random", EDGES, seed=3)
    s = load(gpu, blocks, m, form)
    first = s.rounding_frame(X)
    again = s.rounding_frame(X)
    for a, b in zip(first[:4], again[:4]):
        assert hexes(a) == hexes(b)                                                    # same input, same bits
    base = split(EDGES, *first[:4])
    lam_all = first[0]
    r0 = s.rounding_recombine(lam_all, EPS, 1)
    monkeypatch.setenv("HIPSDP_ROUNDING_CHUNK", "1")
    st0 = gpu.rounding_stats()
    one = s.rounding_frame(X)
    st1 = gpu.rounding_stats()
    r1 = s.rounding_recombine(lam_all, EPS, 1)
    st2 = gpu.rounding_stats()
    monkeypatch.delenv("HIPSDP_ROUNDING_CHUNK")
    for a, b in zip(first[:4], one[:4]):
        assert hexes(a) == hexes(b)
    assert st1[0] - st0[0] == 1 and st1[2] - st0[2] == len(EDGES) and st2[2] - st1[2] == len(EDGES)
    assert st1[1] - st0[1] == sum(frame_formula([n]) for n in EDGES) and st2[1] - st1[1] == 2 * len(EDGES)
    for a, b in zip(r0, r1):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    s.close()
    perm = [5, 2, 7, 0, 3, 6, 1, 4]
    s = load(gpu, [blocks[k] for k in perm], m, form)
    got = split([EDGES[k] for k in perm], *s.rounding_frame([X[k] for k in perm])[:4])
    s.close()
    for pos, k in enumerate(perm):
        for a, b in zip(base[k], got[pos]):
            assert hexes(a) == hexes(b), (form, EDGES[k])
    for k, n in enumerate(EDGES):                                                      # alone in a solver
        s = load(gpu, [blocks[k]], m, form)
        got = split([n], *s.rounding_frame([X[k]])[:4])[0]
        s.close()
        for a, b in zip(base[k], got):
            assert hexes(a) == hexes(b), (form, n)


# ---- 7. launches and read-backs -----------------------------------------------------------------------------------------------------------

def frame_formula(ns):
    small = any(n <= 128 for n in ns)
    nmax = max([n for n in ns if 128 < n <= 512], default=0)
    return (4 if small else 0) + (nmax + 6 + 6 * -(-nmax // 32) if nmax else 0) + 4


def recombine_formula(ns):
    return (2 if any(n <= 128 for n in ns) else 0) + (2 if any(128 < n <= 512 for n in ns) else 0)


@pytest.mark.parametrize("one,eight", [([12], [12, 3, 100, 64, 65, 128, 1, 17]), ([130], [130, 129, 130, 129, 130, 130, 129, 130]),
                                       ([17, 130], [17, 130, 3, 64, 65, 128, 129, 1])])
def test_launches_and_readbacks_are_the_formula(gpu, one, eight, monkeypatch):
    monkeypatch.delenv("HIPSDP_ROUNDING_CHUNK", raising=False)
    m = 2
    deltas = []
    for ns in (one, eight):
        s = load(gpu, matrices(ns, m, seed=6), m, "dense")
        others = (gpu.eigencuts_all_stats(), gpu.eigencuts_all_large_stats(), gpu.check_y_many_stats(), gpu.psd_project_many_stats(),
                  gpu.psd_project_many_large_stats())
        st0 = gpu.rounding_stats()
        eig = s.rounding_frame(xlist("random", ns, seed=6))[0]
        st1 = gpu.rounding_stats()
        s.rounding_recombine(eig, EPS, 0)
        st2 = gpu.rounding_stats()
        assert others == (gpu.eigencuts_all_stats(), gpu.eigencuts_all_large_stats(), gpu.check_y_many_stats(),
                          gpu.psd_project_many_stats(), gpu.psd_project_many_large_stats())
        deltas.append((tuple(b - a for a, b in zip(st0, st1)), tuple(b - a for a, b in zip(st1, st2))))
        assert deltas[-1] == ((1, frame_formula(ns), 1), (1, recombine_formula(ns), 1)), (ns, deltas[-1])
        st0 = gpu.rounding_stats()                                                     # ... and the reverse
        s.check_y_many(np.zeros((1, m)))
        assert gpu.rounding_stats() == st0
        s.close()
    print("blocks %s / %s: (calls, launches, read-backs) per stage %s" % (one, eight, deltas))
    assert deltas[0] == deltas[1]


# ---- 8. stage 2 ----------------------------------------------------------------------------------------------------------------------------

def check_recombination(out, Vs, lams, ns, mode, what):
    o = 0
    for n, V, got in zip(ns, Vs, out):
        lam = lams[o:o + n]
        o += n
        want = ref.recombine(V, lam, mode, dtype=np.longdouble)
        mags = np.abs(np.asarray(want, dtype=np.float64))
        assert not np.any((mags > 1e-11) & (mags < 1e-7)), (what, n)                   # first: no value near epsilon
        r, c, v = ref.kept(np.asarray(want, dtype=np.float64), EPS)
        assert np.array_equal(got[0], r) and np.array_equal(got[1], c), (what, n, mode)
        b = ref.recombine_bound(V, lam, mode)[r, c]
        err = np.abs(np.asarray(got[2], dtype=np.longdouble) - want[r, c]).astype(np.float64)
        assert np.all(err <= b), (what, n, mode, float(np.max(err / np.maximum(b, 1e-300))))


@pytest.mark.parametrize("mode", [0, 1])
def test_recombinations_match_the_restatement_on_the_returned_vectors(gpu, mode):
    m = 1
    blocks, X = matrices(EDGES, m, seed=8), xlist("random", EDGES, seed=8)
    s = load(gpu, blocks, m, "dense")
    eig, _, _, vecs, _ = s.rounding_frame(X)
    Vs = [g[2] for g in split(EDGES, eig, np.zeros_like(eig), np.zeros((len(eig), m)), vecs)]
    rng = np.random.default_rng(mode)
    lam_pos = rng.uniform(0.5, 2.0, len(eig))
    rx = s.rounding_recombine(lam_pos, EPS, mode)                                      # the X of the reference ...
    rz = s.rounding_recombine(eig, EPS, mode)                                          # ... and a second one on the same frame
    r0 = s.rounding_recombine(np.zeros(len(eig)), EPS, mode)
    check_recombination(rx, Vs, lam_pos, EDGES, mode, "lambda >= 0")
    check_recombination(rz, Vs, eig, EDGES, mode, "the frame's eigenvalues")
    assert all(len(g[0]) == 0 and len(g[1]) == 0 and len(g[2]) == 0 for g in r0)       # lambda = 0: nothing is kept
    if mode == 1:
        # the frame's own eigenvalues reproduce X: what the header's residual and orthonormality bounds allow for ||X - V^T L V||_F
        offs = np.concatenate([[0], np.cumsum(EDGES)])
        for k, (n, Xb, V, got) in enumerate(zip(EDGES, X, Vs, rz)):
            R = np.zeros((n, n))
            R[got[0], got[1]] = got[2]
            top = float(np.max(np.abs(eig[offs[k]:offs[k + 1]])))
            lim = 2 * (np.sqrt(n) * 1e-9 + n * 1e-11) * top + EPS * n
            assert np.linalg.norm(np.triu(R) - np.triu(Xb)) <= lim, n
    # writing a constraint matrix does not invalidate the frame
    s.add_entries(0, np.array([1], dtype=np.int32), np.array([0], dtype=np.int32), np.array([0], dtype=np.int32), np.array([0.5]))
    rx2 = s.rounding_recombine(lam_pos, EPS, mode)
    for a, b in zip(rx, rx2):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # one block over its cap: the needed length, HIPSDP_ERR_ARG, the others written
    caps = [n * (n + 1) // 2 for n in EDGES]
    caps[4] = 7
    rc, out = s.rounding_recombine(lam_pos, EPS, mode, caps=caps, raw=True)
    assert rc == ERR_ARG and out[4] == len(rx[4][0])
    for k in range(len(EDGES)):
        if k != 4:
            assert all(np.array_equal(x, y) for x, y in zip(out[k], rx[k])), k
    # a new shape ends the frame
    s.set_shape(m, EDGES, 0)
    rc, _ = s.rounding_recombine(lam_pos, EPS, mode, raw=True)
    assert rc == ERR_ARG
    s.close()
    fresh = load(gpu, matrices([3], 1), 1, "dense")                                    # no frame yet
    rc, _ = fresh.rounding_recombine(np.zeros(3), EPS, mode, raw=True)
    assert rc == ERR_ARG
    fresh.close()


def test_a_recombination_of_a_512_row_block(gpu):
    n, m = 512, 1
    s = load(gpu, matrices([n], m, seed=9), m, "dense")
    X = xlist("random", [n], seed=9)
    eig, _, _, vecs, _ = s.rounding_frame(X)
    V = vecs.reshape(n, n)
    for mode in (0, 1):
        out = s.rounding_recombine(eig, EPS, mode)
        check_recombination(out, [V], eig, [n], mode, "512 rows")
    s.close()


# ---- 9. refusals and errors ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [[513, 12], [12, 513]])
def test_a_block_of_513_rows_is_turned_away_and_the_other_is_served(gpu, ns):
    m = 1
    blocks = matrices(ns, m, seed=4)
    X = xlist("random", ns, seed=4)
    s = load(gpu, blocks, m, "dense")
    eig, obj, coefs, vecs, served = s.rounding_frame(X, fill=-777.25)
    out = s.rounding_recombine(np.where(eig == -777.25, 0.0, eig), EPS, 1)
    s.close()
    got = split(ns, eig, obj, coefs, vecs)
    big, small = ns.index(513), ns.index(12)
    assert list(served) == [(-1 if n == 513 else 0) for n in ns]
    assert all(np.all(a == -777.25) for a in got[big])
    assert out[big] is None and out[small] is not None
    check_pairs(got[small][0], got[small][2], X[small], "beside 513 rows")
    want = ref.coefficients_einsum(got[small][2], blocks[small])
    assert np.all(np.abs(np.asarray(got[small][1], dtype=np.longdouble) - want) <= bound2("dense", got[small][2], blocks[small]))


def test_argument_errors_with_a_solver(gpu):
    lib = gpu.lib()
    ns, m = [3, 4], 2
    s = load(gpu, matrices(ns, m), m, "dense")
    PI, PD = C.POINTER(C.c_int), C.POINTER(C.c_double)
    row = [np.array([0, 1, 1], dtype=np.int32), np.array([3], dtype=np.int32)]
    col = [np.array([0, 0, 1], dtype=np.int32), np.array([3], dtype=np.int32)]
    val = [np.array([1.0, 0.5, 2.0]), np.array([1.0])]
    cnt = np.array([3, 1], dtype=np.int32)
    rows, cols, vals = (PI * 2)(), (PI * 2)(), (PD * 2)()

    def fill():
        cnt[:] = [3, 1]
        row[1][0] = 3
        for b in range(2):
            rows[b], cols[b], vals[b] = row[b].ctypes.data_as(PI), col[b].ctypes.data_as(PI), val[b].ctypes.data_as(PD)

    eig, obj, coefs, vecs = np.full(7, 7.0), np.full(7, 7.0), np.full((7, m), 7.0), np.full(25, 7.0)
    sv = np.full(2, 77, dtype=np.int32)
    dp, ip = (lambda a: a.ctypes.data_as(PD)), (lambda a: a.ctypes.data_as(PI))
    f = lib.hipsdp_rounding_frame
    st0 = gpu.rounding_stats()
    fill()
    assert f(None, ip(cnt), rows, cols, vals, dp(eig), dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    assert f(s.h, None, rows, cols, vals, dp(eig), dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    assert f(s.h, ip(cnt), rows, cols, vals, None, dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    assert f(s.h, ip(cnt), rows, cols, vals, dp(eig), None, dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    assert f(s.h, ip(cnt), rows, cols, vals, dp(eig), dp(obj), None, dp(vecs), ip(sv)) == ERR_ARG
    for arr in (rows, cols, vals):
        fill()
        arr[1] = None
        assert f(s.h, ip(cnt), rows, cols, vals, dp(eig), dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    assert f(s.h, ip(cnt), None, cols, vals, dp(eig), dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    fill()
    cnt[1] = -1
    assert f(s.h, ip(cnt), rows, cols, vals, dp(eig), dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    for bad in (4, -1):
        fill()
        row[1][0] = bad
        assert f(s.h, ip(cnt), rows, cols, vals, dp(eig), dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    fresh = gpu.Solver(0)                                                              # a solver without a shape
    fill()
    assert f(fresh.h, ip(cnt), rows, cols, vals, dp(eig), dp(obj), dp(coefs), dp(vecs), ip(sv)) == ERR_ARG
    fresh.close()
    assert gpu.rounding_stats() == st0
    assert np.all(eig == 7.0) and np.all(obj == 7.0) and np.all(coefs == 7.0) and np.all(vecs == 7.0) and list(sv) == [77, 77]
    fill()
    assert f(s.h, ip(cnt), rows, cols, vals, dp(eig), dp(obj), dp(coefs), None, None) == 0          # vecs and served may be NULL
    assert np.all(eig != 7.0) and np.all(vecs == 7.0)
    assert abs(eig[6] - 1.0) <= 1e-12 and np.all(np.abs(eig[3:6]) <= 1e-12)            # block 1: diag(0, 0, 0, 1)
    # stage 2: its own argument errors
    g = lib.hipsdp_rounding_recombine
    tab = (gpu.RoundingOut * 2)()
    lam = np.zeros(7)
    assert g(s.h, None, C.c_double(EPS), 0, tab) == ERR_ARG and g(s.h, dp(lam), C.c_double(EPS), 0, None) == ERR_ARG
    assert g(s.h, dp(lam), C.c_double(EPS), 2, tab) == ERR_ARG and g(None, dp(lam), C.c_double(EPS), 0, tab) == ERR_ARG
    tab[0].cap = -1
    assert g(s.h, dp(lam), C.c_double(EPS), 0, tab) == ERR_ARG
    tab[0].cap = 3                                                                      # (no output arrays)
    assert g(s.h, dp(lam), C.c_double(EPS), 0, tab) == ERR_ARG
    tab[0].cap = 0
    assert g(s.h, dp(lam), C.c_double(EPS), 0, tab) == 0 and tab[0].nnz_out == 0 and tab[1].nnz_out == 0
    s.close()


def test_a_solver_with_a_communicator_is_not_served(gpu):
    lib = gpu.lib()
    ns, m = [3, 12], 2
    s = gpu.Solver(0)
    comm = C.c_void_p()
    assert lib.hipsdp_comm_create_null(0, 2, C.byref(comm)) == 0
    assert lib.hipsdp_set_comm(s.h, comm, 0, 2) == 0
    s.load_core(ipm_ref.CoreProblem(np.zeros(m), matrices(ns, m), None, None))
    st0 = gpu.rounding_stats()
    eig, obj, coefs, vecs, served = s.rounding_frame(xlist("random", ns), fill=-5.5)
    assert list(served) == [-1, -1] and np.all(eig == -5.5) and np.all(obj == -5.5) and np.all(coefs == -5.5) and np.all(vecs == -5.5)
    assert gpu.rounding_stats() == st0
    assert lib.hipsdp_set_comm(s.h, None, 0, 1) == 0
    s.close()
    lib.hipsdp_comm_destroy(comm)


# ---- 10. two host threads -----------------------------------------------------------------------------------------------------------------

def test_two_host_threads_on_two_solvers_reproduce_the_single_thread_bits(gpu):
    shapes = [([3, 17, 65, 130], 5), ([40, 100, 129], 3)]
    data = [(matrices(ns, m, seed=7 + i), xlist("random", ns, seed=7 + i)) for i, (ns, m) in enumerate(shapes)]
    solvers = [load(gpu, d[0], m, "dense") for d, (ns, m) in zip(data, shapes)]

    def both(i):
        r = solvers[i].rounding_frame(data[i][1])
        out = solvers[i].rounding_recombine(r[0], EPS, 0)
        return [hexes(a) for a in r[:4]] + [[hexes(x) for x in blk] for blk in out]
    single = [both(i) for i in range(2)]
    got, errs = [[], []], []

    def work(i):
        try:
            for _ in range(3):
                got[i].append(both(i))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 3 and all(r == single[i] for r in got[i])
    for s in solvers:
        s.close()
