"""GPU: hipsdp_rank1_check_many - eigenvalues 1, n - 1, n and the two scans over the principal 2 x 2 minors of every Z_b(Y[j]) in one call
(csrc/rank1.hip, the three-index values kernels of csrc/eigi.hip and csrc/syevx.hip) - against numpy, against hipsdp_check_y_many, at
the matrix level through the two unit entries, and for what makes it a batch; and hipsdp_rank1_approx - eigenpair n and the right-hand side
A_0 + (lambda v_i) v_k of the rank-1 approximation heuristic - against numpy on blocks with a planted top eigenvalue.

Bounds.  lam: the header's contract for every eigen entry, |lam - lambda| <= 1e-12 max |lambda| (numpy's eigvalsh of the Z formed in
float64).  minordet and the determinant at detind: numpy's a c - b b bit for bit (both products rounded, then the difference).  minorev:
within 1e-12 max |Z_ik| of the largest smaller eigenvalue numpy's eigvalsh gives over the 2 x 2 minors - the closed form's few ulp of
|a| + |b| + |c| - and numpy's value AT the device's pair within twice that of the maximum, so that a near tie may pick another pair; the
planted cases pin the pair exactly.

Storage forms: as in tests/test_gpu_check_y_many.py - loaded dense a block is kept as dense rows up to 64 rows and swept as packed
triangles above; loaded as triplets under sparse_policy(2) every block is kept as nonzeros."""
import ctypes as C
import threading
import numpy as np
import pytest
import eig_cases
import rank1_cases as r1
from check_y_cases import KINDS, family, load, zmat

pytestmark = pytest.mark.gpu

ERR_ARG = 3
EDGES = [1, 2, 3, 17, 64, 65, 128, 129, 130]
FEASTOL = 1e-6


def hexes(a):
    return [float(v).hex() for v in np.asarray(a).reshape(-1)]


def same(a, b):
    """two results of rank1_check_many, bit for bit"""
    return all(hexes(x) == hexes(y) if x.dtype.kind == "f" else np.array_equal(x, y) for x, y in zip(a[:5], b[:5]))


def rows(res, idx):
    return tuple(x[idx] for x in res[:5])


def check_lam(lam, blocks, Y, what):
    """lam[count, nb, 3] against numpy; prints the worst figure of every block before it asserts"""
    for k, A in enumerate(blocks):
        n = A.shape[1]
        worst = 0.0
        for j, y in enumerate(Y):
            w = np.linalg.eigvalsh(zmat(A, y))
            top = max(abs(w[0]), abs(w[-1]))
            want = np.array([w[0], 0.0 if n == 1 else (w[0] if n == 2 else w[n - 2]), w[-1]])
            worst = max(worst, float(np.max(np.abs(lam[j, k] - want)) / max(top, 1e-300)))
        print("%s n = %3d: largest |lam - lambda| / max |lambda| = %.3g" % (what, n, worst))
        assert worst <= 1e-12, (what, n, worst)
        if n == 1:
            assert np.all(lam[:, k, 1] == 0.0) and hexes(lam[:, k, 0]) == hexes(lam[:, k, 2])
        if n == 2:
            assert hexes(lam[:, k, 0]) == hexes(lam[:, k, 1])


# ---- 1. eigenvalues ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [1, 37])
def test_lam_matches_numpy_and_check_y_many_at_the_class_edges(gpu, m, kind, form):
    G = gpu.check_many_group()
    blocks, Y = family(EDGES, m, kind, 2 * G + 3)
    s = load(gpu, blocks, m, form)
    res = s.rank1_check_many(Y, FEASTOL)
    lmin, _, _ = s.check_y_many(Y)
    s.close()
    lam, served = res[0], res[5]
    assert lam.shape == (2 * G + 3, len(EDGES), 3) and list(served) == [0] * len(EDGES)
    check_lam(lam, blocks, Y, "%s %s m = %d" % (form, kind, m))
    assert hexes(lam[:, :, 0]) == hexes(lmin)


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_a_single_block_of_512_rows(gpu, form):
    blocks, Y = family([512], 2, "negative", 2)
    s = load(gpu, blocks, 2, form)
    res = s.rank1_check_many(Y, FEASTOL)
    lmin, _, _ = s.check_y_many(Y)
    s.close()
    assert list(res[5]) == [0]
    check_lam(res[0], blocks, Y, "512 rows, %s" % form)
    assert hexes(res[0][:, :, 0]) == hexes(lmin)
    for j, y in enumerate(Y):
        Z = zmat(blocks[0], y)
        assert tuple(res[4][j, 0]) == r1.scan_det(Z, FEASTOL)[1]


@pytest.mark.parametrize("n", [64, 65, 128, 129, 512])
def test_lsel_many_unit_on_structured_matrices(gpu, n):
    """the eigen suites' matrices - integer-structured (diagonal-dominated arrow, exact multiplicities, zero), clustered spectra, a plain
    diagonal - and their copies scaled by 1e8 and 1e-8, all of one size class in ONE table"""
    cases = dict(eig_cases.structured(n))
    cases.update(eig_cases.spectra(n))
    mats, names = [], []
    for name, (W, ev, scale) in cases.items():
        for f in (1.0, 1e8, 1e-8):
            mats.append(np.ascontiguousarray(W * f))
            names.append("%s x %g" % (name, f))
    mats.append(np.diag(np.arange(1.0, n + 1.0) - n / 3.0)); names.append("diagonal")
    lam = gpu.lsel_many_unit(mats)
    worst = ("", 0.0)
    for W, name, l in zip(mats, names, lam):
        w = np.linalg.eigvalsh(W)
        top = max(abs(w[0]), abs(w[-1]))
        if top == 0.0:                                       # (the zero matrix: the rule of eig_cases.check_zero)
            assert np.all(np.isfinite(l)) and np.max(np.abs(l)) < 1e-200, name
            continue
        err = float(np.max(np.abs(l - np.array([w[0], w[n - 2], w[-1]]))) / top)
        worst = max(worst, (name, err), key=lambda t: t[1])
        assert err <= 1e-12, (name, err)
    print("n = %d: %d matrices, worst %s: %.3g" % (n, len(mats), worst[0], worst[1]))


def test_lsel_many_unit_mixes_the_classes_and_keeps_the_bits(gpu):
    rng = np.random.default_rng(17)
    ns = [1, 2, 130, 3, 65, 64, 129, 17, 128]
    mats = [(lambda R: (R + R.T) / 2)(rng.standard_normal((n, n))) for n in ns]
    lam = gpu.lsel_many_unit(mats)
    for W, l in zip(mats, lam):
        n = W.shape[0]
        w = np.linalg.eigvalsh(W)
        want = np.array([w[0], 0.0 if n == 1 else (w[0] if n == 2 else w[n - 2]), w[-1]])
        assert np.max(np.abs(l - want)) <= 1e-12 * max(abs(w[0]), abs(w[-1])), n
        assert hexes(gpu.lsel_many_unit([W])[0]) == hexes(l), n          # alone: the same bits


# ---- 2. the minors at the matrix level ---------------------------------------------------------------------------------------------------

MINOR_NS = [1, 2, 3, 63, 64, 65, 128, 129, 512]


def _random_sym(n, seed):
    rng = np.random.default_rng([seed, n])
    R = rng.standard_normal((n, n))
    return (R + R.T) / 2.0


def test_minors_unit_against_numpy(gpu):
    mats = [_random_sym(n, 1) for n in MINOR_NS] + [_random_sym(n, 2) + 3.0 * np.eye(n) for n in MINOR_NS]
    tols = []
    for Z in mats:
        mn = np.abs(r1.minors(Z))
        tols.append(float(np.sort(mn)[(3 * len(mn)) // 4]) if len(mn) else 1.0)     # (a quarter of the minors violate it)
    for Z, tol in zip(mats, tols):
        n = Z.shape[0]
        mev, mind, mdet, dind = [x[0] for x in gpu.rank1_minors_unit([Z], tol)]
        det, pair = r1.scan_det(Z, tol)
        assert float(mdet).hex() == float(det).hex() and tuple(dind) == pair, (n, mdet, det, tuple(dind), pair)
        if n == 1:
            assert mev == 0.0 and tuple(mind) == (-1, -1) and mdet == 0.0
            continue
        if pair != r1.NONE:
            i, k = dind
            assert abs(Z[i, i] * Z[k, k] - Z[i, k] * Z[i, k]) > tol
        ref, ri, rk = r1.ev_reference(Z)
        scale = 1e-12 * float(np.max(np.abs(Z)))
        best = float(ref.max())
        print("n = %3d: minorev %.17g, numpy's maximum %.17g, bound %.3g" % (n, mev, best, scale))
        if best > scale:
            assert abs(mev - best) <= scale and mind[0] > mind[1] >= 0
            at = ref[(ri == mind[0]) & (rk == mind[1])][0]
            assert best - at <= 2 * scale, (n, best, at)
        else:
            assert mev <= scale
    # the same matrices in ONE table: the bits of a matrix do not depend on the table
    all_ = gpu.rank1_minors_unit(mats, tols[0])
    for t, Z in enumerate(mats):
        one = gpu.rank1_minors_unit([Z], tols[0])
        assert hexes(one[0]) == hexes(all_[0][t]) and hexes(one[2]) == hexes(all_[2][t])
        assert np.array_equal(one[1][0], all_[1][t]) and np.array_equal(one[3][0], all_[3][t])


def _planted_positions(n):
    """first, last and a middle row, and across the 64-lane and the workgroup boundaries of the position order"""
    cand = [(0, n - 1), (0, 1), (n - 1, n - 2), (n // 2, 0), (n // 2, n // 2 - 1), (11, 10), (12, 0), (33, 7), (63, 64), (64, 0),
            (23, 22), (32, 15), (n - 1, 0)]
    return sorted({(p, q) for p, q in cand if 0 <= p < n and 0 <= q < n and p != q})


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 128, 129, 512])
def test_minors_unit_planted_pair(gpu, n):
    pos = _planted_positions(n)
    cases = [r1.planted_pair(n, p, q) for p, q in pos]
    mev, mind, _, _ = gpu.rank1_minors_unit([Z for Z, _ in cases], FEASTOL)
    for t, (Z, want) in enumerate(cases):
        assert tuple(mind[t]) == want, (n, pos[t], tuple(mind[t]))
        assert abs(mev[t] - (10.0 - abs(Z[want]))) <= 1e-12 * 10.0


def test_minors_unit_ties_and_nothing_positive(gpu):
    mats = [r1.constant(n) for n in MINOR_NS[1:]] + [r1.negative_definite(n) for n in MINOR_NS]
    mev, mind, mdet, dind = gpu.rank1_minors_unit(mats, 1.0)
    k = len(MINOR_NS) - 1
    for t in range(k):                                       # every minor has the same bits: the first pair
        assert mev[t] == 1.0 and tuple(mind[t]) == (1, 0) and mdet[t] == 3.0 and tuple(dind[t]) == (1, 0), MINOR_NS[1 + t]
    for t in range(k, len(mats)):
        assert mev[t] == 0.0 and tuple(mind[t]) == (-1, -1), MINOR_NS[t - k]
    # ties of the maximum at several pairs of a matrix that is not constant: diagonal (3, 1, 3, 1, 3, ...) with zeros off it
    for n in (3, 65, 129):
        Z = np.diag(np.where(np.arange(n) % 2 == 0, 3.0, 1.0))
        got = gpu.rank1_minors_unit([Z], 1.0)
        assert got[0][0] == 3.0 and tuple(got[1][0]) == (2, 0) == r1.scan_ev(Z)[1]


def test_minors_unit_feastol_edge(gpu):
    """small integers: a minor exactly equal to feastol (or to -feastol) is not a violation"""
    Z = np.array([[2.0, 1.0, 2.0], [1.0, 3.0, 3.0], [2.0, 3.0, 4.0]])          # minors 5, 4, 3
    for tol, want in [(1e-6, (1, 0)), (4.0, (1, 0)), (5.0, (-1, -1)), (4.5, (1, 0))]:
        got = gpu.rank1_minors_unit([Z], tol)
        assert got[2][0] == 5.0 and tuple(got[3][0]) == want == r1.scan_det(Z, tol)[1], tol
    Z = np.array([[1.0, 1.0, 2.0], [1.0, 1.0, 1.0], [2.0, 1.0, 2.0]])          # minors 0, -2, 1
    for tol, want in [(1.5, (2, 0)), (2.0, (-1, -1)), (0.5, (2, 0)), (1.0, (2, 0)), (0.0, (2, 0))]:
        got = gpu.rank1_minors_unit([Z], tol)
        assert got[2][0] == 2.0 and tuple(got[3][0]) == want == r1.scan_det(Z, tol)[1], tol
    big = np.ones((130, 130)) + np.diag(np.arange(130.0))                       # minors (1 + i)(1 + k) - 1: the integers 1, 2, 5, ...
    got = gpu.rank1_minors_unit([big], 2.0)
    assert tuple(got[3][0]) == (2, 1) == r1.scan_det(big, 2.0)[1] and got[2][0] == 130.0 * 129.0 - 1.0


# ---- 3. the minors through the solver ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_the_scans_of_the_call_are_the_unit_entry_on_the_devices_own_z(gpu, form):
    G = gpu.check_many_group()
    m = 5
    blocks, Y = family(EDGES, m, "negative", G + 1, seed=21)
    s = load(gpu, blocks, m, form, units=True)
    Zs, _ = s.form_z_many_unit(Y)
    tol = 0.05
    res = s.rank1_check_many(Y, tol)
    s.close()
    for k in range(len(EDGES)):
        unit = gpu.rank1_minors_unit(list(Zs[k]), tol)
        assert hexes(unit[0]) == hexes(res[1][:, k]) and hexes(unit[2]) == hexes(res[3][:, k]), EDGES[k]
        assert np.array_equal(unit[1], res[2][:, k]) and np.array_equal(unit[3], res[4][:, k]), EDGES[k]
        for j in range(len(Y)):                              # ... and numpy's scan of the same bits
            det, pair = r1.scan_det(Zs[k][j], tol)
            assert float(res[3][j, k]).hex() == float(det).hex() and tuple(res[4][j, k]) == pair


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_exact_rank_one(gpu, form):
    G = gpu.check_many_group()
    m = 4
    blocks, Y, cs = r1.rank_one_blocks(EDGES, m, G + 1, seed=3)
    s = load(gpu, blocks, m, form)
    lam, mev, mind, mdet, dind, served = s.rank1_check_many(Y, 1e-9)
    s.close()
    assert np.all(served == 0)
    assert np.all(mdet == 0.0) and np.all(dind == -1) and np.all(mev == 0.0) and np.all(mind == -1)
    for k, n in enumerate(EDGES):
        want = np.array([n * float(cs[k] @ y) for y in Y])
        assert np.all(np.abs(lam[:, k, 2] - want) <= 1e-12 * want), n
        if n > 1:
            assert np.all(np.abs(lam[:, k, 1]) <= 1e-12 * lam[:, k, 2]), (n, float(np.max(np.abs(lam[:, k, 1]) / lam[:, k, 2])))


# ---- 4. what makes it a batch ------------------------------------------------------------------------------------------------------------

IND_NS = [3, 17, 65, 130]


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_the_bits_of_a_candidate_depend_on_its_row_and_the_block_alone(gpu, form, monkeypatch):
    monkeypatch.delenv("HIPSDP_RANK1_CHUNK", raising=False)
    G = gpu.check_many_group()
    m = 5
    blocks, Y = family(IND_NS, m, "negative", 2 * G + 3, seed=3)
    count = len(Y)
    s = load(gpu, blocks, m, form)
    full = s.rank1_check_many(Y, 0.05)
    assert same(s.rank1_check_many(Y, 0.05), full)
    for c in (1, G - 1, G, G + 1):
        assert same(s.rank1_check_many(Y[:c], 0.05), rows(full, slice(0, c))), c
    assert same(s.rank1_check_many(Y[count - 1:], 0.05), rows(full, slice(count - 1, count)))
    perm = np.random.default_rng(5).permutation(count)
    assert same(s.rank1_check_many(Y[perm], 0.05), rows(full, perm))
    monkeypatch.setenv("HIPSDP_RANK1_CHUNK", "3")
    st0 = gpu.rank1_check_many_stats()
    chunked = s.rank1_check_many(Y, 0.05)
    st1 = gpu.rank1_check_many_stats()
    monkeypatch.delenv("HIPSDP_RANK1_CHUNK")
    chunks = (count + 2) // 3
    assert same(chunked, full)
    assert st1[0] - st0[0] == 1 and st1[2] - st0[2] == chunks and st1[1] - st0[1] == chunks * (3 + 1 + 1 + 131)
    # NULL pairs: lam alone has the same bits
    only = s.rank1_check_many(Y, 0.05, minors=False, dets=False)
    assert only[1] is None and only[4] is None and hexes(only[0]) == hexes(full[0])
    s.close()
    for k in range(len(IND_NS)):                             # every block alone in a solver
        s1 = load(gpu, blocks[k:k + 1], m, form)
        alone = s1.rank1_check_many(Y, 0.05)
        s1.close()
        assert same(alone, tuple(x[:, k:k + 1] for x in full[:5])), IND_NS[k]


def formula(ns):
    small = any(n <= 64 for n in ns)
    mid = any(64 < n <= 128 for n in ns)
    nmax = max([n for n in ns if 128 < n <= 512], default=0)
    return (3 if ns else 0) + int(small) + int(mid) + (nmax + 1 if nmax else 0)


@pytest.mark.parametrize("ns", [[12], [12] * 9, [100], [17, 65, 130], [129, 150]])
def test_launches_and_readbacks_are_the_formula(gpu, ns, monkeypatch):
    monkeypatch.delenv("HIPSDP_RANK1_CHUNK", raising=False)
    G = gpu.check_many_group()
    blocks, Y = family(ns, 2, "negative", 2 * G + 3, seed=6)
    s = load(gpu, blocks, 2, "dense")
    other = gpu.check_y_many_stats()
    deltas = []
    for count in (1, 2 * G + 3):
        st0 = gpu.rank1_check_many_stats()
        s.rank1_check_many(Y[:count], FEASTOL)
        st1 = gpu.rank1_check_many_stats()
        deltas.append(tuple(b - a for a, b in zip(st0, st1)))
    print("blocks %s: (calls, launches, read-backs) %s" % (ns, deltas))
    assert deltas[0] == deltas[1] == (1, formula(ns), 1)
    st0 = gpu.rank1_check_many_stats()
    s.rank1_check_many(Y[:0], FEASTOL)
    assert gpu.rank1_check_many_stats() == st0 and gpu.check_y_many_stats() == other
    s.check_y_many(Y[:1])
    assert gpu.rank1_check_many_stats() == st0                                           # ... and the reverse
    s.close()


@pytest.mark.parametrize("order", [(513, 12), (12, 513)])
def test_a_block_of_513_rows_is_turned_away_and_the_other_is_served(gpu, order):
    m = 1
    small, Y = family([12], m, "negative", 3, seed=4)
    big = np.zeros((m + 1, 513, 513))
    big[0] = -np.eye(513)
    big[1] = np.eye(513)
    blocks = [big, small[0]] if order[0] == 513 else [small[0], big]
    s = load(gpu, blocks, m, "dense")
    lam, mev, mind, mdet, dind, served = s.rank1_check_many(Y, FEASTOL, fill=-777.25)
    s.close()
    b, k = order.index(513), order.index(12)
    assert list(served) == [(-1 if n == 513 else 0) for n in order]
    assert np.all(lam[:, b] == -777.25) and np.all(mev[:, b] == -777.25) and np.all(mdet[:, b] == -777.25)
    assert np.all(mind[:, b] == -7) and np.all(dind[:, b] == -7)
    check_lam(lam[:, k:k + 1], small, Y, "beside 513 rows")
    for j, y in enumerate(Y):
        assert tuple(dind[j, k]) == r1.scan_det(zmat(small[0], y), FEASTOL)[1]


def test_argument_errors_with_a_solver(gpu):
    lib = gpu.lib()
    blocks, Y = family([3], 2, "feasible", 2)
    s = load(gpu, blocks, 2, "dense")
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    lam, me, md = np.full(6, 7.0), np.full(2, 7.0), np.full(2, 7.0)
    mi, di, sv = np.full(4, 77, dtype=np.int32), np.full(4, 77, dtype=np.int32), np.full(1, 77, dtype=np.int32)
    tol = C.c_double(FEASTOL)
    f = lib.hipsdp_rank1_check_many
    st0 = gpu.rank1_check_many_stats()
    assert f(s.h, -1, dp(Y), tol, dp(lam), dp(me), ip(mi), dp(md), ip(di), ip(sv)) == ERR_ARG
    assert f(s.h, 2, None, tol, dp(lam), dp(me), ip(mi), dp(md), ip(di), ip(sv)) == ERR_ARG
    assert f(s.h, 2, dp(Y), tol, None, dp(me), ip(mi), dp(md), ip(di), ip(sv)) == ERR_ARG
    assert f(s.h, 2, dp(Y), C.c_double(-1e-9), dp(lam), dp(me), ip(mi), dp(md), ip(di), ip(sv)) == ERR_ARG
    assert f(s.h, 2, dp(Y), tol, dp(lam), dp(me), None, dp(md), ip(di), ip(sv)) == ERR_ARG
    assert f(s.h, 2, dp(Y), tol, dp(lam), dp(me), ip(mi), None, ip(di), ip(sv)) == ERR_ARG
    assert f(s.h, 0, None, tol, None, None, None, None, None, None) == 0                 # count == 0: nothing happens
    assert f(s.h, 0, dp(Y), tol, dp(lam), dp(me), ip(mi), dp(md), ip(di), ip(sv)) == 0
    assert list(lam) == [7.0] * 6 and list(me) == [7.0] * 2 and list(md) == [7.0] * 2
    assert list(mi) == [77] * 4 and list(di) == [77] * 4 and list(sv) == [77]
    assert gpu.rank1_check_many_stats() == st0
    assert f(s.h, 2, dp(Y), tol, dp(lam), None, None, None, None, None) == 0             # lam alone
    assert np.all(lam > 0.0) and list(me) == [7.0] * 2 and list(mi) == [77] * 4
    s.close()
    fresh = gpu.Solver(0)                                                                # a solver without a shape
    assert f(fresh.h, 2, dp(Y), tol, dp(lam), dp(me), ip(mi), dp(md), ip(di), ip(sv)) == ERR_ARG
    fresh.close()


def test_two_host_threads_on_two_solvers_reproduce_the_single_thread_bits(gpu):
    G = gpu.check_many_group()
    data = [family([3, 17, 65, 130], 5, "negative", 2 * G + 3, seed=7), family([40, 100, 129], 3, "lowrank", G + 1, seed=8)]
    solvers = [load(gpu, d[0], d[1].shape[1], "dense") for d in data]
    single = [s.rank1_check_many(d[1], 0.05) for s, d in zip(solvers, data)]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                got[i].append(solvers[i].rank1_check_many(data[i][1], 0.05))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 3 and all(same(r, single[i]) for r in got[i])
    for s in solvers:
        s.close()


# ---- 5. hipsdp_rank1_approx ---------------------------------------------------------------------------------------------------------------

def tri(A):
    i, k = np.tril_indices(A.shape[0])
    return A[i, k]


def check_approx(out, blocks, y, what):
    """the eigen entries' bounds against numpy, v v^T over the gap, rhs from the RETURNED pair; figures printed before they are asserted"""
    for A, got in zip(blocks, out):
        n = A.shape[1]
        lam, v, rhs = got
        Z = zmat(A, y)
        w, V = np.linalg.eigh(Z)
        scale = float(np.max(np.abs(w)))
        gap = float(w[-1] - w[-2]) if n > 1 else scale
        dl, dn = abs(lam - w[-1]), abs(np.linalg.norm(v) - 1.0)
        res = float(np.linalg.norm(Z @ v - lam * v))
        dp = float(np.max(np.abs(np.outer(v, v) - np.outer(V[:, -1], V[:, -1]))))
        want = r1.rhs(A[0], lam, v)
        bound = 4 * 2.0 ** -53 * (np.abs(tri(A[0])) + np.abs(tri(np.outer(lam * v, v))))
        dr = np.abs(rhs - want)
        print("%s n = %3d: |lam - ev| / scale %.3g, | |v| - 1 | %.3g, residual / scale %.3g, |vv^T - ref| gap / scale %.3g, rhs worst / bound %.3g"
              % (what, n, dl / scale, dn, res / scale, dp * gap / scale, float(np.max(dr / np.maximum(bound, 1e-300)))))
        assert gap >= 0.8 * (w[-1] / 1.1) or n == 1, (n, gap, w[-1])
        assert dl <= 1e-12 * scale and dn <= 1e-12 and res <= 1e-9 * scale, (n, dl, dn, res)
        assert dp <= 1e-9 * scale / gap, (n, dp)
        assert rhs.shape == (n * (n + 1) // 2,) and np.all(dr <= bound), (n, float(dr.max()))


def approx_formula(ns):
    small = any(n <= 128 for n in ns)
    nmax = max([n for n in ns if 128 < n <= 512], default=0)
    return 2 + 3 * int(small) + (nmax + 3 if nmax else 0)


@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("m", [1, 37])
def test_rank1_approx_at_the_class_edges(gpu, m, form, monkeypatch):
    monkeypatch.delenv("HIPSDP_RANK1_APPROX_CHUNK", raising=False)
    blocks, y = r1.planted_top(EDGES, m, seed=5)
    nb = len(EDGES)
    s = load(gpu, blocks, m, form)
    st0 = gpu.rank1_approx_stats()
    out, served = s.rank1_approx(y)
    st1 = gpu.rank1_approx_stats()
    assert list(served) == [0] * nb and tuple(b - a for a, b in zip(st0, st1)) == (1, approx_formula(EDGES), 1)
    check_approx(out, blocks, y, "%s m = %d" % (form, m))
    full = s.rank1_approx(y, raw=True)
    # masks: served = 1 and untouched slices; a block's bits do not depend on the other blocks or on want
    for want in ([1, 0, 0, 0, 0, 0, 0, 0, 0], [0, 1, 0, 1, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0, 1, 1], [0, 0, 0, 0, 0, 0, 0, 0, 2]):
        ns_w = [n for n, t in zip(EDGES, want) if t]
        st0 = gpu.rank1_approx_stats()
        lm, ve, rh, sv = s.rank1_approx(y, want=want, fill=-777.25, raw=True)
        st1 = gpu.rank1_approx_stats()
        assert list(sv) == [0 if t else 1 for t in want], want
        assert tuple(b - a for a, b in zip(st0, st1)) == (1, approx_formula(ns_w), 1), want
        vo = ro = 0
        for b, n in enumerate(EDGES):
            t = n * (n + 1) // 2
            if want[b]:
                assert float(lm[b]).hex() == float(full[0][b]).hex(), (want, n)
                assert hexes(ve[vo:vo + n]) == hexes(full[1][vo:vo + n]) and hexes(rh[ro:ro + t]) == hexes(full[2][ro:ro + t]), (want, n)
            else:
                assert lm[b] == -777.25 and np.all(ve[vo:vo + n] == -777.25) and np.all(rh[ro:ro + t] == -777.25), (want, n)
            vo += n
            ro += t
    # nothing asked for: nothing launched
    st0 = gpu.rank1_approx_stats()
    _, sv = s.rank1_approx(y, want=[0] * nb)
    assert list(sv) == [1] * nb and gpu.rank1_approx_stats() == st0
    # in chunks of two blocks: the same bits, a read-back per chunk
    monkeypatch.setenv("HIPSDP_RANK1_APPROX_CHUNK", "2")
    st0 = gpu.rank1_approx_stats()
    ch = s.rank1_approx(y, raw=True)
    st1 = gpu.rank1_approx_stats()
    monkeypatch.delenv("HIPSDP_RANK1_APPROX_CHUNK")
    assert all(hexes(a) == hexes(b) for a, b in zip(ch[:3], full[:3]))
    assert st1[0] - st0[0] == 1 and st1[2] - st0[2] == (nb + 1) // 2
    # by descending size: (130, 129) (128, 65) (64, 17) (3, 2) (1)
    assert st1[1] - st0[1] == sum(approx_formula(c) for c in ([130, 129], [128, 65], [64, 17], [3, 2], [1]))
    s.close()
    # every block alone in a solver
    for k in (0, 3, 5, 8):
        s1 = load(gpu, blocks[k:k + 1], m, form)
        one = s1.rank1_approx(y, raw=True)
        s1.close()
        n = EDGES[k]
        vo, ro = sum(EDGES[:k]), sum(t * (t + 1) // 2 for t in EDGES[:k])
        assert float(one[0][0]).hex() == float(full[0][k]).hex(), n
        assert hexes(one[1]) == hexes(full[1][vo:vo + n]) and hexes(one[2]) == hexes(full[2][ro:ro + n * (n + 1) // 2]), n


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_rank1_approx_of_a_block_of_512_rows(gpu, form):
    blocks, y = r1.planted_top([512], 2, seed=6)
    s = load(gpu, blocks, 2, form)
    out, served = s.rank1_approx(y)
    s.close()
    assert list(served) == [0]
    check_approx(out, blocks, y, "512 rows, %s" % form)


def test_rank1_approx_turns_a_block_of_513_rows_away(gpu):
    m = 1
    small, y = r1.planted_top([12], m, seed=7)
    big = np.zeros((m + 1, 513, 513))
    big[0] = -np.eye(513)
    big[1] = np.eye(513)
    s = load(gpu, [big, small[0]], m, "dense")
    out, served = s.rank1_approx(y)
    lm, ve, rh, sv = s.rank1_approx(y, want=[1, 0], fill=-777.25, raw=True)
    lib = gpu.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    yy = np.ascontiguousarray(y)
    assert lib.hipsdp_rank1_approx(s.h, None, None, dp(lm), dp(ve), dp(rh), None) == ERR_ARG
    assert lib.hipsdp_rank1_approx(s.h, dp(yy), None, None, dp(ve), dp(rh), None) == ERR_ARG
    assert lib.hipsdp_rank1_approx(s.h, dp(yy), None, dp(lm), dp(ve), dp(rh), None) == 0          # served may be NULL
    s.close()
    assert list(served) == [-1, 0] and out[0] is None
    check_approx(out[1:], small, y, "beside 513 rows")
    assert list(sv) == [-1, 1] and np.all(ve[:513] == -777.25)
    assert float(lm[1]).hex() == float(out[1][0]).hex() and lm[0] == -777.25


# ---- 6. end to end: the rank-1 part of CONSCHECK -----------------------------------------------------------------------------------------

def test_the_conscheck_loop_on_a_problem_shaped_like_example_rank1_dual(gpu):
    """6 blocks of 3 rows, m = 51, synthetic entries: the first 8 variables of a block carry c_i u u^T, the others random symmetric
    matrices; half of the 2 G + 3 points are zero on the random part and multiples of 1 / 8 on the rest, so their Z is exactly rank one"""
    G = gpu.check_many_group()
    m, nb, count = 51, 6, 2 * G + 3
    rng = np.random.default_rng(51)
    blocks = []
    for b in range(nb):
        u = rng.choice([-1.0, 1.0], 3)
        A = np.zeros((m + 1, 3, 3))
        for i in range(1, 9):
            A[i] = float(rng.integers(1, 5)) * np.outer(u, u)
        for i in range(9, m + 1):
            R = rng.standard_normal((3, 3))
            A[i] = (R + R.T) / 2.0
        blocks.append(A)
    Y = rng.uniform(0.0, 1.0, (count, m))
    exact = np.arange(count) % 2 == 0
    Y[exact, 8:] = 0.0
    Y[exact, :8] = rng.integers(1, 9, (int(exact.sum()), 8)) / 8.0
    for form in ("dense", "sparse"):
        s = load(gpu, blocks, m, form)
        lam, mev, mind, _, _, served = s.rank1_check_many(Y, FEASTOL)
        s.close()
        assert np.all(served == 0)
        got = r1.conscheck_from_call(lam, mev, mind, FEASTOL)
        want = r1.conscheck_numpy(blocks, Y, FEASTOL)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]), form
        assert np.array_equal(got[0], np.repeat(exact[:, None], nb, axis=1))
        assert np.all(np.abs(got[1] - want[1]) <= 1e-12 * np.max(np.abs(lam), axis=2)), form
        assert np.all(got[2][exact] == -1) and np.any(got[2][~exact] >= 0)
