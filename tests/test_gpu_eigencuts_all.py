"""GPU: hipsdp_eigencuts_all - the separation round (eigenvector cuts) and the feasibility eigenvalues of ALL blocks in one call
(csrc/eigcuts.hip) - against the numpy restatement oracle/eigcuts_ref.py, against the per-block hipsdp_eigencuts, in the three
storage forms of a block, and for what makes it a batch: a launch and read-back count that does not depend on the number of blocks
or cuts, and decompositions with the bits of hipsdp_syev_small.

The families (block k of sizes ns is instances.planted_dense(n_k, m, seed=20240 + 1000 k) with the constant matrix rebuilt around
the common ys of block 0, minus 10 I for the quiet blocks; the point is ys + 0.7 N(0, 1)) have well separated selected eigenvalues
(relative gaps >= 7.6e-3) and no eigenvalue nearer to -tol than 3.4e-3: counts are immune to rounding, vectors defined up to sign."""
import ctypes as C
import threading
import numpy as np
import pytest
import instances
import ipm_ref
import eigcuts_ref

pytestmark = pytest.mark.gpu

TOL, MAXCUTS = 1e-6, 5
#            sizes                                   m   quiet    seed  cuts of the oracle
FAMILIES = [([3, 9, 10, 17, 33, 64, 65, 100, 128], 20, (2, 5), 0, 30),
            ([12] * 32, 15, (), 1, 96),
            ([40] * 4, 15, (), 1, 20),
            ([16, 150, 48, 200, 10], 25, (2,), 2, 18)]

_cache = {}


def family(ns, m, quiet, seed):
    """(blocks [A_k (m + 1, n_k, n_k)], ys, y, b)"""
    key = (tuple(ns), m, tuple(quiet), seed)
    if key not in _cache:
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
        _cache[key] = (blocks, ys, y, b)
    return _cache[key]


def load_dense(gpu, blocks, b, D=None, c=None):
    s = gpu.Solver(0)
    s.load_core(ipm_ref.CoreProblem(b, blocks, D, c))
    return s


def load_sparse(gpu, blocks, b):
    """the same matrices handed over as lower-triangular triplets with counts: every block is kept as nonzeros"""
    m = len(b)
    s = gpu.Solver(0)
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
    s.set_obj(b)
    for k, t in enumerate(trip):
        s.add_entries(k, *t)
    return s


def lmin_ref(A, y):
    Z = (np.tensordot(y, A[1:], axes=(0, 0)) if len(y) else 0.0) - A[0]
    return float(np.linalg.eigvalsh(Z)[0])


def check_against_oracle(res, blocks, ys, y, quiet, what):
    """item 1 of the issue's checks, for every block"""
    total = 0
    for k, A in enumerate(blocks):
        lmin, ev, co, lh, ve = res[k]
        rev, rco, rlh, rve = eigcuts_ref.cuts_dense(A, y, TOL, MAXCUTS)
        rl = lmin_ref(A, y)
        print("%s block %d (n = %d): ncuts %d / oracle %d, lmin %.12g / %.12g" % (what, k, A.shape[1], len(ev), len(rev), lmin, rl))
        assert len(ev) == len(rev), (what, k)
        assert (len(ev) == 0) == (k in quiet), (what, k)
        assert abs(lmin - rl) <= 1e-9 * max(1.0, abs(rl)), (what, k, lmin, rl)
        total += len(ev)
        if len(ev) == 0:
            continue
        assert np.max(np.abs(ev - rev)) <= 1e-9 * max(1.0, np.max(np.abs(rev))), (what, k)
        assert ev[0] == lmin
        for c in range(len(ev)):
            v = ve[c]
            assert abs(np.linalg.norm(v) - 1.0) <= 1e-10, (what, k, c)
            assert abs(abs(v @ rve[c]) - 1.0) <= 1e-6, (what, k, c)
            assert np.max(np.abs(co[c] - rco[c])) <= 1e-6 * max(1.0, np.max(np.abs(rco[c]))), (what, k, c)
            assert abs(lh[c] - rlh[c]) <= 1e-6 * max(1.0, abs(rlh[c])), (what, k, c)
            assert abs((co[c] @ y - lh[c]) - ev[c]) <= 1e-8 * max(1.0, abs(ev[c])), (what, k, c)
            assert co[c] @ ys - lh[c] >= -1e-9, (what, k, c)
    return total


def same_bits(ra, rb):
    for (la, ea, ca, ha, va), (lb, eb, cb, hb_, vb) in zip(ra, rb):
        if not (la == lb and np.array_equal(ea, eb) and np.array_equal(ca, cb) and np.array_equal(ha, hb_) and np.array_equal(va, vb)):
            return False
    return len(ra) == len(rb)


@pytest.mark.parametrize("fam", range(4))
def test_all_blocks_match_the_oracle(gpu, fam):
    ns, m, quiet, seed, cuts = FAMILIES[fam]
    blocks, ys, y, b = family(ns, m, quiet, seed)
    s = load_dense(gpu, blocks, b)
    res = s.eigencuts_all(y, TOL, MAXCUTS)
    assert len(res) == len(ns)
    assert check_against_oracle(res, blocks, ys, y, quiet, "family %d" % fam) == cuts
    s.close()


@pytest.mark.parametrize("fam", range(4))
def test_all_blocks_agree_with_the_per_block_call(gpu, fam):
    ns, m, quiet, seed, _ = FAMILIES[fam]
    blocks, ys, y, b = family(ns, m, quiet, seed)
    s = load_dense(gpu, blocks, b)
    res = s.eigencuts_all(y, TOL, MAXCUTS)
    lchk, _ = s.check_y(y)
    for k in range(len(ns)):
        lmin, ev, co, lh, ve = res[k]
        pev, pco, plh, pve = s.eigencuts(k, y, TOL, MAXCUTS)
        assert len(ev) == len(pev)
        assert abs(lmin - lchk[k]) <= 1e-8 * max(1.0, abs(lmin)), (k, lmin, lchk[k])
        if len(ev) == 0:
            continue
        assert np.max(np.abs(ev - pev)) <= 1e-9 * max(1.0, np.max(np.abs(pev)))
        for c in range(len(ev)):
            assert np.max(np.abs(co[c] - pco[c])) <= 1e-6 * max(1.0, np.max(np.abs(pco[c])))
            assert abs(lh[c] - plh[c]) <= 1e-6 * max(1.0, abs(plh[c]))
            assert abs(abs(ve[c] @ pve[c]) - 1.0) <= 1e-6
    # a feasible point: nothing to cut anywhere, every block psd
    res0 = s.eigencuts_all(ys, TOL, MAXCUTS)
    l0, _ = s.check_y(ys)
    for k in range(len(ns)):
        assert len(res0[k][1]) == 0 and res0[k][2].shape == (0, m) and res0[k][4].shape == (0, ns[k])
        assert res0[k][0] >= -1e-9
        assert abs(res0[k][0] - l0[k]) <= 1e-8 * max(1.0, abs(l0[k]))
    s.close()


def test_blocks_kept_as_nonzeros_give_the_same_cuts(gpu):
    """family 1 covers the dense rows (up to 64 rows) and the packed lower triangles (above) by itself; loaded a second time as
    triplets every block is kept as nonzeros - both loads match the oracle and each other"""
    ns, m, quiet, seed, cuts = FAMILIES[0]
    blocks, ys, y, b = family(ns, m, quiet, seed)
    sd = load_dense(gpu, blocks, b)
    ss = load_sparse(gpu, blocks, b)
    for k in range(len(ns)):
        assert ss.is_sparse(k), k
        assert not sd.is_sparse(k), k
    rd = sd.eigencuts_all(y, TOL, MAXCUTS)
    rs = ss.eigencuts_all(y, TOL, MAXCUTS)
    assert check_against_oracle(rs, blocks, ys, y, quiet, "nonzeros") == cuts
    for k in range(len(ns)):
        (ld, ed, cd, hd, vd), (ls, es, cs, hs, vs) = rd[k], rs[k]
        assert len(ed) == len(es)
        assert abs(ld - ls) <= 1e-9 * max(1.0, abs(ld))
        if len(ed) == 0:
            continue
        assert np.max(np.abs(ed - es)) <= 1e-9 * max(1.0, np.max(np.abs(ed)))
        for c in range(len(ed)):
            assert abs(abs(vd[c] @ vs[c]) - 1.0) <= 1e-6
            assert np.max(np.abs(cd[c] - cs[c])) <= 1e-6 * max(1.0, np.max(np.abs(cd[c])))
            assert abs(hd[c] - hs[c]) <= 1e-6 * max(1.0, abs(hd[c]))
    sd.close()
    ss.close()


def test_many_form_decomposition_has_the_bits_of_syev_small(gpu):
    """the batched decomposition on the Z_b(y) of family 1 (all three size classes, both sides of every class boundary), matrix for
    matrix against hipsdp_syev_small - in at most three launches"""
    ns, m, quiet, seed, _ = FAMILIES[0]
    blocks, ys, y, b = family(ns, m, quiet, seed)
    Zs = [np.ascontiguousarray(np.tensordot(y, A[1:], axes=(0, 0)) - A[0]) for A in blocks]
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    cat = np.concatenate([Z.reshape(-1) for Z in Zs])
    lam = np.zeros(sum(ns))
    V = np.zeros(sum(n * n for n in ns))
    cns = (C.c_int * len(ns))(*ns)
    nl = C.c_int(-1)
    rc = gpu.ulib().hipsdp_syev_many_unit(0, len(ns), cns, dp(cat), dp(lam), dp(V), C.byref(nl))
    assert rc == 0, gpu.ulib().hipsdp_last_error()
    assert 1 <= nl.value <= 3
    lo = vo = 0
    for n, Z in zip(ns, Zs):
        l1 = np.zeros(n)
        V1 = np.zeros(n * n)
        assert gpu.lib().hipsdp_syev_small(0, n, dp(Z), dp(l1), dp(V1)) == 0
        assert np.array_equal(lam[lo:lo + n], l1), n
        assert np.array_equal(V[vo:vo + n * n], V1), n
        assert np.max(np.abs(l1 - np.linalg.eigvalsh(Z))) <= 1e-9 * max(1.0, np.max(np.abs(l1)))
        lo += n
        vo += n * n
    # twice as many matrices: the same number of launches
    nl2 = C.c_int(-1)
    ns2 = list(ns) + list(ns)
    lam2, V2 = np.zeros(2 * sum(ns)), np.zeros(2 * len(V))
    rc = gpu.ulib().hipsdp_syev_many_unit(0, len(ns2), (C.c_int * len(ns2))(*ns2), dp(np.concatenate([cat, cat])), dp(lam2), dp(V2),
                                          C.byref(nl2))
    assert rc == 0 and nl2.value == nl.value
    assert np.array_equal(lam2[:len(lam)], lam) and np.array_equal(lam2[len(lam):], lam)
    assert np.array_equal(V2[:len(V)], V) and np.array_equal(V2[len(V):], V)


def test_launches_and_readbacks_do_not_depend_on_blocks_or_cuts(gpu):
    deltas = {}
    for fam in (1, 2):
        ns, m, quiet, seed, _ = FAMILIES[fam]
        blocks, ys, y, b = family(ns, m, quiet, seed)
        s = load_dense(gpu, blocks, b)
        s.eigencuts_all(y, TOL, MAXCUTS)               # first use (workspace, job table)
        for mc in (1, MAXCUTS):
            c0, l0, r0 = gpu.eigencuts_all_stats()
            res = s.eigencuts_all(y, TOL, mc)
            c1, l1, r1 = gpu.eigencuts_all_stats()
            assert c1 - c0 == 1
            assert all(1 <= len(r[1]) <= mc for r in res)
            deltas[(fam, mc)] = (l1 - l0, r1 - r0)
            print("family %d (%d blocks), maxcuts %d: %d launches, %d read-backs" % (fam, len(ns), mc, l1 - l0, r1 - r0))
        s.close()
    assert len(set(deltas.values())) == 1, deltas
    launches, readbacks = next(iter(deltas.values()))
    assert 1 <= readbacks <= 2
    assert 3 <= launches <= 5          # Z(y), at most three decomposition classes, selection + coefficients


def test_separateonecut_mode_returns_the_most_negative_eigenpair(gpu):
    ns, m, quiet, seed, _ = FAMILIES[0]
    blocks, ys, y, b = family(ns, m, quiet, seed)
    s = load_dense(gpu, blocks, b)
    r5 = s.eigencuts_all(y, TOL, MAXCUTS)
    r1 = s.eigencuts_all(y, TOL, 1)
    for k in range(len(ns)):
        assert len(r1[k][1]) == min(1, len(r5[k][1]))
        assert r1[k][0] == r5[k][0]
        if len(r1[k][1]):
            assert r1[k][1][0] == r5[k][1][0] and np.array_equal(r1[k][2][0], r5[k][2][0]) and r1[k][3][0] == r5[k][3][0]
            assert np.array_equal(r1[k][4][0], r5[k][4][0])
    s.close()


def test_two_calls_and_two_threads_give_the_same_bits(gpu):
    fams = [FAMILIES[1], FAMILIES[2]]
    data = [family(f[0], f[1], f[2], f[3]) for f in fams]
    solvers = [load_dense(gpu, d[0], d[3]) for d in data]
    single = [s.eigencuts_all(d[2], TOL, MAXCUTS) for s, d in zip(solvers, data)]
    again = [s.eigencuts_all(d[2], TOL, MAXCUTS) for s, d in zip(solvers, data)]
    for a, b_ in zip(single, again):
        assert same_bits(a, b_)
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(6):
                got[i].append(solvers[i].eigencuts_all(data[i][2], TOL, MAXCUTS))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 6
        for r in got[i]:
            assert same_bits(r, single[i])
    for s in solvers:
        s.close()


def test_a_call_between_two_solves_changes_nothing(gpu):
    ns, m, quiet, seed, _ = FAMILIES[2]
    blocks, ys, y, b = family(ns, m, quiet, seed)

    def run(between):
        s = load_dense(gpu, blocks, b)
        i1 = s.solve(gaptol=1e-6, feastol=1e-6)
        y1, X1 = s.y(), s.X(1)
        if between:
            s.eigencuts_all(y, TOL, MAXCUTS)
            assert np.array_equal(s.y(), y1) and np.array_equal(s.X(1), X1)
        i2 = s.solve(gaptol=1e-6, feastol=1e-6)
        out = (i1.status, i1.dobj, y1, i2.status, i2.iterations, i2.dobj, s.y(), s.X(0), s.Z(3))
        s.close()
        return out
    a, c = run(False), run(True)
    assert a[0] == 0 and a[3] == 0
    for u, v in zip(a, c):
        assert np.array_equal(np.asarray(u), np.asarray(v))


def test_arguments(gpu):
    ns, m, quiet, seed, _ = FAMILIES[2]
    blocks, ys, y, b = family(ns, m, quiet, seed)
    s = load_dense(gpu, blocks, b)
    L = gpu.lib()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    nb = len(ns)
    k = (C.c_int * nb)()
    lmin, ev, lh = np.zeros(nb), np.zeros(nb * MAXCUTS), np.zeros(nb * MAXCUTS)
    co, ve = np.zeros(nb * MAXCUTS * m), np.zeros(MAXCUTS * sum(ns))
    NUL = C.POINTER(C.c_double)()
    tol = C.c_double(TOL)
    ERR_ARG = 3
    before = gpu.eigencuts_all_stats()
    unshaped = gpu.Solver(0)
    assert L.hipsdp_eigencuts_all(None, dp(y), tol, MAXCUTS, k, dp(lmin), dp(ev), dp(co), dp(lh), dp(ve)) == ERR_ARG
    assert L.hipsdp_eigencuts_all(unshaped.h, dp(y), tol, MAXCUTS, k, dp(lmin), dp(ev), dp(co), dp(lh), dp(ve)) == ERR_ARG
    assert L.hipsdp_eigencuts_all(s.h, NUL, tol, MAXCUTS, k, dp(lmin), dp(ev), dp(co), dp(lh), dp(ve)) == ERR_ARG
    assert L.hipsdp_eigencuts_all(s.h, dp(y), tol, MAXCUTS, None, dp(lmin), dp(ev), dp(co), dp(lh), dp(ve)) == ERR_ARG
    assert L.hipsdp_eigencuts_all(s.h, dp(y), tol, -1, k, dp(lmin), dp(ev), dp(co), dp(lh), dp(ve)) == ERR_ARG
    assert L.hipsdp_eigencuts_all(s.h, dp(y), tol, MAXCUTS, k, dp(lmin), NUL, dp(co), dp(lh), dp(ve)) == ERR_ARG
    assert L.hipsdp_eigencuts_all(s.h, dp(y), tol, MAXCUTS, k, dp(lmin), dp(ev), NUL, dp(lh), dp(ve)) == ERR_ARG
    assert L.hipsdp_eigencuts_all(s.h, dp(y), tol, MAXCUTS, k, dp(lmin), dp(ev), dp(co), NUL, dp(ve)) == ERR_ARG
    assert gpu.eigencuts_all_stats() == before              # nothing launched, nothing counted
    unshaped.close()
    # lmin and vecs may be NULL
    assert L.hipsdp_eigencuts_all(s.h, dp(y), tol, MAXCUTS, k, NUL, dp(ev), dp(co), dp(lh), NUL) == 0
    full = s.eigencuts_all(y, TOL, MAXCUTS)
    assert [k[i] for i in range(nb)] == [len(r[1]) for r in full]
    assert np.array_equal(ev[:len(full[0][1])], full[0][1])
    # maxcuts = 0: the feasibility check alone
    k2 = (C.c_int * nb)(*([7] * nb))
    assert L.hipsdp_eigencuts_all(s.h, dp(y), tol, 0, k2, dp(lmin), NUL, NUL, NUL, NUL) == 0
    assert [k2[i] for i in range(nb)] == [0] * nb
    assert np.array_equal(lmin, np.array([r[0] for r in full]))
    r0 = s.eigencuts_all(y, TOL, 0)
    assert all(len(r[1]) == 0 and r[0] == f[0] for r, f in zip(r0, full))
    s.close()


def test_one_variable_one_block_and_lp_rows(gpu):
    # m = 1
    blocks, ys, y, b = family([12, 30], 1, (), 5)
    s = load_dense(gpu, blocks, b)
    res = s.eigencuts_all(y, TOL, MAXCUTS)
    for k, A in enumerate(blocks):
        rev, rco, rlh, rve = eigcuts_ref.cuts_dense(A, y, TOL, MAXCUTS)
        assert len(res[k][1]) == len(rev)
        assert abs(res[k][0] - lmin_ref(A, y)) <= 1e-9 * max(1.0, abs(res[k][0]))
        if len(rev):
            assert np.max(np.abs(res[k][1] - rev)) <= 1e-9 * max(1.0, np.max(np.abs(rev)))
            assert np.max(np.abs(res[k][2] - rco)) <= 1e-6 * max(1.0, np.max(np.abs(rco)))
    s.close()
    # one block, and LP rows beside the blocks (ignored by the round)
    for ns, q in [([24], 0), ([24, 70], 6)]:
        blocks, ys, y, b = family(ns, 10, (), 6)
        rng = np.random.default_rng(3)
        D = rng.standard_normal((q, 10)) if q else None
        c = D @ ys - rng.uniform(0.1, 1.0, q) if q else None
        s = load_dense(gpu, blocks, b, D, c)
        res = s.eigencuts_all(y, TOL, MAXCUTS)
        assert len(res) == len(ns)
        for k, A in enumerate(blocks):
            rev, rco, rlh, rve = eigcuts_ref.cuts_dense(A, y, TOL, MAXCUTS)
            assert len(res[k][1]) == len(rev) and len(rev) >= 1
            assert np.max(np.abs(res[k][1] - rev)) <= 1e-9 * max(1.0, np.max(np.abs(rev)))
            assert np.max(np.abs(res[k][2] - rco)) <= 1e-6 * max(1.0, np.max(np.abs(rco)))
            assert np.max(np.abs(res[k][3] - rlh)) <= 1e-6 * max(1.0, np.max(np.abs(rlh)))
        s.close()
