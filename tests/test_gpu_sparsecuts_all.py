"""GPU: hipsdp_sparsecuts_all - the sparse eigenvector cuts (separation mode `multiplesparsecuts`, truncated power method) of ALL
blocks in one call (csrc/sparsecuts.hip) - against the numpy restatement tests/harness/sparsecuts_ref.py, for the properties that
need no oracle, in the three storage forms of a block, and for what makes it a batch: bits that do not depend on the other blocks,
a launch and read-back count that does not depend on the number of blocks, cuts or iterations.  k_sc_tpower alone
(hipsdp_sparsecuts_unit) runs on hand-made matrices: exact ties, the iteration cap, a zero iterate, the extreme sizes.

The families are those of tests/test_gpu_eigencuts_all.py (block k of sizes ns is instances.planted_dense(n_k, m, seed = 20240 +
1000 k) with the constant matrix rebuilt around the common ys of block 0, minus 10 I for the quiet blocks; the point is ys + 0.7
N(0, 1)).  The truncated power method takes data-dependent decisions (which entries stay, when to stop, whether to cut); counts,
supports and iteration numbers are compared only after the restatement has shown that none of its decisions was close: selection
gap >= 1e-9 relative, the two thresholds missed by >= 1e-11 (the restatement on these cases: >= 2.7e-5, >= 5.8e-10, >= 6.8e-7, so rounding
differences of 1e-12 relative move no count, support or iteration number)."""
import ctypes as C
import threading
import numpy as np
import pytest
import instances
import ipm_ref
import sparsecuts_ref as R

pytestmark = pytest.mark.gpu

TOL, FEASTOL, MAXCUTS = 1e-6, 1e-6, 5
#            sizes                                   m   quiet    seed
FAMILIES = [([3, 9, 10, 17, 33, 64, 65, 100, 128], 20, (2, 5), 0),
            ([12] * 32, 15, (), 1),
            ([40] * 4, 15, (), 1),
            ([16, 150, 48, 200, 10], 25, (2,), 2)]
# (family, target size): cuts of the restatement over all blocks (a numpy prototype of the algorithm gave the same)
CASES = {(0, 2): 4, (0, 4): 10, (0, 10): 18, (1, 4): 64, (2, 4): 5, (2, 10): 17, (3, 4): 6, (3, 10): None}

_fam, _ref, _dev = {}, {}, {}


def family(fam):
    """(blocks [A_k (m + 1, n_k, n_k)], ys, y, b)"""
    if fam not in _fam:
        ns, m, quiet, seed = FAMILIES[fam]
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
        _fam[fam] = (blocks, ys, y, b)
    return _fam[fam]


def served(n):
    return n <= 128


def reference(fam, size):
    """the restatement of every served block, computed once; its margins are asserted here, before anything is compared with it"""
    if (fam, size) not in _ref:
        blocks, ys, y, b = family(fam)
        out = []
        for k, A in enumerate(blocks):
            if not served(A.shape[1]):
                out.append(None)
                continue
            r = R.sparse_cuts_dense(A, y, size, TOL, FEASTOL, MAXCUTS)
            mg = r[9]
            print("restatement family %d size %d block %d (n = %d): %d cuts, %d iterations, longest run %d, margins %.2e %.2e %.2e"
                  % (fam, size, k, A.shape[1], r[0], r[7], mg.longest, mg.select, mg.conv, mg.feas))
            assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11, (fam, size, k)
            assert mg.longest <= R.MAXIT // 10, (fam, size, k)
            assert r[8] == 0
            out.append(r)
        _ref[(fam, size)] = out
    return _ref[(fam, size)]


def load_dense(gpu, blocks, b):
    s = gpu.Solver(0)
    s.load_core(ipm_ref.CoreProblem(b, blocks, None, None))
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


def device(gpu, fam, size):
    """the call on the family loaded as dense matrices (blocks of up to 64 rows stay dense rows, larger ones are swept as packed
    lower triangles), once per (family, size)"""
    if (fam, size) not in _dev:
        blocks, ys, y, b = family(fam)
        s = load_dense(gpu, blocks, b)
        _dev[(fam, size)] = s.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS)
        s.close()
    return _dev[(fam, size)]


def support(v):
    return list(np.nonzero(v)[0])


def same_bits(ra, rb):
    if len(ra) != len(rb):
        return False
    for a, b_ in zip(ra, rb):
        if a[0] != b_[0] or a[6:] != b_[6:] or not (a[1] == b_[1] or (np.isnan(a[1]) and np.isnan(b_[1]))):
            return False
        if not all(np.array_equal(u, v) for u, v in zip(a[2:6], b_[2:6])):
            return False
    return True


@pytest.mark.parametrize("fam,size", sorted(CASES))
def test_every_block_matches_the_restatement(gpu, fam, size):
    blocks, ys, y, b = family(fam)
    ref = reference(fam, size)
    res = device(gpu, fam, size)
    assert len(res) == len(blocks)
    total = 0
    for k, A in enumerate(blocks):
        nc, lmin, ev, co, lh, ve, iters, flags = res[k]
        if ref[k] is None:
            assert nc == -1, k
            continue
        rn, rl, rev, rco, rlh, rve, rsup, rit, rfl, mg = ref[k]
        print("family %d size %d block %d (n = %d): ncuts %d / %d, iterations %d / %d, flags %d, lmin %.12g / %.12g"
              % (fam, size, k, A.shape[1], nc, rn, iters, rit, flags, lmin, rl))
        assert nc == rn, k
        assert iters == rit, k
        assert flags == 0, k
        assert abs(lmin - rl) <= 1e-9 * max(1.0, abs(rl)), k
        if size > A.shape[1] or k in FAMILIES[fam][2]:
            assert nc == 0, k
        total += nc
        for c in range(nc):
            assert support(ve[c]) == list(rsup[c]), (k, c)
            assert abs(ev[c] - rev[c]) <= 1e-9 * max(1.0, abs(rev[c])), (k, c)
            assert abs(abs(ve[c] @ rve[c]) - 1.0) <= 1e-6, (k, c)
            assert np.max(np.abs(co[c] - rco[c])) <= 1e-6 * max(1.0, np.max(np.abs(rco[c]))), (k, c)
            assert abs(lh[c] - rlh[c]) <= 1e-6 * max(1.0, abs(rlh[c])), (k, c)
    if CASES[(fam, size)] is not None:
        assert total == CASES[(fam, size)]
    if (fam, size) == (0, 2):
        assert [r[0] for r in res] == [1, 1, 0, 1, 1, 0, 0, 0, 0]
    if (fam, size) == (3, 4):
        assert [r[0] for r in res] == [2, -1, 0, -1, 4]
    if (fam, size) == (3, 10):
        assert res[4][0] >= 1          # the block of 10 rows with size == n


@pytest.mark.parametrize("fam,size", sorted(CASES))
def test_properties_that_need_no_oracle(gpu, fam, size):
    blocks, ys, y, b = family(fam)
    res = device(gpu, fam, size)
    for k, A in enumerate(blocks):
        nc, lmin, ev, co, lh, ve, iters, flags = res[k]
        for c in range(max(nc, 0)):
            x = ve[c]
            assert abs(np.linalg.norm(x) - 1.0) <= 1e-10, (k, c)
            assert len(support(x)) <= size, (k, c)
            viol = co[c] @ y - lh[c]
            want = ev[c] + sum(ev[j] * (ve[j] @ x) ** 2 for j in range(c))
            assert abs(viol - want) <= 1e-8, (k, c, viol, want)
            assert viol <= ev[c] + 1e-8 and viol < -FEASTOL, (k, c, viol)
            assert co[c] @ ys - lh[c] >= -1e-9, (k, c)


def test_the_three_storage_forms_give_the_same_cuts(gpu):
    """family 1 loaded dense has blocks swept as dense rows (up to 64 rows) and as packed lower triangles (above); loaded as
    triplets every block is kept as nonzeros: the same counts and supports, values to 1e-9"""
    fam, size = 0, 4
    blocks, ys, y, b = family(fam)
    rd = device(gpu, fam, size)
    ss = load_sparse(gpu, blocks, b)
    for k in range(len(blocks)):
        assert ss.is_sparse(k), k
    rs = ss.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS)
    ss.close()
    assert sum(r[0] for r in rs) == CASES[(fam, size)]
    for k in range(len(blocks)):
        (nd, ld, ed, cd, hd, vd, itd, fd), (n_s, ls, es, cs, hs, vs, its, fs) = rd[k], rs[k]
        assert nd == n_s and itd == its and fd == fs == 0, k
        assert abs(ld - ls) <= 1e-9 * max(1.0, abs(ld))
        for c in range(nd):
            assert support(vd[c]) == support(vs[c]), (k, c)
            assert abs(ed[c] - es[c]) <= 1e-9 * max(1.0, abs(ed[c])), (k, c)
            assert np.max(np.abs(vd[c] - vs[c])) <= 1e-9, (k, c)
            assert np.max(np.abs(cd[c] - cs[c])) <= 1e-9 * max(1.0, np.max(np.abs(cd[c]))), (k, c)
            assert abs(hd[c] - hs[c]) <= 1e-9 * max(1.0, abs(hd[c])), (k, c)


def test_a_block_alone_and_a_second_call_return_the_same_bits(gpu):
    fam, size = 0, 4
    blocks, ys, y, b = family(fam)
    full = device(gpu, fam, size)
    s = load_dense(gpu, blocks, b)
    again = s.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS)
    assert same_bits(again, full)
    assert same_bits(s.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS), full)
    s.close()
    for k in (1, 3, 4, 6, 8):               # 9, 17, 33 rows (dense rows), 65 and 128 rows (packed)
        s1 = load_dense(gpu, [blocks[k]], b)
        alone = s1.sparsecuts_all(y, [size], TOL, FEASTOL, MAXCUTS)
        s1.close()
        assert same_bits(alone, [full[k]]), k


def test_launches_and_readbacks_do_not_depend_on_blocks_cuts_or_iterations(gpu):
    fam, size = 1, 4
    blocks, ys, y, b = family(fam)
    deltas = {}
    for nblk in (1, 32):
        s = load_dense(gpu, blocks[:nblk], b)
        s.sparsecuts_all(y, [size] * nblk, TOL, FEASTOL, MAXCUTS)               # first use (workspace, job table)
        for mc in (MAXCUTS, 1, 0):
            c0, l0, r0 = gpu.sparsecuts_all_stats()
            res = s.sparsecuts_all(y, [size] * nblk, TOL, FEASTOL, mc)
            c1, l1, r1 = gpu.sparsecuts_all_stats()
            assert c1 - c0 == 1
            deltas[(nblk, mc)] = (l1 - l0, r1 - r0)
            print("%d blocks, maxcuts %d: %d launches, %d read-backs, %d iterations" % (nblk, mc, l1 - l0, r1 - r0, sum(r[6] for r in res)))
            if mc == 0:
                ea = s.eigencuts_all(y, TOL, 0)
                assert all(r[0] == 0 and r[6] == 0 for r in res)
                assert [r[1] for r in res] == [e[0] for e in ea]           # lmin: the bits of hipsdp_eigencuts_all
        s.close()
    for mc in (MAXCUTS, 1, 0):
        assert deltas[(1, mc)] == deltas[(32, mc)], deltas
    launches, readbacks = deltas[(32, MAXCUTS)]
    assert deltas[(32, 1)] == (launches, readbacks)
    assert 4 <= launches <= 6 and readbacks == 1
    assert deltas[(32, 0)] == (launches - 1, 1)


def _raw_call(gpu, s, y, sizes, maxcuts, fill, opts=None, null=()):
    """the C entry itself on arrays filled with a sentinel; null: names of the arguments to pass as NULL"""
    L = gpu.lib()
    nb, m = len(s.ns), len(y)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    mc = max(1, maxcuts)
    arr = dict(ncuts=np.full(nb, 77, dtype=np.int32), lmin=np.full(nb, fill), eigvals=np.full(nb * mc, fill),
               coefs=np.full(nb * mc * m, fill), lhs=np.full(nb * mc, fill), vecs=np.full(mc * sum(s.ns), fill),
               iters=np.full(nb, 77, dtype=np.int32), flags=np.full(nb, 77, dtype=np.int32))
    y = np.ascontiguousarray(y, dtype=np.float64)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    if opts is None:
        opts = gpu.SparsecutOpts(TOL, FEASTOL, 0.0, maxcuts, 0)
    ptr = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in arr.items()}
    rc = L.hipsdp_sparsecuts_all(None if "solver" in null else s.h, None if "y" in null else dp(y),
                                 None if "sizes" in null else ip(sizes), None if "opts" in null else C.byref(opts),
                                 ptr["ncuts"], ptr["lmin"], ptr["eigvals"], ptr["coefs"], ptr["lhs"], ptr["vecs"], ptr["iters"], ptr["flags"])
    return rc, arr


def test_blocks_that_are_not_served_return_minus_one_and_keep_their_slots(gpu):
    fam, size = 3, 4
    ns, m = FAMILIES[fam][0], FAMILIES[fam][1]
    blocks, ys, y, b = family(fam)
    full = device(gpu, fam, size)
    s = load_dense(gpu, blocks, b)
    fill = 777.0
    rc, a = _raw_call(gpu, s, y, [size] * len(ns), MAXCUTS, fill)
    s.close()
    assert rc == 0
    assert list(a["ncuts"]) == [2, -1, 0, -1, 4] == [r[0] for r in full]
    off = 0
    for k, n in enumerate(ns):
        kept = max(int(a["ncuts"][k]), 0)
        sl = slice(k * MAXCUTS + kept, (k + 1) * MAXCUTS)
        assert np.all(a["eigvals"][sl] == fill) and np.all(a["lhs"][sl] == fill), k
        assert np.all(a["coefs"][sl.start * m:sl.stop * m] == fill), k
        assert np.all(a["vecs"][off + kept * n:off + MAXCUTS * n] == fill), k
        if kept:
            assert np.array_equal(a["eigvals"][k * MAXCUTS:k * MAXCUTS + kept], full[k][2])
            assert np.array_equal(a["vecs"][off:off + kept * n].reshape(kept, n), full[k][5])
        if n > 128:
            assert a["lmin"][k] == fill and a["iters"][k] == 77 and a["flags"][k] == 77, k
        else:
            assert a["lmin"][k] == full[k][1] and a["iters"][k] == full[k][6] and a["flags"][k] == 0, k
        off += MAXCUTS * n


def test_a_target_size_above_the_block_gives_no_cut_and_the_right_lmin(gpu):
    fam = 2
    blocks, ys, y, b = family(fam)
    ns = FAMILIES[fam][0]
    sizes = [ns[0] + 1, 4, ns[2], 1000]
    ref4 = reference(fam, 4)
    s = load_dense(gpu, blocks, b)
    res = s.sparsecuts_all(y, sizes, TOL, FEASTOL, MAXCUTS)
    s.close()
    for k in (0, 3):
        assert res[k][0] == 0 and res[k][6] == 0 and res[k][7] == 0
        assert res[k][1] < -TOL
        assert abs(res[k][1] - ref4[k][1]) <= 1e-9 * max(1.0, abs(ref4[k][1]))
    assert same_bits([res[1]], [device(gpu, fam, 4)[1]])
    assert res[2][0] >= 1 and len(support(res[2][5][0])) <= ns[2]       # size == n: the plain power method


def test_argument_errors_launch_nothing(gpu):
    fam = 2
    blocks, ys, y, b = family(fam)
    nb = len(blocks)
    s = load_dense(gpu, blocks, b)
    unshaped = gpu.Solver(0)
    ERR_ARG = 3
    before = gpu.sparsecuts_all_stats()
    sz = [4] * nb
    assert _raw_call(gpu, s, y, sz, MAXCUTS, 0.0, null=("solver",))[0] == ERR_ARG
    assert _raw_call(gpu, unshaped, y, [], MAXCUTS, 0.0)[0] == ERR_ARG
    for name in ("y", "sizes", "opts", "ncuts", "eigvals", "coefs", "lhs"):
        assert _raw_call(gpu, s, y, sz, MAXCUTS, 0.0, null=(name,))[0] == ERR_ARG, name
    assert _raw_call(gpu, s, y, sz, -1, 0.0, opts=gpu.SparsecutOpts(TOL, FEASTOL, 0.0, -1, 0))[0] == ERR_ARG
    assert _raw_call(gpu, s, y, [4, 4, 0, 4], MAXCUTS, 0.0)[0] == ERR_ARG
    assert _raw_call(gpu, s, y, [4, -3, 4, 4], MAXCUTS, 0.0)[0] == ERR_ARG
    assert gpu.sparsecuts_all_stats() == before              # nothing launched, nothing counted
    unshaped.close()
    # lmin, vecs, iters and flags may be NULL; with maxcuts = 0 also eigvals, coefs and lhs
    rc, a = _raw_call(gpu, s, y, sz, MAXCUTS, 0.0, null=("lmin", "vecs", "iters", "flags"))
    assert rc == 0 and list(a["ncuts"]) == [r[0] for r in device(gpu, fam, 4)]
    assert np.array_equal(a["eigvals"][:a["ncuts"][0]], device(gpu, fam, 4)[0][2])
    rc, a = _raw_call(gpu, s, y, sz, 0, 0.0, null=("eigvals", "coefs", "lhs", "vecs"))
    assert rc == 0 and list(a["ncuts"]) == [0] * nb
    assert list(a["lmin"]) == [r[1] for r in device(gpu, fam, 4)]
    s.close()


def _unit_case(rng, n, scale=1.0):
    """a symmetric matrix with a clear most negative direction, a start vector near its smallest eigenvector (not normalised: TPower
    does not need it) and its largest eigenvalue (numpy)"""
    G = rng.standard_normal((n, n))
    u = rng.standard_normal(n)
    u /= np.linalg.norm(u)
    Z = scale * (0.05 * (G + G.T) - 3.0 * np.outer(u, u))
    Z = 0.5 * (Z + Z.T)
    lam, V = np.linalg.eigh(Z)
    return Z, V[:, 0] + 0.2 * rng.standard_normal(n), float(lam[-1])


def test_unit_exact_ties_keep_the_smaller_indices(gpu):
    """Z = -ones with v0 = ones (6 rows, size 3) and with v0 = +-1 alternating (5 rows, size 2): every entry of the first iterate
    has the same absolute value, exactly (sums of small integers), in every later iterate of that run the kept entries tie among
    themselves; the smaller indices stay.  maxcuts = 1: the run behind the cut of the 6-row matrix sees the other three rows lead
    (9 against 6), so its iterations compare too; behind the cut of the 5-row matrix rows tie up to rounding only, so of that
    matrix the first cut alone is compared."""
    ns, sizes = [6, 5], [3, 2]
    Zs = [-np.ones((6, 6)), -np.ones((5, 5))]
    v0s = [np.ones(6), np.array([1.0, -1.0, 1.0, -1.0, 1.0])]
    res = gpu.sparsecuts_unit(ns, Zs, v0s, [0.0, 0.0], sizes, FEASTOL, 1)
    for j in range(2):
        rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Zs[j], v0s[j], 0.0, sizes[j], FEASTOL, 1)
        nc, ev, ve, it, fl = res[j]
        print("ties, matrix %d: %d cuts (restatement %d), values %s, iterations %d / %d" % (j, nc, len(rv), ev, it, rit))
        assert nc == len(rv) == 1 and fl == rfl == 0
        assert support(ve[0]) == list(range(sizes[j])) == list(rsup[0])
        assert abs(ev[0] - rv[0]) <= 1e-9 * max(1.0, abs(rv[0]))
        assert np.max(np.abs(np.abs(ve[0][:sizes[j]]) - 1.0 / np.sqrt(sizes[j]))) <= 1e-15
    assert res[0][3] == R.sparse_cuts_matrix(Zs[0], v0s[0], 0.0, 3, FEASTOL, 1)[3] == 4
    assert abs(res[0][1][0] + 3.0) <= 1e-12 and abs(res[1][1][0] + 2.0) <= 1e-12


def test_unit_iteration_cap_sets_bit_0_and_uses_the_iterate(gpu):
    rng = np.random.default_rng(77)
    Z, v0, maxeig = _unit_case(rng, 40)
    rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, maxeig, 6, FEASTOL, 1, maxit=3)
    free = R.sparse_cuts_matrix(Z, v0, maxeig, 6, FEASTOL, 1)
    assert rfl == 1 and free[4] == 0 and free[3] > rit          # the cap binds
    assert mg.select >= 1e-9 and mg.feas >= 1e-11
    nc, ev, ve, it, fl = gpu.sparsecuts_unit([40], [Z], [v0], [maxeig], [6], FEASTOL, 1, maxit=3)[0]
    print("cap 3: %d cuts / %d, iterations %d / %d, flags %d" % (nc, len(rv), it, rit, fl))
    assert fl == 1 and it == rit and nc == len(rv) == 1
    assert it == 3 * 2                                           # the run before the cut and the run behind it, 3 each
    assert support(ve[0]) == list(rsup[0])
    assert abs(abs(ve[0] @ rx[0]) - 1.0) <= 1e-6 and abs(ev[0] - rv[0]) <= 1e-9 * max(1.0, abs(rv[0]))


def test_unit_zero_iterate_sets_bit_1_and_gives_no_cut(gpu):
    n = 4
    Z = -2.0 * np.eye(n)
    v0 = np.array([1.0, 0.0, 0.0, 0.0])
    rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, -2.0, 2, FEASTOL, 3)
    assert len(rv) == 0 and rfl == 2 and rit == 0
    nc, ev, ve, it, fl = gpu.sparsecuts_unit([n], [Z], [v0], [-2.0], [2], FEASTOL, 3)[0]
    assert (nc, it, fl) == (0, 0, 2)


def test_unit_extreme_sizes(gpu):
    """1, 2, 64, 65 and 128 rows with size 1 and size n, all in ONE launch; each against the restatement, margins first"""
    rng = np.random.default_rng(20260)
    ns, Zs, v0s, me, sizes = [], [], [], [], []
    for n in (1, 2, 64, 65, 128):
        for size in sorted({1, n}):
            Z, v0, maxeig = _unit_case(rng, n)
            if n == 1:
                maxeig = 0.0            # (with its own eigenvalue M is the zero matrix: the case of the test above)
            ns.append(n); Zs.append(Z); v0s.append(v0); me.append(maxeig); sizes.append(size)
    res = gpu.sparsecuts_unit(ns, Zs, v0s, me, sizes, FEASTOL, 3)
    for j, n in enumerate(ns):
        rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Zs[j], v0s[j], me[j], sizes[j], FEASTOL, 3)
        nc, ev, ve, it, fl = res[j]
        print("n %d size %d: %d cuts / %d, iterations %d / %d, margins %.2e %.2e %.2e" % (n, sizes[j], nc, len(rv), it, rit, mg.select,
                                                                                           mg.conv, mg.feas))
        assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11 and mg.longest <= R.MAXIT // 5, (n, sizes[j])
        assert nc == len(rv) >= 1 and it == rit and fl == rfl == 0, (n, sizes[j])
        for c in range(nc):
            assert support(ve[c]) == list(rsup[c]), (n, sizes[j], c)
            assert abs(np.linalg.norm(ve[c]) - 1.0) <= 1e-10
            assert abs(ev[c] - rv[c]) <= 1e-9 * max(1.0, abs(rv[c])), (n, sizes[j], c)
            assert abs(abs(ve[c] @ rx[c]) - 1.0) <= 1e-6, (n, sizes[j], c)


def test_two_host_threads_reproduce_the_single_thread_bits(gpu):
    cases = [(1, 4), (2, 4)]
    data = [family(f) for f, _ in cases]
    solvers = [load_dense(gpu, d[0], d[3]) for d in data]
    single = [device(gpu, f, sz) for f, sz in cases]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(4):
                got[i].append(solvers[i].sparsecuts_all(data[i][2], [cases[i][1]] * len(data[i][0]), TOL, FEASTOL, MAXCUTS))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 4
        for r in got[i]:
            assert same_bits(r, single[i])
    for s in solvers:
        s.close()
