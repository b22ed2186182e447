"""GPU: hipsdp_sparsecuts - the sparse eigenvector cuts (separation mode `multiplesparsecuts`, truncated power method) of ONE block of
up to 512 rows - against the numpy restatement tests/harness/sparsecuts_ref.py on the cases of tests/harness/
sparsecuts_large_cases.py, for the properties that need no oracle, in the storage forms of a block, for blocks of at most 128 rows
against hipsdp_sparsecuts_all, and for what makes it one call: n + 7 launches and one read-back whatever the cuts and iterations.
k_sc_tpower_large alone (hipsdp_sparsecuts_large_unit) runs on the matrices of the table and on hand-made ones: exact ties, the
iteration cap, a zero iterate, the extreme sizes.  A last test alternates all cut calls on ONE solver - they share a grow-only workspace
and the cached job tables - and compares every call with the same call on a fresh solver, bit for bit.

The truncated power method takes data-dependent decisions; counts, supports and iteration numbers are compared only after the
restatement has shown that none of its decisions was close (sparsecuts_large_cases.reference asserts: selection gap >= 1e-9
relative, the two thresholds missed by >= 1e-11, longest run <= MAXIT / 10).  The device's v0 and maxeig come from the stages of
hipsdp_syevx, not from numpy.linalg.eigh: the cases were checked to keep every count, support and iteration number under
perturbations of 1e-12 .. 1e-8 of both."""
import ctypes as C
import threading
import numpy as np
import pytest
import instances
import ipm_ref
import sparsecuts_ref as R
import sparsecuts_large_cases as L

pytestmark = pytest.mark.gpu

TOL, FEASTOL, MAXCUTS = L.TOL, L.FEASTOL, L.MAXCUTS
CASE_IDS = ["%s-size%d" % (t[0], t[2]) for t in L.TABLE]
NEW_ROWS = [t for t in L.TABLE if t[1][0] == "own"]
ERR_ARG = 3

_dev = {}


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


def device(gpu, spec, size):
    """the call on the block loaded dense and alone (swept as packed lower triangles), once per case"""
    if (spec, size) not in _dev:
        A, ys, y, b = L.block(spec)
        s = load_dense(gpu, [A], b)
        _dev[(spec, size)] = s.sparsecuts(0, y, size, TOL, FEASTOL, MAXCUTS)
        s.close()
    return _dev[(spec, size)]


def support(v):
    return list(np.nonzero(v)[0])


def same_bits(a, b_):
    if a[0] != b_[0] or a[6:] != b_[6:] or not (a[1] == b_[1] or (np.isnan(a[1]) and np.isnan(b_[1]))):
        return False
    return all(np.array_equal(u, v) for u, v in zip(a[2:6], b_[2:6]))


def compare_with_restatement(res, ref, what):
    nc, lmin, ev, co, lh, ve, iters, flags = res
    rn, rl, rev, rco, rlh, rve, rsup, rit, rfl, mg = ref
    print("%s: ncuts %d / %d, iterations %d / %d, flags %d, lmin %.12g / %.12g" % (what, nc, rn, iters, rit, flags, lmin, rl))
    assert nc == rn, what
    assert iters == rit, what
    assert flags == 0, what
    assert abs(lmin - rl) <= 1e-9 * max(1.0, abs(rl)), what
    for c in range(nc):
        assert support(ve[c]) == list(rsup[c]), (what, c)
        assert abs(ev[c] - rev[c]) <= 1e-9 * max(1.0, abs(rev[c])), (what, c)
        assert abs(abs(ve[c] @ rve[c]) - 1.0) <= 1e-6, (what, c)
        if co.shape[1] > 0:
            assert np.max(np.abs(co[c] - rco[c])) <= 1e-6 * max(1.0, np.max(np.abs(rco[c]))), (what, c)
        assert abs(lh[c] - rlh[c]) <= 1e-6 * max(1.0, abs(rlh[c])), (what, c)


# ---- 1. the kernel alone --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,spec,size,cuts,its", NEW_ROWS, ids=["%s-size%d" % (t[0], t[2]) for t in NEW_ROWS])
def test_unit_matches_the_restatement_from_the_same_inputs(gpu, name, spec, size, cuts, its):
    Z, v0, maxeig = L.matrix_inputs(spec)
    n = Z.shape[0]
    rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, maxeig, size, FEASTOL, MAXCUTS)
    assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11 and mg.longest <= R.MAXIT // 10
    assert (len(rv), rit, rfl) == (cuts, its, 0)
    nc, ev, ve, it, fl = gpu.sparsecuts_large_unit(n, Z, v0, maxeig, size, FEASTOL, MAXCUTS)
    print("unit n %d size %d: %d cuts / %d, iterations %d / %d, flags %d" % (n, size, nc, cuts, it, its, fl))
    assert (nc, it, fl) == (cuts, its, 0)
    for c in range(nc):
        assert support(ve[c]) == list(rsup[c]), c
        assert abs(ev[c] - rv[c]) <= 1e-9 * max(1.0, abs(rv[c])), c
        assert abs(abs(ve[c] @ rx[c]) - 1.0) <= 1e-6, c


def _unit_case(rng, n, scale=1.0):
    """a symmetric matrix with a clear most negative direction, a start vector near its smallest eigenvector (not normalised) and its
    largest eigenvalue (numpy): the construction of tests/test_gpu_sparsecuts_all.py"""
    G = rng.standard_normal((n, n))
    u = rng.standard_normal(n)
    u /= np.linalg.norm(u)
    Z = scale * (0.05 * (G + G.T) - 3.0 * np.outer(u, u))
    Z = 0.5 * (Z + Z.T)
    lam, V = np.linalg.eigh(Z)
    return Z, V[:, 0] + 0.2 * rng.standard_normal(n), float(lam[-1])


def test_unit_exact_ties_keep_the_smaller_indices(gpu):
    """Z = -ones (130 rows), v0 = ones, size 3: every entry of the first iterate has the same absolute value, exactly (sums of small
    integers), in every later iterate of that run the kept entries tie among themselves; the indices 0, 1, 2 stay"""
    n = 130
    Z, v0 = -np.ones((n, n)), np.ones(n)
    rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, 0.0, 3, FEASTOL, 1)
    nc, ev, ve, it, fl = gpu.sparsecuts_large_unit(n, Z, v0, 0.0, 3, FEASTOL, 1)
    print("ties: %d cuts (restatement %d), values %s, iterations %d / %d" % (nc, len(rv), ev, it, rit))
    assert nc == len(rv) == 1 and fl == rfl == 0
    assert support(ve[0]) == [0, 1, 2] == list(rsup[0])
    assert abs(ev[0] - rv[0]) <= 1e-9 * max(1.0, abs(rv[0])) and abs(ev[0] + 3.0) <= 1e-12
    assert np.max(np.abs(np.abs(ve[0][:3]) - 1.0 / np.sqrt(3.0))) <= 1e-15
    assert it == rit == 4       # behind the cut rows 3 .. 129 lead (133 against 130) and tie: 3, 4, 5 stay, two iterations again


def test_unit_iteration_cap_sets_bit_0_and_uses_the_iterate(gpu):
    rng = np.random.default_rng(77)
    n = 140
    Z, v0, maxeig = _unit_case(rng, n)
    rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, maxeig, 6, FEASTOL, 1, maxit=3)
    free = R.sparse_cuts_matrix(Z, v0, maxeig, 6, FEASTOL, 1)
    assert rfl == 1 and free[4] == 0 and free[3] > rit          # the cap binds
    assert mg.select >= 1e-9 and mg.feas >= 1e-11
    nc, ev, ve, it, fl = gpu.sparsecuts_large_unit(n, Z, v0, maxeig, 6, FEASTOL, 1, maxit=3)
    print("cap 3: %d cuts / %d, iterations %d / %d, flags %d" % (nc, len(rv), it, rit, fl))
    assert fl == 1 and it == rit and nc == len(rv) == 1
    assert it == 3 * 2                                           # the run before the cut and the run behind it, 3 each
    assert support(ve[0]) == list(rsup[0])
    assert abs(abs(ve[0] @ rx[0]) - 1.0) <= 1e-6 and abs(ev[0] - rv[0]) <= 1e-9 * max(1.0, abs(rv[0]))


def test_unit_zero_iterate_sets_bit_1_and_gives_no_cut(gpu):
    n = 131
    Z = -2.0 * np.eye(n)
    v0 = np.zeros(n)
    v0[0] = 1.0
    rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, -2.0, 2, FEASTOL, 3)
    assert len(rv) == 0 and rfl == 2 and rit == 0
    nc, ev, ve, it, fl = gpu.sparsecuts_large_unit(n, Z, v0, -2.0, 2, FEASTOL, 3)
    assert (nc, it, fl) == (0, 0, 2)


@pytest.mark.parametrize("n", [129, 192, 193, 512])
def test_unit_extreme_sizes(gpu, n):
    """size 1 and size n at the smallest and the largest matrix and on both sides of a wavefront boundary (3 and 3 + 1 / 64
    wavefronts of rows); each against the restatement, margins first.  With size n TPower is the plain power method: its runs take
    up to 2740 iterations on these matrices, so the bound on the longest run is the one that keeps the cap of 10000 out of play
    with room to spare, MAXIT / 2.  With size 1 a cut leaves a matrix whose next candidate is 0 up to rounding: one or two cuts,
    none at 129 rows, where the first candidate is already not negative."""
    rng = np.random.default_rng(20260 + n)
    for size in (1, n):
        Z, v0, maxeig = _unit_case(rng, n)
        rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, maxeig, size, FEASTOL, 3)
        nc, ev, ve, it, fl = gpu.sparsecuts_large_unit(n, Z, v0, maxeig, size, FEASTOL, 3)
        print("n %d size %d: %d cuts / %d, iterations %d / %d, margins %.2e %.2e %.2e" % (n, size, nc, len(rv), it, rit, mg.select,
                                                                                           mg.conv, mg.feas))
        assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11 and mg.longest <= R.MAXIT // 2, (n, size)
        assert nc == len(rv) and it == rit and fl == rfl == 0, (n, size)
        assert nc == 3 or size == 1, (n, size)
        for c in range(nc):
            assert support(ve[c]) == list(rsup[c]), (n, size, c)
            assert abs(np.linalg.norm(ve[c]) - 1.0) <= 1e-10
            assert abs(ev[c] - rv[c]) <= 1e-9 * max(1.0, abs(rv[c])), (n, size, c)
            assert abs(abs(ve[c] @ rx[c]) - 1.0) <= 1e-6, (n, size, c)


@pytest.mark.parametrize("size", [63, 64])
def test_unit_both_sides_of_the_candidate_threshold(gpu, size):
    """below a target size of 64 the kernel ranks inside the wavefronts first and then among the candidates, from 64 on among all
    rows: the last size of the one path and the first of the other on the matrix of 257 rows (two cuts each; the restatement's
    margins there: 2.0e-4, 9.3e-9, 4.3)"""
    Z, v0, maxeig = L.matrix_inputs(("own", 257, 6, 31257, 2.0))
    n = Z.shape[0]
    rv, rx, rsup, rit, rfl, mg = R.sparse_cuts_matrix(Z, v0, maxeig, size, FEASTOL, 2)
    assert mg.select >= 1e-9 and mg.conv >= 1e-11 and mg.feas >= 1e-11 and mg.longest <= R.MAXIT // 10
    assert (len(rv), rit, rfl) == {63: (2, 221, 0), 64: (2, 201, 0)}[size]
    nc, ev, ve, it, fl = gpu.sparsecuts_large_unit(n, Z, v0, maxeig, size, FEASTOL, 2)
    assert (nc, it, fl) == (len(rv), rit, 0)
    for c in range(nc):
        assert support(ve[c]) == list(rsup[c]) and len(rsup[c]) == size, c
        assert abs(ev[c] - rv[c]) <= 1e-9 * max(1.0, abs(rv[c])), c
        assert abs(abs(ve[c] @ rx[c]) - 1.0) <= 1e-6, c


# ---- 2. through the solver, against the restatement ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,spec,size,cuts,its", L.TABLE, ids=CASE_IDS)
def test_every_case_matches_the_restatement(gpu, name, spec, size, cuts, its):
    ref = L.reference(spec, size)
    assert (ref[0], ref[7]) == (cuts, its)              # the fixture itself: the totals of the table
    res = device(gpu, spec, size)
    compare_with_restatement(res, ref, "%s size %d" % (name, size))
    assert (res[0], res[6]) == (cuts, its)


def test_family_4_whole_sparsecuts_fills_the_gaps_of_sparsecuts_all(gpu):
    size = 4
    blocks, ys, y, b = L.family4()
    s = load_dense(gpu, blocks, b)
    full = s.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS)
    assert [r[0] for r in full] == [2, -1, 0, -1, 4]
    for k in (1, 3):
        res = s.sparsecuts(k, y, size, TOL, FEASTOL, MAXCUTS)
        compare_with_restatement(res, L.reference(("f4", k), size), "family 4 block %d" % k)
        assert same_bits(res, device(gpu, ("f4", k), size)), k          # the other blocks of the solver change nothing
    assert [r[0] for r in s.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS)] == [2, -1, 0, -1, 4]
    s.close()


# ---- 3. properties that need no oracle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,spec,size,cuts,its", L.TABLE, ids=CASE_IDS)
def test_properties_that_need_no_oracle(gpu, name, spec, size, cuts, its):
    A, ys, y, b = L.block(spec)
    nc, lmin, ev, co, lh, ve, iters, flags = device(gpu, spec, size)
    for c in range(nc):
        x = ve[c]
        assert abs(np.linalg.norm(x) - 1.0) <= 1e-10, c
        assert len(support(x)) <= size, c
        viol = co[c] @ y - lh[c]
        want = ev[c] + sum(ev[j] * (ve[j] @ x) ** 2 for j in range(c))
        assert abs(viol - want) <= 1e-8, (c, viol, want)
        assert viol < -FEASTOL, (c, viol)
        assert co[c] @ ys - lh[c] >= -1e-9, c


# ---- 4. storage forms -------------------------------------------------------------------------------------------------------------

def test_a_block_kept_as_nonzeros_gives_the_cuts_of_the_dense_block(gpu):
    spec = ("f4", 1)
    A, ys, y, b = L.block(spec)
    for size in (4, 10):
        nd, ld, ed, cd, hd, vd, itd, fd = device(gpu, spec, size)
        ss = load_sparse(gpu, [A], b)
        assert ss.is_sparse(0)
        n_s, ls, es, cs, hs, vs, its, fs = ss.sparsecuts(0, y, size, TOL, FEASTOL, MAXCUTS)
        ss.close()
        assert nd == n_s >= 1 and itd == its and fd == fs == 0, size
        assert abs(ld - ls) <= 1e-9 * max(1.0, abs(ld))
        for c in range(nd):
            assert support(vd[c]) == support(vs[c]), (size, c)
            assert abs(ed[c] - es[c]) <= 1e-9 * max(1.0, abs(ed[c])), (size, c)
            assert np.max(np.abs(vd[c] - vs[c])) <= 1e-9, (size, c)
            assert np.max(np.abs(cd[c] - cs[c])) <= 1e-9 * max(1.0, np.max(np.abs(cd[c]))), (size, c)
            assert abs(hd[c] - hs[c]) <= 1e-9 * max(1.0, abs(hd[c])), (size, c)


# ---- 5. small blocks --------------------------------------------------------------------------------------------------------------

def test_small_blocks_return_the_bits_of_sparsecuts_all(gpu):
    blocks, ys, y, b = L.family4()
    s = load_dense(gpu, blocks, b)
    for size in (4, 10):
        full = s.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS)
        a0 = gpu.sparsecuts_all_stats()
        for k in (0, 2, 4):                     # 16, 48 (quiet) and 10 rows
            one = s.sparsecuts(k, y, size, TOL, FEASTOL, MAXCUTS)
            assert same_bits(one, full[k]), (size, k)
        assert gpu.sparsecuts_all_stats() == a0
        assert same_bits(s.sparsecuts_all(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS)[0], full[0])
    s.close()


# ---- 6. what makes it one call ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("spec", [("f4", 1), ("own", 257, 6, 31257, 2.0)], ids=["n150", "n257"])
def test_launches_and_readbacks_do_not_depend_on_cuts_or_iterations(gpu, spec):
    A, ys, y, b = L.block(spec)
    n = A.shape[1]
    s = load_dense(gpu, [A], b)
    first = s.sparsecuts(0, y, 10, TOL, FEASTOL, MAXCUTS)              # first use (workspace, job table)
    assert same_bits(first, device(gpu, spec, 10))                     # a second solver, a second call: the same bits
    all0 = gpu.sparsecuts_all_stats()
    seen = []
    for size, mc in ((10, MAXCUTS), (4, MAXCUTS), (10, 1), (n + 1, MAXCUTS)):
        c0, l0, r0 = gpu.sparsecuts_stats()
        res = s.sparsecuts(0, y, size, TOL, FEASTOL, mc)
        c1, l1, r1 = gpu.sparsecuts_stats()
        print("n %d size %d maxcuts %d: %d launches, %d read-backs, %d cuts, %d iterations" % (n, size, mc, l1 - l0, r1 - r0, res[0], res[6]))
        assert (c1 - c0, l1 - l0, r1 - r0) == (1, n + 7, 1), (size, mc)
        seen.append((res[0], res[6]))
    assert len(set(seen)) == len(seen)                                  # the four calls differed in cuts or iterations
    assert same_bits(s.sparsecuts(0, y, 10, TOL, FEASTOL, MAXCUTS), first)
    c0, l0, r0 = gpu.sparsecuts_stats()
    nc, lmin, ev, co, lh, ve, iters, flags = s.sparsecuts(0, y, 10, TOL, FEASTOL, 0)
    c1, l1, r1 = gpu.sparsecuts_stats()
    assert (c1 - c0, l1 - l0, r1 - r0) == (1, n + 2, 1)
    assert (nc, iters, flags) == (0, 0, 0) and lmin == first[1]        # lmin: the bits of the full call
    assert gpu.sparsecuts_all_stats() == all0
    s.close()


def test_two_host_threads_reproduce_the_single_thread_bits(gpu):
    cases = [(("f4", 1), 10), (("own", 129, 6, 31129, 2.0), 10)]
    data = [L.block(spec) for spec, _ in cases]
    solvers = [load_dense(gpu, [d[0]], d[3]) for d in data]
    single = [device(gpu, spec, size) for spec, size in cases]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                got[i].append(solvers[i].sparsecuts(0, data[i][2], cases[i][1], TOL, FEASTOL, MAXCUTS))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 3
        for r in got[i]:
            assert same_bits(r, single[i])
    for s in solvers:
        s.close()


# ---- 7. edges ---------------------------------------------------------------------------------------------------------------------

def _raw_call(gpu, s, block, y, size, maxcuts, fill, n, opts=None, null=()):
    """the C entry itself on arrays filled with a sentinel; null: names of the arguments to pass as NULL"""
    lib = gpu.lib()
    m = len(y)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    mc = max(1, maxcuts)
    arr = dict(ncuts=np.full(1, 77, dtype=np.int32), lmin=np.full(1, fill), eigvals=np.full(mc, fill), coefs=np.full(mc * max(1, m), fill),
               lhs=np.full(mc, fill), vecs=np.full(mc * n, fill), iters=np.full(1, 77, dtype=np.int32), flags=np.full(1, 77, dtype=np.int32))
    y = np.ascontiguousarray(y, dtype=np.float64)
    if opts is None:
        opts = gpu.SparsecutOpts(TOL, FEASTOL, 0.0, maxcuts, 0)
    ptr = {k: (None if k in null else (ip(v) if v.dtype == np.int32 else dp(v))) for k, v in arr.items()}
    rc = lib.hipsdp_sparsecuts(None if "solver" in null else s.h, block, None if "y" in null else dp(y), size,
                               None if "opts" in null else C.byref(opts), ptr["ncuts"], ptr["lmin"], ptr["eigvals"], ptr["coefs"],
                               ptr["lhs"], ptr["vecs"], ptr["iters"], ptr["flags"])
    return rc, arr


def test_argument_errors_launch_nothing_and_optional_outputs_may_be_null(gpu):
    spec, size = ("f4", 1), 4
    A, ys, y, b = L.block(spec)
    n = A.shape[1]
    full = device(gpu, spec, size)
    s = load_dense(gpu, [A], b)
    s.sparsecuts(0, y, size, TOL, FEASTOL, MAXCUTS)
    unshaped = gpu.Solver(0)
    before = gpu.sparsecuts_stats()
    assert _raw_call(gpu, s, 0, y, size, MAXCUTS, 0.0, n, null=("solver",))[0] == ERR_ARG
    assert _raw_call(gpu, unshaped, 0, y, size, MAXCUTS, 0.0, n)[0] == ERR_ARG
    for blk in (-1, 1):
        assert _raw_call(gpu, s, blk, y, size, MAXCUTS, 0.0, n)[0] == ERR_ARG, blk
    for name in ("y", "opts", "ncuts", "eigvals", "coefs", "lhs"):
        assert _raw_call(gpu, s, 0, y, size, MAXCUTS, 0.0, n, null=(name,))[0] == ERR_ARG, name
    for bad in (0, -3):
        assert _raw_call(gpu, s, 0, y, bad, MAXCUTS, 0.0, n)[0] == ERR_ARG, bad
    assert _raw_call(gpu, s, 0, y, size, -1, 0.0, n, opts=gpu.SparsecutOpts(TOL, FEASTOL, 0.0, -1, 0))[0] == ERR_ARG
    assert gpu.sparsecuts_stats() == before                 # nothing launched, nothing counted
    unshaped.close()
    # lmin, vecs, iters and flags may be NULL, each alone and together; with maxcuts = 0 also eigvals, coefs and lhs
    fill = 777.0
    for null in (("lmin",), ("vecs",), ("iters",), ("flags",), ("lmin", "vecs", "iters", "flags")):
        rc, a = _raw_call(gpu, s, 0, y, size, MAXCUTS, fill, n, null=null)
        k = full[0]
        assert rc == 0 and a["ncuts"][0] == k >= 1, null
        assert np.array_equal(a["eigvals"][:k], full[2]) and np.all(a["eigvals"][k:] == fill), null
        assert np.array_equal(a["lhs"][:k], full[4]) and np.all(a["lhs"][k:] == fill), null
        assert np.array_equal(a["coefs"][:k * len(y)].reshape(k, -1), full[3]) and np.all(a["coefs"][k * len(y):] == fill), null
        assert np.array_equal(a["vecs"][:k * n].reshape(k, n), full[5]) or "vecs" in null, null
        assert np.all(a["vecs"][k * n:] == fill), null          # slots c >= ncuts are not written
        assert (a["lmin"][0] == full[1]) != ("lmin" in null) and (a["iters"][0] == full[6]) != ("iters" in null), null
        assert (a["flags"][0] == 0) != ("flags" in null), null
    rc, a = _raw_call(gpu, s, 0, y, size, 0, fill, n, null=("eigvals", "coefs", "lhs", "vecs"))
    assert rc == 0 and a["ncuts"][0] == 0 and a["lmin"][0] == full[1] and a["iters"][0] == 0 and a["flags"][0] == 0
    s.close()


def test_a_block_of_513_rows_is_not_served_and_nothing_is_launched(gpu):
    n = 513
    A = np.zeros((2, n, n))
    A[0] = np.diag(np.linspace(-1.0, 1.0, n))
    A[1] = np.eye(n)
    s = load_dense(gpu, [A], np.ones(1))
    before = gpu.sparsecuts_stats()
    fill = 777.0
    rc, a = _raw_call(gpu, s, 0, np.zeros(1), 4, MAXCUTS, fill, n)
    assert rc == 0 and a["ncuts"][0] == -1
    assert a["lmin"][0] == fill and a["iters"][0] == 77 and a["flags"][0] == 77
    assert np.all(a["eigvals"] == fill) and np.all(a["lhs"] == fill) and np.all(a["coefs"] == fill) and np.all(a["vecs"] == fill)
    assert gpu.sparsecuts_stats() == before
    res = s.sparsecuts(0, np.zeros(1), 4, TOL, FEASTOL, MAXCUTS)
    assert res[0] == -1 and np.isnan(res[1]) and len(res[2]) == 0
    s.close()


def test_an_oversized_target_and_a_quiet_block_give_no_cut_and_the_right_lmin(gpu):
    spec = ("f4", 1)
    A, ys, y, b = L.block(spec)
    n = A.shape[1]
    ref = L.reference(spec, 4)
    s = load_dense(gpu, [A], b)
    for size in (n + 1, 1000):
        nc, lmin, ev, co, lh, ve, iters, flags = s.sparsecuts(0, y, size, TOL, FEASTOL, MAXCUTS)
        assert (nc, iters, flags) == (0, 0, 0) and lmin < -TOL
        assert abs(lmin - ref[1]) <= 1e-9 * max(1.0, abs(ref[1]))
    s.close()
    Aq = A.copy()
    Aq[0] -= 10.0 * np.eye(n)
    rq = R.sparse_cuts_dense(Aq, y, 4, TOL, FEASTOL, MAXCUTS)
    assert rq[0] == 0 and rq[1] > 1.0
    s = load_dense(gpu, [Aq], b)
    nc, lmin, ev, co, lh, ve, iters, flags = s.sparsecuts(0, y, 4, TOL, FEASTOL, MAXCUTS)
    s.close()
    assert (nc, iters, flags) == (0, 0, 0)
    assert abs(lmin - rq[1]) <= 1e-9 * max(1.0, abs(rq[1]))


# ---- 8. one workspace and one set of job tables behind all cut calls ----------------------------------------------------------------

def _mixed_solver(gpu, blocks, b):
    """blocks 0 and 2 dense, block 1 handed over as lower-triangular triplets with a count and kept as nonzeros"""
    m = len(b)
    s = gpu.Solver(0)
    s.sparse_policy(2)
    il = np.tril_indices(blocks[1].shape[1])
    var = np.repeat(np.arange(m + 1, dtype=np.int32), len(il[0]))
    row = np.tile(il[0].astype(np.int32), m + 1)
    col = np.tile(il[1].astype(np.int32), m + 1)
    val = np.concatenate([blocks[1][i][il] for i in range(m + 1)])
    keep = val != 0.0
    s.set_shape(m, [A.shape[1] for A in blocks], 0, nnz=[-1, int(keep.sum()), -1])
    s.set_obj(b)
    s.set_block_dense(0, blocks[0])
    s.add_entries(1, var[keep], row[keep], col[keep], val[keep])
    s.set_block_dense(2, blocks[2])
    assert [s.is_sparse(k) for k in range(3)] == [False, True, False]
    return s


def _bits(x):
    """a result of any of the cut calls (nested tuples and lists of numbers and arrays) as bytes: equal bytes, equal bits (nan included)"""
    if isinstance(x, (list, tuple)):
        return b"(" + b"|".join(_bits(v) for v in x) + b")"
    a = np.asarray(x)
    return str((a.dtype, a.shape)).encode() + a.tobytes()


def test_call_forms_sharing_one_workspace_reproduce_a_fresh_solver(gpu):
    """Blocks of 5, 40 (kept as nonzeros) and 130 rows, m = 6.  The cut calls of one solver share a grow-only workspace and the job
    tables cached on the device; every call form lays the workspace out differently and needs other tables.  A sequence that makes the
    workspace grow between calls and the cached tables go stale across call forms must return, call by call, the bits of the same
    call made first on a freshly created solver with the same data."""
    m, ns = 6, (5, 40, 130)
    blocks, ys, b = [], None, np.zeros(m)
    for k, n in enumerate(ns):
        _, A, ysk, Xs, Zs = instances.planted_dense(n, m, seed=41900 + 1000 * k)
        ys = ysk if k == 0 else ys
        blocks.append(L.rebuilt(A, ys, Zs))
        b += blocks[-1][1:].reshape(m, -1) @ Xs.reshape(-1)
    y = ys + 2.0 * np.random.default_rng(419).standard_normal(m)
    sizes = [3, 8, 10]
    steps = [("eigencuts_all, 2 cuts", lambda s: s.eigencuts_all(y, TOL, 2)),
             ("sparsecuts, 130 rows", lambda s: s.sparsecuts(2, y, 10, TOL, FEASTOL, MAXCUTS)),
             ("sparsecuts_all", lambda s: s.sparsecuts_all(y, sizes, TOL, FEASTOL, MAXCUTS)),
             ("sparsecuts, 5 rows", lambda s: s.sparsecuts(0, y, 3, TOL, FEASTOL, MAXCUTS)),
             ("eigencuts_all, 5 cuts", lambda s: s.eigencuts_all(y, TOL, MAXCUTS)),
             ("sparsecuts, 130 rows, no cuts", lambda s: s.sparsecuts(2, y, 10, TOL, FEASTOL, 0)),
             ("sparsecuts_all again", lambda s: s.sparsecuts_all(y, sizes, TOL, FEASTOL, MAXCUTS))]
    shared = _mixed_solver(gpu, blocks, b)
    got, want = [], []
    for what, call in steps:
        fresh = _mixed_solver(gpu, blocks, b)
        want.append(call(fresh))
        fresh.close()
        got.append(call(shared))
    shared.close()
    for (what, call), g, w in zip(steps, got, want):
        assert _bits(g) == _bits(w), what
    # the sequence computed something in every form: cuts from the dense rounds, from the sparse round and from the large block
    assert sum(len(r[1]) for r in want[4]) >= 3 and want[1][0] >= 1 and sum(max(0, r[0]) for r in want[2]) >= 1
    assert want[2][2][0] == -1 and want[5][0] == 0 and want[5][1] == want[1][1]
    assert _bits(want[6]) == _bits(want[2])
