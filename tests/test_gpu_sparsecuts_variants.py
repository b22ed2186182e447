"""GPU: hipsdp_sparsecuts_all_ex / hipsdp_sparsecuts_ex - the sparse eigenvector cuts with the reference's switches recomputesparseev,
recomputeinitial and exacttrans as a bit mask (csrc/sparsecuts_rounds.hip: the loop as rounds on the device, one read-back) - against
the numpy restatement tests/harness/sparsecuts_variants_ref.py on the cases of tests/harness/sparsecuts_variants_cases.py, for the
properties that need no oracle, and for what makes it a batch: bits that do not depend on the other blocks, a launch count that is a
function of (variant, maxcuts) alone.

The loop takes data-dependent decisions (which entries stay, when to stop, whether to cut, lambda against -tol) and takes vectors
from decompositions; counts, supports and iteration numbers are compared only after the restatement has shown the case stable
(check_margins: no decision close, gaps >= 1e-4, three re-runs with every eigenpair perturbed by 1e-9 change nothing).  Tolerances
are those of tests/test_gpu_sparsecuts_all.py."""
import ctypes as C
import threading
import numpy as np
import pytest
import ipm_ref
import sparsecuts_variants_cases as K
from test_gpu_sparsecuts_all import load_dense, load_sparse, same_bits, support

pytestmark = pytest.mark.gpu

TOL, FEASTOL, MAXCUTS = K.TOL, K.FEASTOL, K.MAXCUTS
ERR_ARG = 3
_dev = {}


def device(gpu, name, size, variant):
    """the all-blocks call on the family loaded as dense matrices (blocks of up to 64 rows stay dense rows, larger ones are swept as
    packed lower triangles), once per case"""
    key = (name, size, variant)
    if key not in _dev:
        blocks, ys, y, b = K.family(name)
        s = load_dense(gpu, blocks, b)
        _dev[key] = s.sparsecuts_all_ex(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS, variant)
        s.close()
    return _dev[key]


def bound(variant, maxcuts):
    s, d = int(bool(variant & 1)), int(bool(variant & 6))
    return 5 + (maxcuts + 1) * (2 + 3 * s + 3 * d)


@pytest.mark.parametrize("name,size,variant", K.CASES)
def test_every_block_matches_the_restatement(gpu, name, size, variant):
    K.check_margins(name, size, variant)
    blocks, ys, y, b = K.family(name)
    ref = K.reference(name, size, variant)
    res = device(gpu, name, size, variant)
    assert len(res) == len(blocks)
    for k, A in enumerate(blocks):
        nc, lmin, ev, co, lh, ve, iters, flags = res[k]
        rn, rl, rev, rco, rlh, rve, rsup, rit, rfl, mg, runs = ref[k]
        print("%s size %d variant %d block %d (n = %d): ncuts %d / %d, iterations %d / %d, flags %d / %d, lmin %.12g / %.12g"
              % (name, size, variant, k, A.shape[1], nc, rn, iters, rit, flags, rfl, lmin, rl))
        assert nc == rn, k
        assert iters == rit, k
        assert flags == rfl, k
        assert abs(lmin - rl) <= 1e-9 * max(1.0, abs(rl)), k
        if size > A.shape[1] or k in K.FAMILIES[name][2]:
            assert nc == 0, k
        for c in range(nc):
            assert support(ve[c]) == list(rsup[c]), (k, c)
            assert abs(ev[c] - rev[c]) <= 1e-9 * max(1.0, abs(rev[c])), (k, c)
            assert abs(abs(ve[c] @ rve[c]) - 1.0) <= 1e-6, (k, c)
            assert np.max(np.abs(co[c] - rco[c])) <= 1e-6 * max(1.0, np.max(np.abs(rco[c]))), (k, c)
            assert abs(lh[c] - rlh[c]) <= 1e-6 * max(1.0, abs(rlh[c])), (k, c)
    assert sum(r[0] for r in res) >= 1                     # (every case cuts somewhere: nothing above compared empty lists alone)


@pytest.mark.parametrize("name,size,variant", K.CASES)
def test_properties_that_need_no_oracle(gpu, name, size, variant):
    """Z_c is the matrix after the deflations the outputs themselves describe, Z_c = Z(y) - sum_{j < c} eigvals[j] x_j x_j^T.  The cut is
    built from the A_i, so coefs @ y - lhs is x^T Z(y) x; the value of the cut is x^T Z_c x = coefs @ y - lhs - sum_{j < c} eigvals[j]
    (x_j . x)^2 (the form tests/test_gpu_sparsecuts_all.py checks), which lies above it: both are asserted to 1e-8."""
    blocks, ys, y, b = K.family(name)
    res = device(gpu, name, size, variant)
    for k, A in enumerate(blocks):
        nc, lmin, ev, co, lh, ve, iters, flags = res[k]
        Z0 = np.tensordot(y, A[1:], axes=(0, 0)) - A[0]
        Zc = Z0.copy()
        znorm = np.linalg.norm(Z0, 2)
        for c in range(max(nc, 0)):
            x = ve[c]
            S = support(x)
            assert abs(np.linalg.norm(x) - 1.0) <= 1e-10, (k, c)
            assert len(S) <= size, (k, c)
            viol = co[c] @ y - lh[c]
            assert abs(viol - x @ Z0 @ x) <= 1e-8, (k, c, viol)
            assert abs(viol - sum(ev[j] * (ve[j] @ x) ** 2 for j in range(c)) - x @ Zc @ x) <= 1e-8, (k, c, viol)
            assert abs(ev[c] - x @ Zc @ x) <= 1e-8, (k, c, ev[c])
            assert viol <= ev[c] + 1e-8 and viol < -FEASTOL, (k, c, viol)
            assert co[c] @ ys - lh[c] >= -1e-9, (k, c)
            if variant & 1:
                sub = Zc[np.ix_(S, S)]
                assert abs(ev[c] - np.linalg.eigvalsh(sub)[0]) <= 1e-8 * znorm, (k, c)
                assert np.linalg.norm(sub @ x[S] - ev[c] * x[S]) <= 1e-8 * znorm, (k, c)
            Zc = Zc - ev[c] * np.outer(x, x)


def test_hand_example_through_the_product_call(gpu):
    """3 rows, size 2, convtol 0.5: variant 1 cuts with the smallest eigenvalue of the 2 x 2 submatrix, variant 0 with the visibly
    larger x^T Z x of the unconverged TPower vector"""
    A, y = K.hand_block()
    s = load_dense(gpu, [A], np.zeros(1))
    r0 = s.sparsecuts_all_ex(y, [K.HAND_SIZE], TOL, FEASTOL, 1, 0, convtol=K.HAND_CONVTOL)[0]
    r1 = s.sparsecuts_all_ex(y, [K.HAND_SIZE], TOL, FEASTOL, 1, 1, convtol=K.HAND_CONVTOL)[0]
    p1 = s.sparsecuts_ex(0, y, K.HAND_SIZE, TOL, FEASTOL, 1, 1, convtol=K.HAND_CONVTOL)
    s.close()
    assert r0[0] == r1[0] == 1 and support(r0[5][0]) == support(r1[5][0]) == [0, 1]
    sub = -1.95 - np.sqrt(0.0125)
    print("hand example: variant 0 %.15g, variant 1 %.15g, submatrix %.15g" % (r0[2][0], r1[2][0], sub))
    assert abs(r1[2][0] - sub) <= 1e-12 * abs(sub)
    assert r0[2][0] > r1[2][0] + 0.1
    assert abs(r0[2][0] - r0[5][0] @ K.HAND_Z @ r0[5][0]) <= 1e-12
    assert same_bits([p1], [r1])


def test_the_tol_rule_ends_the_loop_and_sets_bit_2(gpu):
    """the hand matrix with tol = 2.2: lmin = -2.207 lets the block take part, the smallest eigenvalue of the submatrix, -2.118, is not
    below -tol - no cut from that run, flags bit 2, the run's iterations counted (with tol = feastol, as in the named cases, the rule
    cannot fire: lambda <= x^T Z x < -feastol)"""
    import sparsecuts_variants_ref as V
    A, y = K.hand_block()
    s = load_dense(gpu, [A], np.zeros(1))
    for variant in (1, 7):
        ref = V.sparse_cuts_dense_ex(A, y, K.HAND_SIZE, 2.2, FEASTOL, 3, variant)
        assert ref[0] == 0 and ref[8] == 4 and ref[9].tol >= 1e-2 and ref[9].conv >= 1e-11 and ref[9].select >= 1e-9
        r = s.sparsecuts_all_ex(y, [K.HAND_SIZE], 2.2, FEASTOL, 3, variant)[0]
        p = s.sparsecuts_ex(0, y, K.HAND_SIZE, 2.2, FEASTOL, 3, variant)
        print("tol rule, variant %d: ncuts %d, iterations %d / %d, flags %d" % (variant, r[0], r[6], ref[7], r[7]))
        assert (r[0], r[6], r[7]) == (0, ref[7], 4) and same_bits([p], [r])
        assert abs(r[1] - ref[1]) <= 1e-9 * abs(ref[1])
    s.close()


def test_variant_0_is_the_existing_call(gpu):
    name, size = "f3", 4
    blocks, ys, y, b = K.family(name)
    nb = len(blocks)
    s = load_dense(gpu, blocks, b)
    want = s.sparsecuts_all(y, [size] * nb, TOL, FEASTOL, MAXCUTS)
    want1 = [s.sparsecuts(k, y, size, TOL, FEASTOL, MAXCUTS) for k in range(nb)]
    ex0, all0, one0 = gpu.sparsecuts_ex_stats(), gpu.sparsecuts_all_stats(), gpu.sparsecuts_stats()
    got = s.sparsecuts_all_ex(y, [size] * nb, TOL, FEASTOL, MAXCUTS, 0)
    all1 = gpu.sparsecuts_all_stats()
    got1 = [s.sparsecuts_ex(k, y, size, TOL, FEASTOL, MAXCUTS, 0) for k in range(nb)]
    one1 = gpu.sparsecuts_stats()
    s.close()
    assert same_bits(got, want) and same_bits(got1, want1)
    assert [r[0] for r in got] == [2, -1, 0, -1, 4] and all(r[0] >= 0 for r in got1[:4])      # (150 and 200 rows: the large path)
    assert all1[0] - all0[0] == 1 and 4 <= all1[1] - all0[1] <= 6 and all1[2] - all0[2] == 1
    assert one1[0] - one0[0] == nb and one1[1] > one0[1]
    assert gpu.sparsecuts_ex_stats() == ex0


def test_a_block_alone_in_its_family_and_through_the_per_block_call_has_the_same_bits(gpu):
    name, size = "f0", 4
    blocks, ys, y, b = K.family(name)
    for variant in (1, 6, 7):
        full = device(gpu, name, size, variant)
        s = load_dense(gpu, blocks, b)
        assert same_bits(s.sparsecuts_all_ex(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS, variant), full)       # the same call twice
        assert same_bits(s.sparsecuts_all_ex(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS, variant), full)
        for k in range(len(blocks)):
            assert same_bits([s.sparsecuts_ex(k, y, size, TOL, FEASTOL, MAXCUTS, variant)], [full[k]]), (variant, k)
        s.close()
        for k in (1, 3, 6, 8):              # 9, 17 rows (dense rows), 65 and 128 rows (packed)
            s1 = load_dense(gpu, [blocks[k]], b)
            alone = s1.sparsecuts_all_ex(y, [size], TOL, FEASTOL, MAXCUTS, variant)
            s1.close()
            assert same_bits(alone, [full[k]]), (variant, k)


def test_the_three_storage_forms_give_the_same_cuts(gpu):
    name, size = "f0", 4
    blocks, ys, y, b = K.family(name)
    ss = load_sparse(gpu, blocks, b)
    for k in range(len(blocks)):
        assert ss.is_sparse(k), k
    for variant in (1, 7):
        rd = device(gpu, name, size, variant)
        rs = ss.sparsecuts_all_ex(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS, variant)
        for k in range(len(blocks)):
            (nd, ld, ed, cd, hd, vd, itd, fd), (n_s, ls, es, cs, hs, vs, its, fs) = rd[k], rs[k]
            assert nd == n_s and itd == its and fd == fs, (variant, k)
            assert abs(ld - ls) <= 1e-9 * max(1.0, abs(ld))
            for c in range(nd):
                assert support(vd[c]) == support(vs[c]), (variant, k, c)
                assert abs(ed[c] - es[c]) <= 1e-9 * max(1.0, abs(ed[c])), (variant, k, c)
                assert np.max(np.abs(cd[c] - cs[c])) <= 1e-9 * max(1.0, np.max(np.abs(cd[c]))), (variant, k, c)
                assert abs(hd[c] - hs[c]) <= 1e-9 * max(1.0, abs(hd[c])), (variant, k, c)
    ss.close()


def test_launches_are_a_function_of_variant_and_maxcuts_alone(gpu):
    """one block (17 rows: one class of the decompositions) and the nine of family 0 (all three classes)"""
    name, size = "f0", 4
    blocks, ys, y, b = K.family(name)
    deltas = {}
    for nblk, sel in ((1, [3]), (9, list(range(9)))):
        s = load_dense(gpu, [blocks[k] for k in sel], b)
        for variant in (1, 2, 4, 7):
            s.sparsecuts_all_ex(y, [size] * nblk, TOL, FEASTOL, MAXCUTS, variant)              # first use (workspace, job tables)
            for mc in (MAXCUTS, 1, 0):
                c0, l0, r0 = gpu.sparsecuts_ex_stats()
                res = s.sparsecuts_all_ex(y, [size] * nblk, TOL, FEASTOL, mc, variant)
                c1, l1, r1 = gpu.sparsecuts_ex_stats()
                assert c1 - c0 == 1
                deltas[(nblk, variant, mc)] = (l1 - l0, r1 - r0)
                print("%d blocks, variant %d, maxcuts %d: %d launches (bound %d), %d read-backs, %d cuts" %
                      (nblk, variant, mc, l1 - l0, bound(variant, mc), r1 - r0, sum(r[0] for r in res)))
                assert l1 - l0 <= bound(variant, mc) and r1 - r0 == 1
                if mc == 0:
                    assert all(r[0] == 0 and r[6] == 0 for r in res)
        # the per-block call: the same sequence
        c0, l0, r0 = gpu.sparsecuts_ex_stats()
        s.sparsecuts_ex(0, y, size, TOL, FEASTOL, MAXCUTS, 7)
        c1, l1, r1 = gpu.sparsecuts_ex_stats()
        assert (c1 - c0, l1 - l0, r1 - r0) == (1,) + deltas[(nblk, 7, MAXCUTS)]
        s.close()
    for variant in (1, 2, 4, 7):
        for mc in (MAXCUTS, 1, 0):
            assert deltas[(1, variant, mc)] == deltas[(9, variant, mc)], (variant, mc, deltas)
    assert deltas[(9, 2, MAXCUTS)] == deltas[(9, 4, MAXCUTS)]


def _raw_all(gpu, s, y, sizes, maxcuts, variant, fill):
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
    opts = gpu.SparsecutOpts(TOL, FEASTOL, 0.0, maxcuts, 0)
    rc = L.hipsdp_sparsecuts_all_ex(s.h, dp(y), ip(sizes), C.byref(opts), C.c_uint(variant), ip(arr["ncuts"]), dp(arr["lmin"]),
                                    dp(arr["eigvals"]), dp(arr["coefs"]), dp(arr["lhs"]), dp(arr["vecs"]), ip(arr["iters"]), ip(arr["flags"]))
    return rc, arr


def test_blocks_above_128_rows_are_not_served_with_a_switch_set(gpu):
    name, size = "f3", 4
    ns, m = K.FAMILIES[name][0], K.FAMILIES[name][1]
    blocks, ys, y, b = K.family(name)
    s = load_dense(gpu, blocks, b)
    fill = 777.0
    for variant in (1, 2, 4):
        rc, a = _raw_all(gpu, s, y, [size] * len(ns), MAXCUTS, variant, fill)
        assert rc == 0
        off = 0
        for k, n in enumerate(ns):
            if n > 128:
                assert a["ncuts"][k] == -1 and a["lmin"][k] == fill and a["iters"][k] == 77 and a["flags"][k] == 77, (variant, k)
                assert np.all(a["eigvals"][k * MAXCUTS:(k + 1) * MAXCUTS] == fill) and np.all(a["vecs"][off:off + MAXCUTS * n] == fill)
                one = s.sparsecuts_ex(k, y, size, TOL, FEASTOL, MAXCUTS, variant)
                assert one[0] == -1 and np.isnan(one[1]) and one[6] == one[7] == 0, (variant, k)
            else:
                kept = int(a["ncuts"][k])
                assert kept >= 0 and a["lmin"][k] != fill, (variant, k)
                assert np.all(a["eigvals"][k * MAXCUTS + kept:(k + 1) * MAXCUTS] == fill), (variant, k)       # slots c >= ncuts: not written
                assert np.all(a["vecs"][off + kept * n:off + MAXCUTS * n] == fill), (variant, k)
                one = s.sparsecuts_ex(k, y, size, TOL, FEASTOL, MAXCUTS, variant)
                assert one[0] == kept and np.array_equal(one[2], a["eigvals"][k * MAXCUTS:k * MAXCUTS + kept]), (variant, k)
            off += MAXCUTS * n
        assert a["ncuts"][2] == 0 and sum(max(int(v), 0) for v in a["ncuts"]) >= 1           # block 2 is quiet, the others cut
    s.close()


def test_limits_size_above_the_block_no_cuts_wanted_and_an_unknown_bit(gpu):
    name = "b40"
    blocks, ys, y, b = K.family(name)
    nb = len(blocks)
    s = load_dense(gpu, blocks, b)
    for variant in (1, 6):
        res = s.sparsecuts_all_ex(y, [41, 4, 40, 1000], TOL, FEASTOL, MAXCUTS, variant)
        for k in (0, 3):
            assert res[k][0] == 0 and res[k][6] == 0 and res[k][7] == 0 and res[k][1] < -TOL, (variant, k)
        assert same_bits([res[1]], [device(gpu, name, 4, variant)[1]])        # whatever sizes the other blocks have
        assert res[2][0] >= 1 and len(support(res[2][5][0])) <= 40            # size == n
        ea = s.eigencuts_all(y, TOL, 0)
        res0 = s.sparsecuts_all_ex(y, [4] * nb, TOL, FEASTOL, 0, variant)
        assert all(r[0] == 0 and r[6] == 0 and r[7] == 0 for r in res0)
        assert [r[1] for r in res0] == [e[0] for e in ea]                     # lmin: the bits of hipsdp_eigencuts_all
    before = gpu.sparsecuts_ex_stats()
    rc, a = _raw_all(gpu, s, y, [4] * nb, MAXCUTS, 8, 777.0)
    assert rc == ERR_ARG and list(a["ncuts"]) == [77] * nb
    opts = gpu.SparsecutOpts(TOL, FEASTOL, 0.0, MAXCUTS, 0)
    k = C.c_int(77)
    yy = np.ascontiguousarray(y, dtype=np.float64)
    buf = np.zeros(MAXCUTS * 40)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    assert gpu.lib().hipsdp_sparsecuts_ex(s.h, 0, dp(yy), 4, C.byref(opts), C.c_uint(9), C.byref(k), None, dp(buf), dp(buf), dp(buf), None,
                                          None, None) == ERR_ARG and k.value == 77
    assert _raw_all(gpu, s, y, [4, 0, 4, 4], MAXCUTS, 1, 0.0)[0] == ERR_ARG
    assert gpu.sparsecuts_ex_stats() == before                                # nothing launched, nothing counted
    s.close()


def test_two_host_threads_reproduce_the_single_thread_bits(gpu):
    cases = [("b12", 4, 7), ("b40", 4, 1)]
    data = [K.family(f) for f, _, _ in cases]
    solvers = [load_dense(gpu, d[0], d[3]) for d in data]
    single = [device(gpu, *c) for c in cases]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(4):
                got[i].append(solvers[i].sparsecuts_all_ex(data[i][2], [cases[i][1]] * len(data[i][0]), TOL, FEASTOL, MAXCUTS, cases[i][2]))
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
