"""GPU: hipsdp_onevar_bounds_all - the one-variable SDPs of ALL blocks of a solver in one call - against hipsdp_onevar_bounds on
the same solver (bit for bit: the two calls share their device code, and a job's block and n come from its row of the table) and
against the numpy restatement of tests/onevar_cases.py.

The family: five blocks of 3, 17, 64, 65 and 128 rows that share six variables (onevar_all_cases.multi_family) - both class edges and the
odd small sizes; no block is larger than 128 rows except the one that must be turned away.  The bounds are those of
tests/test_gpu_onevar.py: on decidable jobs status and evaluation count equal the restatement's, a bound is returned exactly, and
    |optval - ref| <= 0.8 feastol / g        (onevar_cases.inner_bound: derived from concavity, not measured);
an EXTREMES job is held to |lambda - numpy| <= 1e-12 max|ev(A_i)|, the bound of the eigenvalue entry points
(tests/test_gpu_eig_structured.py)."""
import ctypes as C
import glob
import threading
import numpy as np
import pytest
import ipm_ref
import onevar_cases as K
import onevar_all_cases as KA

pytestmark = pytest.mark.gpu

NB, M = len(KA.MULTI_BLOCKS), KA.MULTI_M
ROWS = [n for n, _ in KA.MULTI_BLOCKS]


def load_dense(gpu, blocks, b):
    """blocks of up to 64 rows stay dense rows, larger ones are swept as packed lower triangles"""
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


def _solver(gpu, blocks, how):
    b = np.ones(blocks[0].shape[0] - 1)
    s = (load_dense if how == "dense" else load_sparse)(gpu, list(blocks), b)
    if how == "sparse":
        assert all(s.is_sparse(k) for k in range(len(blocks)))
    return s


def _bits(res):
    return [np.asarray(a).tobytes() for a in res]


def _take(res, idx):
    return [np.asarray(a)[idx] for a in res]


def _per_block(s, nb, u, lb, ub, **kw):
    """the loop the new call replaces: one hipsdp_onevar_bounds call per block, results in block-major order"""
    parts = [s.onevar_bounds(b, u, lb, ub, K.FEASTOL, **kw) for b in range(nb)]
    return [np.concatenate([p[k] for p in parts]) for k in range(5)]


def _all_jobs(nb, m):
    return np.repeat(np.arange(nb, dtype=np.int32), m), np.tile(np.arange(m, dtype=np.int32), nb)


def _compute_units():
    """compute units of the first GPU node of the KFD topology (read-only); 256 (an MI355X) when it cannot be read: the number only
    decides how many rounds the workgroups of the striding test make"""
    for path in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")):
        try:
            with open(path) as f:
                p = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            simd, per = int(p.get("simd_count", 0)), int(p.get("simd_per_cu", 0))
            if simd > 0 and per > 0:
                return simd // per
        except (OSError, ValueError):
            continue
    return 256


def _mat(A, u, i, mu):
    return K.z_of(A, u) + (mu - u[i]) * A[i + 1]


def _check_properties(A, u, i, lb, ub, st, ov, feastol):
    """what the status promises, with numpy on M(optval) (as tests/test_gpu_onevar.py states it)"""
    assert st in (K.LB, K.INNER, K.INFEASIBLE, K.UBONLY), st
    w = np.linalg.eigvalsh(_mat(A, u, i, ov))
    scale = float(np.max(np.abs(w)))
    if st in (K.LB, K.INNER, K.UBONLY):
        assert w[0] >= -feastol - 1e-12 * scale, (st, w[0])
    if st == K.INNER:
        assert w[0] <= -feastol / 4.0, w[0]
    if st == K.INFEASIBLE:
        assert w[0] < -feastol + 1e-12 * scale, w[0]
    assert lb <= ov
    if st != K.INFEASIBLE:
        assert ov <= ub


def _check_against_ref(A, u, i, ref, st, ov, ne, feastol, lb, ub, tag):
    """a decidable job: the restatement's decisions; returns |optval - ref| g / feastol of an INNER job, else 0"""
    assert (st, ne) == (ref[0], ref[4]), (tag, K.STATUS_NAMES.get(st), K.STATUS_NAMES[ref[0]], ne, ref[4])
    if ref[1] == lb or ref[1] == ub:
        assert ov == ref[1], tag                         # a bound is copied
        return 0.0
    bound, g = K.inner_bound(K.z_of(A, u), A[i + 1], u[i], ov, ref[1], feastol)
    assert abs(ov - ref[1]) <= bound, (tag, ov, ref[1], bound)
    return abs(ov - ref[1]) * g / feastol if st == K.INNER else 0.0


_first = {}


def _reference_bits(gpu, fl_index, how):
    """the five per-block calls on the instance (flavour, seed 1), once per (flavour, loader)"""
    key = (fl_index, how)
    if key not in _first:
        blocks, lb, ub, refs = KA.multi_instance(K.FLAVOURS[fl_index], 1)
        s = _solver(gpu, blocks, how)
        _first[key] = _bits(_per_block(s, NB, ub, lb, ub))
        s.close()
    return _first[key]


@pytest.mark.parametrize("how", ["dense", "sparse"])
@pytest.mark.parametrize("fl_index", [1, 3, 6, 8])
def test_bits_equal_the_per_block_calls(gpu, fl_index, how):
    """1: one call over all 30 jobs, u = ub, equals five hipsdp_onevar_bounds calls on the same solver bit for bit; so does a shuffled
    subset, and the same call made twice"""
    blocks, lb, ub, refs = KA.multi_instance(K.FLAVOURS[fl_index], 1)
    s = _solver(gpu, blocks, how)
    per = _per_block(s, NB, ub, lb, ub)
    lbj, ubj = np.tile(lb, NB), np.tile(ub, NB)
    full = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL)
    assert sorted(set(int(x) for x in full[0])) != [-1]
    assert _bits(full) == _bits(per)
    assert _bits(s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL)) == _bits(full)                 # same input, same bits
    jb, jv = _all_jobs(NB, M)
    explicit = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, blocks=jb, vars=jv)
    assert _bits(explicit) == _bits(full)
    sub = np.random.default_rng([fl_index, 30]).permutation(NB * M)[:17]
    part = s.onevar_bounds_all(ub, lbj[sub], ubj[sub], K.FEASTOL, blocks=jb[sub], vars=jv[sub])
    assert _bits(part) == _bits(_take(per, sub))                                               # neither the other jobs nor the order
    s.close()
    assert _bits(per) == _reference_bits(gpu, fl_index, how)


def test_family_matches_the_restatement(gpu):
    """2: all 18 instances, u = ub, every (block, variable) pair in one call.  The worst |optval - ref| g / feastol of the INNER jobs is
    printed per block size before it is checked against 0.8.  Measured on an MI355X: n = 3: 4.2e-9, 17: 1.4e-8, 64: 5.8e-8,
    65: 2.1e-8, 128: 2.8e-8; 1 of the 540 jobs undecidable."""
    worst, jobs, und = [0.0] * NB, 0, 0
    for fl, sd, blocks, lb, ub, refs in KA.multi_instances():
        s = _solver(gpu, blocks, "dense")
        st, ov, lmin, grad, ne = s.onevar_bounds_all(ub, np.tile(lb, NB), np.tile(ub, NB), K.FEASTOL)
        s.close()
        for b in range(NB):
            for i, r in enumerate(refs[b]):
                j = b * M + i
                jobs += 1
                tag = (fl, sd, b, i)
                _check_properties(blocks[b], ub, i, lb[i], ub[i], int(st[j]), float(ov[j]), K.FEASTOL)
                if st[j] == K.LB:
                    assert grad[j] == 0.0, tag
                if not K.decidable(K.NEWTON, r[5]):
                    und += 1
                    continue
                worst[b] = max(worst[b], _check_against_ref(blocks[b], ub, i, r, int(st[j]), float(ov[j]), int(ne[j]), K.FEASTOL,
                                                            lb[i], ub[i], tag))
    for b in range(NB):
        print("n = %3d: worst |optval - ref| g / feastol = %.3g (bound 0.8)" % (ROWS[b], worst[b]))
    print("%d jobs, %d undecidable" % (jobs, und))
    assert max(worst) <= 0.8
    assert jobs == 540 and und < K.UNDECIDABLE_CAP * jobs


def _with_a_zero_matrix(blocks):
    """variable 3 has no entry in the blocks of 17 and 65 rows"""
    out = [np.array(A) for A in blocks]
    out[1][4] = 0.0
    out[3][4] = 0.0
    return out


@pytest.mark.parametrize("how", ["dense", "sparse"])
def test_extremes(gpu, how):
    """3: lambda_min and lambda_max of every A_i of every block, alone and mixed with the other kinds"""
    for fl_index, sd in ((1, 1), (6, 2)):
        blocks, lb, ub, refs = KA.multi_instance(K.FLAVOURS[fl_index], sd)
        if fl_index == 6:
            blocks = _with_a_zero_matrix(blocks)
        s = _solver(gpu, blocks, how)
        lbj, ubj = np.tile(lb, NB), np.tile(ub, NB)
        ex = np.full(NB * M, KA.EXTREMES, dtype=np.int32)
        c0 = gpu.onevar_bounds_all_stats()
        st, ov, lmin, grad, ne = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, kind=ex)
        c1 = gpu.onevar_bounds_all_stats()
        assert tuple(c1[k] - c0[k] for k in range(3)) == (1, 2, 1)                # no Z(u): one launch per class with jobs
        st1, ov1, lmin1, grad1, ne1 = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, kind=ex, maxevals=1)
        # (the bounds are not read: infinite ones decline nothing)
        inf = s.onevar_bounds_all(ub, np.full(NB * M, -1e20), np.full(NB * M, 1e20), K.FEASTOL, kind=ex)
        assert _bits(inf) == _bits((st, ov, lmin, grad, ne))
        worst = 0.0
        for b in range(NB):
            for i in range(M):
                j = b * M + i
                lo, hi = KA.extremes_ref(blocks[b][i + 1])
                scale = max(abs(lo), abs(hi))
                assert (st[j], ne[j], grad[j]) == (KA.DONE, 2, 0.0), (b, i)
                assert (st1[j], ne1[j], grad1[j]) == (KA.DONE, 1, 0.0) and ov1[j] == lmin1[j] and lmin1[j] == lmin[j], (b, i)
                if scale == 0.0:
                    assert abs(lmin[j]) < 1e-200 and abs(ov[j]) < 1e-200, (b, i, lmin[j], ov[j])
                    continue
                worst = max(worst, abs(lmin[j] - lo) / scale, abs(ov[j] - hi) / scale)
                assert abs(lmin[j] - lo) <= 1e-12 * scale and abs(ov[j] - hi) <= 1e-12 * scale, (b, i, lmin[j], lo, ov[j], hi)
        print("%s, flavour %d: worst |lambda - numpy| / max|ev| = %.3g (bound 1e-12)" % (how, fl_index, worst))
        # mixed with the other kinds: their bits stay
        plain = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, kind=np.array([j % 2 for j in range(NB * M)], dtype=np.int32))
        mixed_kind = np.array([KA.EXTREMES if j % 3 == 0 else j % 2 for j in range(NB * M)], dtype=np.int32)
        mixed = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, kind=mixed_kind)
        keep = np.nonzero(mixed_kind != KA.EXTREMES)[0]
        exj = np.nonzero(mixed_kind == KA.EXTREMES)[0]
        assert _bits(_take(mixed, keep)) == _bits(_take(plain, keep))
        assert _bits(_take(mixed, exj)) == _bits(_take((st, ov, lmin, grad, ne), exj))
        s.close()


def test_contract_launches_stats_declined_and_gaveup(gpu):
    """4: (calls, launches, read-backs) per call, the two sets of totals apart, a declined job, a bounded loop"""
    blocks, lb, ub, refs = KA.multi_instance(K.FLAVOURS[1], 1)
    s = _solver(gpu, blocks, "dense")
    lbj, ubj = np.tile(lb, NB), np.tile(ub, NB)
    jb, jv = _all_jobs(NB, M)
    o0, c0 = gpu.onevar_bounds_stats(), gpu.onevar_bounds_all_stats()
    full = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL)
    c1 = gpu.onevar_bounds_all_stats()
    assert tuple(c1[k] - c0[k] for k in range(3)) == (1, 3, 1)                    # Z(u), the small class, the 65-128 class
    sm = np.nonzero(jb <= 2)[0]
    small = s.onevar_bounds_all(ub, lbj[sm], ubj[sm], K.FEASTOL, blocks=jb[sm], vars=jv[sm])
    c2 = gpu.onevar_bounds_all_stats()
    assert tuple(c2[k] - c1[k] for k in range(3)) == (1, 2, 1)
    assert _bits(small) == _bits(_take(full, sm))
    one = s.onevar_bounds_all(ub, lbj[20:21], ubj[20:21], K.FEASTOL, blocks=jb[20:21], vars=jv[20:21])
    c3 = gpu.onevar_bounds_all_stats()
    assert tuple(c3[k] - c2[k] for k in range(3)) == (1, 2, 1)
    assert _bits(one) == _bits(_take(full, [20]))
    assert gpu.onevar_bounds_stats() == o0                                         # the per-block totals did not move
    s.onevar_bounds(1, ub, lb, ub, K.FEASTOL)
    assert gpu.onevar_bounds_all_stats() == c3 and gpu.onevar_bounds_stats() != o0     # ... and the reverse
    # a declined job beside served ones
    ub2 = np.array(ubj)
    ub2[7] = 1e20
    ub2[25] = 1e20
    dec = s.onevar_bounds_all(ub, lbj, ub2, K.FEASTOL)
    for j in (7, 25):
        assert dec[0][j] == K.DECLINED and dec[4][j] == 0 and dec[1][j] == 0.0
    keep = [j for j in range(NB * M) if j not in (7, 25)]
    assert _bits(_take(dec, keep)) == _bits(_take(full, keep))
    # a bounded loop: two evaluations are not enough for an INNER job (one per class)
    for b in (1, 3):
        inner = [i for i in range(M) if refs[b][i][0] == K.INNER and refs[b][i][4] > 2]
        assert inner, b
        i = inner[0]
        g = s.onevar_bounds_all(ub, lb[i:i + 1], ub[i:i + 1], K.FEASTOL, blocks=[b], vars=[i], maxevals=2)
        assert g[0][0] == K.GAVEUP and g[4][0] == 2 and g[1][0] == lb[i]
        r2 = K.onevar_ref(K.z_of(blocks[b], ub), blocks[b][i + 1], ub[i], K.NEWTON, lb[i], ub[i], K.FEASTOL, maxevals=2)
        assert r2[0] == K.GAVEUP and r2[1] == lb[i]
    s.close()


def test_a_block_of_129_rows_is_turned_away_and_the_others_are_served(gpu):
    """5: the jobs of the sixth block get status -1 with nothing else written; the other 30 return the bits of test 1"""
    blocks, lb, ub, refs = KA.multi_instance(K.FLAVOURS[1], 1)
    rng = np.random.default_rng(129)
    big = np.zeros((M + 1, 129, 129))
    for i in range(M + 1):
        B = rng.standard_normal((129, 3))
        big[i] = B @ B.T + np.eye(129)
    s = _solver(gpu, list(blocks) + [big], "dense")
    st, ov, lmin, grad, ne = s.onevar_bounds_all(ub, np.tile(lb, NB + 1), np.tile(ub, NB + 1), K.FEASTOL)
    s.close()
    tail = slice(NB * M, (NB + 1) * M)
    assert list(st[tail]) == [-1] * M
    assert np.all(np.isnan(ov[tail])) and np.all(np.isnan(lmin[tail])) and np.all(np.isnan(grad[tail])) and list(ne[tail]) == [0] * M
    head = slice(0, NB * M)
    assert _bits([a[head] for a in (st, ov, lmin, grad, ne)]) == _reference_bits(gpu, 1, "dense")


def test_striding_through_the_unit_entry(gpu):
    """6a: seven jobs of the 65-128 class on TWO workgroups (each runs three or four jobs one after the other in its slab, blocks of
    different n in turn) return the bits each job returns alone on one workgroup"""
    ns = [65, 128, 65, 97, 128, 66, 127]
    Z, A, sh, lo, hi, kind = [], [], [], [], [], []
    for k, n in enumerate(ns):
        Ab, lb, ub = K.family(n, 3, 6, 3 + k, 0.6, 0.0, 0)
        i = k % 3
        Z.append(K.z_of(Ab, ub)); A.append(Ab[i + 1]); sh.append(ub[i]); lo.append(lb[i]); hi.append(ub[i])
        kind.append([K.NEWTON, K.NEWTON, K.TWOPOINT, K.NEWTON, KA.EXTREMES, K.NEWTON, K.NEWTON][k])
    together = gpu.onevar_all_unit(Z, A, sh, lo, hi, K.FEASTOL, kind=kind, mid_cap=2)
    assert all(int(x) in (K.LB, K.INNER, K.INFEASIBLE, K.UBONLY, KA.DONE) for x in together[0]), together[0]
    for k in range(len(ns)):
        alone = gpu.onevar_all_unit(Z[k:k + 1], A[k:k + 1], sh[k:k + 1], lo[k:k + 1], hi[k:k + 1], K.FEASTOL, kind=kind[k:k + 1], mid_cap=1)
        assert _bits(alone) == _bits(_take(together, [k])), (k, ns[k])
        if kind[k] != KA.EXTREMES:
            old = gpu.onevar_unit(ns[k], Z[k], [A[k]], [sh[k]], [lo[k]], [hi[k]], K.FEASTOL, kind=[kind[k]])
            assert _bits(old) == _bits(alone), (k, ns[k])                         # ... and those of the per-block kernel
    assert sorted(set(int(x) for x in together[0])) != [K.LB]


def test_striding_through_the_product_call(gpu):
    """6b: one block of 65 rows with 2 x (compute units) + 3 jobs - variables repeat, bounds vary: every workgroup runs two or three
    jobs; every job returns the bits of the per-block call for it"""
    A, lb, ub = K.family(65, 8, 6, 1, 0.6, 0.0, 0)
    m = 8
    count = 2 * _compute_units() + 3
    rng = np.random.default_rng([65, count])
    var = (np.arange(count) % m).astype(np.int32)
    lbj = lb[var] - rng.uniform(0.0, 0.2, count)
    ubj = ub[var] * rng.uniform(0.7, 1.0, count)
    # a third of the jobs with a small upper bound (INFEASIBLE by the restatement), a third with a lower bound close below
    # t ub_i = 0.6 ub_i (LB or INNER), the rest INNER: chains of different lengths side by side
    third = np.arange(count) % 3
    ubj = np.where(third == 1, ub[var] * rng.uniform(0.1, 0.4, count), ubj)
    lbj = np.where(third == 2, ub[var] * rng.uniform(0.5, 0.69, count), lbj)
    s = _solver(gpu, [A], "dense")
    c0 = gpu.onevar_bounds_all_stats()
    got = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, blocks=np.zeros(count, dtype=np.int32), vars=var)
    c1 = gpu.onevar_bounds_all_stats()
    want = s.onevar_bounds(0, ub, lbj, ubj, K.FEASTOL, vars=var)
    s.close()
    assert tuple(c1[k] - c0[k] for k in range(3)) == (1, 2, 1)
    assert _bits(got) == _bits(want)
    assert set(int(x) for x in got[0]) == {K.LB, K.INNER, K.INFEASIBLE}, set(got[0])


def test_null_blocks_and_vars_is_the_block_major_list(gpu):
    """7: three blocks of 3, 17 and 65 rows"""
    blocks, lb, ub = KA.multi_family(2, 0.6, 0.02, 0, blocks=[(3, 1), (17, 3), (65, 6)])
    s = _solver(gpu, blocks, "dense")
    jb, jv = _all_jobs(3, M)
    lbj, ubj = np.tile(lb, 3), np.tile(ub, 3)
    implicit = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL)
    explicit = s.onevar_bounds_all(ub, lbj, ubj, K.FEASTOL, blocks=jb, vars=jv)
    per = _per_block(s, 3, ub, lb, ub)
    s.close()
    assert _bits(implicit) == _bits(explicit) == _bits(per)


def test_by_hand(gpu):
    """8: block 0: A_1 = I, A_0 = I / 2 (2 x 2): M(mu) = (mu - 0.5) I whatever u is; block 1 (1 x 1): A_1 = 1, A_0 = 0.5: M(mu) = mu - 0.5"""
    b0 = np.stack([0.5 * np.eye(2), np.eye(2)])
    b1 = np.array([[[0.5]], [[1.0]]])
    s = _solver(gpu, [b0, b1], "dense")
    blk = [0, 0, 0, 1, 1, 1, 0, 1]
    kind = [K.TWOPOINT] * 3 + [K.NEWTON] * 3 + [KA.EXTREMES] * 2
    lb = [0.6, 0.0, 0.0, 0.0, 0.0, 0.6, 0.0, 0.0]
    ub = [1.0, 1.0, 0.25, 1.0, 0.25, 1.0, 1.0, 1.0]
    st, ov, lmin, grad, ne = s.onevar_bounds_all([0.3], lb, ub, 1e-6, blocks=blk, vars=[0] * 8, kind=kind)
    s.close()
    assert list(st) == [K.LB, K.UBONLY, K.INFEASIBLE, K.INNER, K.INFEASIBLE, K.LB, KA.DONE, KA.DONE]
    assert list(ne) == [1, 2, 2, 3, 1, 2, 2, 2]
    assert list(ov[:3]) == [0.6, 1.0, 0.25] and np.max(np.abs(lmin[:3] - np.array([0.1, 0.5, -0.25]))) <= 1e-14
    assert abs(ov[3] - (0.5 - 0.5e-6)) <= 1e-15 and ov[4] == 0.25 and ov[5] == 0.6
    assert list(grad) == [0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0, 0.0]
    assert abs(lmin[3] + 0.5e-6) <= 1e-15 and lmin[4] == -0.25
    assert abs(lmin[6] - 1.0) <= 1e-14 and abs(ov[6] - 1.0) <= 1e-14 and lmin[7] == 1.0 and ov[7] == 1.0


def test_two_host_threads_on_different_solvers_reproduce_the_single_thread_bits(gpu):
    """9: one solver per thread, four calls each"""
    data = [KA.multi_instance(K.FLAVOURS[3], sd) for sd in (1, 2)]
    solvers = [_solver(gpu, d[0], "dense") for d in data]

    def call(i):
        blocks, lb, ub, refs = data[i]
        return _bits(solvers[i].onevar_bounds_all(ub, np.tile(lb, NB), np.tile(ub, NB), K.FEASTOL))
    single = [call(i) for i in range(2)]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(4):
                got[i].append(call(i))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for s in solvers:
        s.close()
    assert not errs, errs
    for i in range(2):
        assert got[i] == [single[i]] * 4


def test_argument_errors_and_an_empty_call(gpu):
    """10: every argument error returns HIPSDP_ERR_ARG (3) with nothing launched, the totals unchanged and status untouched;
    count == 0 returns 0 with nothing launched"""
    blocks, lb, ub = KA.multi_family(1, 0.6, 0.0, 0, blocks=[(3, 1), (17, 3)])
    nb, m = 2, M
    cnt = nb * m
    s = _solver(gpu, blocks, "dense")
    f = gpu.lib().hipsdp_onevar_bounds_all
    dp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    u, l, h = np.array(ub), np.tile(lb, nb), np.tile(ub, nb)
    st, ov = np.full(cnt, 7, dtype=np.int32), np.zeros(cnt)
    jb, jv = _all_jobs(nb, m)
    kind = np.zeros(cnt, dtype=np.int32)
    opts = gpu.OnevarOpts(1e-6, 1e20, 0)
    o = C.byref(opts)
    c0 = gpu.onevar_bounds_all_stats()
    fresh = gpu.Solver(0)                                                         # no shape
    assert f(fresh.h, dp(u), cnt, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    fresh.close()
    assert f(None, dp(u), cnt, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, None, cnt, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, None, dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), None, o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), None, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), o, None, dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), o, ip(st), None, None, None, None) == 3
    assert f(s.h, dp(u), -1, ip(jb), ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt - 1, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3     # both NULL, count != nb m
    assert f(s.h, dp(u), cnt, ip(jb), None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3       # one without the other
    assert f(s.h, dp(u), cnt, None, ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    for bad in (-1, nb):
        b2 = jb.copy()
        b2[5] = bad
        assert f(s.h, dp(u), cnt, ip(b2), ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    for bad in (-1, m):
        v2 = jv.copy()
        v2[2] = bad
        assert f(s.h, dp(u), cnt, ip(jb), ip(v2), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    for bad in (-1, 3):
        k2 = kind.copy()
        k2[3] = bad
        assert f(s.h, dp(u), cnt, ip(jb), ip(jv), ip(k2), dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    neg = gpu.OnevarOpts(-1e-6, 1e20, 0)
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), C.byref(neg), ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), 0, ip(jb), ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 0        # count == 0
    assert list(st) == [7] * cnt and gpu.onevar_bounds_all_stats() == c0
    # ... and the call with everything in place, the optional outputs missing; the per-block call still refuses kind 2
    k2 = kind.copy()
    k2[4] = KA.EXTREMES
    assert f(s.h, dp(u), cnt, ip(jb), ip(jv), ip(k2), dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 0
    assert st[4] == KA.DONE and all(x in (K.LB, K.INNER, K.INFEASIBLE) for x in np.delete(st, 4))
    g = gpu.lib().hipsdp_onevar_bounds
    assert g(s.h, 0, dp(u), m, None, ip(k2[:m].copy()), dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    s.close()
