"""GPU: constraint matrices kept as nonzeros (csrc/sparse.hip) - what both reference backends hand their solver
(sdpisolver_dsdp.c:1126-1195 SDPConeSetASparseVecMat, sdpisolver_sdpa.cpp:1223-1267 inputElement).  The sparse block mode must give
the dense path's results (same algorithm, Schur entries from the nonzeros instead of the three GEMMs) without
ever allocating the (m + 1) x n^2 array."""
import ctypes as C
import os
import numpy as np
import pytest

import instances
import ipm_ref

pytestmark = pytest.mark.gpu


def _solve(gpu, n, m, b, coo, A0, policy, tol=1e-7):
    s = gpu.Solver(0)
    s.sparse_policy(policy)
    s.load_sparse(m, n, b, coo, A0)
    sparse = s.is_sparse(0)
    info = s.solve(gaptol=tol, feastol=tol)
    y = s.y()
    X = s.X(0)
    s.close()
    return sparse, info, y, X


@pytest.mark.parametrize("n,m,k", [(96, 120, 3), (150, 100, 2), (130, 260, 8), (200, 90, 12)])
def test_sparse_block_matches_the_dense_block_and_the_oracle(gpu, n, m, k):
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=100 + n + m)
    opt = float(b @ ys)
    sp_d, info_d, y_d, X_d = _solve(gpu, n, m, b, coo, A0, 0)
    sp_s, info_s, y_s, X_s = _solve(gpu, n, m, b, coo, A0, 2)
    assert not sp_d and sp_s
    assert info_d.status == 0 and info_s.status == 0
    assert abs(info_s.dobj - opt) <= 1e-6 * (1 + abs(opt)) and abs(info_d.dobj - opt) <= 1e-6 * (1 + abs(opt))
    assert info_s.iterations == info_d.iterations
    assert np.max(np.abs(y_s - y_d)) <= 1e-7 * (1 + np.max(np.abs(y_d)))
    assert np.max(np.abs(X_s - X_d)) <= 1e-6 * (1 + np.max(np.abs(X_d)))
    # the oracle on the dense expansion of the same instance
    core = ipm_ref.CoreProblem(b, [instances.coo_to_dense(n, m, coo, A0)])
    ref = ipm_ref.hsd_solve(core, ipm_ref.Params(gaptol=1e-7, feastol=1e-7))
    assert ref.status == 0 and ref.iterations == info_s.iterations
    assert np.max(np.abs(y_s - ref.y)) <= 1e-6 * (1 + np.max(np.abs(ref.y)))


@pytest.mark.parametrize("n,m,k", [(70, 40, 4), (96, 120, 3), (130, 60, 9)])
def test_schur_entries_of_the_sparse_assembly_against_the_oracle(gpu, n, m, k):
    """the kernels of csrc/sparse.hip themselves (hipsdp_schur_sparse_unit runs hs_sp_schur as the engine calls it), entry by entry
    against the oracle's restatement of the same two-stage sum (ipm_ref.schur_rows_sparse), its pair formula and the dense
    three-product formula on the expanded matrices"""
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=9)
    rng = np.random.default_rng(1)
    X = rng.standard_normal((n, n)); X = X @ X.T + n * np.eye(n)
    Z = rng.standard_normal((n, n)); Z = Z @ Z.T + n * np.eye(n)
    Zi = np.linalg.inv(Z); Zi = 0.5 * (Zi + Zi.T)
    Mg = gpu.schur_sparse_unit(n, m, coo, X, Zi)[1:, 1:]
    M1 = ipm_ref.schur_block(instances.coo_to_dense(n, m, coo, A0), X, Zi)[1:, 1:]
    M2 = ipm_ref.schur_pairs_sparse(m, coo, X, Zi)
    M3 = ipm_ref.schur_rows_sparse(m, n, coo, X, Zi)
    il = np.tril_indices(m)
    scale = np.max(np.abs(M1))
    assert np.max(np.abs(M1 - M2)) <= 1e-12 * scale
    assert np.max(np.abs(Mg[il] - M3[il])) <= 1e-13 * scale
    assert np.max(np.abs(Mg[il] - M2[il])) <= 1e-12 * scale
    assert np.max(np.abs(Mg[il] - M1[il])) <= 1e-12 * scale


@pytest.mark.parametrize("n,m,k,policy", [(70, 40, 4, 2), (88, 60, 3, 2), (40, 30, 3, 2), (64, 50, 2, 2)])
def test_sparse_blocks_of_at_most_90_rows_are_solved_by_the_engine(gpu, n, m, k, policy):
    """blocks of at most 90 rows kept as nonzeros (policy 2 forces it at any size; the default policy does it from 65 rows on when the
    caller's count makes it the cheaper assembly): such a block has no dense rows A_i, so none of the fused small-problem kernels
    (which read A + i n^2) may take it (advisor finding of round 3: small_problem() did not exclude them)"""
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=300 + n)
    sp, info, y, X = _solve(gpu, n, m, b, coo, A0, policy, tol=1e-6)
    assert sp
    core = ipm_ref.CoreProblem(b, [instances.coo_to_dense(n, m, coo, A0)])
    ref = ipm_ref.hsd_solve(core, ipm_ref.Params(gaptol=1e-6, feastol=1e-6))
    assert info.status == ref.status == 0 and info.iterations == ref.iterations
    assert abs(info.dobj - float(b @ ys)) <= 1e-5 * (1 + abs(float(b @ ys)))
    assert np.max(np.abs(y - ref.y)) <= 1e-6 * (1 + np.max(np.abs(ref.y)))


def test_three_nonzeros_per_matrix_n500_m2000_takes_megabytes_not_gigabytes(gpu):
    """n = 500, m = 2000, three nonzeros per matrix: dense storage would be 8 (m + 1) n^2 = 4 GB (plus its packed copy and 8 GB of
    Schur workspace); kept as nonzeros the whole problem - work matrices, the 2001 x 2001 Schur matrix and its factor included -
    stays below 300 MB, of which the constraint matrices are 6000 triplets and one dense constant matrix"""
    n, m, k = 500, 2000, 3
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=77)
    opt = float(b @ ys)
    lib = gpu.lib()
    f0, f1, tot = C.c_double(0), C.c_double(0), C.c_double(0)
    s = gpu.Solver(0)
    assert lib.hipsdp_mem_info(0, C.byref(f0), C.byref(tot)) == 0
    s.load_sparse(m, n, b, coo, A0)
    assert s.is_sparse(0)                                   # the default policy picks the pair formula here
    info = s.solve(gaptol=1e-5, feastol=1e-5)
    assert lib.hipsdp_mem_info(0, C.byref(f1), C.byref(tot)) == 0
    used = f0.value - f1.value
    y = s.y()
    lmin, lpv = s.check_y(y)
    s.close()
    print("n=500 m=2000 k=3: %d iterations, %.3f s, device memory taken by the problem %.1f MB (dense storage alone: %.0f MB)"
          % (info.iterations, info.solve_seconds, used / 1e6, 8.0 * (m + 1) * n * n / 1e6))
    assert info.status == 0
    assert abs(info.dobj - opt) <= 1e-5 * (1 + abs(opt))
    assert lmin[0] >= -1e-5
    assert used < 300e6


def test_density_one_tenth_stays_dense_by_the_cost_rule_and_agrees_when_forced(gpu):
    """rho = 0.1: n = 200, m = 400 with 2000 lower-triangular nonzeros per matrix - 4 (sum nnz)^2 = 2.6e12 against
    1.9e10 for the dense formulation, so the default policy keeps the block dense; forced into the sparse mode it still gives the
    same solve"""
    n, m = 200, 400
    k = int(0.1 * n * (n + 1) / 2)
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=5)
    opt = float(b @ ys)
    sp_a, info_a, y_a, _ = _solve(gpu, n, m, b, coo, A0, 1, tol=1e-6)
    assert not sp_a and info_a.status == 0 and abs(info_a.dobj - opt) <= 1e-5 * (1 + abs(opt))
    sp_s, info_s, y_s, _ = _solve(gpu, n, m, b, coo, A0, 2, tol=1e-6)
    assert sp_s and info_s.status == 0 and info_s.iterations == info_a.iterations
    assert np.max(np.abs(y_s - y_a)) <= 1e-6 * (1 + np.max(np.abs(y_a)))


def test_sparse_blocks_behind_the_solver_interface(gpu):
    """SCIPsdpiSolverLoadAndSolve hands the engine the nonzero counts (hipsdp_set_shape2): a node with a 150 x 150 block of
    three-nonzero matrices is solved without a dense master copy and agrees with the numpy backend of the harness"""
    import sdpi_prepare
    import sdpi_call
    rng = np.random.default_rng(3)
    n, m, k = 150, 60, 3
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=11)
    var, row, col, val = coo
    blocks = [dict(n=n, vars={v: [(int(r), int(c), float(x)) for r, c, x in zip(row[var == v + 1], col[var == v + 1], val[var == v + 1])]
                              for v in range(m)},
                   const=[(int(r), int(c), float(A0[r, c])) for r in range(n) for c in range(r + 1) if A0[r, c] != 0.0])]
    prob = sdpi_prepare.SdpiProblem(b, [-1e20] * m, [1e20] * m, blocks, [])
    P = sdpi_prepare.prepare(prob)
    s = sdpi_call.SdpiSolver(gpu.lib())
    for par in (1, 2, 3):
        assert s.set_real(par, 1e-6) == sdpi_call.SCIP_OKAY
    rc, _, _ = s.solve(P)
    assert rc == sdpi_call.SCIP_OKAY and s.flag("IsOptimal")
    rc, obj, y = s.dual_sol()
    s.free()
    assert abs(obj - float(b @ ys)) <= 1e-5 * (1 + abs(float(b @ ys)))


def test_tree_of_example_tt_with_blocks_kept_as_nonzeros(gpu, monkeypatch):
    """The whole B&B tree of example_TT through SCIPsdpiSolverLoadAndSolve with the SDP block kept as nonzeros on the general path
    (HIPSDP_SPARSE=2, one-launch kernel off) beside the dense block: same outcome at every node, iteration counts within one.  The
    nodes without an optimum (tau -> 0) are what separates a Schur assembly in the association of the dense formula, T_j = A_j Zinv
    first (csrc/sparse.hip since round 4), from the pair formula of rounds 2-3: with that one this tree took 1644 engine solves of
    76 iterations on average (settings ladder, penalty formulations) instead of 569 of 14.7."""
    import bnb, sdpa_io, sdpi_call
    inst = sdpa_io.read_sdpa(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances", "example_TT.dat-s.gz"))
    prob = bnb.instance_to_sdpi(inst)
    monkeypatch.setenv("HIPSDP_SOLVE1", "0")
    monkeypatch.setenv("HIPSDP_SPARSE", "2")
    sa = sdpi_call.SdpiSolver(gpu.lib())
    monkeypatch.setenv("HIPSDP_SPARSE", "0")
    sb = sdpi_call.SdpiSolver(gpu.lib())
    for s in (sa, sb):
        for p in (1, 2, 3):
            assert s.set_real(p, 1e-6) == sdpi_call.SCIP_OKAY
    tot = dict(a=0, b=0, n=0, diff=0)

    def outcome(s):
        if s.flag("IsDualInfeasible"):
            return 'infeasible', None
        if not s.flag("IsOptimal"):
            return 'failed', None
        rc, obj, y = s.dual_sol()
        return 'optimal', (obj, y)

    def solve(P):
        monkeypatch.setenv("HIPSDP_SPARSE", "2")
        sa.solve(P)
        ia, oa = sa.iterations(), outcome(sa)
        monkeypatch.setenv("HIPSDP_SPARSE", "0")
        sb.solve(P)
        ib, ob = sb.iterations(), outcome(sb)
        tot['a'] += ia; tot['b'] += ib; tot['n'] += 1
        if oa[0] != ob[0] or abs(ia - ib) > 1 or (oa[0] == 'optimal' and abs(oa[1][0] - ob[1][0]) > 1e-5 * (1 + abs(ob[1][0]))):
            tot['diff'] += 1
        return bnb.NodeResult(oa[0]) if oa[0] != 'optimal' else bnb.NodeResult('optimal', oa[1][0], oa[1][1])
    best, y, nodes, failed = bnb.branch_and_bound(prob, inst.intvars, solve)
    sa.free(); sb.free()
    print("example_TT: %d nodes, iterations sparse %d / dense %d, differing nodes %d" % (nodes, tot['a'], tot['b'], tot['diff']))
    assert abs(best - 2.11803) <= 1e-4 and failed == 0
    assert tot['diff'] == 0
    assert abs(tot['a'] - tot['b']) <= 0.005 * tot['b']


# ---- problems with several blocks, LP rows and variables that do not occur in a block ------------------------------------------------

def _planted_blocks(seed, m, specs, q, rank=None):
    """a planted optimum as tests/stress_cases.py builds it (rand_core, kinds 0 / 1) over blocks given as (n, k, absent): k lower nonzeros
    per matrix, one of them on the diagonal, and the variables v with v % 3 == absent do not occur in the block at all; k = None: a
    dense block.  The planted X of a block has rank n // 3 as there, or `rank`.  Returns (b, blocks [m + 1, n, n], coos (triplets of the variables, None for a dense block), D, c, planted value)."""
    import sparse_kernel_cases as skc
    rng = np.random.default_rng(seed)
    blocks, coos = [], []
    for (n, k, absent) in specs:
        A = np.zeros((m + 1, n, n))
        if k is None:
            for i in range(1, m + 1):
                G = rng.standard_normal((n, n))
                A[i] = (G + G.T) / np.sqrt(2 * n)
            coos.append(None)
        else:
            var, row, col = [], [], []
            for v in range(1, m + 1):
                if v % 3 == absent:
                    continue
                for (r, c) in sorted(skc.draw_positions(rng, n, 1, k - 1)):
                    var.append(v); row.append(r); col.append(c)
            var = np.array(var, dtype=np.int32); row = np.array(row, dtype=np.int32); col = np.array(col, dtype=np.int32)
            val = rng.standard_normal(len(var))
            A[var, row, col] = val
            A[var, col, row] = val
            coos.append((var, row, col, val))
        blocks.append(A)
    D = rng.standard_normal((q, m)) * (rng.random((q, m)) < 0.3)
    y0 = rng.uniform(-1, 1, m)
    b = np.zeros(m)
    for A in blocks:
        n = A.shape[1]
        Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
        r = max(1, n // 3) if rank is None else rank
        ev = rng.uniform(1, 2, n)
        Xs = (Q * np.where(np.arange(n) < r, ev, 0)) @ Q.T
        Zs = (Q * np.where(np.arange(n) < r, 0, ev)) @ Q.T
        A[0] = np.tensordot(y0, A[1:], axes=(0, 0)) - Zs
        A[0] = 0.5 * (A[0] + A[0].T)
        b += A[1:].reshape(m, -1) @ Xs.reshape(-1)
    xs = rng.uniform(0, 1, q) * (rng.random(q) < 0.5)
    zs = rng.uniform(0.5, 1.5, q) * (xs == 0)
    c = D @ y0 - zs
    b += D.T @ xs
    return b, blocks, coos, D, c, float(b @ y0)


def _load_blocks(gpu, m, b, blocks, coos, D, c, policy):
    """blocks with triplets through hipsdp_add_entries (constant matrix as var 0) and their count, dense ones through
    hipsdp_set_block_dense with the count unknown"""
    s = gpu.Solver(0)
    s.sparse_policy(policy)
    cnt, ents = [], []
    for A, coo in zip(blocks, coos):
        if coo is None:
            cnt.append(-1); ents.append(None)
            continue
        n = A.shape[1]
        il = np.tril_indices(n)
        keep = A[0][il] != 0.0
        ents.append((np.concatenate([np.zeros(int(keep.sum()), dtype=np.int32), coo[0]]), np.concatenate([il[0][keep].astype(np.int32), coo[1]]),
                     np.concatenate([il[1][keep].astype(np.int32), coo[2]]), np.concatenate([A[0][il][keep], coo[3]])))
        cnt.append(len(ents[-1][3]))
    s.set_shape(m, [A.shape[1] for A in blocks], len(c), nnz=cnt)
    s.set_obj(b)
    for k, (A, e) in enumerate(zip(blocks, ents)):
        if e is None:
            s.set_block_dense(k, A)
        else:
            s.add_entries(k, *e)
    if len(c):
        s.set_lp(np.concatenate([np.asarray(c).reshape(-1, 1), D], axis=1))
    return s


def _solve_blocks_against_dense_storage_and_the_oracle(gpu, seed, m, specs, q, rank=None):
    b, blocks, coos, D, c, opt = _planted_blocks(seed, m, specs, q, rank)
    out = {}
    for policy in (2, 0):
        s = _load_blocks(gpu, m, b, blocks, coos, D, c, policy)
        for k, coo in enumerate(coos):
            assert s.is_sparse(k) == (policy == 2 and coo is not None)
        info = s.solve(gaptol=1e-7, feastol=1e-7)
        y = s.y()
        Xs = [s.X(k) for k in range(len(blocks))]
        if policy == 2:
            # a second solve of the same solver: the same bits, and no block kept as nonzeros goes through the cold-start store
            info2 = s.solve(gaptol=1e-7, feastol=1e-7)
            assert info2.status == info.status and info2.iterations == info.iterations
            assert np.array_equal(s.y().view(np.uint64), y.view(np.uint64))
            for k in range(len(blocks)):
                assert np.array_equal(s.X(k).view(np.uint64), Xs[k].view(np.uint64))
            assert s.gram_cache_stats() == (0, 0)
        s.close()
        out[policy] = (info, y, Xs)
    (info_s, y_s, X_s), (info_d, y_d, X_d) = out[2], out[0]
    assert info_d.status == 0 and info_s.status == 0
    assert abs(info_s.dobj - opt) <= 1e-6 * (1 + abs(opt)) and abs(info_d.dobj - opt) <= 1e-6 * (1 + abs(opt))
    assert info_s.iterations == info_d.iterations
    assert np.max(np.abs(y_s - y_d)) <= 1e-7 * (1 + np.max(np.abs(y_d)))
    for Xa, Xb in zip(X_s, X_d):
        assert np.max(np.abs(Xa - Xb)) <= 1e-6 * (1 + np.max(np.abs(Xb)))
    ref = ipm_ref.hsd_solve(ipm_ref.CoreProblem(b, blocks, D, c), ipm_ref.Params(gaptol=1e-7, feastol=1e-7))
    if ref.iterations != info_s.iterations:
        print("iterations: device %d, oracle %d" % (info_s.iterations, ref.iterations))
    assert ref.status == info_s.status
    assert abs(ref.iterations - info_s.iterations) <= 1
    assert np.max(np.abs(y_s - ref.y)) <= 1e-6 * (1 + np.max(np.abs(ref.y)))


def test_a_sparse_and_a_dense_block_with_lp_rows_in_one_problem(gpu):
    """mixed storage: a block of 70 rows kept as nonzeros (3 per matrix, a third of the variables absent from it) beside a dense block
    of 24 rows and 5 LP rows - the cold start's Gram form of the dense block, behind it the sparse loop adding into the same matrix,
    the LP term, and no fused small-problem assembly (the sparse block has no dense rows)"""
    _solve_blocks_against_dense_storage_and_the_oracle(gpu, 501, 40, [(70, 3, 0), (24, None, None)], 5)


def test_two_sparse_blocks_with_lp_rows(gpu):
    """66 and 70 rows, each without another third of the variables, 4 LP rows"""
    _solve_blocks_against_dense_storage_and_the_oracle(gpu, 502, 40, [(66, 3, 0), (70, 4, 1)], 4)


def test_the_wavefront_schur_kernel_serves_a_small_solve(gpu):
    """n = 70, m = 20, 20 nonzeros per matrix: 39 full entries on average, so every assembly of the solve is k_sp_schur's.

    The planted X has rank 5 here.  With 20 variables an optimal X of rank r is the only one when r (r + 1) / 2 <= 20 at most; at the
    rank n // 3 = 23 of the generator the optimal X form a face of dimension 256, an interior-point method ends near that face's
    analytic centre, and where exactly is decided by the roundings of the last iterations - two storages of the same problem then
    agree in y to 1e-14 while their X differ by more than the 1e-6 asked below, without either being wrong."""
    import sparse_kernel_cases as skc
    b, blocks, coos, D, c, opt = _planted_blocks(503, 20, [(70, 20, 3)], 0, rank=5)
    assert skc.rule_kernel(70, 20, coos[0]) == 1
    _solve_blocks_against_dense_storage_and_the_oracle(gpu, 503, 20, [(70, 20, 3)], 0, rank=5)


def test_either_triangle_and_duplicates_are_stored_as_the_dense_scatter_stores_them(gpu):
    """messy_input (entries of either triangle, positions given twice with different values) through hipsdp_add_entries: the block
    kept as nonzeros and the dense block hold the same matrices, the last of equal positions, and the device structure has the
    deduplicated count"""
    import sparse_kernel_cases as skc
    n, m, coo = skc.case("messy_input")
    cl = skc.clean(n, m, coo)
    got = {}
    for policy in (2, 0):
        s = gpu.Solver(0, units=True)
        s.sparse_policy(policy)
        s.set_shape(m, [n], 0, nnz=[len(coo[3])])
        s.set_obj(np.zeros(m))
        s.add_entries(0, *coo)
        assert s.is_sparse(0) == (policy == 2)
        got[policy] = s.get_block_dense(0)
        if policy == 2:
            assert s.sparse_dump(0)["nnz"] == len(cl[3]) < len(coo[3])
        s.close()
    assert np.array_equal(got[2].view(np.uint64), got[0].view(np.uint64))
    assert np.array_equal(got[2][1:], skc.expand(n, m, coo, dtype=np.float64)) and np.all(got[2][0] == 0.0)
