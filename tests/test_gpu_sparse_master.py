"""GPU: the master copy of a block kept as triplets (csrc/sp_master.hip) and the gather of a node from it.

The device only moves and renumbers values, so every comparison here is exact equality, doubles by their bits: the reference for
every array of a gathered block is what the host builder (hs_sp_build) makes of the triplets the direct load would have marshalled
for the same node, and the reference for every solve is the direct load on a fresh solver.  All solvers use sparse_policy(2) so that
small blocks are kept as nonzeros.

Shapes (tests/harness/sp_master_cases.py): A (N = 12, 6 slots, one of them dense: a segment longer than a wavefront; nodes with
removed rows, an emptied slot, absent variables, inactive slots, trailing empty variables, nothing kept, slot order not monotone),
B (N = 40, 64 slots, 2560 entries, positions shared by several variables), and two that the kernels' own thresholds ask for: `wide`
(more variables and positions than the 1024 of one scan workgroup) and `long` (more than 256 scan workgroups: the carry of the top
scan).  C (N = 96, 60 slots, 3 entries each) carries the solves."""
import os
import numpy as np
import pytest

import instances
import sp_master_cases as cases

pytestmark = pytest.mark.gpu

INT_KEYS = ("voff", "vrow", "vcol", "poff", "prow", "pcol", "pvar", "foff", "frow", "fcol", "soff", "srow", "sent")
VAL_KEYS = ("vval", "pval", "fval")
COUNTS = ("n", "m", "nnz", "npos", "nfull", "nslots")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_structure(got, ref, what):
    for k in COUNTS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in INT_KEYS:
        assert np.array_equal(got[k], ref[k]), (what, k)
    for k in VAL_KEYS:
        assert np.array_equal(bits(got[k]), bits(ref[k])), (what, k)


def define_master(s, N, slots, triplets=True):
    total = sum(len(v) for _, _, v in slots)
    s.master_define(len(slots), [N], [len(slots)], nnz=[total] if triplets else None)
    assert s.master_block_is_sparse(0) == triplets
    assert s.master_add_vars(0, [r for r, _, _ in slots], [c for _, c, _ in slots], [v for _, _, v in slots]) == 0


def host_built(hb, N, slots, node):
    """hipsdp_set_shape2 + hipsdp_add_entries of the node's marshalled triplets: the structure hs_sp_build makes"""
    s = hb.Solver(0, units=True)
    s.sparse_policy(2)
    var, row, col, val = cases.marshal(slots, N, node)
    s.set_shape(node.m, [len(node.kept)], 0, nnz=[len(val)])
    assert s.is_sparse(0)
    s.add_entries(0, var, row, col, val)
    d = s.sparse_dump(0)
    assert s.master_gather_stats()[:2] == (0, 1)
    s.close()
    return d


def gather_node(s, N, slots, node):
    var, row, col, val = cases.marshal(slots, N, node)
    s.set_shape(node.m, [len(node.kept)], 0, nnz=[len(val)])
    assert s.is_sparse(0)
    rc = s.master_gather(0, 0, node.act, node.kept)
    assert rc == 0, (rc, s.last_error())


# ---- 1. structure ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["shape_a", "shape_b", "shape_wide", "shape_long"])
def test_gathered_structure_is_the_host_builders(gpu, shape):
    """every array and the four counts, for every node of the shape, gathered one after the other on ONE solver (the workspace of the
    master block is reused from node to node); the counters say who built what"""
    N, slots, nodes = getattr(cases, shape)()
    s = gpu.Solver(0, units=True)
    s.sparse_policy(2)
    define_master(s, N, slots)
    launches = []
    for i, node in enumerate(nodes):
        before = s.master_gather_stats()
        gather_node(s, N, slots, node)
        got = s.sparse_dump(0)
        after = s.master_gather_stats()
        same_structure(got, host_built(gpu, N, slots, node), (shape, node.name))
        assert after[0] == before[0] + 1 and after[1] == 0 and after[3] == before[3] + 1, (node.name, before, after)
        launches.append(after[2] - before[2])
        print("%s / %s: nnz %d npos %d nfull %d nslots %d, %d launches" % (shape, node.name, got["nnz"], got["npos"], got["nfull"],
                                                                            got["nslots"], launches[-1]))
    s.close()
    # a constant, plus the ordering launch where the slots do not increase with the variable
    base = set()
    for node, l in zip(nodes, launches):
        mono = [a for a in node.act if a >= 0]
        base.add(l - (0 if mono == sorted(mono) else 1))
    assert len(base) == 1, list(zip([nd.name for nd in nodes], launches))


# ---- 2. / 3. solves --------------------------------------------------------------------------------------------------------

class SolveCase:
    pass


_C = {}


def shape_c():
    if _C:
        return _C
    n, m, k = 96, 60, 3
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=96)
    var, row, col, val = coo
    slots = [(row[var == v + 1], col[var == v + 1], val[var == v + 1]) for v in range(m)]
    A = instances.coo_to_dense(n, m, coo, A0)

    def make(name, act, kept):
        c = SolveCase()
        c.node = cases.Node(name, act, kept)
        fixed = [v for v in range(m) if v not in act]
        # variables fixed at their planted value move into the constant matrix; removed rows take the principal submatrix
        C0 = A0 - sum(ys[v] * A[v + 1] for v in fixed) if fixed else A0.copy()
        C0 = C0[np.ix_(kept, kept)]
        il = np.tril_indices(len(kept))
        nz = C0[il] != 0.0
        c.const = (np.zeros(int(nz.sum()), dtype=np.int32), il[0][nz].astype(np.int32), il[1][nz].astype(np.int32), C0[il][nz])
        c.b = b[list(act)]
        return c
    _C["n"], _C["slots"] = n, slots
    _C["root"] = make("root", list(range(m)), list(range(n)))
    _C["fixed"] = make("fixed", [v for v in range(m) if v % 4 != 1], list(range(n)))
    _C["rows"] = make("rows+fixed", [v for v in range(m) if v % 5 != 2], [r for r in range(n) if r not in (5, 40, 95)])
    _C["small"] = make("small", [7, 3], list(range(20, 90)))
    _C["direct"] = {}
    return _C


def snap(s, info):
    return (info.status, info.iterations, bits([info.dobj]).tobytes(), bits(s.y()).tobytes(), bits(s.X(0)).tobytes(), bits(s.Z(0)).tobytes())


def load_and_solve(s, C, c, gathered):
    var, row, col, val = cases.marshal(C["slots"], C["n"], c.node)
    s.set_shape(c.node.m, [len(c.node.kept)], 0, nnz=[len(val) + len(c.const[3])])
    s.set_obj(c.b)
    if gathered:
        assert s.master_gather(0, 0, c.node.act, c.node.kept) == 0, s.last_error()
        s.add_entries(0, *c.const)
    else:
        s.add_entries(0, np.concatenate([var, c.const[0]]), np.concatenate([row, c.const[1]]), np.concatenate([col, c.const[2]]),
                      np.concatenate([val, c.const[3]]))
    assert s.is_sparse(0)
    info = s.solve(gaptol=1e-6, feastol=1e-6)
    assert s.solve_path() == 0                  # the general path: Schur assembly, A(V) and A^T(coef) from the block's structure
    return snap(s, info)


def direct_sequence(gpu, C, names):
    """the direct loads of a sequence of nodes, in that order on one fresh solver (kept: several tests ask for the same sequences)"""
    key = tuple(names)
    if key not in C["direct"]:
        s = gpu.Solver(0)
        s.sparse_policy(2)
        C["direct"][key] = [load_and_solve(s, C, C[nm], False) for nm in names]
        assert s.master_gather_stats()[:2] == (0, len(names))
        s.close()
    return C["direct"][key]


def gathered_sequence(gpu, C, names):
    s = gpu.Solver(0)
    s.sparse_policy(2)
    define_master(s, C["n"], C["slots"])
    out = [load_and_solve(s, C, C[nm], True) for nm in names]
    assert s.master_gather_stats()[:2] == (len(names), 0)
    s.close()
    return out


def test_solves_from_gathered_blocks_are_the_direct_loads(gpu):
    C = shape_c()
    names = ["root", "fixed", "rows"]
    ref = direct_sequence(gpu, C, names)
    got = gathered_sequence(gpu, C, names)
    for nm, g, r in zip(names, got, ref):
        print("%s: status %d, %d iterations" % (nm, g[0], g[1]))
        assert g[:2] == r[:2], (nm, g[:2], r[:2])
        assert g == r, nm
    assert ref[0][0] == 0                                         # the root is the planted instance: it has an optimum
    assert gathered_sequence(gpu, C, names) == got                # two gathers of the same nodes: the same bits


def test_workspace_of_the_master_block_carries_nothing_over(gpu):
    """a large node, the smallest one, the large one again on one solver; each against a FRESH directly loaded solver"""
    C = shape_c()
    got = gathered_sequence(gpu, C, ["root", "small", "root"])
    for nm, g in zip(["root", "small", "root"], got):
        assert g == direct_sequence(gpu, C, [nm])[0], nm


# ---- 4. dense target, read-back of the matrices ------------------------------------------------------------------------------

def test_dense_engine_block_and_get_block_dense(gpu):
    """a triplet master block gathered into a DENSE engine block against the dense master's gather, and hipsdp_get_block_dense of a
    gathered block kept as nonzeros against the direct load's.  The dense master scatters its entries in no order - which of two
    entries at one position stays is not defined there - so both masters of the first comparison get every position once; the
    blocks kept as nonzeros, where the later entry counts by rule, get the repeated positions of shape A as they are."""
    N, slots, nodes = cases.shape_a()
    st = gpu.Solver(0); st.sparse_policy(0); define_master(st, N, cases.once_per_position(slots), triplets=True)
    sd = gpu.Solver(0); sd.sparse_policy(0); define_master(sd, N, cases.once_per_position(slots), triplets=False)
    sg = gpu.Solver(0); sg.sparse_policy(2); define_master(sg, N, slots, triplets=True)
    sh = gpu.Solver(0); sh.sparse_policy(2)
    for node in nodes:
        var, row, col, val = cases.marshal(slots, N, node)
        dense = []
        for s in (st, sd):
            s.set_shape(node.m, [len(node.kept)], 0, nnz=[len(val)])
            assert not s.is_sparse(0)
            assert s.master_gather(0, 0, node.act, node.kept) == 0, s.last_error()
            dense.append(s.get_block_dense(0))
        assert np.array_equal(bits(dense[0]), bits(dense[1])), node.name
        gather_node(sg, N, slots, node)
        sh.set_shape(node.m, [len(node.kept)], 0, nnz=[len(val)])
        sh.add_entries(0, var, row, col, val)
        got, ref = sg.get_block_dense(0), sh.get_block_dense(0)
        assert np.array_equal(bits(got), bits(ref)), node.name
        assert np.array_equal(bits(got), bits(dense[1])), node.name
    assert st.master_gather_stats()[:2] == (0, 0) and st.master_gather_stats()[2] == sum(1 for nd in nodes if len(nd.act) > 0)
    for s in (st, sd, sg, sh):
        s.close()


# ---- 5. consumers --------------------------------------------------------------------------------------------------------------

def test_eigencuts_and_check_y_on_a_gathered_block(gpu):
    N, slots, nodes = cases.shape_b()
    node = nodes[1]
    var, row, col, val = cases.marshal(slots, N, node)
    nk = len(node.kept)
    rng = np.random.default_rng(5)
    il = np.tril_indices(nk)
    const = (np.zeros(len(il[0]), dtype=np.int32), il[0].astype(np.int32), il[1].astype(np.int32), rng.standard_normal(len(il[0])))
    y = rng.standard_normal(node.m)
    out = []
    for gathered in (True, False):
        s = gpu.Solver(0)
        s.sparse_policy(2)
        s.set_shape(node.m, [nk], 0, nnz=[len(val) + len(const[3])])
        if gathered:
            define_master(s, N, slots)
            assert s.master_gather(0, 0, node.act, node.kept) == 0, s.last_error()
            s.add_entries(0, *const)
        else:
            s.add_entries(0, np.concatenate([const[0], var]), np.concatenate([const[1], row]), np.concatenate([const[2], col]),
                          np.concatenate([const[3], val]))
        lmin, viol = s.check_y(y)
        cuts = s.eigencuts_all(y, 1e-6, 4)
        assert s.master_gather_stats()[:2] == ((1, 0) if gathered else (0, 1))
        s.close()
        out.append((bits(lmin).tobytes(), viol, [(bits([c[0]]).tobytes(),) + tuple(bits(a).tobytes() for a in c[1:]) for c in cuts]))
        assert len(cuts[0][1]) > 0                                   # an indefinite Z(y): there are cuts to compare
    assert out[0] == out[1]


# ---- 6. contract ---------------------------------------------------------------------------------------------------------------

def test_contract_of_a_gathered_block(gpu):
    N, slots, nodes = cases.shape_a()
    node = nodes[1]
    s = gpu.Solver(0)
    s.sparse_policy(2)
    define_master(s, N, slots)
    gather_node(s, N, slots, node)
    one = lambda v: (np.array([v], dtype=np.int32), np.array([2], dtype=np.int32), np.array([1], dtype=np.int32), np.array([0.5]))
    with pytest.raises(RuntimeError, match="rc=3"):
        s.add_entries(0, *one(1))                                    # a variable's matrix after the gather: refused, with a message
    assert "gathered" in s.last_error()
    s.add_entries(0, *one(0))                                        # the constant matrix: as ever
    A = s.get_block_dense(0)
    assert A[0][2, 1] == 0.5 and A[0][1, 2] == 0.5
    assert s.master_gather_stats()[:2] == (1, 0)
    # slots and rows out of range, a slot named twice, rows not increasing
    nk = len(node.kept)
    assert s.master_gather(0, 0, [0, 6], node.kept) == 3
    assert s.master_gather(0, 0, [0, -2], node.kept) == 3
    assert s.master_gather(0, 0, [2, 2], node.kept) == 3
    assert s.master_gather(0, 0, [0, 1], node.kept[:-1] + [N]) == 3
    assert s.master_gather(0, 0, [0, 1], node.kept[1:] + node.kept[:1]) == 3
    assert s.master_gather(0, 0, [0, 1], node.kept[:-1]) == 3        # not the engine block's size
    assert nk == len(node.kept)
    # the rule ends with the next set_shape
    s.set_shape(node.m, [nk], 0, nnz=[4])
    s.add_entries(0, *one(1))
    # entries of a triplet master block are checked on the host
    assert s.master_add_entries(0, [0], [N], [0], [1.0]) == 3
    assert s.master_add_entries(0, [6], [0], [0], [1.0]) == 3
    assert s.master_add_entries(0, [5], [0], [N - 1], [1.0]) == 0
    s.close()
    # a DENSE master block into a block kept as nonzeros: the error and message of before
    s = gpu.Solver(0)
    s.sparse_policy(2)
    define_master(s, N, slots, triplets=False)
    s.set_shape(node.m, [nk], 0, nnz=[10])
    assert s.is_sparse(0)
    assert s.master_gather(0, 0, node.act, node.kept) == 3
    assert "not available with matrices sharded by variable or kept as nonzeros" in s.last_error()
    s.close()


def test_launches_and_readbacks_do_not_depend_on_the_size(gpu):
    per = []
    for shape in ("shape_a", "shape_b", "shape_wide"):
        N, slots, nodes = getattr(cases, shape)()
        s = gpu.Solver(0)
        s.sparse_policy(2)
        define_master(s, N, slots)
        gather_node(s, N, slots, nodes[0])
        d0 = s.master_gather_stats()
        gather_node(s, N, slots, nodes[0])
        d1 = s.master_gather_stats()
        s.close()
        assert d0[:2] == (1, 0) and d1[:2] == (2, 0)
        assert d0[3] == 1 and d1[3] == 2                             # one read-back per gather
        assert d1[2] == 2 * d0[2]
        per.append(d0[2])
    assert per[0] == per[1] == per[2], per


# ---- 7. boundary ---------------------------------------------------------------------------------------------------------------

def two_block_misdp():
    """example_TT (a 10 x 10 block, 85 LP rows, 37 variables) with a second, planted block of 70 rows: three small nonzeros per variable
    and the constant matrix -10 I, so that it is positive definite wherever the tree goes and takes part in every solve"""
    import bnb, sdpa_io, sdpi_prepare
    inst = sdpa_io.read_sdpa(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances", "example_TT.dat-s.gz"))
    prob = bnb.instance_to_sdpi(inst)
    rng = np.random.default_rng(70)
    n = 70
    vars_ = {}
    for v in range(inst.m):
        ent = {}
        while len(ent) < 3:
            r, c = int(rng.integers(0, n)), int(rng.integers(0, n))
            ent[(max(r, c), min(r, c))] = 1e-3 * float(rng.standard_normal())
        vars_[v] = [(r, c, x) for (r, c), x in sorted(ent.items())]
    extra = dict(n=n, vars=vars_, const=[(i, i, -10.0) for i in range(n)])
    return sdpi_prepare.SdpiProblem(prob.obj, prob.lb, prob.ub, list(prob.blocks) + [extra], prob.lp, isintegral=prob.isintegral), inst.intvars


@pytest.mark.parametrize("policy", ["2", "1"])
def test_tree_through_the_solver_interface_cached_against_uncached(gpu, monkeypatch, policy):
    """60 nodes of a branch-and-bound run through SCIPsdpiSolverLoadAndSolve, every node on two solvers: one with HIPSDP_NOCACHE=1
    (the direct load of every node, as before) and one with the master copy.  HIPSDP_SPARSE=2 keeps both blocks as nonzeros;
    with the default policy (1) the cost rule keeps the planted block as nonzeros and example_TT's 10 x 10 block dense, which is the
    problem with one block of each kind.  Outcome, objective, y and iteration count of every node: the same bits."""
    import ctypes as C
    import bnb, sdpi_call
    prob, intvars = two_block_misdp()
    monkeypatch.setenv("HIPSDP_SOLVE1", "0")
    monkeypatch.setenv("HIPSDP_SPARSE", policy)
    lib = gpu.lib()
    sa, sb = sdpi_call.SdpiSolver(lib), sdpi_call.SdpiSolver(lib)
    for s in (sa, sb):
        for p in (1, 2, 3):
            assert s.set_real(p, 1e-6) == sdpi_call.SCIP_OKAY

    def stats(s):
        v = [C.c_longlong(-1) for _ in range(4)]
        assert lib.hipsdp_compat_gather_stats(s.h, *[C.byref(x) for x in v]) == 0
        return tuple(x.value for x in v)

    def outcome(s):
        if s.flag("IsDualInfeasible"):
            return ('infeasible', s.iterations())
        if not s.flag("IsOptimal"):
            return ('failed', s.iterations())
        rc, obj, y = s.dual_sol()
        return ('optimal', s.iterations(), bits([obj]).tobytes(), bits(y).tobytes(), obj, y)
    seen = dict(nodes=0, after_first=None, roots=[])

    def solve(P):
        if not seen["roots"]:
            seen["roots"].append(P)
        monkeypatch.setenv("HIPSDP_NOCACHE", "1")
        sa.solve(P)
        oa = outcome(sa)
        monkeypatch.delenv("HIPSDP_NOCACHE")
        sb.solve(P)
        ob = outcome(sb)
        assert oa[:4] == ob[:4], (seen["nodes"], oa[:2], ob[:2])
        seen["nodes"] += 1
        if seen["nodes"] == 1:
            seen["after_first"] = stats(sb)
        return bnb.NodeResult(oa[0]) if oa[0] != 'optimal' else bnb.NodeResult('optimal', oa[4], oa[5])
    bnb.branch_and_bound(prob, intvars, solve, maxnodes=60)
    assert seen["nodes"] >= 20
    first, last, unc = seen["after_first"], stats(sb), stats(sa)
    print("policy %s: %d nodes; cached solver: device builds %d, host builds %d, launches %d, read-backs %d; uncached: host builds %d"
          % (policy, seen["nodes"], last[0], last[1], last[2], last[3], unc[1]))
    assert last[0] > first[0] > 0 and last[1] == first[1] == 0        # built on the device from the first node on, never on the host
    assert unc[0] == 0 and unc[1] >= seen["nodes"]                    # HIPSDP_NOCACHE=1: the direct load of before
    # one node with the penalty formulation: the block kept as nonzeros is loaded directly, and the solve succeeds
    rc, feasorig, pbound = sb.solve(seen["roots"][0], penaltyparam=1e5, withobj=True, rbound=True)
    assert rc == sdpi_call.SCIP_OKAY and sb.flag("IsOptimal")
    pen = stats(sb)
    assert pen[1] > last[1] and pen[0] == last[0]
    sa.free(); sb.free()
