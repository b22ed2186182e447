"""GPU: the routes by which matrices reach the device - hipsdp_add_entries (through the staging arena as a deferred command, through
pooled buffers with a wait), the master copy's two uploads, and the gathers from a dense and from a triplet master block with and
without the arena (HIPSDP_NO_STAGING=1 takes it away, so every small call falls through to its blocking route).

The device only moves values, so every comparison is equality of the doubles' bits against arrays built with numpy.  The last test
sends one problem through both sites that allocate the buffers of the preoptimal iterate."""
import os
import numpy as np
import pytest

import ipm_ref
import sdpa_io
import sp_master_cases as cases
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

SMALL_CALL = 16384                      # hipsdp_add_entries: calls of at most this many triplets try the arena


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def staging(monkeypatch, on):
    if on:
        monkeypatch.delenv("HIPSDP_NO_STAGING", raising=False)
    else:
        monkeypatch.setenv("HIPSDP_NO_STAGING", "1")


def dense_solver(gpu, m, n):
    s = gpu.Solver(0)
    s.sparse_policy(0)
    s.set_shape(m, [n], 0)
    assert not s.is_sparse(0)
    return s


def symmetric(m1, n, var, row, col, val):
    """what the scatter leaves of triplets that name every position at most once: both triangles"""
    A = np.zeros((m1, n, n))
    A[var, row, col] = val
    A[var, col, row] = val
    return A


_FULL = {}


def full_lower():
    """n = 32, m = 40: every lower-triangle position of all 41 matrices once, in random order: 21 648 triplets, more than a small call"""
    if not _FULL:
        n, m = 32, 40
        rng = np.random.default_rng(3240)
        il = np.tril_indices(n)
        L = len(il[0])
        var = np.repeat(np.arange(m + 1), L).astype(np.int32)
        row = np.tile(il[0], m + 1).astype(np.int32)
        col = np.tile(il[1], m + 1).astype(np.int32)
        p = rng.permutation(len(var))
        var, row, col = var[p], row[p], col[p]
        val = rng.standard_normal(len(var))
        assert len(val) == 21648 > SMALL_CALL
        _FULL.update(n=n, m=m, coo=(var, row, col, val), A=symmetric(m + 1, n, var, row, col, val))
    return _FULL


# ---- 1. the three routes of hipsdp_add_entries into a dense block --------------------------------------------------------------

@pytest.mark.parametrize("route", ["direct", "arena", "small-calls-without-arena"])
def test_add_entries_routes_store_the_same_block(gpu, monkeypatch, route):
    F = full_lower()
    staging(monkeypatch, route != "small-calls-without-arena")
    s = dense_solver(gpu, F["m"], F["n"])
    var, row, col, val = F["coo"]
    step = len(val) if route == "direct" else SMALL_CALL
    for e0 in range(0, len(val), step):
        s.add_entries(0, var[e0:e0 + step], row[e0:e0 + step], col[e0:e0 + step], val[e0:e0 + step])
    got = s.get_block_dense(0)
    s.close()
    assert np.array_equal(bits(got), bits(F["A"]))


# ---- 2. repeated positions on the small route --------------------------------------------------------------------------------------

def test_small_call_keeps_the_last_entry_of_a_repeated_position(gpu, monkeypatch):
    """50 triplets, six positions named twice - as (r, c) and later as (c, r), with another value: the later one stays, in both
    triangles, through the arena and through the pooled buffers alike"""
    n, m = 12, 5
    rng = np.random.default_rng(50)
    il = np.tril_indices(n, -1)
    pick = rng.choice(len(il[0]), size=44, replace=False)
    var = rng.integers(0, m + 1, size=44).astype(np.int32)
    row, col = il[0][pick].astype(np.int32), il[1][pick].astype(np.int32)
    again = rng.choice(44, size=6, replace=False)
    var, row, col = np.concatenate([var, var[again]]), np.concatenate([row, col[again]]), np.concatenate([col, row[again]])
    val = rng.standard_normal(50)
    assert len(val) == 50 and np.all(val[44:] != val[again])
    ref = np.zeros((m + 1, n, n))
    for v, r, c, x in zip(var, row, col, val):                      # in the caller's order: the later entry overwrites
        ref[v, r, c] = x
        ref[v, c, r] = x
    out = []
    for on in (True, False):
        staging(monkeypatch, on)
        s = dense_solver(gpu, m, n)
        s.add_entries(0, var, row, col, val)
        out.append(s.get_block_dense(0))
        s.close()
    assert np.array_equal(bits(out[0]), bits(ref))
    assert np.array_equal(bits(out[1]), bits(out[0]))


# ---- 3. an index out of range, on each route ---------------------------------------------------------------------------------------

def test_add_entries_refuses_an_index_out_of_range_on_both_routes(gpu):
    """the small route checks on the host and writes nothing; the direct route checks on the device, writes the entries in range and
    reports the one that is not.  After either, the solver takes the next call as ever."""
    F = full_lower()
    n, m = F["n"], F["m"]
    var, row, col, val = F["coo"]
    s = dense_solver(gpu, m, n)
    s.add_entries(0, var[:100], row[:100], col[:100], val[:100])
    before = s.get_block_dense(0)
    assert np.array_equal(bits(before), bits(symmetric(m + 1, n, var[:100], row[:100], col[:100], val[:100])))
    bad = row[100:110].copy()
    bad[4] = n
    with pytest.raises(RuntimeError, match="rc=3"):
        s.add_entries(0, var[100:110], bad, col[100:110], val[100:110])
    assert "hipsdp_add_entries: index out of range" in s.last_error()
    assert np.array_equal(bits(s.get_block_dense(0)), bits(before))
    # the direct route: all triplets at once, one row out of range
    bad = row.copy()
    k = 12345
    bad[k] = n
    with pytest.raises(RuntimeError, match="rc=3"):
        s.add_entries(0, var, bad, col, val)
    assert "hipsdp_add_entries: index out of range" in s.last_error()
    ref = F["A"].copy()
    ref[var[k], row[k], col[k]] = 0.0                                 # (every position is named once: nothing else wrote it)
    ref[var[k], col[k], row[k]] = 0.0
    assert np.array_equal(bits(s.get_block_dense(0)), bits(ref))
    s.add_entries(0, var[k:k + 1], row[k:k + 1], col[k:k + 1], val[k:k + 1])
    assert np.array_equal(bits(s.get_block_dense(0)), bits(F["A"]))
    s.close()


def master_as_gathered(s, N, S):
    """the whole dense master block, read through a gather of every slot and row into a dense engine block"""
    s.set_shape(S, [N], 0)
    assert s.master_gather(0, 0, list(range(S)), list(range(N))) == 0, s.last_error()
    return s.get_block_dense(0)[1:]


@pytest.mark.parametrize("call", ["master_add_entries", "master_add_vars"])
def test_dense_master_refuses_a_column_out_of_range(gpu, call):
    N, S = 12, 6
    rng = np.random.default_rng(126)
    il = np.tril_indices(N)
    slots = []
    for k in range(S):
        p = rng.choice(len(il[0]), size=9, replace=False)
        slots.append((il[0][p].astype(np.int32), il[1][p].astype(np.int32), rng.standard_normal(9)))
    s = gpu.Solver(0)
    s.sparse_policy(0)
    s.master_define(S, [N], [S])
    assert not s.master_block_is_sparse(0)
    flat = lambda sl: (np.concatenate([np.full(len(v), k, dtype=np.int32) for k, (_, _, v) in enumerate(sl)]),
                       np.concatenate([r for r, _, _ in sl]), np.concatenate([c for _, c, _ in sl]), np.concatenate([v for _, _, v in sl]))

    def add(sl):
        if call == "master_add_entries":
            return s.master_add_entries(0, *flat(sl))
        return s.master_add_vars(0, [r for r, _, _ in sl], [c for _, c, _ in sl], [v for _, _, v in sl])
    bad = [(r.copy(), c.copy(), v) for r, c, v in slots[:3]]
    bad[1][1][4] = N
    assert add(bad) == 3
    assert "hipsdp_%s: index out of range" % call in s.last_error()
    assert add(slots) == 0, s.last_error()
    var, row, col, val = flat(slots)
    assert np.array_equal(bits(master_as_gathered(s, N, S)), bits(symmetric(S, N, var, row, col, val)))
    s.close()


# ---- 4. gathers with and without the arena -----------------------------------------------------------------------------------------

def numpy_gather(N, slots, node):
    nk = len(node.kept)
    A = np.zeros((node.m + 1, nk, nk))
    for a, k in enumerate(node.act):
        if k < 0:
            continue
        M = np.zeros((N, N))
        r, c, v = slots[k]
        M[r, c] = v
        M[c, r] = v
        A[a + 1] = M[np.ix_(node.kept, node.kept)]
    return A


def gather_cases():
    """N = 96, 8 slots, each position at most once per slot.  Seven variables on all rows touch 7 * 96^2 = 64 512 elements, which a
    deferred command may (at most 65 536); eight touch 73 728, and the gather is a launch of its own.  And one node of shape A with
    removed rows and an absent variable."""
    N, S = 96, 8
    rng = np.random.default_rng(96)
    il = np.tril_indices(N)
    big = []
    for k in range(S):
        p = rng.choice(len(il[0]), size=400, replace=False)
        big.append((il[0][p].astype(np.int32), il[1][p].astype(np.int32), rng.standard_normal(400)))
    assert 7 * N * N <= 65536 < 8 * N * N
    Na, sa, na = cases.shape_a()
    node_a = na[7]
    assert -1 in node_a.act and len(node_a.kept) < Na
    return [(N, big, [cases.Node("seven", [3, 0, 6, 1, 5, 2, 4], range(N)), cases.Node("eight", [7, 3, 0, 6, 1, 5, 2, 4], range(N))]),
            (Na, cases.once_per_position(sa), [node_a])]


@pytest.mark.parametrize("triplets", [False, True], ids=["dense-master", "triplet-master"])
@pytest.mark.parametrize("arena", [True, False], ids=["arena", "no-staging"])
def test_gathers_into_a_dense_block(gpu, monkeypatch, triplets, arena):
    staging(monkeypatch, arena)
    for N, slots, nodes in gather_cases():
        s = gpu.Solver(0)
        s.sparse_policy(0)
        total = sum(len(v) for _, _, v in slots)
        s.master_define(len(slots), [N], [len(slots)], nnz=[total] if triplets else None)
        assert s.master_block_is_sparse(0) == triplets
        assert s.master_add_vars(0, [r for r, _, _ in slots], [c for _, c, _ in slots], [v for _, _, v in slots]) == 0
        for node in nodes:
            s.set_shape(node.m, [len(node.kept)], 0)
            assert not s.is_sparse(0)
            assert s.master_gather(0, 0, node.act, node.kept) == 0, s.last_error()
            got = s.get_block_dense(0)
            assert np.array_equal(bits(got), bits(numpy_gather(N, slots, node))), (N, node.name)
        stats = s.master_gather_stats()
        s.close()
        print("N %d, %s master, %s: stats %s" % (N, "triplet" if triplets else "dense", "arena" if arena else "no staging", stats))
        assert stats[:2] == (0, 0)
        # read-backs: none with the arena; without it, the blocking gather from a triplet master counts one each
        assert stats[3] == (len(nodes) if triplets and not arena else 0)


# ---- 5. the buffers of the preoptimal iterate, allocated by either path --------------------------------------------------------------

def test_preoptimal_iterate_from_both_paths(gpu, monkeypatch):
    """example_TT with preoptgap > 0: the one-launch path allocates the buffers before its launch, the general path at the capture;
    the iterate is there after both and agrees to the tolerances tests/test_gpu_solve1.py uses for it"""
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", "example_TT.dat-s.gz"))
    D, c = sdpa_io.lp_dense(inst)
    core = ipm_ref.CoreProblem(inst.obj, sdpa_io.dense_blocks(inst), D, c)
    pre = []
    for path in (1, 0):
        monkeypatch.setenv("HIPSDP_SOLVE1", str(path))
        s = gpu.Solver(0)
        s.load_core(core)
        info = s.solve(gaptol=1e-7, feastol=1e-6, preoptgap=1e-2)
        assert s.solve_path() == path and info.status == 0
        pre.append(s.preoptimal())
        s.close()
        assert pre[-1] is not None
    one, gen = pre
    assert np.allclose(one[0], gen[0], atol=1e-7, rtol=1e-6)
    assert np.allclose(one[1][0], gen[1][0], atol=1e-6, rtol=1e-6)
    assert np.allclose(one[2], gen[2], atol=1e-6, rtol=1e-6)
