"""GPU: hipsdp_solve_objectives - ONE loaded problem under many objectives in one call: one workgroup of the one-launch kernel per
objective on the solver's matrices, each on a lane of its own (objective, iterate, workspace, results), filled by one fan-out launch.
Every job must end exactly as hipsdp_set_obj + hipsdp_solve + hipsdp_get_y end on a solver loaded the same way (and given the same
start point): every field of hipsdp_info but the two wall times and every y, compared as float.hex().  Jobs the kernel declines or
gives up on go to the general path from the same start; a problem the one-launch path is not offered is the loop."""
import ctypes as C
import os
import threading
import numpy as np
import pytest

import bnb
import bnb_many
import fuzz_shapes
import instances
import ipm_ref
import obbt
import sdpa_io
import sdpi_prepare
import test_gpu_solve_many as sm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TIMED = ("solve_seconds", "schur_seconds")
HIPSDP_ERR_ARG = 3                      # include/hipsdp.h
TOL = dict(gaptol=1e-6, feastol=1e-6, pabstol=1e-5)


@pytest.fixture(autouse=True)
def default_path(monkeypatch):
    for v in ("HIPSDP_SOLVE1", "HIPSDP_SOLVE1_NO_FALLBACK", "HIPSDP_SOLVE1_PROF", "HIPSDP_SOLVE1_HIST", "HIPSDP_OBJECTIVES_CHUNK"):
        monkeypatch.delenv(v, raising=False)


def rec(hb, info, y, path=None):
    d = {f: (getattr(info, f).hex() if isinstance(getattr(info, f), float) else getattr(info, f))
         for f, _ in hb.Info._fields_ if f not in TIMED}
    d["y"] = sm.hexes(y)
    if path is not None:
        d["path"] = path
    return d


def loop_ref(hb, core, B, start=None, fresh=True, pre=None, params=TOL, tail_b=None):
    """the reference: set_start (if any), set_obj, solve, get_y per job - on a fresh solver per job, or on one solver for all.
    pre(s): further calls behind the load.  Returns the records (with the solve path), the counters' increase, the Gram store's
    counts and, with tail_b, the record of one more solve of the last solver under that objective."""
    dc = np.zeros(3, dtype=np.int64)           # (the jobs' solves alone: pre may solve as well)
    out = []
    s = None
    for bj in B:
        if s is None or fresh:
            if s is not None:
                s.close()
            s = hb.Solver(0)
            s.load_core(core)
            if pre is not None:
                pre(s)
        if start is not None:
            s.set_start(*start)
        s.set_obj(bj)
        c0 = sm.counters(hb)
        info = s.solve(**params)
        dc += sm.counters(hb) - c0
        out.append(rec(hb, info, s.y(), s.solve_path()))
    gc = s.gram_cache_stats()
    if tail_b is not None:
        s.set_obj(tail_b)
        info = s.solve(**params)
        tail = rec(hb, info, s.y(), s.solve_path())
        s.close()
        return out, dc, gc, tail
    s.close()
    return out, dc, gc


def call(hb, core, B, start=None, pre=None, params=TOL, after=False):
    """the call on a freshly loaded solver; after: a plain solve behind it as well.  Returns records, counters, stats increase, ..."""
    s = hb.Solver(0)
    s.load_core(core)
    if pre is not None:
        pre(s)
    if start is not None:
        s.set_start(*start)
    c0 = sm.counters(hb)
    st0 = np.array(hb.solve_objectives_stats())
    infos, Y = s.solve_objectives(B, **params)
    dst = np.array(hb.solve_objectives_stats()) - st0
    dc = sm.counters(hb) - c0
    out = [rec(hb, i, Y[j]) for j, i in enumerate(infos)]
    gc = s.gram_cache_stats()
    tail = None
    if after:
        info = s.solve(**params)
        tail = rec(hb, info, s.y(), s.solve_path())
    s.close()
    return out, dc, dst, gc, tail


def assert_jobs(got, ref, tag):
    assert len(got) == len(ref)
    for j, (g, r) in enumerate(zip(got, ref)):
        for k in g:
            assert g[k] == r[k], "%s job %d: %s differs (%s / %s)" % (tag, j, k, g[k], r[k])


def six_objectives(core, seed=5):
    m = core.m
    rng = np.random.default_rng(seed)
    e0 = np.zeros(m); e0[0] = 1.0
    el = np.zeros(m); el[m - 1] = -1.0
    return np.array([core.b, e0, -e0, el, rng.standard_normal(m), rng.standard_normal(m)])


def class_shapes():
    """from seed 30000 on: the first shape of each size class, and further ones until a shape with LP rows and one with two or more
    blocks are among them"""
    picked, seen = [], set()
    have_q = have_blocks = False
    seed = 30000
    while len(seen) < 4 or not (have_q and have_blocks):
        core, tag = fuzz_shapes.problem(seed)
        c = sm.size_class(core)
        need = c not in seen or (not have_q and core.q > 0) or (not have_blocks and len(core.blocks) >= 2)
        if need:
            seen.add(c)
            have_q = have_q or core.q > 0
            have_blocks = have_blocks or len(core.blocks) >= 2
            picked.append((seed, c, core, tag))
        seed += 1
    return picked


SHAPES = class_shapes()


@pytest.mark.parametrize("seed,cls", [(s, c) for s, c, _, _ in SHAPES])
def test_six_objectives_per_size_class(gpu, seed, cls):
    core = [x[2] for x in SHAPES if x[0] == seed][0]
    B = six_objectives(core)
    ref, dref, _ = loop_ref(gpu, core, B)
    got, dgot, dst, _, _ = call(gpu, core, B)
    assert_jobs(got, ref, "seed %d class %d" % (seed, cls))
    assert np.array_equal(dgot, dref)
    served = sum(1 for r in ref if r["path"] == 1)
    print("seed %d class %d: %d of 6 jobs on the one-launch path, statuses %s" % (seed, cls, served, [r["status"] for r in ref]))
    assert list(dst) == [1, 2, served]          # one call: 1 fan-out + 1 solve launch


def test_classes_cover_the_four_instances_lp_rows_and_blocks():
    assert {c for _, c, _, _ in SHAPES} == {10, 16, 64, 1064}
    assert any(core.q > 0 for _, _, core, _ in SHAPES) and any(len(core.blocks) >= 2 for _, _, core, _ in SHAPES)


def small_shape():
    return [x[2] for x in SHAPES if x[1] == 10][0]


def test_one_objective(gpu):
    core = small_shape()
    B = six_objectives(core)[1:2]
    ref, dref, _ = loop_ref(gpu, core, B)
    got, dgot, dst, _, _ = call(gpu, core, B)
    assert_jobs(got, ref, "count 1")
    assert np.array_equal(dgot, dref) and list(dst)[:2] == [1, 2]


def test_one_variable(gpu):
    """m = 1, a 2 x 2 block: Z = y A_1 - A_0 with A_1 = I, A_0 = [[1, 0.5], [0.5, -2]]; min y is bounded, min -y is not"""
    A = np.zeros((2, 2, 2))
    A[0] = [[1.0, 0.5], [0.5, -2.0]]
    A[1] = np.eye(2)
    core = ipm_ref.CoreProblem(np.array([1.0]), [A])
    B = np.array([[1.0], [-1.0]])
    ref, dref, _ = loop_ref(gpu, core, B)
    got, dgot, dst, _, _ = call(gpu, core, B)
    assert_jobs(got, ref, "m = 1")
    assert np.array_equal(dgot, dref)
    assert ref[0]["status"] == 0 and ref[1]["status"] != 0


@pytest.mark.parametrize("chunk", [None, "128"])
def test_three_hundred_objectives(gpu, monkeypatch, chunk):
    """more workgroups than compute units; with HIPSDP_OBJECTIVES_CHUNK=128 three chunks (128 + 128 + 44) on 128 lanes"""
    core = small_shape()
    rng = np.random.default_rng(17)
    B = rng.standard_normal((300, core.m))
    B[0] = core.b
    ref, dref, _ = loop_ref(gpu, core, B, fresh=False)
    if chunk is not None:
        monkeypatch.setenv("HIPSDP_OBJECTIVES_CHUNK", chunk)
    got, dgot, dst, _, _ = call(gpu, core, B)
    assert_jobs(got, ref, "300 objectives")
    assert np.array_equal(dgot, dref)
    nchunks = 1 if chunk is None else 3
    assert list(dst) == [1, 2 * nchunks, sum(1 for r in ref if r["path"] == 1)]


def test_warm_start_and_the_solve_behind_it(gpu, monkeypatch):
    core = [x[2] for x in SHAPES if x[1] == 16][0]
    st = sm.loose_start(gpu, core, monkeypatch, 1e-2)
    B = six_objectives(core)[:5]
    ref, dref, _ = loop_ref(gpu, core, B, start=st)
    got, dgot, dst, _, tail = call(gpu, core, B, start=st, after=True)
    assert_jobs(got, ref, "warm")
    assert np.array_equal(dgot, dref)
    assert any(r["warm_started"] == 1 for r in ref)
    # the solver afterwards: its own objective back, the start consumed, no solution held - a fresh solver's solve
    fresh = gpu.Solver(0); fresh.load_core(core)
    info = fresh.solve(**TOL)
    assert tail == rec(gpu, info, fresh.y(), fresh.solve_path())
    assert tail["warm_started"] == 0
    fresh.close()


def test_warm_start_in_chunks(gpu, monkeypatch):
    """two lanes for five jobs: every chunk's fan-out starts its lanes from the solver's start point again"""
    core = small_shape()
    st = sm.loose_start(gpu, core, monkeypatch, 1e-2)
    B = six_objectives(core)[:5]
    ref, dref, _ = loop_ref(gpu, core, B, start=st)
    monkeypatch.setenv("HIPSDP_OBJECTIVES_CHUNK", "2")
    got, dgot, dst, _, _ = call(gpu, core, B, start=st)
    assert_jobs(got, ref, "warm, chunks of 2")
    assert list(dst)[:2] == [1, 6]


@pytest.mark.parametrize("warm", [False, True])
def test_numerical_fallback_in_the_middle(gpu, monkeypatch, warm):
    """seed 30123: its own objective makes the kernel give up (test_gpu_solve1.py) - row 2 of 5; the general path solves it from the
    same start, the counters move as in the loop, the rows around it are what they are without it"""
    core, _ = fuzz_shapes.problem(30123)
    st = sm.loose_start(gpu, core, monkeypatch, 1e-2) if warm else None
    six = six_objectives(core)
    B = np.array([six[1], six[4], core.b, six[2], six[5]])
    ref, dref, _ = loop_ref(gpu, core, B, start=st)
    got, dgot, dst, _, tail = call(gpu, core, B, start=st, after=True)
    assert_jobs(got, ref, "fallback")
    assert np.array_equal(dgot, dref)
    print("fallback counters (solves, fallbacks, warm):", dref, "paths", [r["path"] for r in ref])
    assert dref[1] >= 1
    if warm:
        assert dref[2] >= 1                       # (from the loose start the kernel gives up on other rows than it does cold)
    else:
        assert ref[2]["path"] == 0 and ref[2]["status"] == 0
    assert list(dst) == [1, 2, sum(1 for r in ref if r["path"] == 1)]
    fresh = gpu.Solver(0); fresh.load_core(core)
    info = fresh.solve(**TOL)
    assert tail == rec(gpu, info, fresh.y(), fresh.solve_path())
    fresh.close()


def test_never_offered_is_the_loop_with_the_gram_store(gpu):
    b, A, ys, Xs, Zs = instances.planted_dense(100, 20)
    core = ipm_ref.CoreProblem(b, [A])
    rng = np.random.default_rng(3)
    B = np.array([b, b + 0.1 * rng.standard_normal(20), b - 0.1 * rng.standard_normal(20)])
    ref, dref, gref, rtail = loop_ref(gpu, core, B, fresh=False, tail_b=b)
    got, dgot, dst, gc, tail = call(gpu, core, B, after=True)
    assert_jobs(got, ref, "100-row block")
    assert all(r["path"] == 0 for r in ref)
    assert np.array_equal(dgot, dref)
    assert gc[0] == 2 and gc == gref              # cold-start store: every job after the first is a hit
    assert list(dst) == [1, 0, 0]
    # the solver's own objective is back: the next solve is the one that follows the loop (the store serves it as well, so its
    # executed flops are not a fresh solver's) and differs from a fresh solver's in the flop counts alone
    assert tail == rtail
    fresh = gpu.Solver(0); fresh.load_core(core)
    info = fresh.solve(**TOL)
    ftail = rec(gpu, info, fresh.y(), fresh.solve_path())
    assert {k: v for k, v in tail.items() if not k.startswith("schur_flops")} == {k: v for k, v in ftail.items() if not k.startswith("schur_flops")}
    fresh.close()


def test_path_switched_off_with_a_start_point(gpu, monkeypatch):
    """HIPSDP_SOLVE1=0: never offered, so the call is the loop - here with a start point, which every job gets back from the home lane"""
    core = [x[2] for x in SHAPES if x[1] == 16][0]
    st = sm.loose_start(gpu, core, monkeypatch, 1e-2)
    B = six_objectives(core)[:4]
    monkeypatch.setenv("HIPSDP_SOLVE1", "0")
    ref, dref, _ = loop_ref(gpu, core, B, start=st)
    got, dgot, dst, _, tail = call(gpu, core, B, start=st, after=True)
    assert_jobs(got, ref, "switched off, warm")
    assert all(r["path"] == 0 for r in ref) and any(r["warm_started"] == 1 for r in ref)
    assert np.array_equal(dgot, dref) and list(dst) == [1, 0, 0]
    fresh = gpu.Solver(0); fresh.load_core(core)
    info = fresh.solve(**TOL)
    ftail = rec(gpu, info, fresh.y(), fresh.solve_path())
    # (the general path's cold-start store may serve the solve behind the call: the flop counts are not a fresh solver's)
    assert {k: v for k, v in tail.items() if not k.startswith("schur_flops")} == {k: v for k, v in ftail.items() if not k.startswith("schur_flops")}
    assert tail["warm_started"] == 0
    fresh.close()


def test_objectives_without_the_staging_arena(gpu, monkeypatch):
    """HIPSDP_NO_STAGING=1: the objectives reach the fan-out through device memory behind the lanes instead of the pinned arena"""
    core = small_shape()
    B = six_objectives(core)
    ref, dref, _ = loop_ref(gpu, core, B)
    monkeypatch.setenv("HIPSDP_NO_STAGING", "1")
    got, dgot, dst, _, _ = call(gpu, core, B)
    assert_jobs(got, ref, "no staging")
    assert np.array_equal(dgot, dref) and list(dst)[:2] == [1, 2]


def test_declined_by_the_kernel(gpu):
    core = sm.dense_lp_declined()
    rng = np.random.default_rng(4)
    B = np.array([core.b, core.b + 0.05 * rng.standard_normal(core.m)])
    ref, dref, _ = loop_ref(gpu, core, B)
    got, dgot, dst, _, _ = call(gpu, core, B)
    assert_jobs(got, ref, "declined")
    assert all(r["path"] == 0 for r in ref)
    assert np.array_equal(dgot, dref)


def test_pending_setters_are_flushed_once(gpu):
    core = [x[2] for x in SHAPES if x[1] == 16][0]
    A2 = core.blocks[0].copy()
    A2[0] = A2[0] - 0.25 * np.eye(A2.shape[1])
    rng = np.random.default_rng(9)
    lp = np.concatenate([np.asarray(core.c).reshape(-1, 1) - 0.125, core.D], axis=1) if core.q else None

    def pre(s):
        s.solve(**TOL)
        s.set_block_dense(0, A2)          # a changed constant matrix
        if lp is not None:
            s.set_lp(lp)                  # a deferred setter of shared data: it waits in the arena when the call comes
        s.set_obj(core.b * 0.5)           # ... and so does the solver's own objective
    B = six_objectives(core)
    ref, dref, _ = loop_ref(gpu, core, B, pre=pre)
    got, dgot, dst, _, tail = call(gpu, core, B, pre=pre, after=True)
    assert_jobs(got, ref, "pending setters")
    assert np.array_equal(dgot, dref)
    # the solver's own objective (the pending one) is back
    fresh = gpu.Solver(0); fresh.load_core(core); pre(fresh)
    info = fresh.solve(**TOL)
    assert tail == rec(gpu, info, fresh.y(), fresh.solve_path())
    fresh.close()


def free_bytes(hb):
    fr, tot = C.c_double(0), C.c_double(0)
    assert hb.lib().hipsdp_mem_info(0, C.byref(fr), C.byref(tot)) == 0
    return fr.value


def test_second_call_allocates_nothing(gpu):
    core = small_shape()
    rng = np.random.default_rng(2)
    B = rng.standard_normal((40, core.m))
    s = gpu.Solver(0)
    s.load_core(core)
    s.solve_objectives(B, **TOL)                  # warm-up: lanes, staging, the kernel's code
    f0 = free_bytes(gpu)
    i1, Y1 = s.solve_objectives(B, **TOL)
    f1 = free_bytes(gpu)
    i2, Y2 = s.solve_objectives(B[:17], **TOL)
    f2 = free_bytes(gpu)
    s.close()
    assert f0 == f1 == f2
    assert [rec(gpu, i, y) for i, y in zip(i2, Y2)] == [rec(gpu, i, y) for i, y in zip(i1[:17], Y1[:17])]


def test_two_host_threads(gpu):
    cores = [fuzz_shapes.problem(30000 + t)[0] for t in range(2)]
    Bs = [np.random.default_rng(40 + t).standard_normal((32, cores[t].m)) for t in range(2)]
    refs = [loop_ref(gpu, cores[t], Bs[t], fresh=False)[0] for t in range(2)]
    sol = [gpu.Solver(0) for _ in range(2)]
    for t in range(2):
        sol[t].load_core(cores[t])
    res, err = [None, None], []
    go = threading.Barrier(2)

    def run(t):
        try:
            go.wait()
            res[t] = sol[t].solve_objectives(Bs[t], **TOL)
        except Exception as e:          # (re-raised below, in the main thread)
            err.append(e)
    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err
    for t in range(2):
        assert_jobs([rec(gpu, i, y) for i, y in zip(*res[t])], refs[t], "thread %d" % t)
    for s in sol:
        s.close()


def test_argument_errors_change_nothing(gpu):
    lib = gpu.lib()
    core = small_shape()
    a = gpu.Solver(0)
    a.load_core(core)
    info = a.solve(**TOL)
    before = sm.snap(gpu, a, info)
    unshaped = gpu.Solver(0)
    m = core.m
    B = np.ascontiguousarray(six_objectives(core))
    pB = B.ctypes.data_as(C.POINTER(C.c_double))
    infos = (gpu.Info * 6)()
    Y = np.zeros((6, m))
    pY = Y.ctypes.data_as(C.POINTER(C.c_double))
    rcs = (C.c_int * 6)()
    p = gpu.Params(); lib.hipsdp_default_params(C.byref(p))
    pre = gpu.Params(); lib.hipsdp_default_params(C.byref(pre)); pre.preoptgap = 1e-2
    st0 = gpu.solve_objectives_stats()
    f = lib.hipsdp_solve_objectives
    assert f(None, 6, pB, C.byref(p), infos, pY, rcs) == HIPSDP_ERR_ARG
    assert f(unshaped.h, 6, pB, C.byref(p), infos, pY, rcs) == HIPSDP_ERR_ARG
    assert f(a.h, -1, pB, C.byref(p), infos, pY, rcs) == HIPSDP_ERR_ARG
    assert f(a.h, 6, None, C.byref(p), infos, pY, rcs) == HIPSDP_ERR_ARG
    assert f(a.h, 6, pB, C.byref(p), None, pY, rcs) == HIPSDP_ERR_ARG
    assert f(a.h, 6, pB, C.byref(pre), infos, pY, rcs) == HIPSDP_ERR_ARG
    assert "preoptgap" in lib.hipsdp_last_error().decode()
    assert f(a.h, 0, None, None, None, None, None) == 0
    assert gpu.solve_objectives_stats() == st0
    assert sm.snap(gpu, a, info) == before
    a.close(); unshaped.close()


def test_communicator_or_sharded_matrices_are_refused(gpu):
    """a solver with a communicator (rank 0 of 2 on the measurement transport; nothing is solved), replicated and with its matrices
    sharded by variable, and the latter once more when the communicator is gone"""
    lib = gpu.lib()
    core = small_shape()
    B = np.ascontiguousarray(six_objectives(core))
    pB = B.ctypes.data_as(C.POINTER(C.c_double))
    infos = (gpu.Info * 6)()
    p = gpu.Params(); lib.hipsdp_default_params(C.byref(p))
    st0 = gpu.solve_objectives_stats()
    for shard in (0, 1):
        s = gpu.Solver(0)
        comm = C.c_void_p()
        assert lib.hipsdp_comm_create_null(0, 2, C.byref(comm)) == 0
        assert lib.hipsdp_set_comm(s.h, comm, 0, 2) == 0
        assert lib.hipsdp_shard_matrices(s.h, shard) == 0
        s.load_core(core)
        assert lib.hipsdp_matrices_sharded(s.h) == shard
        assert lib.hipsdp_solve_objectives(s.h, 6, pB, C.byref(p), infos, None, None) == HIPSDP_ERR_ARG
        assert lib.hipsdp_set_comm(s.h, None, 0, 1) == 0
        if shard:
            assert lib.hipsdp_solve_objectives(s.h, 6, pB, C.byref(p), infos, None, None) == HIPSDP_ERR_ARG
        s.close()
        lib.hipsdp_comm_destroy(comm)
    assert gpu.solve_objectives_stats() == st0


@pytest.mark.parametrize("K", [1, 3, 257])
@pytest.mark.parametrize("m", [1, 7, 108])
def test_fanout_unit(gpu, K, m):
    rng = np.random.default_rng(1000 * K + m)
    guard = -7.25
    for ns in ([3], [10, 5], [37]):
        for q in (0, 5):
            for warm in (False, True):
                B = rng.standard_normal((K, m))
                b_own = rng.standard_normal(m)
                start = None
                if warm:
                    start = (rng.standard_normal(m), rng.standard_normal(q), rng.standard_normal(q),
                             [rng.standard_normal((n, n)) for n in ns], [rng.standard_normal((n, n)) for n in ns])
                lanes, offs, launches = gpu.objs_fanout_unit(B, b_own, ns, q=q, start=start, gap=2, guard=guard)
                assert launches == 1 and lanes.shape[0] == K + 1
                want = np.full(lanes.shape, guard)
                lens = [m, m, q, q] + [n * n for n in ns for _ in (0, 1)]
                for j in range(K + 1):
                    want[j, offs[0]:offs[0] + m] = b_own if j == 0 else B[j - 1]
                    if warm:
                        parts = [start[0], start[1], start[2]] + [M for k in range(len(ns)) for M in (start[3][k], start[4][k])]
                        for o, ln, src in zip(offs[1:], lens[1:], parts):
                            want[j, o:o + ln] = np.asarray(src).ravel()
                assert all(int(o) % 2 == 0 for o in offs)
                assert np.array_equal(lanes.view(np.uint64), want.view(np.uint64)), (K, m, ns, q, warm)


def tt_root():
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", "example_TT.dat-s.gz"))
    prob = bnb.instance_to_sdpi(inst)
    P = sdpi_prepare.prepare(prob)
    return inst, prob, P


def test_obbt_round_on_the_root_of_example_TT(gpu):
    inst, prob, P = tt_root()
    node = obbt.node_with_cutoff(P, 2.11803 + 1.0)
    assert node.core.m == 37 and node.core.blocks[0].shape[1] == 10
    # the relaxation the round starts from: the root itself (own objective, no cutoff row needed for it)
    b, blk, D, c, maps = sdpi_prepare.to_core(P)
    s = gpu.Solver(0)
    s.load_core(ipm_ref.CoreProblem(b, blk, D, c))
    assert s.solve(gaptol=1e-6, feastol=1e-6).status == 0
    relaxy = s.y()
    s.close()
    keep1, keep2 = [], []
    st0 = np.array(gpu.solve_objectives_stats())
    r1 = obbt.run(node, relaxy, obbt.engine_call_solver(gpu, 1e-6, keep1), gaptol=1e-6)
    dst = np.array(gpu.solve_objectives_stats()) - st0
    r2 = obbt.run(node, relaxy, obbt.engine_loop_solver(gpu, 1e-6, keep2), gaptol=1e-6)
    print("example_TT root: %d jobs, result %s, %d bounds accepted, stats %s" % (len(r1.jobs), r1.result, len(r1.newbounds), dst))
    assert len(r1.jobs) >= 37 and r1.jobs == r2.jobs
    assert [x.status for x in r1.results] == [x.status for x in r2.results]
    assert_jobs([rec(gpu, i, y) for i, y in zip(*keep1[0])], [rec(gpu, i, y) for i, y in zip(*keep2[0])], "obbt")
    assert r1.result == r2.result and r1.used == r2.used
    assert [(k, sd, float(v).hex()) for k, sd, v in r1.newbounds] == [(k, sd, float(v).hex()) for k, sd, v in r2.newbounds]
    assert dst[0] == 1 and dst[1] == 2
    # every job's value against the numpy oracle, at the project's parity tolerance
    ro = obbt.run(node, relaxy, obbt.oracle_solver(1e-6), gaptol=1e-6)
    assert [x.status for x in ro.results] == [x.status for x in r1.results]
    for j, (a, o) in enumerate(zip(r1.results, ro.results)):
        if o.status == 'optimal':
            assert abs(a.obj - o.obj) <= 1e-5 * max(1.0, abs(o.obj)), (j, a.obj, o.obj)
    # the tree from the tightened bounds still finds the optimum
    lb, ub = obbt.tightened_bounds(P, node, r1)
    prob2 = sdpi_prepare.SdpiProblem(prob.obj, lb, ub, prob.blocks, prob.lp, isintegral=prob.isintegral)
    solve_nodes, close = bnb_many.engine_node_solver(gpu, 16)
    best, y, nodes, failed = bnb_many.branch_and_bound_many(prob2, inst.intvars, solve_nodes, 16)
    close()
    print("B&B from the tightened bounds: optimum %s, %d nodes" % (best, nodes))
    assert failed == 0 and best is not None and abs(best - 2.11803) <= 1e-4
