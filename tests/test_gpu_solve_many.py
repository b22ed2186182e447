"""GPU: hipsdp_solve_many - many independent problems in one call, the one-launch kernel once per size class with one workgroup per
problem, the rest on the general path.  Every problem must end exactly as hipsdp_solve alone leaves it: status, iterations, solve
path, every field of hipsdp_info but the two wall times (solve_seconds, schur_seconds), y, x, z, every X and Z and the preoptimal
iterate, compared as float.hex().  The reference of each problem is a fresh solver that goes through the same calls with
hipsdp_solve."""
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
import sdpa_io
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TIMED = ("solve_seconds", "schur_seconds")
HIPSDP_ERR_ARG = 3                      # include/hipsdp.h
TOL = dict(gaptol=1e-6, feastol=1e-6, pabstol=1e-5)


def hexes(a):
    return [float(v).hex() for v in np.asarray(a, dtype=float).ravel()]


def snap(hb, s, info):
    d = {f: (getattr(info, f).hex() if isinstance(getattr(info, f), float) else getattr(info, f))
         for f, _ in hb.Info._fields_ if f not in TIMED}
    d["path"] = s.solve_path()
    d["y"] = hexes(s.y())
    for k in range(len(s.ns)):
        d["X%d" % k] = hexes(s.X(k))
        d["Z%d" % k] = hexes(s.Z(k))
    if s.q:
        x, z = s.lp()
        d["x"], d["z"] = hexes(x), hexes(z)
    pre = s.preoptimal()
    d["pre"] = None if pre is None else [hexes(pre[0]), [hexes(X) for X in pre[1]], hexes(pre[2])]
    return d


def instance_core(name):
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", name))
    D, c = sdpa_io.lp_dense(inst)
    return ipm_ref.CoreProblem(inst.obj, sdpa_io.dense_blocks(inst), D, c)


ROOTS = ["example_TT.dat-s.gz", "example_MkP.dat-s.gz", "example_small.dat-s", "example_tightenmatrices.dat-s"]


def size_class(core):
    nmax = max(A.shape[1] for A in core.blocks)
    return 1064 if core.m > 64 else (10 if nmax <= 10 else (16 if nmax <= 16 else 64))


def load(s, spec):
    """spec: dict(core=CoreProblem) or dict(sparse=(n, m, b, coo, A0)); optional start=(y, X, Z, x, z)"""
    if "sparse" in spec:
        s.sparse_policy(2)
        s.load_sparse(*spec["sparse"])
    else:
        s.load_core(spec["core"])
    if spec.get("start") is not None:
        s.set_start(*spec["start"])


def counters(hb):
    lib = hb.lib()
    for f in ("hipsdp_solve1_solves", "hipsdp_solve1_fallbacks", "hipsdp_solve1_fallbacks_warm"):
        getattr(lib, f).restype = C.c_longlong
    return np.array([lib.hipsdp_solve1_solves(), lib.hipsdp_solve1_fallbacks(), lib.hipsdp_solve1_fallbacks_warm()])


def solo(hb, specs, params):
    """the reference: one fresh solver per problem, hipsdp_solve; snapshots and the counters' increase"""
    c0 = counters(hb)
    out = []
    for spec, p in zip(specs, params):
        s = hb.Solver(0)
        load(s, spec)
        info = s.solve(**p)
        out.append(snap(hb, s, info))
        s.close()
    return out, counters(hb) - c0


def many(hb, specs, params):
    sol = [hb.Solver(0) for _ in specs]
    for s, spec in zip(sol, specs):
        load(s, spec)
    c0 = counters(hb)
    infos = hb.solve_many(sol, params)
    dc = counters(hb) - c0
    out = [snap(hb, s, i) for s, i in zip(sol, infos)]
    for s in sol:
        s.close()
    return out, dc


def assert_same(got, ref, tags):
    assert len(got) == len(ref)
    for g, r, t in zip(got, ref, tags):
        for k in r:
            assert g[k] == r[k], "%s: %s differs" % (t, k)


def loose_start(hb, core, monkeypatch, tol):
    """a start point: the general path's iterate at a loose tolerance"""
    monkeypatch.setenv("HIPSDP_SOLVE1", "0")
    s = hb.Solver(0)
    s.load_core(core)
    s.solve(gaptol=tol, feastol=tol, pabstol=tol)
    K = len(core.blocks)
    x, z = s.lp() if core.q else (None, None)
    st = (s.y(), [s.X(k) for k in range(K)], [s.Z(k) for k in range(K)], x, z)
    s.close()
    monkeypatch.delenv("HIPSDP_SOLVE1")
    return st


@pytest.fixture(autouse=True)
def default_path(monkeypatch):
    for v in ("HIPSDP_SOLVE1", "HIPSDP_SOLVE1_NO_FALLBACK", "HIPSDP_SOLVE1_PROF", "HIPSDP_SOLVE1_HIST"):
        monkeypatch.delenv(v, raising=False)


def test_three_hundred_problems_in_one_call(gpu):
    """280 shapes of the fuzz family in the class of blocks of at most 10 rows (one launch of 280 workgroups: more than the 256
    compute units, so some wait in the dispatcher), the first 24 shapes of the other classes, the roots of four examples"""
    specs, tags, seen = [], [], {10: 0}
    seed = 30000
    while len(specs) < 304 - len(ROOTS):
        core, tag = fuzz_shapes.problem(seed)
        c = size_class(core)
        if (c == 10 and seen[10] < 280) or (c != 10 and seed < 30060 and len(specs) - seen[10] < 24):
            seen[c] = seen.get(c, 0) + 1
            specs.append(dict(core=core)); tags.append("seed %d %s" % (seed, tag))
        seed += 1
    for name in ROOTS:
        specs.append(dict(core=instance_core(name))); tags.append(name)
    params = [TOL] * len(specs)
    ref, dref = solo(gpu, specs, params)
    l0, p0 = gpu.solve_many_stats()
    got, dgot = many(gpu, specs, params)
    l1, p1 = gpu.solve_many_stats()
    assert_same(got, ref, tags)
    assert np.array_equal(dgot, dref)
    served = [r for r in ref if r["path"] == 1]
    classes = {size_class(sp["core"]) for sp, r in zip(specs, ref) if r["path"] == 1}
    assert len(served) >= 270 and classes == {10, 16, 64, 1064}
    assert sum(1 for sp, r in zip(specs, ref) if r["path"] == 1 and size_class(sp["core"]) == 10) > 256
    assert l1 - l0 == len(classes) and p1 - p0 == len(served)


def dense_lp_declined():
    """test_gpu_solve1.test_many_dense_lp_rows_beyond_lds_are_declined's shape: 3000 dense LP rows over 60 variables"""
    rng = np.random.default_rng(3)
    m, n, q = 60, 8, 3000
    ystar = rng.standard_normal(m)
    A = np.zeros((m + 1, n, n))
    for i in range(1, m + 1):
        r, c = rng.integers(0, n, 2)
        A[i, r, c] += 1.0
        A[i, c, r] += 1.0 if r != c else 0.0
    Zs = rng.standard_normal((n, n)); Zs = Zs @ Zs.T + 0.5 * np.eye(n)
    A[0] = np.tensordot(ystar, A[1:], axes=(0, 0)) - Zs
    D = rng.standard_normal((q, m))
    c = D @ ystar - rng.random(q) - 0.1
    b = np.array([np.trace(A[i]) for i in range(1, m + 1)]) + D.T @ np.ones(q)
    return ipm_ref.CoreProblem(b, [A], D, c)


def test_mixed_call_every_class_declined_and_never_offered(gpu):
    specs, tags = [], []
    want = {10: 2, 16: 2, 64: 2, 1064: 2}
    seed = 30000
    while any(want.values()):
        core, tag = fuzz_shapes.problem(seed)
        c = size_class(core)
        if want[c] and core.m <= 100:
            want[c] -= 1
            specs.append(dict(core=core)); tags.append("seed %d %s" % (seed, tag))
        seed += 1
    specs.append(dict(core=dense_lp_declined())); tags.append("3000 dense LP rows")
    specs.append(dict(core=instance_core("example_CLS.dat-s.gz"))); tags.append("example_CLS")
    b, A, ys, Xs, Zs = instances.planted_dense(100, 20)
    specs.append(dict(core=ipm_ref.CoreProblem(b, [A]))); tags.append("100-row block")
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(40, 30, 3, seed=11)
    specs.append(dict(sparse=(30, 40, b, coo, A0))); tags.append("sparse block")
    # the examples of one class in the middle of the list, the others around them
    order = [8, 0, 9, 2, 10, 4, 11, 6, 1, 3, 5, 7]
    specs = [specs[i] for i in order]; tags = [tags[i] for i in order]
    params = [TOL] * len(specs)
    ref, dref = solo(gpu, specs, params)
    l0, _ = gpu.solve_many_stats()
    got, dgot = many(gpu, specs, params)
    l1, _ = gpu.solve_many_stats()
    assert_same(got, ref, tags)
    assert np.array_equal(dgot, dref)
    paths = {t: r["path"] for t, r in zip(tags, ref)}
    assert paths["3000 dense LP rows"] == 0 and paths["example_CLS"] == 0 and paths["100-row block"] == 0 and paths["sparse block"] == 0
    served = {size_class(sp["core"]) for sp, r in zip(specs, ref) if "core" in sp and r["path"] == 1}
    assert served == {10, 16, 64, 1064}
    assert l1 - l0 == 4


def test_warm_starts_deferred_setters_and_a_second_call(gpu, monkeypatch):
    """every other solver warm-started, objlimit / preoptgap / settings per solver; the same solvers reloaded and solved by a second
    call; then one plain hipsdp_solve - each step against a solver that goes through the same calls with hipsdp_solve"""
    cores = [fuzz_shapes.problem(s)[0] for s in range(30000, 30016)]
    starts = [loose_start(gpu, c, monkeypatch, 1e-2) for c in cores]
    first = [st if i % 2 == 0 else None for i, st in enumerate(starts)]
    second = [st if i % 2 == 1 else None for i, st in enumerate(starts)]
    params = []
    for i in range(len(cores)):
        p = dict(TOL)
        p["settings"] = i % 3
        if i % 4 == 1:
            p["preoptgap"] = 1e-2
        if i % 5 == 2:
            p["objlimit"] = -1.0
        params.append(p)
    params2 = [dict(params[(i + 1) % len(params)]) for i in range(len(params))]
    ref_sol = [gpu.Solver(0) for _ in cores]
    sol = [gpu.Solver(0) for _ in cores]
    ref = [[], [], []]
    got = [[], [], []]
    # first pass
    for s, c, st in zip(ref_sol + sol, cores + cores, first + first):
        load(s, dict(core=c, start=st))
    for s, p in zip(ref_sol, params):
        ref[0].append(snap(gpu, s, s.solve(**p)))
    got[0] = [snap(gpu, s, i) for s, i in zip(sol, gpu.solve_many(sol, params))]
    # second pass: reloaded, warm starts on the other half
    for s, c, st in zip(ref_sol + sol, cores + cores, second + second):
        load(s, dict(core=c, start=st))
    for s, p in zip(ref_sol, params2):
        ref[1].append(snap(gpu, s, s.solve(**p)))
    got[1] = [snap(gpu, s, i) for s, i in zip(sol, gpu.solve_many(sol, params2))]
    # a plain solve of one of them afterwards
    ref[2].append(snap(gpu, ref_sol[3], ref_sol[3].solve(**params[3])))
    got[2].append(snap(gpu, sol[3], sol[3].solve(**params[3])))
    for s in ref_sol + sol:
        s.close()
    tags = ["problem %d" % i for i in range(len(cores))]
    for k in range(3):
        assert_same(got[k], ref[k], tags)
    assert any(r["warm_started"] for r in ref[0]) and any(r["warm_started"] for r in ref[1])


def test_numerical_fallback_cold_and_warm(gpu, monkeypatch):
    """seed 30123 (the kernel gives up, test_gpu_solve1.py), cold and warm-started, and seed 70387 warm-started, among eligible
    problems: the general path's retry from the same start, the same fallback counters"""
    core, _ = fuzz_shapes.problem(30123)
    core2, _ = fuzz_shapes.problem(70387)
    st = loose_start(gpu, core, monkeypatch, 1e-2)
    st2 = loose_start(gpu, core2, monkeypatch, 1e-4)
    specs = [dict(core=fuzz_shapes.problem(s)[0]) for s in range(30000, 30006)]
    specs[1:1] = [dict(core=core)]
    specs[4:4] = [dict(core=core, start=st)]
    specs.append(dict(core=core2, start=st2))
    params = [TOL] * len(specs)
    ref, dref = solo(gpu, specs, params)
    got, dgot = many(gpu, specs, params)
    assert_same(got, ref, ["problem %d" % i for i in range(len(specs))])
    assert np.array_equal(dgot, dref)
    assert dref[1] >= 1 and dref[2] >= 1
    assert ref[1]["path"] == 0 and ref[1]["status"] == 0


def test_two_host_threads(gpu):
    cores = [[fuzz_shapes.problem(30000 + 64 * t + i)[0] for i in range(64)] for t in range(2)]
    ref = [solo(gpu, [dict(core=c) for c in cs], [TOL] * 64)[0] for cs in cores]
    sol = [[gpu.Solver(0) for _ in range(64)] for _ in range(2)]
    for t in range(2):
        for s, c in zip(sol[t], cores[t]):
            load(s, dict(core=c))
    res = [None, None]
    err = []
    go = threading.Barrier(2)

    def run(t):
        try:
            go.wait()
            res[t] = gpu.solve_many(sol[t], TOL)
        except Exception as e:          # (re-raised below, in the main thread)
            err.append(e)
    th = [threading.Thread(target=run, args=(t,)) for t in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    assert not err, err
    for t in range(2):
        got = [snap(gpu, s, i) for s, i in zip(sol[t], res[t])]
        assert_same(got, ref[t], ["thread %d problem %d" % (t, i) for i in range(64)])
    for s in sol[0] + sol[1]:
        s.close()


def test_argument_errors_change_nothing(gpu):
    lib = gpu.lib()
    core, _ = fuzz_shapes.problem(30000)
    a, b = gpu.Solver(0), gpu.Solver(0)
    a.load_core(core); b.load_core(core)
    info = a.solve(**TOL)
    before = snap(gpu, a, info)
    unshaped = gpu.Solver(0)
    infos = (gpu.Info * 3)()
    rcs = (C.c_int * 3)()
    p = gpu.Params(); lib.hipsdp_default_params(C.byref(p))
    ps = (gpu.Params * 3)(p, p, p)
    l0 = gpu.solve_many_stats()
    for hs in ([a.h, None, b.h], [a.h, b.h, a.h], [a.h, unshaped.h, b.h]):
        arr = (C.c_void_p * 3)(*hs)
        assert lib.hipsdp_solve_many(3, arr, ps, infos, rcs) == HIPSDP_ERR_ARG
    arr = (C.c_void_p * 1)(a.h)
    assert lib.hipsdp_solve_many(-1, arr, ps, infos, rcs) == HIPSDP_ERR_ARG
    assert lib.hipsdp_solve_many(0, arr, ps, infos, rcs) == 0
    assert gpu.solve_many([]) == []
    assert gpu.solve_many_stats() == l0
    assert snap(gpu, a, info) == before
    # b was loaded and never solved: its waiting setters are still there and solve as they would have
    ref = gpu.Solver(0); ref.load_core(core)
    assert snap(gpu, b, b.solve(**TOL)) == snap(gpu, ref, ref.solve(**TOL))
    for s in (a, b, unshaped, ref):
        s.close()


SOLU = {"example_small.dat-s": -8.0, "example_tightenmatrices.dat-s": -9.0, "example_TT.dat-s.gz": 2.11803, "example_inf.dat-s": None}


@pytest.mark.parametrize("name", sorted(SOLU))
def test_bnb_many_reproduces_short_solu(gpu, name):
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", name))
    prob = bnb.instance_to_sdpi(inst)
    stats = {}
    solve_nodes, close = bnb_many.engine_node_solver(gpu, 16, stats=stats)
    best, y, nodes, failed = bnb_many.branch_and_bound_many(prob, inst.intvars, solve_nodes, 16)
    close()
    print("%s: optimum %s, %d nodes, %d calls, %d node solves, %d unresolved" % (name, best, nodes, stats["calls"], stats["nodes"], failed))
    assert failed == 0
    if SOLU[name] is None:
        assert best is None
    else:
        assert best is not None and abs(best - SOLU[name]) <= 1e-4 * max(1.0, abs(SOLU[name]))
        assert all(abs(y[v] - round(y[v])) <= 1e-9 for v in inst.intvars)


def test_bnb_many_width_one_is_the_tree_of_hipsdp_solve(gpu):
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", "example_TT.dat-s.gz"))
    prob = bnb.instance_to_sdpi(inst)
    one, close1 = bnb_many.engine_node_solver(gpu, 1, many=False)
    r1 = bnb.branch_and_bound(prob, inst.intvars, lambda P: one([P])[0])
    close1()
    solve_nodes, close = bnb_many.engine_node_solver(gpu, 1)
    rm = bnb_many.branch_and_bound_many(prob, inst.intvars, solve_nodes, 1)
    close()
    assert rm[2] == r1[2] and rm[3] == r1[3] == 0
    assert rm[0] == r1[0] and abs(rm[0] - SOLU["example_TT.dat-s.gz"]) <= 1e-4
