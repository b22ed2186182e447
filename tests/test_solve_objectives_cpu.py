"""CPU: hipsdp_solve_objectives is declared, exported and bound, and refuses a missing solver without looking at a device; the
bound-tightening harness (tests/harness/obbt.py) with the numpy oracle as solver tightens the roots of two example instances
without losing their known optimum, and its job-order rules (stop at an unsolved job, cutoff at an infeasible one, unbounded jobs
skipped, the improvement threshold) each decide a scripted round the way the reference's loop does."""
import ctypes as C
import importlib.util
import inspect
import os
import re
import numpy as np
import pytest
from conftest import ROOT, GOLDEN
import bnb
import ipm_ref
import obbt
import sdpa_io
import sdpi_prepare


def _hdr(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return f.read()


def test_the_two_calls_are_declared_and_bound():
    hdr = _hdr("hipsdp.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_solve_objectives\s*\(\s*hipsdp_solver\s*\*\s*solver\s*,\s*int\s+count\s*,\s*const\s+double\s*\*\s*B\s*,"
                     r"\s*const\s+hipsdp_params\s*\*\s*params\s*,\s*hipsdp_info\s*\*\s*infos\s*,\s*double\s*\*\s*Y\s*,\s*int\s*\*\s*rcs\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_solve_objectives_stats\s*\(\s*long\s+long\s*\*\s*calls\s*,\s*long\s+long\s*\*\s*launches\s*,"
                     r"\s*long\s+long\s*\*\s*problems\s*\)", hdr)
    assert re.search(r"preoptimal iterate is kept per solver,\s*\*?\s*not per job", hdr)
    units = _hdr("hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_objs_fanout_unit\s*\(\s*int\s+device\s*,\s*int\s+count\s*,", units)
    assert "hipsdp_objs_fanout_unit" not in hdr
    spec = importlib.util.spec_from_file_location("hipsdp_binding_objs", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert list(inspect.signature(mod.Solver.solve_objectives).parameters) == ["self", "B", "kw"]
    assert callable(mod.solve_objectives_stats) and callable(mod.objs_fanout_unit)
    # the solver-interface boundary is what it was: the call is the engine's, not the SCIPsdpiSolver* layer's
    assert "solve_objectives" not in _hdr("sdpisolver_hip.h")


def test_libraries_export_the_calls_and_refuse_a_missing_solver(hb):
    lib = hb.lib()
    assert hasattr(lib, "hipsdp_solve_objectives") and hasattr(lib, "hipsdp_solve_objectives_stats")
    assert hasattr(hb.ulib(), "hipsdp_objs_fanout_unit") and not hasattr(lib, "hipsdp_objs_fanout_unit")
    v = [C.c_longlong(-1) for _ in range(3)]
    assert lib.hipsdp_solve_objectives_stats(*[C.byref(x) for x in v]) == 0
    assert all(x.value >= 0 for x in v)
    assert lib.hipsdp_solve_objectives_stats(None, None, None) == 0
    one = (C.c_double * 1)(1.0)
    infos = (hb.Info * 1)()
    rcs = (C.c_int * 1)(7)
    assert lib.hipsdp_solve_objectives(None, 1, one, None, infos, one, rcs) == 3
    assert lib.hipsdp_solve_objectives(None, 0, None, None, None, None, None) == 3
    assert lib.hipsdp_solve_objectives(None, -1, one, None, infos, one, rcs) == 3
    assert rcs[0] == 7 and one[0] == 1.0
    w = [C.c_longlong(-1) for _ in range(3)]
    assert lib.hipsdp_solve_objectives_stats(*[C.byref(x) for x in w]) == 0
    assert [x.value for x in w] == [x.value for x in v]


SOLU = {"example_small.dat-s": -8.0, "example_tightenmatrices.dat-s": -9.0}


@pytest.mark.parametrize("name", sorted(SOLU))
def test_oracle_round_keeps_the_known_optimum(name):
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", name))
    prob = bnb.instance_to_sdpi(inst)
    best, ystar, nodes, failed = bnb.branch_and_bound(prob, inst.intvars, bnb.oracle_node_solver())
    assert failed == 0 and abs(best - SOLU[name]) <= 1e-4
    P = sdpi_prepare.prepare(prob)
    assert P.status == 'ok'
    node = obbt.node_with_cutoff(P, SOLU[name] + 1.0)
    assert node.core.q == sdpi_prepare.to_core(P)[2].shape[0] + 1
    b, blk, D, c, maps = sdpi_prepare.to_core(P)
    root = ipm_ref.hsd_solve(ipm_ref.CoreProblem(b, blk, D, c), ipm_ref.Params(gaptol=1e-6, feastol=1e-6))
    assert root.status == ipm_ref.STATUS_OPTIMAL
    rnd = obbt.run(node, root.y, obbt.oracle_solver(1e-6), gaptol=1e-6)
    print("%s: %d jobs, result %s, bounds %s" % (name, len(rnd.jobs), rnd.result, rnd.newbounds))
    assert len(rnd.jobs) > 0 and rnd.used == len(rnd.jobs) and rnd.result in ('didnotfind', 'reduceddom')
    assert all(r.status in ('optimal', 'unbounded') for r in rnd.results)
    # the cutoff row lies above the optimum: the optimal point is feasible for every job, so every bounded job's value bounds it
    for (k, sgn), r in zip(rnd.jobs, rnd.results):
        if r.status == 'optimal':
            assert r.obj <= sgn * ystar[node.active[k]] + 1e-5
    lb, ub = obbt.tightened_bounds(P, node, rnd)
    for k, side, val in rnd.newbounds:
        v = node.active[k]
        assert (val <= ystar[v] + 1e-5) if side == 'lb' else (val >= ystar[v] - 1e-5)
        assert (val > P.lb[v]) if side == 'lb' else (val < P.ub[v])
    assert np.all(lb <= ystar + 1e-5) and np.all(ystar <= ub + 1e-5)


def _node(lb, ub):
    m = len(lb)
    A = np.zeros((m + 1, 1, 1))
    return obbt.Node(ipm_ref.CoreProblem(np.zeros(m), [A]), list(range(m)), lb, ub)


def _scripted(script):
    """a solver that returns the scripted results and records the objectives it was given"""
    seen = []

    def solve(core, B):
        seen.append(np.array(B))
        assert len(B) == len(script)
        return [obbt.JobResult(*r) for r in script]
    return solve, seen


def test_jobs_follow_the_relaxation_value():
    node = _node([0.0, 0.0, -obbt.INF], [1.0, 1.0, obbt.INF])
    jobs, B = obbt.objectives(node, np.array([0.0, 0.5, 3.0]))
    assert jobs == [(0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]            # y_0 sits at its lower bound: no min job for it
    assert B.shape == (5, 3) and B[0].tolist() == [-1.0, 0.0, 0.0] and B[3].tolist() == [0.0, 0.0, 1.0]
    jobs, _ = obbt.objectives(node, np.array([5e-7, 1.0 - 5e-7, 0.0]))    # within the feasibility tolerance of a bound
    assert jobs == [(0, -1), (1, 1), (2, 1), (2, -1)]


def test_rule_unsolved_job_stops_the_round():
    node = _node([0.0, 0.0], [1.0, 1.0])
    y = np.array([0.5, 0.5])
    solve, seen = _scripted([('optimal', 0.25), ('failed',), ('optimal', 0.4), ('optimal', -0.6)])
    r = obbt.run(node, y, solve, gaptol=1e-6)
    assert len(seen) == 1 and r.used == 2 and r.result == 'reduceddom' and r.newbounds == [(0, 'lb', 0.25)]
    solve, _ = _scripted([('failed',), ('optimal', -0.5), ('optimal', 0.4), ('optimal', -0.6)])
    r = obbt.run(node, y, solve, gaptol=1e-6)
    assert r.used == 1 and r.result == 'didnotrun' and r.newbounds == []


def test_rule_infeasible_job_cuts_off():
    node = _node([0.0, 0.0], [1.0, 1.0])
    y = np.array([0.5, 0.5])
    # found by a min job: what was collected stays; found by a max job: dropped
    solve, _ = _scripted([('optimal', 0.25), ('optimal', -0.75), ('infeasible',), ('optimal', -0.6)])
    r = obbt.run(node, y, solve, gaptol=1e-6)
    assert r.used == 3 and r.result == 'cutoff' and r.newbounds == [(0, 'lb', 0.25), (0, 'ub', 0.75)]
    solve, _ = _scripted([('optimal', 0.25), ('infeasible',), ('optimal', 0.4), ('optimal', -0.6)])
    r = obbt.run(node, y, solve, gaptol=1e-6)
    assert r.used == 2 and r.result == 'cutoff' and r.newbounds == []


def test_rule_unbounded_jobs_are_skipped_and_small_improvements_refused():
    node = _node([0.0, 0.0], [1.0, 1.0])
    y = np.array([0.5, 0.5])
    thr = obbt.TOLERANCE_FACTOR * 1e-6
    solve, _ = _scripted([('unbounded',), ('optimal', -(1.0 - 0.5 * thr)), ('optimal', 1.5 * thr), ('unbounded',)])
    r = obbt.run(node, y, solve, gaptol=1e-6)
    assert r.used == 4 and r.result == 'reduceddom' and r.newbounds == [(1, 'lb', 1.5 * thr)]
    solve, _ = _scripted([('optimal', 0.5 * thr), ('optimal', -(1.0 - 1.5 * thr)), ('optimal', thr), ('optimal', -(1.0 - thr))])
    r = obbt.run(node, y, solve, gaptol=1e-6)
    assert r.newbounds == [(0, 'ub', 1.0 - 1.5 * thr)] and r.result == 'reduceddom'
    lb, ub = obbt.tightened_bounds(type("P", (), dict(lb=[0.0, 0.0], ub=[1.0, 1.0]))(), node, r)
    assert lb.tolist() == [0.0, 0.0] and ub.tolist() == [1.0 - 1.5 * thr, 1.0]
