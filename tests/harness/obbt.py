"""obbt.py - TEST INFRASTRUCTURE.  One round of optimisation-based bound tightening over a node relaxation, our own restatement of
the loop of the reference's propagator (prop_sdpobbt.c:282-480) WITHOUT SCIP: the objective cutoff row is added to the node, the
objective is zeroed, and for every variable v whose relaxation value is not at its bound the node is solved for min y_v and for
max y_v.  The solves differ in the objective alone and their outcomes are applied only after the loop, so they are independent: the
solver is pluggable and gets ALL objectives at once - hipsdp_solve_objectives in one call, the loop of hipsdp_set_obj + hipsdp_solve,
or the numpy oracle.  The reference's rules are then applied IN JOB ORDER:

   a job that was not solved      the round stops there; what was collected before stays
   an infeasible job              the node is cut off and the round stops; found by a max job, the collected bounds are dropped as well
   an unbounded job               skipped
   a bounded job                  its bound is accepted only if it improves the variable's by more than TOLERANCE_FACTOR * gaptol

The comparisons are SCIP's: isFeasGT / isFeasLT on the relative difference with the feasibility tolerance, isGT / isLT absolute with
epsilon.  This is a parity harness, not a propagator."""
import numpy as np
import ipm_ref
import sdpi_prepare

INF = 1e20
TOLERANCE_FACTOR = 2000.0
EPSILON = 1e-9
FEASTOL = 1e-6


def _reldiff(a, b):
    return (a - b) / max(abs(a), abs(b), 1.0)


def is_feas_gt(a, b, feastol=FEASTOL):
    return _reldiff(a, b) > feastol


def is_feas_lt(a, b, feastol=FEASTOL):
    return _reldiff(a, b) < -feastol


class Node:
    """a prepared node with the cutoff row: the oracle's CoreProblem (objective zero), the variables behind its columns and
    their bounds"""

    def __init__(self, core, active, lb, ub):
        self.core, self.active, self.lb, self.ub = core, list(active), np.asarray(lb, float), np.asarray(ub, float)


def node_with_cutoff(P, cutoff):
    """P: sdpi_prepare.prepare(...) of the node; the row  obj^T y <= cutoff  joins its LP rows (fixed variables moved to the side)"""
    b, blocks, D, c, maps = sdpi_prepare.to_core(P)
    active = maps["active"]
    obj = P.prob.obj
    fixedpart = sum(obj[v] * P.lb[v] for v in range(P.prob.nvars) if v not in set(active))
    row = -np.array([obj[v] for v in active], dtype=float)
    D2 = np.vstack([D.reshape(-1, len(active)), row[None, :]])
    c2 = np.concatenate([np.asarray(c, float).ravel(), [-(cutoff - fixedpart)]])
    core = ipm_ref.CoreProblem(np.zeros(len(active)), blocks, D2, c2)
    return Node(core, active, [P.lb[v] for v in active], [P.ub[v] for v in active])


def objectives(node, relaxy, feastol=FEASTOL):
    """the jobs in the reference's order - per variable min, then max - as (column, sign) with sign +1: min y_v, -1: max y_v, and
    their objectives, one row each"""
    jobs = []
    for k in range(len(node.active)):
        if is_feas_gt(relaxy[k], node.lb[k], feastol):
            jobs.append((k, 1))
        if is_feas_lt(relaxy[k], node.ub[k], feastol):
            jobs.append((k, -1))
    B = np.zeros((len(jobs), len(node.active)))
    for j, (k, sgn) in enumerate(jobs):
        B[j, k] = float(sgn)
    return jobs, B


class JobResult:
    def __init__(self, status, obj=None, y=None):
        self.status = status        # 'optimal' | 'infeasible' | 'unbounded' | 'failed'
        self.obj = obj              # the job's objective value (min y_v: y_v, max y_v: -y_v)
        self.y = y


def _from_status(status, obj, y):
    if status in (ipm_ref.STATUS_DINF, ipm_ref.STATUS_PDINF):
        return JobResult('infeasible')
    if status == ipm_ref.STATUS_DUNB:
        return JobResult('unbounded')
    if status != ipm_ref.STATUS_OPTIMAL:
        return JobResult('failed')
    return JobResult('optimal', obj, y)


def oracle_solver(tol=1e-6):
    def solve(core, B):
        out = []
        for bj in B:
            r = ipm_ref.hsd_solve(ipm_ref.CoreProblem(bj, core.blocks, core.D, core.c), ipm_ref.Params(gaptol=tol, feastol=tol))
            out.append(_from_status(r.status, None if r.status != ipm_ref.STATUS_OPTIMAL else float(r.dobj), r.y))
        return out
    return solve


def engine_call_solver(hb, tol=1e-6, keep=None):
    """all objectives in ONE call of hipsdp_solve_objectives; keep (list): the (Info list, Y) of every call, for bit comparisons"""
    def solve(core, B):
        s = hb.Solver(0)
        s.load_core(core)
        infos, Y = s.solve_objectives(B, gaptol=tol, feastol=tol)
        s.close()
        if keep is not None:
            keep.append((infos, Y))
        return [_from_status(i.status, i.dobj, Y[j]) for j, i in enumerate(infos)]
    return solve


def engine_loop_solver(hb, tol=1e-6, keep=None):
    """the loop the call replaces: hipsdp_set_obj + hipsdp_solve + hipsdp_get_y per objective on one loaded solver"""
    def solve(core, B):
        s = hb.Solver(0)
        s.load_core(core)
        infos, Y = [], np.zeros(B.shape)
        for j, bj in enumerate(B):
            s.set_obj(bj)
            infos.append(s.solve(gaptol=tol, feastol=tol))
            Y[j] = s.y()
        s.close()
        if keep is not None:
            keep.append((infos, Y))
        return [_from_status(i.status, i.dobj, Y[j]) for j, i in enumerate(infos)]
    return solve


class Round:
    def __init__(self):
        self.jobs = []              # (column, sign)
        self.results = []           # JobResult per job (all of them, also those behind the stop)
        self.used = 0               # jobs the rules looked at
        self.newbounds = []         # (column, 'lb' | 'ub', value) in the order they were accepted
        self.result = 'didnotfind'  # 'didnotfind' | 'reduceddom' | 'cutoff' | 'didnotrun'


def apply_rules(node, jobs, results, gaptol):
    """the reference's decisions over the jobs in order"""
    R = Round()
    R.jobs, R.results = list(jobs), list(results)
    for (k, sgn), res in zip(jobs, results):
        R.used += 1
        if res.status == 'failed':
            if R.result != 'reduceddom':
                R.result = 'didnotrun'
            break
        if res.status == 'infeasible':
            R.result = 'cutoff'
            if sgn < 0:
                R.newbounds = []
            break
        if res.status == 'unbounded':
            continue
        if sgn > 0:
            if res.obj - TOLERANCE_FACTOR * gaptol - node.lb[k] > EPSILON:
                R.newbounds.append((k, 'lb', res.obj))
                R.result = 'reduceddom'
        else:
            if -res.obj + TOLERANCE_FACTOR * gaptol - node.ub[k] < -EPSILON:
                R.newbounds.append((k, 'ub', -res.obj))
    if R.newbounds and R.result == 'didnotfind':
        R.result = 'reduceddom'         # (upper bounds alone: the reference reports it when it applies them)
    return R


def run(node, relaxy, solver, gaptol=1e-6, feastol=FEASTOL):
    """one round: Round with the jobs, every job's result and the accepted bounds"""
    jobs, B = objectives(node, relaxy, feastol)
    results = solver(node.core, B) if len(jobs) else []
    return apply_rules(node, jobs, results, gaptol)


def tightened_bounds(P, node, rnd):
    """the node's bounds (all variables of the problem) with the round's bounds applied, as the reference applies them after the loop"""
    lb, ub = np.array(P.lb, dtype=float), np.array(P.ub, dtype=float)
    for k, side, val in rnd.newbounds:
        v = node.active[k]
        if side == 'lb':
            lb[v] = val
        else:
            ub[v] = val
    return lb, ub
