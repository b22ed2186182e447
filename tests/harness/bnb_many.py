"""bnb_many.py - TEST INFRASTRUCTURE.  The best-bound-first branch-and-bound of bnb.py with many nodes in flight: up to `width`
open nodes that the incumbent does not prune are popped, prepared (sdpi_prepare.prepare / to_core) and handed to the node
solver as ONE list, and the results are then processed in pop order with the branching, bounding and incumbent rules of
bnb.branch_and_bound.  With width = 1 it visits exactly the nodes bnb.branch_and_bound visits.

Node solvers take a list of prepared nodes and return one bnb.NodeResult per node:
- engine_node_solver: a pool of `width` binding Solvers, one node loaded into each (load_core), all of them solved by one
  hipsdp_solve_many call with the objective limit at the incumbent (or one hipsdp_solve per node, many=False: the reference);
- oracle_node_solver: the numpy oracle (ipm_ref), one node after another - the driver itself on the CPU."""
import heapq
import math
import numpy as np
import bnb
import sdpi_prepare


def branch_and_bound_many(prob, intvars, solve_nodes, width, inttol=1e-5, maxnodes=20000, verbose=False):
    """returns (best objective or None if infeasible, best y, number of nodes, number of failed node solves)"""
    best = [math.inf, None]
    nnodes = 0
    nfailed = 0
    counter = [0]
    heap = []                       # best-bound-first: (parent bound, tie-break, lb, ub, parent aux)

    def push(bound, aux, lb, ub):
        counter[0] += 1
        heapq.heappush(heap, (bound, counter[0], lb, ub, aux))

    def prunes(bound):
        return bound >= best[0] - 1e-6 * max(1.0, abs(best[0]))

    push(-math.inf, None, prob.lb.copy(), prob.ub.copy())
    while heap and nnodes < maxnodes:
        # ---- up to `width` nodes that need a relaxation solved (infeasible and fixed nodes are settled on the way, in pop order)
        batch = []
        while heap and nnodes < maxnodes and len(batch) < width:
            pbound, _, lb, ub, paux = heapq.heappop(heap)
            if prunes(pbound):
                continue                                   # the parent's bound already prunes this node
            nnodes += 1
            node = sdpi_prepare.SdpiProblem(prob.obj, lb, ub, prob.blocks, prob.lp, isintegral=prob.isintegral)
            P = sdpi_prepare.prepare(node)
            if P.status == 'infeasible':
                continue
            if P.status == 'allfixed':
                y = np.array(P.lb, dtype=float)
                if bnb.check_fixed_point(prob, y):
                    val = float(prob.obj @ y)
                    if val < best[0] - 1e-9:
                        best = [val, y]
                continue
            P.parent_aux = paux
            P.cutoff = best[0]        # incumbent value: a node solver may stop as soon as its lower bound exceeds it
            batch.append((P, pbound, paux))
        if not batch:
            continue
        results = solve_nodes([P for (P, _, _) in batch])
        assert len(results) == len(batch)
        # ---- the results in pop order, with bnb.branch_and_bound's rules
        for (P, pbound, paux), res in zip(batch, results):
            bound = res.obj if res.status == 'optimal' else pbound
            aux = res.aux if res.status == 'optimal' else paux
            if res.status in ('infeasible', 'cutoff'):
                continue
            if res.status != 'optimal':
                nfailed += 1
                # cannot bound this node: branch anyway on the first unfixed integer variable
                cand = [v for v in intvars if P.ub[v] - P.lb[v] > 0.5]
                if not cand:
                    continue
                v = cand[0]
                mid = math.floor(0.5 * (max(P.lb[v], -1e6) + min(P.ub[v], 1e6)))
                l1, u1 = np.array(P.lb), np.array(P.ub); u1[v] = mid
                l2, u2 = np.array(P.lb), np.array(P.ub); l2[v] = mid + 1
                push(bound, aux, l1, u1); push(bound, aux, l2, u2)
                continue
            if prunes(res.obj):
                continue                                   # bound
            frac = [(abs(res.y[v] - round(res.y[v])), v) for v in intvars]
            f, v = max(frac) if frac else (0.0, -1)
            if f <= inttol:
                y = res.y.copy()
                for w in intvars:
                    y[w] = round(y[w])
                best = [res.obj, y]
                if verbose:
                    print("  new incumbent %.8g at node %d" % (res.obj, nnodes))
                continue
            fl = math.floor(res.y[v])
            lo_l, lo_u = np.array(P.lb), np.array(P.ub); lo_u[v] = fl
            hi_l, hi_u = np.array(P.lb), np.array(P.ub); hi_l[v] = fl + 1
            # explore the nearer child first (it is pushed last)
            if res.y[v] - fl > 0.5:
                push(bound, aux, lo_l, lo_u); push(bound, aux, hi_l, hi_u)
            else:
                push(bound, aux, hi_l, hi_u); push(bound, aux, lo_l, lo_u)
    return (None if best[1] is None else best[0]), best[1], nnodes, nfailed


def oracle_node_solver(tol=1e-6):
    """bnb.oracle_node_solver for a list of nodes"""
    one = bnb.oracle_node_solver(tol)

    def solve_nodes(Ps):
        return [one(P) for P in Ps]
    return solve_nodes


def _fixed_part(P):
    """objective of the fixed variables at their bounds (the core problem of to_core leaves it out)"""
    y = np.array(P.lb, dtype=float)
    for v in range(P.prob.nvars):
        if P.ub[v] - P.lb[v] > sdpi_prepare.EPS:
            y[v] = 0.0
    return float(P.prob.obj @ y)


def engine_node_solver(hb, width, tol=1e-6, device=0, many=True, stats=None):
    """node solver over libhipsdp.so: a pool of `width` Solvers; each node of a list is loaded into one of them and all of them are
    solved by one hipsdp_solve_many call (many=False: one hipsdp_solve per node, the same parameters).  Objective limit: the
    incumbent, less the objective of the fixed variables.  Returns (solve_nodes, close); stats (dict): calls, nodes, iterations."""
    pool = [hb.Solver(device) for _ in range(width)]

    def solve_nodes(Ps):
        assert len(Ps) <= len(pool)
        import ipm_ref
        maps, params = [], []
        for s, P in zip(pool, Ps):
            b, blk, D, c, mp = sdpi_prepare.to_core(P)
            s.load_core(ipm_ref.CoreProblem(b, blk, D, c))
            fx = _fixed_part(P)
            lim = P.cutoff - fx if math.isfinite(P.cutoff) else 1e20
            params.append(dict(gaptol=tol, feastol=tol, objlimit=lim))
            maps.append(mp)
        sol = pool[:len(Ps)]
        if many:
            infos = hb.solve_many(sol, params)
        else:
            infos = [s.solve(**p) for s, p in zip(sol, params)]
        if stats is not None:
            stats["calls"] = stats.get("calls", 0) + 1
            stats["nodes"] = stats.get("nodes", 0) + len(Ps)
            stats["iters"] = stats.get("iters", 0) + sum(i.iterations for i in infos)
        out = []
        for s, P, info, mp in zip(sol, Ps, infos, maps):
            if info.status in (1, 3):
                out.append(bnb.NodeResult('infeasible'))
            elif info.status == 2:
                out.append(bnb.NodeResult('unbounded'))
            elif info.status == 7:
                out.append(bnb.NodeResult('cutoff'))
            elif info.status != 0:
                out.append(bnb.NodeResult('failed'))
            else:
                y = np.array(P.lb, dtype=float)
                yk = s.y()
                for k, v in enumerate(mp["active"]):
                    y[v] = yk[k]
                out.append(bnb.NodeResult('optimal', float(P.prob.obj @ y), y))
        return out

    def close():
        for s in pool:
            s.close()
    return solve_nodes, close

