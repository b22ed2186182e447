"""rounding.py - TEST INFRASTRUCTURE.  Randomized roundings of a relaxation solution, the candidate points of heur_sdprand.c, and
their feasibility check in ONE hipsdp_check_y_many call.

The reference's heuristic (heur_sdprand.c:300-420) walks over the integer variables of the relaxation's solution and rounds one
variable at a time (:353-359): with r uniform in [0, 1), down when feasfrac(val) <= r, else up - unless the bounds leave one direction
only (:340-348) or none (cutoff) -, then checks the ONE point it made (:395-420).  Here R such points are made from R independent
streams of one seed, and `check_roundings` hands them all to the device at once.  No propagation between two roundings (the reference
propagates in a probing node): this is a parity harness for the check, not a heuristic."""
import math
import numpy as np

FEASTOL = 1e-6      # SCIP's default feasibility tolerance, the one feasFloor / feasCeil / feasFrac use


def feas_floor(v, tol=FEASTOL):
    return math.floor(v + tol)


def feas_ceil(v, tol=FEASTOL):
    return math.ceil(v - tol)


def round_one(val, lb, ub, r, tol=FEASTOL):
    """the new value of one integer variable (heur_sdprand.c:335-359), or None where the reference cuts the probing off; r is only
    looked at when both directions are open"""
    up, down = feas_ceil(val, tol), feas_floor(val, tol)
    if lb > up + 0.5 or ub < down - 0.5:
        return None
    if abs(lb - up) <= tol:
        return float(up)
    if abs(ub - down) <= tol:
        return float(down)
    return float(down) if val - down <= r else float(up)


def roundings(y, isint, lb, ub, count, seed, tol=FEASTOL):
    """count roundings of y (m values): Y[count, m] and keep[count] (False: a variable had no integer left inside its bounds - the
    row is not a candidate).  Variables with isint False keep their value, moved into [lb, ub] where the relaxation's tolerance left it
    outside (the reference solves a final SDP for them, :421-470; here the point is checked as it stands).  Candidate j takes the draws j m .. (j + 1) m - 1 of the
    stream of `seed`, one per variable in index order whether or not the rule looks at it: candidate j does not depend on count."""
    y = np.asarray(y, dtype=np.float64)
    m = len(y)
    cont = np.array([not f for f in isint], dtype=bool)
    y = np.where(cont, np.minimum(np.maximum(y, np.asarray(lb, dtype=np.float64)), np.asarray(ub, dtype=np.float64)), y)
    Y = np.tile(y, (count, 1))
    keep = np.ones(count, dtype=bool)
    draws = np.random.default_rng(seed).random((count, m))
    for j in range(count):
        r = draws[j]
        for i in range(m):
            if not isint[i]:
                continue
            v = round_one(float(y[i]), float(lb[i]), float(ub[i]), float(r[i]), tol)
            if v is None:
                keep[j] = False
                break
            Y[j, i] = v
    return Y, keep


def check_roundings(solver, Y, obj, lmintol=1e-6, lptol=1e-6):
    """ONE hipsdp_check_y_many call over all rows of Y on a loaded solver; returns (order, lmin, lpviol): `order` lists the rows that are
    feasible - every served block's lmin >= -lmintol and lpviol <= lptol - by ascending obj @ Y[j] (ties by index).  A block the call
    does not serve makes every row infeasible here: the caller checks such blocks some other way."""
    Y = np.ascontiguousarray(Y, dtype=np.float64)
    lmin, lpviol, served = solver.check_y_many(Y)
    if np.any(served != 0):
        return [], lmin, lpviol
    ok = np.all(lmin >= -lmintol, axis=1) & (lpviol <= lptol)
    val = Y @ np.asarray(obj, dtype=np.float64)
    order = sorted((j for j in range(len(Y)) if ok[j]), key=lambda j: (val[j], j))
    return order, lmin, lpviol
