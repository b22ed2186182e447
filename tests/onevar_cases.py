"""onevar_cases.py - TEST INFRASTRUCTURE shared by test_onevar_cpu.py, test_gpu_onevar.py and tests/devtools/onevar_rate.py: the
numpy restatement of what hipsdp_onevar_bounds computes per job, the instance family of its tests, and the rule that says which
jobs the device must reproduce decision for decision.

A job works on  M(mu) = Z + (mu - u_i) A_i,  f(mu) = lambda_min(M(mu)),  g(mu) = v^T A_i v  at the unit eigenvector v of f(mu).
NEWTON is SCIPsolveOneVarSDPDense with obj = 1 (solveonevarsdp.c:434-525), TWOPOINT the binary-variable branch of tightenBounds
(cons_sdp.c:2102-2153)."""
import numpy as np

NEWTON, TWOPOINT = 0, 1
LB, INNER, INFEASIBLE, UBONLY, DECLINED, GAVEUP = 0, 1, 2, 3, 4, 5
STATUS_NAMES = {LB: "LB", INNER: "INNER", INFEASIBLE: "INFEASIBLE", UBONLY: "UBONLY", DECLINED: "DECLINED", GAVEUP: "GAVEUP", -1: "not served"}
FEASTOL = 1e-6
INF = 1e20

# (n, m, rank): the class edges of the two eigenpair bodies (64 | 65, 128) and the smallest blocks
SIZES = [(2, 3, 1), (3, 4, 1), (16, 12, 2), (17, 12, 3), (63, 10, 5), (64, 10, 6), (65, 8, 6), (127, 6, 10), (128, 6, 12)]
# (t, pert, indef, lbfrac): A_0 = t sum ub_k A_k + pert sym(E); indef: the last variable gets - C C^T; lbfrac: lb_i = lbfrac ub_i.
# The last flavour is the one that brings the status LB to the blocks of 63 rows and more (there M(lb) of the drawn lb_i <= 0 is
# never psd): lb_i = 0.98 ub_i at t = 0.3 leaves M_i(lb) = 0.7 sum ub_k A_k - 0.02 ub_i A_i positive definite.
FLAVOURS = [(0.3, 0.0, 0, None), (0.6, 0.0, 0, None), (0.9, 0.0, 0, None), (0.6, 0.02, 0, None), (0.9, 0.02, 0, None),
            (1.2, 0.0, 0, None), (0.6, 0.0, 1, None), (0.0, 1.0, 0, None), (0.3, 0.0, 0, 0.98)]
SEEDS = (1, 2)
# a job is DECIDABLE when every evaluation of the restatement is this far from a branch: the device's eigenvalue error (1e-12 of
# the matrix's scale, the bound of its eigenpair tests) can then neither flip a comparison nor make the supergradient ambiguous
DEC_D, DEC_G, DEC_GAP = 0.02, 1e-6, 1e-6
UNDECIDABLE_CAP = 0.05


def eval_point(Z, Ai, ui, mu):
    """f, g and the spectrum of M(mu) = Z + (mu - u_i) A_i"""
    w, V = np.linalg.eigh(Z + (mu - ui) * Ai)
    v = V[:, 0]
    return float(w[0]), float(v @ Ai @ v), w


def onevar_ref(Z, Ai, ui, kind, lb, ub, feastol, maxevals=100, infinity=INF):
    """the algorithm of a job with numpy.linalg.eigh: (status, optval, f, g, evals, log); f, g: the last eigenvalue and supergradient
    (g = 0 for LB, as the reference sets it, and for TWOPOINT); log: per evaluation (mu, f, g, d, gn, gap) with
    d = |f + feastol| / feastol,  gn = |g| / ||A_i||_2,  gap = (lambda_2 - lambda_1) / max |lambda|  (inf for one row)."""
    log = []
    if lb <= -infinity or ub >= infinity:
        return DECLINED, 0.0, 0.0, 0.0, 0, log
    anorm = float(np.linalg.norm(Ai, 2)) if Ai.size else 0.0

    def f(mu):
        ev, g, w = eval_point(Z, Ai, ui, mu)
        scale = float(np.max(np.abs(w)))
        gap = float((w[1] - w[0]) / scale) if len(w) > 1 and scale > 0.0 else np.inf
        log.append((mu, ev, g, abs(ev + feastol) / feastol if feastol > 0.0 else np.inf, abs(g) / anorm if anorm > 0.0 else 0.0, gap))
        return ev, g

    if kind == TWOPOINT:
        ev, g = f(lb)
        if ev >= -feastol:
            return LB, lb, ev, 0.0, 1, log
        if maxevals < 2:
            return GAVEUP, lb, ev, 0.0, 1, log
        ev, g = f(ub)
        return (INFEASIBLE if ev < -feastol else UBONLY), ub, ev, 0.0, 2, log
    ev, g = f(ub)
    if ev < -feastol and g > 0.0:
        return INFEASIBLE, ub, ev, g, 1, log
    if maxevals < 2:
        return GAVEUP, ub, ev, g, 1, log
    ev, g = f(lb)
    if ev >= -feastol:
        return LB, lb, ev, 0.0, 2, log
    if g <= 0.0:
        return INFEASIBLE, lb, ev, g, 2, log
    mu = lb
    while ev < -feastol and g > 0.0:
        nxt = mu - (feastol / 2.0 + ev) / g
        if nxt > ub:
            return INFEASIBLE, nxt, ev, g, len(log), log
        if len(log) >= maxevals:
            return GAVEUP, mu, ev, g, len(log), log
        mu = nxt
        ev, g = f(mu)
    return (INFEASIBLE if ev < -feastol else INNER), mu, ev, g, len(log), log


def decidable(kind, log):
    """far from every branch (a TWOPOINT job uses no eigenvector: only its eigenvalues have to be)"""
    if kind == TWOPOINT:
        return all(e[3] >= DEC_D for e in log)
    return all(e[3] >= DEC_D and e[4] >= DEC_G and e[5] >= DEC_GAP for e in log)


def inner_bound(Z, Ai, ui, a, b, feastol):
    """|a - b| of two INNER answers of the same job: both f values lie in [-feastol - tau, -feastol / 4] (tau: the eigenvalue error,
    far below feastol / 20), and f is concave with supergradient g: f(hi) - f(lo) >= g(hi) (hi - lo) for lo < hi, so
    hi - lo <= (3/4 feastol + tau) / g(hi) <= 0.8 feastol / g(hi).  g(hi): numpy's, at the larger of the two points."""
    hi = max(a, b)
    g = eval_point(Z, Ai, ui, hi)[1]
    return 0.8 * feastol / g if g > 0.0 else np.inf, g


def family(n, m, rank, seed, t, pert, indef, lbfrac=None):
    """one block: A [m + 1, n, n] (A[0] the constant matrix), lb [m], ub [m]"""
    rng = np.random.default_rng([n, m, seed])
    A = np.zeros((m + 1, n, n))
    for i in range(1, m + 1):
        B = rng.standard_normal((n, rank))
        A[i] = B @ B.T + np.diag(rng.uniform(0.02, 0.1, n))
    if indef:
        Cm = rng.standard_normal((n, rank))
        A[m] -= Cm @ Cm.T
    ub = rng.uniform(0.5, 2.0, m)
    lb = np.where(rng.uniform(0.0, 1.0, m) < 0.5, -rng.uniform(0.0, 0.5, m), 0.0)
    E = rng.standard_normal((n, n))
    A[0] = t * np.tensordot(ub, A[1:], axes=1) + pert * 0.5 * (E + E.T)
    if lbfrac is not None:
        lb = lbfrac * ub
    A = 0.5 * (A + np.transpose(A, (0, 2, 1)))
    return A, lb, ub


def z_of(A, u):
    """Z(u) = sum_k u_k A_k - A_0"""
    return np.tensordot(np.asarray(u, dtype=np.float64), A[1:], axes=1) - A[0]


_cache = {}


def instance(size, flavour, seed):
    """(A, lb, ub, refs) of a family member, u = ub; refs[i] = onevar_ref of variable i (NEWTON).  Computed once, never changed."""
    key = (size, flavour, seed)
    if key not in _cache:
        n, m, rank = size
        A, lb, ub = family(n, m, rank, seed, *flavour)
        Z = z_of(A, ub)
        refs = [onevar_ref(Z, A[i + 1], ub[i], NEWTON, lb[i], ub[i], FEASTOL) for i in range(m)]
        for a in (A, lb, ub):
            a.setflags(write=False)
        _cache[key] = (A, lb, ub, refs)
    return _cache[key]


def instances(size):
    return [(fl, sd) + instance(size, fl, sd) for fl in FLAVOURS for sd in SEEDS]


def size_class(n):
    return 0 if n <= 64 else 1
