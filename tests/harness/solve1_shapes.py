"""Planted node SDPs at the edges of what the one-launch kernel (csrc/solve1_body.h) admits, and the kernel's own decline rules restated
for them.  Every problem is strictly feasible on both sides unless asked otherwise: y* with Z(y*) = sum_i y*_i A_i - A_0 positive
definite and D y* - c > 0, X = I and x = 1 for the primal side (b = A(I) + D^T 1).

Variable matrices come in three kinds, by their entry count (both triangles: what the kernel counts, S1_LIGHT_MAX = 24):
   "light3"  three random positions, at most 6 entries;
   "light24" twelve distinct off-diagonal pairs: exactly 24 entries, the largest light matrix;
   "heavy25" twelve pairs and one diagonal entry: exactly 25 entries, the smallest heavy matrix.
The constant matrices are dense or diagonal.  LP rows are dense-ish ("dens" 0.3) or bound-like (two nonzeros per row)."""
import numpy as np
import ipm_ref

LIGHT_MAX = 24                  # S1_LIGHT_MAX of csrc/solve1_body.h
MAXWORK = 3e6                   # maxwork of solve1_prepare, csrc/ipm.hip
LP_COST_MAX = 2e6               # the LP-part decline of csrc/solve1_body.h (fl[34])


def _pairs(rng, n, k):
    """k distinct off-diagonal positions (r > c) of an n x n matrix"""
    allp = [(r, c) for r in range(n) for c in range(r)]
    idx = rng.choice(len(allp), size=k, replace=False)
    return [allp[i] for i in idx]


def _var_matrix(rng, n, kind):
    A = np.zeros((n, n))
    if kind == "light3":
        for _ in range(3):
            r, c = rng.integers(0, n, 2)
            v = rng.standard_normal()
            A[r, c] += v
            if r != c:
                A[c, r] += v
        return A
    need = 12
    if n * (n - 1) // 2 < need:
        raise ValueError("a %s matrix needs at least 6 rows" % kind)
    for r, c in _pairs(rng, n, need):
        v = rng.standard_normal()
        v = v if abs(v) > 0.1 else 0.5            # (no entry that rounds away)
        A[r, c] = A[c, r] = v
    if kind == "heavy25":
        i = int(rng.integers(0, n))
        A[i, i] = 1.0 + rng.random()
    return A


def planted(sizes, m, q, seed, kinds="light3", heavy=0, const="dense", lp="dens", infeasible=None):
    """sizes: rows of each block; kinds: the kind of every variable matrix; the first `heavy` variables of every block are "heavy25"
    instead.  lp: "dens" (density 0.3) or "bounds" (two nonzeros per row).  infeasible: None, "dinf" (two LP rows that contradict
    each other: no y at all, an X-ray proves it) or "dunb" (b_1 = -1 where A_1 = e_j e_j^T in the first block and nothing else:
    no X at all, y = e_1 proves it)"""
    rng = np.random.default_rng(seed)
    ystar = rng.standard_normal(m)
    blocks = []
    for bi, n in enumerate(sizes):
        A = np.zeros((m + 1, n, n))
        for i in range(1, m + 1):
            if infeasible == "dunb" and i == 1:
                if bi == 0:
                    A[1, 0, 0] = 1.0
                continue
            A[i] = _var_matrix(rng, n, "heavy25" if i <= heavy else kinds)
        Ay = np.tensordot(ystar, A[1:], axes=(0, 0))
        if const == "dense":
            Zs = rng.standard_normal((n, n))
            Zs = Zs @ Zs.T + 0.5 * np.eye(n)
            A[0] = Ay - Zs
        else:
            off = Ay - np.diag(np.diag(Ay))
            A[0] = np.diag(np.diag(Ay)) - (np.linalg.norm(off, 2) + 0.5 + rng.random(n)) * np.eye(n)
        blocks.append(A)
    if lp == "dens":
        D = rng.standard_normal((q, m)) * (rng.random((q, m)) < 0.3)
    else:
        D = np.zeros((q, m))
        for r in range(q):
            cols = rng.choice(m, size=min(2, m), replace=False)
            D[r, cols] = rng.standard_normal(len(cols))
    if infeasible == "dunb" and q:
        D[:, 0] = 0.0
    c = D @ ystar - rng.random(q) - 0.1
    if infeasible == "dinf":
        if q < 2:
            raise ValueError("an LP contradiction needs two rows")
        D[1] = -D[0]
        c[1] = -c[0] + 1.0                           # d y >= c0 and -d y >= 1 - c0: 0 >= 1
        if not D[0].any():
            D[0, 0], D[1, 0] = 1.0, -1.0
    b = sum(np.array([np.trace(A[i]) for i in range(1, m + 1)]) for A in blocks) + (D.T @ np.ones(q) if q else 0.0)
    if infeasible == "dunb":
        b[0] = -1.0
    return ipm_ref.CoreProblem(b, blocks, D, c)


def entry_counts(core):
    """per block: entries (both triangles) of A_0 .. A_m - what the kernel's voff counts"""
    return [np.count_nonzero(A.reshape(A.shape[0], -1), axis=1) for A in core.blocks]


def schur_work(core):
    """the kernel's estimate of the multiply-adds of one Schur assembly (csrc/solve1_body.h, second allocation step: work += ...),
    restated per block: with nz the entries of all matrices A_0 .. A_m, nh the heavy ones (more than LIGHT_MAX entries) and nzh their
    entries,  nzh n + nh n^3 + nz nh + 0.75 (nz - nzh)^2.  The kernel declines above maxwork (3e6)."""
    work = 0.0
    for A, cnt in zip(core.blocks, entry_counts(core)):
        n = A.shape[1]
        heavy = cnt > LIGHT_MAX
        nz, nh, nzh = int(cnt.sum()), int(heavy.sum()), int(cnt[heavy].sum())
        work += nzh * n + nh * n * (n * n) + nz * nh + 0.5 * (nz - nzh) * (nz - nzh) * 1.5
    return work


def lp_cost_bounds(core):
    """(lower, upper) of the kernel's cheaper form of the LP part of the Schur matrix (csrc/solve1_body.h, after the lists: the product
    at 800 cycles per tile step from LDS or 2400 from global memory, against the walk of the nonzeros at 500 per entry of the busiest
    variable); above LP_COST_MAX the kernel declines"""
    q, m = core.q, core.m
    if q == 0:
        return 3000.0, 3000.0
    D = core.D != 0
    rown = D.sum(axis=1) + (core.c != 0)             # (the kernel's rows hold c as well)
    worst = int(max((rown[D[:, i]].sum() for i in range(m)), default=0))
    nt1 = (m + 1 + 15) >> 4
    K = len(core.blocks)
    nwv = 8 - (2 * K if 2 * K < 7 else 7)
    steps = ((nt1 * nt1 + nwv - 1) // nwv) * ((q + 7) >> 3)
    row = 500.0 * worst + 3000.0
    return min(steps * 800.0, row), min(steps * 2400.0, row)
