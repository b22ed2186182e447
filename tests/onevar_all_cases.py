"""onevar_all_cases.py - TEST INFRASTRUCTURE shared by test_onevar_all_cpu.py, test_gpu_onevar_all.py and
tests/devtools/onevar_all_rate.py: what hipsdp_onevar_bounds_all adds to tests/onevar_cases.py (which stays as it is) - the kind
EXTREMES with its status DONE, the family of blocks that share their variables, and the numpy restatement of EXTREMES.  The
restatement of a NEWTON / TWOPOINT job, the flavours, the seeds and the rule of decidable jobs are those of onevar_cases."""
import numpy as np
from onevar_cases import FEASTOL, FLAVOURS, NEWTON, SEEDS, family, onevar_ref, z_of

# ---- hipsdp_onevar_bounds_all: the jobs of ALL blocks in one call ---------------------------------------------------------------------
EXTREMES = 2            # kind: lambda_min and lambda_max of A_i alone
DONE = 6                # status of an EXTREMES job
# (n, rank) of the blocks of the multi-block family: both class edges (64 | 65, 128) and the odd small sizes, sharing MULTI_M variables
MULTI_BLOCKS = [(3, 1), (17, 3), (64, 6), (65, 6), (128, 12)]
MULTI_M = 6


def multi_family(seed, t, pert, indef, lbfrac=None, blocks=MULTI_BLOCKS, m=MULTI_M):
    """blocks that share m variables: ub and lb are drawn ONCE (default_rng([m, seed, 77]), in the order and ranges of family());
    block b's A_1 .. A_m are those of family(n, m, rank, seed, 0, 0, indef), and A_0^b = t sum ub_k A_k^b + pert sym(E) with E from
    default_rng([n, m, seed, 5]).  Returns ([A_b [m + 1, n, n]], lb [m], ub [m])."""
    rng = np.random.default_rng([m, seed, 77])
    ub = rng.uniform(0.5, 2.0, m)
    lb = np.where(rng.uniform(0.0, 1.0, m) < 0.5, -rng.uniform(0.0, 0.5, m), 0.0)
    if lbfrac is not None:
        lb = lbfrac * ub
    out = []
    for n, rank in blocks:
        A = np.array(family(n, m, rank, seed, 0.0, 0.0, indef)[0])
        E = np.random.default_rng([n, m, seed, 5]).standard_normal((n, n))
        A[0] = t * np.tensordot(ub, A[1:], axes=1) + pert * 0.5 * (E + E.T)
        out.append(0.5 * (A + np.transpose(A, (0, 2, 1))))
    return out, lb, ub


_multi_cache = {}


def multi_instance(flavour, seed):
    """(blocks, lb, ub, refs) of a member of the multi-block family, u = ub; refs[b][i] = onevar_ref of variable i in block b
    (NEWTON).  Computed once, never changed."""
    key = (flavour, seed)
    if key not in _multi_cache:
        blocks, lb, ub = multi_family(seed, *flavour)
        refs = [[onevar_ref(z_of(A, ub), A[i + 1], ub[i], NEWTON, lb[i], ub[i], FEASTOL) for i in range(len(ub))] for A in blocks]
        for a in blocks + [lb, ub]:
            a.setflags(write=False)
        _multi_cache[key] = (blocks, lb, ub, refs)
    return _multi_cache[key]


def multi_instances():
    return [(fl, sd) + multi_instance(fl, sd) for fl in FLAVOURS for sd in SEEDS]


def extremes_ref(Ai):
    """(lambda_min, lambda_max) of A_i by numpy"""
    w = np.linalg.eigvalsh(Ai)
    return float(w[0]), float(w[-1])
