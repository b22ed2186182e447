"""onevar_large_cases.py - TEST INFRASTRUCTURE shared by test_onevar_large_cpu.py, test_gpu_onevar_large.py and
tests/devtools/onevar_large_rate.py: the family of hipsdp_onevar_bounds_large - blocks of 129 .. 512 rows.  The restatement of a job,
the generator, the flavours, the seeds and the rule of decidable jobs are those of tests/onevar_cases.py (imported, not changed)."""
import onevar_cases as K

# (n, m, rank): the first size the call serves and the one behind it, a size between, one past a multiple of 256 (the column kernel
# reads 64 entries per lane and step; a form launch gives every workgroup a range of rows), and the two largest
SIZES = [(129, 6, 10), (130, 6, 10), (192, 6, 12), (257, 6, 12), (511, 4, 16), (512, 4, 16)]
SPARSE_SIZES = [(129, 6, 10), (257, 6, 12), (512, 4, 16)]
# what the restatement gives on the family, per size: (INNER, INFEASIBLE, LB) and the undecidable jobs (K.decidable)
STATUS_MIX = {129: (38, 58, 12), 130: (38, 58, 12), 192: (38, 58, 12), 257: (38, 58, 12), 511: (26, 38, 8), 512: (26, 38, 8)}
UNDECIDABLE = {129: 0, 130: 0, 192: 1, 257: 0, 511: 1, 512: 4}
JOBS = 576

_cache = {}


def instance(size, flavour, seed):
    """(A, lb, ub, refs) of a family member, u = ub; refs[i] = K.onevar_ref of variable i (NEWTON).  Computed once, never changed.
    (A cache of its own: K.instance keeps every member alive, and a member here is up to 10 MB.)"""
    key = (size, flavour, seed)
    if key not in _cache:
        n, m, rank = size
        A, lb, ub = K.family(n, m, rank, seed, *flavour)
        Z = K.z_of(A, ub)
        refs = [K.onevar_ref(Z, A[i + 1], ub[i], K.NEWTON, lb[i], ub[i], K.FEASTOL) for i in range(m)]
        for a in (A, lb, ub):
            a.setflags(write=False)
        _cache[key] = (A, lb, ub, refs)
    return _cache[key]


def instances(size):
    return [(fl, sd) + instance(size, fl, sd) for fl in K.FLAVOURS for sd in K.SEEDS]


def launches(nmax, rounds, z):
    """the documented launches of a call of one chunk: z (0 or 1: Z(u) formed) + R (nmax + 5)"""
    return z + rounds * (nmax + 5)
