"""The cold-start store (csrc/hs_gram_cache.h, csrc/ipm.hip: GeneralSolve::assemble_forms).

A cold solve starts from X = Z = xi I, where the first Schur matrix is M_ij = <A_i, A_j>: a function of the constraint matrices alone.
The solver keeps it and a later cold solve of the SAME matrices copies it instead of computing it.  Everything here is BITWISE: a hit must
give what the computation would have given (the Gram kernels are deterministic), a miss must give what a fresh handle gives.

Shapes: the smallest that reach the general path and the packed identity form (n > 64, so the packed copy exists), from
tests/test_gpu_cold_start_packed.py.  (n, m) = (65, 120): odd n, m1 = 121 - below one 128-wide tile row and no multiple of it.
(150, 320): m1 = 321 - three tile rows and no multiple of 128, so padding columns of the last tiles and the 32 padding rows of Mx are part
of what is copied.

Decisions of the implementation the tests state: several dense blocks ARE cached (M is accumulated over the blocks in the same order,
the store holds the sum); LP rows ARE cached (the LP term is added after the store is taken or filled, from the same bits); at the sdpi
boundary every SCIPsdpiSolverLoadAndSolve gathers the node's block again, so the first solve of a call is a miss and only the re-solves
inside one call (settings ladder, tolerance loop) hit."""
import ctypes as C
import functools

import numpy as np
import pytest

import instances
import ipm_ref

pytestmark = pytest.mark.gpu

SMALL = (65, 120)
BIG = (150, 320)
SCALARS = ("status", "iterations", "pobj", "dobj", "pinf", "dinf", "dabs", "gap", "mu", "tau", "kappa", "schur_calls", "warm_started")


@functools.lru_cache(maxsize=None)
def planted(n, m, seed=20240):
    """(b, A, ys, Xs, Zs), computed once per shape and shared (nobody writes into them)"""
    out = instances.planted_dense(n, m, seed=seed)
    for a in out:
        a.setflags(write=False)
    return out


def core_of(n, m, seed=20240):
    b, A, ys, Xs, Zs = planted(n, m, seed)
    return ipm_ref.CoreProblem(b, [A])


def snap(s, info):
    """every bit a caller receives from a solve: y, X and Z of every block, the LP part and the info scalars that do not depend on time"""
    out = [s.y().tobytes()]
    for k in range(len(s.ns)):
        out += [s.X(k).tobytes(), s.Z(k).tobytes()]
    if s.q:
        out += [a.tobytes() for a in s.lp()]
    out.append(np.array([float(getattr(info, k)) for k in SCALARS]).tobytes())
    return out


def fresh(gpu, core, load=None, **kw):
    """the solve of a fresh handle: (info, snapshot, stats)"""
    s = gpu.Solver(0)
    try:
        s.load_core(core)
        if load is not None:
            load(s)
        info = s.solve(**kw)
        return info, snap(s, info), s.gram_cache_stats()
    finally:
        s.close()


@pytest.mark.parametrize("n,m", [SMALL, BIG], ids=["65x120", "150x320"])
def test_second_cold_solve_copies_the_first_assembly(gpu, n, m):
    """two cold solves on one handle: equal bits, 1 miss then 1 hit, and the second executed exactly the first assembly's matrix-core
    flops less (that figure: a fresh handle stopped after one iteration has executed the first assembly and nothing else)"""
    core = core_of(n, m)
    s = gpu.Solver(0)
    try:
        s.load_core(core)
        i1 = s.solve(gaptol=1e-6, feastol=1e-6)
        s1 = snap(s, i1)
        assert s.gram_cache_stats() == (0, 1) and s.solve_path() == 0
        i2 = s.solve(gaptol=1e-6, feastol=1e-6)
        s2 = snap(s, i2)
        assert s.gram_cache_stats() == (1, 1)
    finally:
        s.close()
    assert i1.status == 0 and s1 == s2
    first, _, _ = fresh(gpu, core, maxiter=1)
    assert first.schur_calls == 1 and first.schur_flops_executed > 0.0
    print("(n, m) = (%d, %d): first assembly %.6e executed flops; solves %.6e and %.6e" % (n, m, first.schur_flops_executed,
          i1.schur_flops_executed, i2.schur_flops_executed))
    assert i1.schur_flops_executed - i2.schur_flops_executed == first.schur_flops_executed
    # the algorithmic count loses the Gram term m1^2 n^2 of that assembly; the copy is still a call: one assembly per iteration
    assert i1.schur_flops - i2.schur_flops == float(m + 1) ** 2 * n ** 2
    assert i2.schur_calls == i2.iterations == i1.schur_calls


def _entry(var):
    def write(s):
        s.add_entries(0, [var], [7], [3], [0.3125])
    return write


@pytest.mark.parametrize("var", [5, 0], ids=["entry_of_A_5", "entry_of_A_0"])
def test_add_entries_invalidates(gpu, var):
    n, m = SMALL
    core = core_of(n, m)
    s = gpu.Solver(0)
    try:
        s.load_core(core)
        s.solve()
        _entry(var)(s)
        info = s.solve()
        got = snap(s, info)
        assert s.gram_cache_stats() == (0, 2)
        info = s.solve()                        # ... and the new matrices are what is stored now
        assert snap(s, info) == got and s.gram_cache_stats() == (1, 2)
    finally:
        s.close()
    _, want, _ = fresh(gpu, core, load=_entry(var))
    assert got == want


def test_regenerating_reshaping_and_reloading_invalidate(gpu):
    """one handle through: device generator with another seed, set_shape to another size and back, load_core of another problem of
    the same shape - every cold solve after a change is a miss and equals a fresh handle's"""
    n, m = SMALL
    b, A, ys, Xs, Zs = planted(n, m)

    def generated(s, seed):
        s.set_shape(m, [n], 0)
        s.gen_planted(n, m, seed, Xs, Zs, ys)

    def fresh_generated(seed):
        f = gpu.Solver(0)
        try:
            generated(f, seed)
            info = f.solve()
            return snap(f, info)
        finally:
            f.close()

    other = ipm_ref.CoreProblem(*(lambda t: (t[0], [t[1]]))(planted(n, m, 777)))
    s = gpu.Solver(0)
    try:
        generated(s, 11)
        s.solve()
        assert s.gram_cache_stats() == (0, 1)
        s.gen_planted(n, m, 12, Xs, Zs, ys)                     # same shape, same allocations, other matrices
        info = s.solve()
        assert s.gram_cache_stats() == (0, 2) and snap(s, info) == fresh_generated(12)
        s.set_shape(60, [70], 0)                                # another size ...
        s.load_core(core_of(n, m))                              # ... and back
        info = s.solve()
        assert s.gram_cache_stats() == (0, 3) and snap(s, info) == fresh(gpu, core_of(n, m))[1]
        s.load_core(other)                                      # same shape: the allocations are kept, the matrices replaced
        info = s.solve()
        assert s.gram_cache_stats() == (0, 4) and snap(s, info) == fresh(gpu, other)[1]
        info = s.solve()
        assert s.gram_cache_stats() == (1, 4) and snap(s, info) == fresh(gpu, other)[1]
    finally:
        s.close()


def test_warm_start_and_general_first_assembly_bypass(gpu, monkeypatch):
    """a warm-started solve and a solve with HIPSDP_NO_IDENTITY_START=1 on a handle whose store is filled: no hit, no miss, the bits of
    a fresh handle"""
    n, m = SMALL
    core = core_of(n, m)
    monkeypatch.delenv("HIPSDP_NO_IDENTITY_START", raising=False)
    s = gpu.Solver(0)
    try:
        s.load_core(core)
        i0 = s.solve(maxiter=3)                 # a well-centred interior point
        y0, X0, Z0 = s.y(), s.X(0), s.Z(0)
        assert s.gram_cache_stats() == (0, 1)

        def warm(t):
            t.set_start(y0, [X0], [Z0])

        warm(s)
        info = s.solve()
        assert info.warm_started == 1 and s.gram_cache_stats() == (0, 1)
        assert snap(s, info) == fresh(gpu, core, load=warm)[1]
        monkeypatch.setenv("HIPSDP_NO_IDENTITY_START", "1")
        info = s.solve()
        assert s.gram_cache_stats() == (0, 1)
        want_info, want, stats = fresh(gpu, core)
        assert snap(s, info) == want and stats == (0, 0)
        assert info.schur_flops_executed == want_info.schur_flops_executed
    finally:
        monkeypatch.delenv("HIPSDP_NO_IDENTITY_START", raising=False)
        s.close()
    assert i0.iterations == 3


def test_sparse_block_and_one_launch_path_bypass(gpu):
    """a block kept as nonzeros and a problem the one-launch kernel solves: the store is never touched, repeated solves repeat the bits"""
    n, m, k = 96, 120, 3
    b, coo, A0, ys, Xs, Zs = instances.planted_sparse(n, m, k, seed=100 + n + m)
    s = gpu.Solver(0)
    try:
        s.sparse_policy(2)
        s.load_sparse(m, n, b, coo, A0)
        assert s.is_sparse(0)
        i1 = s.solve()
        s1 = snap(s, i1)
        i2 = s.solve()
        assert s.solve_path() == 0 and s.gram_cache_stats() == (0, 0) and snap(s, i2) == s1
    finally:
        s.close()
    b, A, ys, Xs, Zs = planted(24, 40)
    s = gpu.Solver(0)
    try:
        s.load_core(ipm_ref.CoreProblem(b, [A]))
        i1 = s.solve()
        s1 = snap(s, i1)
        i2 = s.solve()
        assert s.solve_path() == 1 and s.gram_cache_stats() == (0, 0) and snap(s, i2) == s1
    finally:
        s.close()


def test_other_objective_tolerances_and_settings_hit(gpu):
    """the store depends on the matrices alone: another b, other tolerances, another rung of the settings ladder are hits and equal the
    same solve on a fresh handle"""
    n, m = SMALL
    b, A, ys, Xs, Zs = planted(n, m)
    core = ipm_ref.CoreProblem(b, [A])
    b2 = b * 1.25 + 0.01
    s = gpu.Solver(0)
    try:
        s.load_core(core)
        s.solve()
        s.set_obj(b2)
        info = s.solve()
        assert s.gram_cache_stats() == (1, 1)
        assert snap(s, info) == fresh(gpu, ipm_ref.CoreProblem(b2, [A]))[1]
        s.set_obj(b)
        info = s.solve(gaptol=1e-3, feastol=1e-4)
        assert s.gram_cache_stats() == (2, 1)
        assert snap(s, info) == fresh(gpu, core, gaptol=1e-3, feastol=1e-4)[1]
        info = s.solve(settings=2)
        assert s.gram_cache_stats() == (3, 1)
        assert snap(s, info) == fresh(gpu, core, settings=2)[1]
    finally:
        s.close()


def test_two_dense_blocks_with_lp_rows_are_cached(gpu):
    """Two dense blocks (65 and 70 rows, the same planted y) and 5 LP rows D y - c >= 0 with slack 1 at the optimum.  DECISION: cached.
    The blocks' Gram matrices are accumulated into Mx in block order exactly as before and the store holds their sum; the LP term
    D~^T diag(x / z) D~ is added afterwards by its own product, so the store is taken before it and never contains it.  Second solve: a
    hit with equal bits; after other LP rows (the matrices untouched) still a hit, equal to a fresh handle."""
    m = 100
    b1, A1, ys, _, _ = planted(65, m)
    b2, A2, ys2, _, _ = planted(70, m)
    assert np.array_equal(ys, ys2)
    rng = np.random.default_rng(5)
    D = rng.standard_normal((5, m))
    core = ipm_ref.CoreProblem(b1 + b2, [A1, A2], D, D @ ys - 1.0)
    D2 = rng.standard_normal((5, m))
    core2 = ipm_ref.CoreProblem(b1 + b2, [A1, A2], D2, D2 @ ys - 1.0)
    s = gpu.Solver(0)
    try:
        s.load_core(core)
        i1 = s.solve()
        s1 = snap(s, i1)
        assert s.solve_path() == 0 and s.gram_cache_stats() == (0, 1)
        i2 = s.solve()
        assert s.gram_cache_stats() == (1, 1) and snap(s, i2) == s1
        s.set_lp(np.concatenate([core2.c.reshape(-1, 1), core2.D], axis=1))
        i3 = s.solve()
        assert s.gram_cache_stats() == (2, 1)
        assert snap(s, i3) == fresh(gpu, core2)[1]
    finally:
        s.close()
    assert i1.status == 0 and abs(i1.dobj - (b1 + b2) @ ys) <= 1e-4 * (1 + abs((b1 + b2) @ ys))


def test_sdpi_boundary_repeated_call(gpu):
    """Two identical SCIPsdpiSolverLoadAndSolve calls on one dense block of 65 rows with 120 variables: the second call gives the
    objective and the bits of y of the first call of a fresh interface handle.  RECORDED: every call shapes the engine and gathers the
    node's block from the master copy again - a writer, so the first solve of each call is a miss; hits come only from re-solves inside
    one call (ladder, tolerance loop), none on this well-conditioned case."""
    n, m = SMALL
    b, A, ys, Xs, Zs = planted(n, m)
    lib = gpu.lib()
    lib.SCIPsdpiSolverGetSolverPointer.restype = C.c_void_p
    il = np.tril_indices(n)
    rows = np.ascontiguousarray(il[0], dtype=np.int32)
    cols = np.ascontiguousarray(il[1], dtype=np.int32)
    nnz_per = len(rows)
    vals = np.ascontiguousarray(A[1:, il[0], il[1]])
    cval = np.ascontiguousarray(A[0, il[0], il[1]])
    PD, PI = C.POINTER(C.c_double), C.POINTER(C.c_int)
    PPD, PPI = C.POINTER(PD), C.POINTER(PI)
    pi = lambda a: a.ctypes.data_as(PI)
    pd = lambda a: a.ctypes.data_as(PD)
    prow = (PI * m)(*[pi(rows)] * m)
    pcol = (PI * m)(*[pi(cols)] * m)
    pval = (PD * m)(*[vals[j].ctypes.data_as(PD) for j in range(m)])
    srow, scol, sval = (PPI * 1)(prow), (PPI * 1)(pcol), (PPD * 1)(pval)
    nvarnonz = np.full(m, nnz_per, dtype=np.int32)
    sdpvar = np.arange(m, dtype=np.int32)
    pnn, pvar = (PI * 1)(pi(nvarnonz)), (PI * 1)(pi(sdpvar))
    obj = np.ascontiguousarray(b, dtype=np.float64)
    lb, ub = np.full(m, -1e20), np.full(m, 1e20)
    sizes, nbv = np.array([n], dtype=np.int32), np.array([m], dtype=np.int32)
    constn = np.array([nnz_per], dtype=np.int32)
    pcr, pcc, pcv = (PI * 1)(pi(rows)), (PI * 1)(pi(cols)), (PD * 1)(pd(cval))
    indch = np.zeros(n, dtype=np.int32)
    pind = (PI * 1)(pi(indch))
    nrem, bic = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    di, dd = np.zeros(1, dtype=np.int32), np.zeros(1)

    def call(h):
        rc = lib.SCIPsdpiSolverLoadAndSolve(
            h, C.c_int(m), pd(obj), pd(lb), pd(ub), C.c_int(1), pi(sizes), pi(nbv),
            C.c_int(nnz_per), pi(constn), pcr, pcc, pcv,
            C.c_int(int(m * nnz_per)), pnn, pvar, srow, scol, sval,
            pind, pi(nrem), pi(bic), C.c_int(0),
            C.c_int(0), pi(di), pd(dd), pd(dd), C.c_int(0), pi(di), pi(di), pd(dd),
            None, None, None, None, None, None, None, None, None,
            C.c_int(-1), C.c_double(1e20), None)
        assert rc == 1 and lib.SCIPsdpiSolverIsOptimal(h)
        o, y = C.c_double(0.0), np.zeros(m)
        assert lib.SCIPsdpiSolverGetDualSol(h, C.byref(o), pd(y)) == 1
        hits, misses = C.c_longlong(0), C.c_longlong(0)
        assert lib.hipsdp_gram_cache_stats(C.c_void_p(lib.SCIPsdpiSolverGetSolverPointer(h)), C.byref(hits), C.byref(misses)) == 0
        return o.value, y.tobytes(), (hits.value, misses.value)

    def handle():
        h = C.c_void_p()
        assert lib.SCIPsdpiSolverCreate(C.byref(h), None, None, None) == 1
        for par, val in ((1, 1e-5), (2, 1e-5), (3, 1e-5)):
            lib.SCIPsdpiSolverSetRealpar(h, par, C.c_double(val))
        return h

    h = handle()
    try:
        o1, y1, st1 = call(h)
        o2, y2, st2 = call(h)
    finally:
        lib.SCIPsdpiSolverFree(C.byref(h))
    g = handle()
    try:
        of, yf, stf = call(g)
    finally:
        lib.SCIPsdpiSolverFree(C.byref(g))
    print("cold-start store at the sdpi boundary (hits, misses): after call 1 %s, after call 2 %s, fresh handle %s" % (st1, st2, stf))
    assert (o2, y2) == (of, yf) and (o1, y1) == (of, yf)
    assert abs(of - b @ ys) <= 1e-4 * (1 + abs(b @ ys))
    # the gather is a writer: the second call's first solve is a miss; whatever hits there are come from re-solves inside a call
    assert st2[1] == 2 * st1[1] and st1[1] >= 1 and stf == st1 and st2[0] == 2 * st1[0]
