"""GPU: hipsdp_onevar_bounds - all one-variable SDPs of a block in one call - against the numpy restatement of
tests/onevar_cases.py (itself set against the oracle and the reference's known answers in tests/test_onevar_cpu.py).

On decidable jobs (far from every branch, onevar_cases.decidable) status and evaluation count equal the restatement's; LB and
INFEASIBLE jobs return the restatement's point (lb and ub are copied, a mu is held to the bound below); for INNER jobs
    |optval - ref| <= 0.8 feastol / g(b),      g(b): numpy's supergradient at the larger of the two points,
which follows from concavity, f(b) - f(a) >= g(b) (b - a), with both f values in [-feastol - tau, -feastol / 4] - derived, not
measured.  Every job, decidable or not, has to have the properties of its status, checked with numpy on M(optval).

Measured on an MI355X, worst |optval - ref| g / feastol per block size (bound 0.8): at most 3.5e-8; the figures per size stand in the
docstring of test_family_matches_the_restatement and in DESIGN.md 6.8."""
import ctypes as C
import json
import os
import numpy as np
import pytest
from conftest import GOLDEN
import ipm_ref
import sdpi_driver
import onevar_cases as K
from test_gpu_sparsecuts_all import load_dense, load_sparse

pytestmark = pytest.mark.gpu

# both loaders at the class edges and the smallest odd sizes: load_dense keeps blocks of up to 64 rows as dense rows and sweeps larger
# ones as packed lower triangles, load_sparse keeps every block as nonzeros - the three storage forms of a block
BOTH_FORMS = (3, 17, 64, 65, 128)


def _loaders(n):
    return ("dense", "sparse") if n in BOTH_FORMS else ("dense",)


def _solver(gpu, A, how):
    b = np.ones(A.shape[0] - 1)
    s = (load_dense if how == "dense" else load_sparse)(gpu, [A], b)
    if how == "sparse":
        assert s.is_sparse(0)
    return s


def _mat(A, u, i, mu):
    return K.z_of(A, u) + (mu - u[i]) * A[i + 1]


def _check_properties(A, u, i, kind, lb, ub, st, ov, feastol):
    """what the status promises, with numpy on M(optval)"""
    assert st in (K.LB, K.INNER, K.INFEASIBLE, K.UBONLY), st
    w = np.linalg.eigvalsh(_mat(A, u, i, ov))
    scale = float(np.max(np.abs(w)))
    if st in (K.LB, K.INNER, K.UBONLY):
        assert w[0] >= -feastol - 1e-12 * scale, (st, w[0])
    if st == K.INNER:
        assert w[0] <= -feastol / 4.0, w[0]
    if st == K.INFEASIBLE:
        assert w[0] < -feastol + 1e-12 * scale, w[0]
    assert lb <= ov
    if st != K.INFEASIBLE:
        assert ov <= ub


def _check_against_ref(A, u, i, ref, st, ov, ne, feastol, lb, ub, tag):
    """a decidable job: the restatement's decisions; returns |optval - ref| g / feastol of an INNER job, else 0"""
    assert (st, ne) == (ref[0], ref[4]), (tag, K.STATUS_NAMES.get(st), K.STATUS_NAMES[ref[0]], ne, ref[4])
    if ref[1] == lb or ref[1] == ub:
        assert ov == ref[1], tag                         # a bound is copied
        return 0.0
    bound, g = K.inner_bound(K.z_of(A, u), A[i + 1], u[i], ov, ref[1], feastol)
    assert abs(ov - ref[1]) <= bound, (tag, ov, ref[1], bound)
    return abs(ov - ref[1]) * g / feastol if st == K.INNER else 0.0


def test_known_answers_of_the_reference_unit_test(gpu):
    with open(os.path.join(GOLDEN, "onevar_cases.json")) as f:
        G = json.load(f)
    for c in G["cases"]:
        n = c["n"]
        A = np.stack([sdpi_driver._dense(n, c["const"]), sdpi_driver._dense(n, c["var"])])
        s = _solver(gpu, A, "dense")
        st, ov, lmin, grad, ne = s.onevar_bounds(0, [0.0], [c["lb"]], [c["ub"]], G["eps"], infinity=G["infinity"])
        s.close()
        ref = K.onevar_ref(-A[0], A[1], 0.0, K.NEWTON, c["lb"], c["ub"], G["eps"])
        print(c["name"], K.STATUS_NAMES[int(st[0])], ov[0], ne[0], "restatement", K.STATUS_NAMES[ref[0]], ref[1], ref[4])
        if c["infeasible"]:
            assert st[0] == K.INFEASIBLE, c["name"]
        else:
            assert st[0] in (K.LB, K.INNER) and abs(ov[0] - c["optval"]) <= G["eps"], (c["name"], ov[0])
        if K.decidable(K.NEWTON, ref[5]):
            assert (st[0], ne[0]) == (ref[0], ref[4]), c["name"]
        _check_properties(A, np.zeros(1), 0, K.NEWTON, c["lb"], c["ub"], int(st[0]), float(ov[0]), G["eps"])


@pytest.mark.parametrize("size", K.SIZES, ids=lambda s: "n%d" % s[0])
def test_family_matches_the_restatement(gpu, size):
    """every instance of the family, u = ub, all variables in one call.  Worst |optval - ref| g / feastol of the INNER jobs is printed
    per size and storage form before it is checked against 0.8.  Measured on an MI355X (the same for both loaders of a size):
    n = 2: 2.1e-9, 3: 8.4e-10, 16: 1.5e-8, 17: 2.3e-8, 63: 3.5e-8, 64: 3.2e-8, 65: 2.6e-8, 127: 2.9e-8, 128: 2.8e-8; undecidable
    jobs 1, 1, 0, 0, 1, 0, 1, 0, 0 of 54, 72, 216, 216, 180, 180, 144, 108, 108."""
    n, m, rank = size
    for how in _loaders(n):
        worst, jobs, und = 0.0, 0, 0
        for fl, sd, A, lb, ub, refs in K.instances(size):
            s = _solver(gpu, A, how)
            st, ov, lmin, grad, ne = s.onevar_bounds(0, ub, lb, ub, K.FEASTOL)
            s.close()
            for i, r in enumerate(refs):
                jobs += 1
                tag = (how, fl, sd, i)
                _check_properties(A, ub, i, K.NEWTON, lb[i], ub[i], int(st[i]), float(ov[i]), K.FEASTOL)
                if st[i] == K.LB:
                    assert grad[i] == 0.0, tag
                if not K.decidable(K.NEWTON, r[5]):
                    und += 1
                    continue
                worst = max(worst, _check_against_ref(A, ub, i, r, int(st[i]), float(ov[i]), int(ne[i]), K.FEASTOL, lb[i], ub[i], tag))
        print("n = %3d %-6s: %4d jobs, %d undecidable, worst |optval - ref| g / feastol = %.3g (bound 0.8)" % (n, how, jobs, und, worst))
        assert worst <= 0.8


@pytest.mark.parametrize("size", [(3, 4, 1), (17, 12, 3), (65, 8, 6)], ids=lambda s: "n%d" % s[0])
def test_twopoint_mixed_with_newton(gpu, size):
    """binary variables: lb = 0, ub = 1, the kinds alternating inside one call"""
    n, m, rank = size
    seen = set()
    for fl in K.FLAVOURS[:8]:
        A, lb0, ub0, _ = K.instance(size, fl, 1)
        u = np.asarray(ub0)
        lb, ub = np.zeros(m), np.ones(m)
        kind = np.array([K.TWOPOINT if i % 2 == 0 else K.NEWTON for i in range(m)], dtype=np.int32)
        s = _solver(gpu, A, "dense")
        st, ov, lmin, grad, ne = s.onevar_bounds(0, u, lb, ub, K.FEASTOL, kind=kind)
        s.close()
        Z = K.z_of(A, u)
        for i in range(m):
            r = K.onevar_ref(Z, A[i + 1], u[i], int(kind[i]), 0.0, 1.0, K.FEASTOL)
            _check_properties(A, u, i, int(kind[i]), 0.0, 1.0, int(st[i]), float(ov[i]), K.FEASTOL)
            if kind[i] == K.TWOPOINT:
                assert ne[i] <= 2 and grad[i] == 0.0, (fl, i)
                assert st[i] in (K.LB, K.INFEASIBLE, K.UBONLY)
            if K.decidable(int(kind[i]), r[5]):
                _check_against_ref(A, u, i, r, int(st[i]), float(ov[i]), int(ne[i]), K.FEASTOL, 0.0, 1.0, (fl, i))
                if kind[i] == K.TWOPOINT:
                    seen.add(int(st[i]))
    print("n = %d: TWOPOINT outcomes seen" % n, sorted(K.STATUS_NAMES[x] for x in seen))


def test_twopoint_three_outcomes_by_hand(gpu):
    """A_1 = diag(1, 1), A_0 = diag(0.5, 0.5): M(mu) = (mu - 0.5) I whatever u is"""
    A = np.stack([0.5 * np.eye(2), np.eye(2)])
    s = _solver(gpu, A, "dense")
    kind = [K.TWOPOINT] * 3
    st, ov, lmin, grad, ne = s.onevar_bounds(0, [0.3], [0.6, 0.0, 0.0], [1.0, 1.0, 0.25], 1e-6, vars=[0, 0, 0], kind=kind)
    s.close()
    assert list(st) == [K.LB, K.UBONLY, K.INFEASIBLE]
    assert list(ov) == [0.6, 1.0, 0.25] and list(ne) == [1, 2, 2] and list(grad) == [0.0, 0.0, 0.0]
    assert np.max(np.abs(lmin - np.array([0.1, 0.5, -0.25]))) <= 1e-14


@pytest.mark.parametrize("size", [(16, 12, 2), (127, 6, 10)], ids=lambda s: "n%d" % s[0])
def test_u_zero_is_tighten_matrices(gpu, size):
    """tightenMatrices (cons_sdp.c:1913-1955): u = 0, lb = 0, ub = 1 - the restatement is built from A_0 alone, M(mu) = mu A_i - A_0.
    The family's A_i (each >= 0.02 I) with a constant matrix of their smallest eigenvalues' size: a diagonal in [0, 0.022] (INNER
    where A_i - A_0 is psd, INFEASIBLE where not), and a negative diagonal in [-0.02, -0.005] (M(0) is positive definite: LB)"""
    n, m, rank = size
    seen = set()
    for which in (0, 1):
        A, lb0, ub0, _ = K.instance(size, K.FLAVOURS[0], 2)
        A = np.array(A)
        A[0] = np.diag(np.random.default_rng([n, 7]).uniform(0.0, 0.022, n)) if which == 0 else \
            -np.diag(np.random.default_rng([n, 8]).uniform(0.005, 0.02, n))
        fl = which
        u, lb, ub = np.zeros(m), np.zeros(m), np.ones(m)
        s = _solver(gpu, A, "dense")
        st, ov, lmin, grad, ne = s.onevar_bounds(0, u, lb, ub, K.FEASTOL)
        s.close()
        for i in range(m):
            r = K.onevar_ref(-A[0], A[i + 1], 0.0, K.NEWTON, 0.0, 1.0, K.FEASTOL)
            _check_properties(A, u, i, K.NEWTON, 0.0, 1.0, int(st[i]), float(ov[i]), K.FEASTOL)
            if K.decidable(K.NEWTON, r[5]):
                _check_against_ref(A, u, i, r, int(st[i]), float(ov[i]), int(ne[i]), K.FEASTOL, 0.0, 1.0, (fl, i))
                seen.add(int(st[i]))
    print("n = %d: statuses seen" % n, sorted(K.STATUS_NAMES[x] for x in seen))
    assert K.LB in seen and K.INNER in seen


def _bits(res):
    return [np.asarray(a).tobytes() for a in res]


@pytest.mark.parametrize("size", [(17, 12, 3), (65, 8, 6)], ids=lambda s: "n%d" % s[0])
def test_contract_launches_bits_subsets_and_a_declined_job(gpu, size):
    n, m, rank = size
    A, lb, ub, refs = K.instance(size, K.FLAVOURS[1], 1)
    s = _solver(gpu, A, "dense")
    c0 = gpu.onevar_bounds_stats()
    full = s.onevar_bounds(0, ub, lb, ub, K.FEASTOL)
    c1 = gpu.onevar_bounds_stats()
    assert (c1[0] - c0[0], c1[1] - c0[1], c1[2] - c0[2]) == (1, 2, 1)            # m jobs: two launches, one read-back
    one = s.onevar_bounds(0, ub, lb[2:3], ub[2:3], K.FEASTOL, vars=[2])
    c2 = gpu.onevar_bounds_stats()
    assert (c2[0] - c1[0], c2[1] - c1[1], c2[2] - c1[2]) == (1, 2, 1)            # one job: the same
    again = s.onevar_bounds(0, ub, lb, ub, K.FEASTOL)
    assert _bits(again) == _bits(full)                                            # same input, same bits
    assert _bits(one) == _bits([a[2:3] for a in full])
    sub = [m - 1, 0, 3]
    part = s.onevar_bounds(0, ub, lb[sub], ub[sub], K.FEASTOL, vars=sub)
    assert _bits(part) == _bits([a[sub] for a in full])                           # a job's bits do not depend on the other jobs
    # a declined job beside served ones
    ub2 = np.array(ub)
    ub2[1] = 1e20
    u = np.array(ub)                                                              # (u stays: only the job's bound is infinite)
    dec = s.onevar_bounds(0, u, lb, ub2, K.FEASTOL)
    assert dec[0][1] == K.DECLINED and dec[4][1] == 0
    keep = [i for i in range(m) if i != 1]
    assert _bits([a[keep] for a in dec]) == _bits([a[keep] for a in full])
    # a bounded loop: two evaluations are not enough for an INNER job
    inner = [i for i in range(m) if refs[i][0] == K.INNER and refs[i][4] > 2]
    assert inner
    i = inner[0]
    g = s.onevar_bounds(0, ub, lb[i:i + 1], ub[i:i + 1], K.FEASTOL, vars=[i], maxevals=2)
    assert g[0][0] == K.GAVEUP and g[4][0] == 2 and g[1][0] == lb[i]
    r2 = K.onevar_ref(K.z_of(A, ub), A[i + 1], ub[i], K.NEWTON, lb[i], ub[i], K.FEASTOL, maxevals=2)
    assert r2[0] == K.GAVEUP and r2[1] == lb[i]
    s.close()


def test_two_host_threads_on_different_solvers_reproduce_the_single_thread_bits(gpu):
    """one solver per thread, a block of each size class"""
    import threading
    sizes = [(17, 12, 3), (65, 8, 6)]
    data = [K.instance(sz, K.FLAVOURS[3], 1) for sz in sizes]
    solvers = [_solver(gpu, d[0], "dense") for d in data]
    single = [_bits(solvers[i].onevar_bounds(0, data[i][2], data[i][1], data[i][2], K.FEASTOL)) for i in range(2)]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(4):
                got[i].append(_bits(solvers[i].onevar_bounds(0, data[i][2], data[i][1], data[i][2], K.FEASTOL)))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert got[i] == [single[i]] * 4
    for s in solvers:
        s.close()


def test_a_block_of_129_rows_is_not_served(gpu):
    n, m = 129, 2
    rng = np.random.default_rng(129)
    A = np.zeros((m + 1, n, n))
    for i in range(m + 1):
        B = rng.standard_normal((n, 3))
        A[i] = B @ B.T + np.eye(n)
    s = _solver(gpu, A, "dense")
    c0 = gpu.onevar_bounds_stats()
    st, ov, lmin, grad, ne = s.onevar_bounds(0, np.ones(m), np.zeros(m), np.ones(m), K.FEASTOL)
    c1 = gpu.onevar_bounds_stats()
    s.close()
    assert list(st) == [-1] * m and c1 == c0
    assert np.all(np.isnan(ov)) and np.all(np.isnan(lmin)) and list(ne) == [0] * m          # nothing else written


def test_argument_errors_and_an_empty_call(gpu):
    """every argument error returns HIPSDP_ERR_ARG (3) with nothing launched; count == 0 returns 0 with nothing launched"""
    A, lb, ub, refs = K.instance((3, 4, 1), K.FLAVOURS[0], 1)
    m = 4
    s = _solver(gpu, A, "dense")
    lib = gpu.lib()
    f = lib.hipsdp_onevar_bounds
    dp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    u, l, h = np.array(ub), np.array(lb), np.array(ub)
    st, ev = np.full(m, 7, dtype=np.int32), np.zeros(m, dtype=np.int32)
    ov = np.zeros(m)
    var, kind = np.arange(m, dtype=np.int32), np.zeros(m, dtype=np.int32)
    opts = gpu.OnevarOpts(1e-6, 1e20, 0)
    o = C.byref(opts)
    c0 = gpu.onevar_bounds_stats()
    fresh = gpu.Solver(0)                                                         # no shape
    assert f(fresh.h, 0, dp(u), m, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    fresh.close()
    assert f(None, 0, dp(u), m, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, -1, dp(u), m, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 1, dp(u), m, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 0, None, m, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 0, dp(u), m, None, None, None, dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 0, dp(u), m, None, None, dp(l), None, o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 0, dp(u), m, None, None, dp(l), dp(h), None, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 0, dp(u), m, None, None, dp(l), dp(h), o, None, dp(ov), None, None, None) == 3
    assert f(s.h, 0, dp(u), m, None, None, dp(l), dp(h), o, ip(st), None, None, None, None) == 3
    assert f(s.h, 0, dp(u), -1, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 0, dp(u), m - 1, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3      # vars NULL, count != m
    for bad in (-1, m):
        v2 = var.copy()
        v2[2] = bad
        assert f(s.h, 0, dp(u), m, ip(v2), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    for bad in (-1, 2):
        k2 = kind.copy()
        k2[3] = bad
        assert f(s.h, 0, dp(u), m, ip(var), ip(k2), dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    neg = gpu.OnevarOpts(-1e-6, 1e20, 0)
    assert f(s.h, 0, dp(u), m, None, None, dp(l), dp(h), C.byref(neg), ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, 0, dp(u), 0, ip(var), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 0        # count == 0
    assert list(st) == [7] * m and gpu.onevar_bounds_stats() == c0
    # ... and the call with everything in place, the optional outputs missing
    assert f(s.h, 0, dp(u), m, ip(var), ip(kind), dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 0
    assert all(x in (K.LB, K.INNER, K.INFEASIBLE) for x in st)
    s.close()


@pytest.mark.parametrize("n", [1, 2, 64, 65, 128])
def test_unit_entry_on_given_matrices(gpu, n):
    """the Newton kernel alone: Z and one dense A per job from the caller"""
    if n == 1:
        # M(mu) = mu - 0.5 by hand: inner optimum 0.5 - feastol / 2 in three evaluations; infeasible on [0, 0.25]; LB on [0.6, 1]
        st, ov, lmin, grad, ne = gpu.onevar_unit(1, [[-0.5]], [[[1.0]]] * 3, [0.0] * 3, [0.0, 0.0, 0.6], [1.0, 0.25, 1.0], 1e-6)
        assert list(st) == [K.INNER, K.INFEASIBLE, K.LB] and list(ne) == [3, 1, 2]
        assert abs(ov[0] - (0.5 - 0.5e-6)) <= 1e-15 and ov[1] == 0.25 and ov[2] == 0.6
        assert list(grad) == [1.0, 1.0, 0.0] and abs(lmin[0] + 0.5e-6) <= 1e-15 and lmin[1] == -0.25
        return
    size = {2: (2, 3, 1), 64: (64, 10, 6), 65: (65, 8, 6), 128: (128, 6, 12)}[n]
    m = size[1]
    for fl in (K.FLAVOURS[1], K.FLAVOURS[6]):
        A, lb, ub, refs = K.instance(size, fl, 2)
        Z = K.z_of(A, ub)
        st, ov, lmin, grad, ne = gpu.onevar_unit(n, Z, A[1:], ub, lb, ub, K.FEASTOL)
        for i, r in enumerate(refs):
            _check_properties(A, ub, i, K.NEWTON, lb[i], ub[i], int(st[i]), float(ov[i]), K.FEASTOL)
            if K.decidable(K.NEWTON, r[5]):
                _check_against_ref(A, ub, i, r, int(st[i]), float(ov[i]), int(ne[i]), K.FEASTOL, lb[i], ub[i], (fl, i))
