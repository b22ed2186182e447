"""Every form of the Schur assembly M_ij = tr(A_i X A_j Z^-1) at the matrix level (scip-sdp_amd/csrc/schur.hip through
hipsdp_schur_form_unit / hipsdp_schur_small_unit; families, references and figures: tests/harness/schur_cases.py, held to their
own claims by tests/test_schur_cases_cpu.py).

1. exact family, every form: the device EQUALS float64 numpy bit for bit (every partial sum is an integer below 2^53), Mx is symmetric
   bit for bit, and the counters of the call (products taken by the persistent kernels, by the paired-band kernel, by the Gram kernel)
   are those the restated dispatch rules give for the shape - a shape that silently falls to another kernel fails.  The same family
   goes through hipsdp_schur_identity_unit, hipsdp_schur_sparse_unit and hipsdp_dgemm.
2. hs_schur_small on the exact family, with LP rows, the Lm / diagM copies, and the shapes it must refuse untouched.
3. iterate family (near-complementary X, Z^-1 of condition 1e4 .. 1e12): component-wise F = max |M - M_ref| / (eps B) against an
   extended-precision reference; F_device <= 10 F_numpy (the same terms in another order; the margin of the Cholesky tests) and
   F_device <= n^2 + 2 n + 2 (Higham's first-order constant of the three chained sums).  One lost term of the K = n^2 shows at
   F of the order 1 / (K eps), twelve decades above.  Nothing is excluded from the maximum.
4. scaled family: M(2^k_i A_i) = 2^(k_i + k_j) M(A_i) bit for bit in every form.
5. edges as ordinary cases: m1 = 1, n = 1, n = 2, a zero A_j, more parts than slices exist."""
import numpy as np
import pytest

import schur_cases as sc
from test_gpu_cold_start_packed import SHAPES as COLD_SHAPES

pytestmark = pytest.mark.gpu

_PLANS = {}


def has_plan(gpu):
    """whether gram.hip has a plan for (M, K) with the 64 slabs of a full workspace: device code decides, asked once per shape"""
    def f(M, K):
        if (M, K) not in _PLANS:
            _PLANS[(M, K)] = gpu.gram_plan_info(M, K, 64) is not None
        return _PLANS[(M, K)]
    return f


def operands(form, case):
    A, R, G, X, Zi = case
    return (A, R, G) if form in sc.W_FORMS else (A, X, Zi)


def run_exact(gpu, form, m1, n, parts=1, ws=0.0, case=None, ref=None, bad=None):
    """one form on an exact case: bits of numpy, symmetric, counters as predicted -> Mx"""
    case = sc.exact(m1, n) if case is None else case
    ref = sc.exact_ref(m1, n) if ref is None else ref
    A, P, Q = operands(form, case)
    M, used = gpu.schur_form_unit(form, A, P, Q, parts=parts, ws_gbytes=ws)
    want = sc.predict_used(form, m1, n, parts=parts, ws_gbytes=ws, has_plan=has_plan(gpu))
    what = "%s (m1, n) = (%d, %d) parts %d ws %.3g" % (sc.FORM_NAMES[form], m1, n, parts, ws)
    d = sc.first_difference(M, ref)
    print("%-62s used %s predicted %s  %s" % (what, used, want, "equal to numpy" if d is None else d))
    if d is not None:
        if form == 1:
            print("   column slices (c0, cw):", sc.col_slices(m1, n, parts))
        if form == 2:
            print("   row chunks [r0, r1):", sc.row_chunks(m1, parts))
        bad.append((what, d))
    if not np.array_equal(M, M.T):
        bad.append((what, "not symmetric"))
    if used != want:
        bad.append((what, "used", used, "predicted", want))
    return M


@pytest.mark.parametrize("m1,n", sc.LADDER, ids=["%dx%d" % s for s in sc.LADDER])
def test_exact_family_every_form_on_the_ladder_of_product_kernels(gpu, m1, n):
    assert sc.exact_premise(m1, n) < 2.0 ** 53
    bad = []
    M0 = run_exact(gpu, 0, m1, n, bad=bad)
    for form, parts in ((1, 2), (2, 2), (3, 1), (4, 64)):
        M = run_exact(gpu, form, m1, n, parts=parts, bad=bad)
        if not np.array_equal(M, M0):
            bad.append((sc.FORM_NAMES[form], "differs from hs_schur_W", sc.first_difference(M, M0)))
    assert not bad, bad


def test_the_ladder_reaches_every_rung(gpu):
    """what the shapes were chosen for, said by the counters of hs_schur_W itself: (192, 131) no persistent kernel, (192, 130) both
    triangular products on the paired-band kernel, and the Gram kernel at (401, 300) - its plan for M = 401, K = 90000 exists"""
    got = {}
    for m1, n in ((192, 131), (192, 130), (401, 300)):
        A, R, G, _, _ = sc.exact(m1, n)
        got[(m1, n)] = gpu.schur_form_unit(0, A, R, G)[1]
    print(got, "Gram plans:", {k: gpu.gram_plan_info(k[0], k[1] ** 2, 64) for k in got})
    assert got[(192, 131)] == (0, 0, 0) and got[(192, 130)] == (2, 2, 0)
    assert got[(401, 300)] == (2, 2, 1)


@pytest.mark.parametrize("form,m1,n,parts,ws",
                         [(1,) + s + (0.0,) for s in sc.FORM1] + [(2,) + s + (0.0,) for s in sc.FORM2]
                         + [(3,) + s + (1, 0.0) for s in sc.FORM3] + [(3,) + s + (1, sc.chunk_gbytes(s[1])) for s in sc.FORM3]
                         + [(4,) + s + (0.0,) for s in sc.FORM4],
                         ids=lambda v: ("%.0e" % v if isinstance(v, float) else str(v)))
def test_exact_family_sharded_and_chunked_forms(gpu, form, m1, n, parts, ws):
    assert sc.exact_premise(m1, n) < 2.0 ** 53
    bad = []
    M = run_exact(gpu, form, m1, n, parts=parts, ws=ws, bad=bad)
    A, R, G, _, _ = sc.exact(m1, n)
    M0 = gpu.schur_form_unit(0, A, R, G)[0]
    if not np.array_equal(M, M0):
        bad.append(("differs from hs_schur_W", sc.first_difference(M, M0)))
    assert not bad, bad


def _int_stack(m1, n, seed):
    rng = np.random.default_rng([seed, m1, n])
    T = np.tril(rng.integers(-1, 2, (m1, n, n), dtype=np.int8))
    return np.ascontiguousarray((T + np.tril(T, -1).transpose(0, 2, 1)).astype(np.float64))


@pytest.mark.parametrize("m1,n,ws", [s[:3] for s in COLD_SHAPES], ids=["%dx%d" % s[:2] for s in COLD_SHAPES])
def test_exact_family_through_the_cold_start_assembly(gpu, m1, n, ws):
    """<A_i, A_j> of matrices with entries in {-1, 0, 1}: at most n^2, and 2 P P^T - D D^T at most 2 n^2 + n, in every partial sum"""
    assert 2 * n * n + n < 2 ** 53
    A = _int_stack(m1, n, 7)
    F = A.reshape(m1, -1)
    ref = F @ F.T
    assert np.array_equal(ref, ref.T) and np.array_equal(ref, np.round(ref))
    il = np.tril_indices(m1)
    bad = []
    for full in (False, True):
        M, _ = gpu.schur_identity_unit(A, ws_gbytes=ws, full_storage=full)
        d = sc.first_difference(np.tril(M), np.tril(ref))
        print("(m1, n) = (%d, %d) ws %.3g %s: %s" % (m1, n, ws, "full rows" if full else "packed", "equal to numpy" if d is None else d))
        if d is not None:
            bad.append((full, d))
    assert not bad, bad


@pytest.mark.parametrize("n,m,k", [(70, 40, 4), (96, 120, 3), (130, 60, 9)])
def test_exact_family_through_the_sparse_assembly(gpu, n, m, k):
    """integer triplets: the sparse assembly equals numpy and the dense U form on the expanded matrices"""
    import instances
    rng = np.random.default_rng([n, m, k])
    _, coo, _, _, _, _ = instances.planted_sparse(n, m, k, seed=9)
    var, row, col, _ = coo
    coo = (var, row, col, rng.choice([-1.0, 1.0], len(var)))
    _, R, G, X, Zi = sc.exact(2, n)
    A = instances.coo_to_dense(n, m, coo, np.zeros((n, n)))
    assert float(np.max(sc.u_chain(A, X, Zi))) < 2.0 ** 53
    ref = sc.u_matrix(A, X, Zi)
    Ms = gpu.schur_sparse_unit(n, m, coo, X, Zi)
    Md, _ = gpu.schur_form_unit(3, A, X, Zi)
    il = np.tril_indices(m)
    ds, dd = sc.first_difference(np.tril(Ms[1:, 1:]), np.tril(ref[1:, 1:])), sc.first_difference(Md, ref)
    print("sparse against numpy:", ds or "equal", " dense U form against numpy:", dd or "equal")
    assert ds is None and dd is None and np.array_equal(Ms[1:, 1:][il], Md[1:, 1:][il])


@pytest.mark.parametrize("M,N,K,lower,splitk", [(3001, 2001, 402, False, 0),        # 24 x 16 = 384 tiles: the persistent kernel (A K-contiguous)
                                                (1000, 1000, 4000, True, 11),       # 36 lower tiles x 11 slices = 396: persistent, split-K
                                                (131, 67, 50, False, 0), (131, 67, 50, False, 3), (67, 67, 50, True, 2)])
@pytest.mark.parametrize("layA,layB", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_exact_family_through_hipsdp_dgemm(gpu, M, N, K, lower, splitk, layA, layB):
    rng = np.random.default_rng([M, N, K, layA, layB])
    A = rng.integers(-1, 2, (M, K) if layA == 0 else (K, M)).astype(np.float64)
    B = rng.integers(-1, 2, (N, K) if layB == 0 else (K, N)).astype(np.float64)
    C0 = rng.integers(-9, 10, (M, N)).astype(np.float64)
    ref = 2.0 * ((A if layA == 0 else A.T) @ (B.T if layB == 0 else B)) - C0                  # integers of at most 2 K + 9
    out = gpu.dgemm(A, B, layA, layB, alpha=2.0, beta=-1.0, Cin=C0, lower_only=lower, splitk=splitk)
    if lower:
        ref = np.where(np.tril(np.ones((M, N), dtype=bool)), ref, C0)                          # the other entries stay the caller's
    d = sc.first_difference(out, ref)
    print("dgemm %d x %d x %d layA %d layB %d lower %d splitk %d: %s" % (M, N, K, layA, layB, lower, splitk, d or "equal to numpy"))
    assert d is None


# ---- 2. the one-launch kernel -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m1,ns,q", sc.SMALL + [sc.SMALL_EDGE_TAKEN], ids=lambda v: str(v).replace(" ", ""))
def test_small_kernel_on_the_exact_family(gpu, m1, ns, q):
    As, Xs, Zs, D, x, z = sc.exact_small(m1, ns, q)
    assert sc.exact_small_premise(m1, ns, q) < 2.0 ** 53 and sc.small_admitted(m1, ns, q)
    ref = sc.small_matrix(As, Xs, Zs, D, x, z)
    taken, M, Lm, dg = gpu.schur_small_unit(As, Xs, Zs, D, x, z, fill=np.nan)
    d = sc.first_difference(M, ref)
    print("hs_schur_small m1 %d blocks %s LP rows %d: taken %d, %s" % (m1, ns, q, taken, d or "equal to numpy"))
    assert taken == 1 and d is None
    assert np.array_equal(M, M.T)
    assert np.array_equal(Lm, M[1:, 1:]) and np.array_equal(dg, np.diag(M)[1:])
    if len(ns) == 1 and q == 0 and m1 > 1:
        M3, _ = gpu.schur_form_unit(3, As[0], Xs[0], Zs[0])
        assert np.array_equal(M, M3)


@pytest.mark.parametrize("m1,ns,q", sc.SMALL_REFUSED, ids=lambda v: str(v).replace(" ", ""))
def test_small_kernel_refuses_what_it_does_not_admit_and_writes_nothing(gpu, m1, ns, q):
    As, Xs, Zs, D, x, z = sc.exact_small(m1, ns, q)
    assert not sc.small_admitted(m1, ns, q)
    taken, M, Lm, dg = gpu.schur_small_unit(As, Xs, Zs, D, x, z, fill=3.25)
    assert taken == 0 and np.all(M == 3.25) and np.all(Lm == 3.25) and np.all(dg == 3.25)


# ---- 3. iterates ---------------------------------------------------------------------------------------------------------------

ITER_FORMS = [(0, 1, 0.0), (1, 3, 0.0), (2, 2, 0.0), (3, 1, 0.0), (3, 1, None), (4, 48, 0.0)]        # (form, parts, ws; None: chunked)


def iterate_figures(gpu, m1, n, cond, bad):
    """F of every form and of the small kernel on one iterate case, each against the margin over numpy and against the cap"""
    case = sc.iterate(m1, n, cond)
    Mw, Bw, Mu, Bu = sc.iterate_ref(m1, n, cond)
    fw, fu = sc.numpy_figures(m1, n, cond)
    what = "n=%d m1=%d cond=%.0e" % (n, m1, cond)
    runs = []
    for form, parts, ws in ITER_FORMS:
        A, P, Q = operands(form, case)
        M, _ = gpu.schur_form_unit(form, A, P, Q, parts=parts, ws_gbytes=sc.chunk_gbytes(n) if ws is None else ws)
        runs.append((sc.FORM_NAMES[form] + (" chunked" if ws is None else ""), form in sc.W_FORMS, M))
    if sc.small_admitted(m1, (n,), 0):
        taken, M, _, _ = gpu.schur_small_unit([case[0]], [case[3]], [case[4]])
        assert taken == 1
        runs.append((sc.FORM_NAMES["small"], False, M))
    for name, wform, M in runs:
        f = sc.figure(M, Mw if wform else Mu, Bw if wform else Bu)
        fn = fw if wform else fu
        sc.check("iterate %s / numpy" % name, what, f, sc.MARGIN * fn, ref=fn, bad=bad)
        sc.check("iterate %s / cap" % name, what, f, sc.cap(n), bad=bad)
        if not np.array_equal(M, M.T):
            bad.append((name, what, "not symmetric"))


@pytest.mark.parametrize("m1,n", sc.ITERATE, ids=["%dx%d" % s for s in sc.ITERATE])
def test_iterate_family_component_wise_against_extended_precision(gpu, m1, n):
    if not sc.longdouble_ok():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here: no reference for the iterate family")
    bad = []
    for cond in sc.CONDS:
        iterate_figures(gpu, m1, n, cond, bad)
    assert not bad, bad


# ---- 4. scaling ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m1,n", sc.ITERATE, ids=["%dx%d" % s for s in sc.ITERATE])
def test_scaled_family_scales_bit_for_bit(gpu, m1, n):
    case = sc.iterate(m1, n, 1e8)
    k, s = sc.scaling(m1)
    scaled = (case[0] * s[:, None, None],) + tuple(case[1:])
    ss = s[:, None] * s[None, :]
    bad = []
    for form, parts, ws in ITER_FORMS:
        ws = sc.chunk_gbytes(n) if ws is None else ws
        M0, _ = gpu.schur_form_unit(form, *operands(form, case), parts=parts, ws_gbytes=ws)
        M1, _ = gpu.schur_form_unit(form, *operands(form, scaled), parts=parts, ws_gbytes=ws)
        d = sc.first_difference(M1, M0 * ss)
        print("%-16s n=%d m1=%d: %s" % (sc.FORM_NAMES[form], n, m1, d or "M(2^k A) = 2^(k_i + k_j) M(A) bit for bit"))
        if d is not None:
            bad.append((sc.FORM_NAMES[form], d))
    if sc.small_admitted(m1, (n,), 0):
        M0 = gpu.schur_small_unit([case[0]], [case[3]], [case[4]])[1]
        M1 = gpu.schur_small_unit([scaled[0]], [case[3]], [case[4]])[1]
        d = sc.first_difference(M1, M0 * ss)
        if d is not None:
            bad.append((sc.FORM_NAMES["small"], d))
    assert not bad, bad


# ---- 5. edges ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m1,n", [(1, 5), (4, 1), (4, 2), (1, 1)])
def test_edges_one_matrix_and_one_or_two_rows(gpu, m1, n):
    bad = []
    for form, parts in ((0, 1), (1, 1), (1, 5), (2, 1), (2, 3), (3, 1), (4, 1), (4, 7)):
        run_exact(gpu, form, m1, n, parts=parts, bad=bad)
    As, Xs, Zs, _, _, _ = sc.exact_small(m1, (n,), 0)
    taken, M, Lm, dg = gpu.schur_small_unit(As, Xs, Zs)
    assert taken == 1 and np.array_equal(M, sc.small_matrix(As, Xs, Zs)) and np.array_equal(Lm, M[1:, 1:])
    assert not bad, bad


@pytest.mark.parametrize("m1,n,zero", [(20, 24, 7), (60, 40, 0), (33, 130, 32)])
def test_edges_a_zero_matrix_gives_an_exactly_zero_row_and_column(gpu, m1, n, zero):
    A, R, G, X, Zi = sc.iterate(m1, n, 1e8)
    A = A.copy()
    A[zero] = 0.0
    for form, parts, ws in ITER_FORMS:
        P, Q = (R, G) if form in sc.W_FORMS else (X, Zi)
        M, _ = gpu.schur_form_unit(form, A, P, Q, parts=parts, ws_gbytes=sc.chunk_gbytes(n) if ws is None else ws)
        assert np.all(M[zero, :] == 0.0) and np.all(M[:, zero] == 0.0) and np.all(np.isfinite(M)), sc.FORM_NAMES[form]
        assert np.count_nonzero(M) == (m1 - 1) ** 2
    if sc.small_admitted(m1, (n,), 0):
        M = gpu.schur_small_unit([A], [X], [Zi])[1]
        assert np.all(M[zero, :] == 0.0) and np.all(M[:, zero] == 0.0)


@pytest.mark.parametrize("form,m1,n,parts", [(1, 60, 20, 64), (1, 9, 17, 40), (2, 5, 12, 64), (2, 41, 20, 30), (4, 20, 24, 1000), (4, 9, 17, 17)])
def test_edges_more_parts_than_slices_exist(gpu, form, m1, n, parts):
    bad = []
    run_exact(gpu, form, m1, n, parts=parts, bad=bad)
    assert not bad, bad


def test_unit_entries_refuse_bad_arguments(gpu):
    A, R, G, X, Zi = sc.exact(4, 3)
    for kw in (dict(form=5), dict(form=-1), dict(form=1, parts=0), dict(form=1, parts=65), dict(form=2, parts=0), dict(form=4, parts=0)):
        form = kw.pop("form")
        with pytest.raises(RuntimeError):
            gpu.schur_form_unit(form, A, R, G, **kw)
    import ctypes as C
    M = np.zeros((4, 4))
    assert gpu.ulib().hipsdp_schur_form_unit(0, 0, 1, 4, 3, None, gpu._dp(R), gpu._dp(G), C.c_double(0.0), gpu._dp(M), None) != 0
    assert gpu.ulib().hipsdp_schur_form_unit(0, 0, 1, 0, 3, gpu._dp(A), gpu._dp(R), gpu._dp(G), C.c_double(0.0), gpu._dp(M), None) != 0
    assert gpu.ulib().hipsdp_schur_small_unit(0, 4, 0, None, None, None, None, 0, None, None, None, gpu._dp(M), gpu._dp(M), gpu._dp(M), None) != 0
