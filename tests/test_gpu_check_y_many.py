"""GPU: hipsdp_check_y_many - the feasibility check of many candidate points in one call (csrc/check_many.hip, the values-only
many-matrix kernels of csrc/eigi.hip, the batched tridiagonal path of csrc/syevx.hip) - against numpy on small solvers with entries
and points of order 1, against what the other calls return for one point, and for what makes it a batch: bits that depend on the
block and the candidate's row alone, a launch count that does not depend on the number of candidates, one read-back per chunk.

Bounds.  lmin: the header's own contract for every eigen entry, |lmin - lambda_1| <= 1e-12 max |lambda| (lambda: numpy's eigvalsh of the
Z formed in float64) - the bound the eigen-solver tests use.  lpviol: 4 (m + 1) 2^-53 max_r (|c_r| + sum_i |D_ri y_i|), the rounding
bound of a sum of m + 1 terms.  Z of the unit entry: the same bound entry by entry.  Agreement with hipsdp_eigencuts_all[_large]:
2e-12 max |lambda|, both being within 1e-12 of the truth.

Storage forms.  A solver loaded with dense matrices keeps a block of at most 64 rows as dense rows and sweeps a larger one as packed
lower triangles; loaded as triplets under sparse_policy(2) every block is kept as nonzeros (the way the cut tests make the forms).  So the
class of at most 64 rows is run as dense rows and nonzeros, the classes of 65 .. 128 and 129 .. 512 rows as packed triangles and
nonzeros: every form the engine can hold a block of that class in."""
import ctypes as C
import os
import threading
import numpy as np
import pytest
from conftest import GOLDEN
import ipm_ref
import rounding
from check_y_cases import KINDS, family, load, zmat, spectra, check_lmin

pytestmark = pytest.mark.gpu

ERR_ARG = 3
EDGES = [1, 3, 17, 64, 65, 128, 129, 130]       # the class edges and an odd size
U = 2.0 ** -53


def hexes(a):
    return [float(v).hex() for v in np.asarray(a).reshape(-1)]


# ---- 1. accuracy against numpy -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m", [1, 2, 37])
def test_lmin_matches_numpy_at_the_class_edges(gpu, m, kind, form):
    G = gpu.check_many_group()
    blocks, Y = family(EDGES, m, kind, 2 * G + 3)
    s = load(gpu, blocks, m, form)
    lmin, lpviol, served = s.check_y_many(Y)
    s.close()
    assert lmin.shape == (2 * G + 3, len(EDGES)) and list(served) == [0] * len(EDGES) and np.all(lpviol == 0.0)
    lam1 = check_lmin(lmin, blocks, Y, "%s %s m = %d" % (form, kind, m))
    if kind == "feasible":
        assert np.all(lam1 > 0.0) and np.all(lmin > 0.0)
    elif kind == "negative":
        assert np.all(lam1[:, 2:] < 0.0) and np.all(lmin[:, 2:] < 0.0)          # (every block of 17 rows and more)
    else:
        # n - r copies of the shift at the bottom
        for k, A in enumerate(blocks):
            n = A.shape[1]
            if n - max(1, min(m, n // 3)) >= 2:
                w = np.linalg.eigvalsh(zmat(A, Y[0]))
                assert abs(w[1] - w[0]) <= 1e-12 * abs(w[-1]) and abs(w[0] - 0.75) <= 1e-12 * abs(w[-1]), n


@pytest.mark.parametrize("m,kind", [(37, "negative"), (2, "lowrank")])
def test_lmin_matches_numpy_for_every_count_across_the_group_edges(gpu, m, kind):
    G = gpu.check_many_group()
    blocks, Y = family(EDGES, m, kind, 2 * G + 3)
    s = load(gpu, blocks, m, "dense")
    for count in (1, G - 1, G, G + 1, 2 * G + 3):
        lmin, _, served = s.check_y_many(Y[:count])
        assert lmin.shape == (count, len(EDGES)) and np.all(served == 0)
        check_lmin(lmin, blocks, Y[:count], "count %d" % count)
    s.close()


@pytest.mark.parametrize("kind,form", [("feasible", "dense"), ("negative", "dense"), ("lowrank", "dense"), ("negative", "sparse")])
def test_a_single_block_of_512_rows(gpu, kind, form):
    blocks, Y = family([512], 2, kind, 2)
    s = load(gpu, blocks, 2, form)
    lmin, _, served = s.check_y_many(Y)
    s.close()
    assert list(served) == [0]
    check_lmin(lmin, blocks, Y, "512 rows, %s %s" % (form, kind))


# ---- 2. lpviol against numpy -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q,m", [(0, 5), (1, 1), (1, 37), (86, 2), (86, 37)])
def test_lpviol_matches_numpy(gpu, q, m):
    """D and the first point are small integers, so the three kinds of rows are what they are in every arithmetic: row r is violated
    by 0.75, met exactly, or has a slack of 0.5 at point 0, by r mod 3; the other points are of order 1"""
    G = gpu.check_many_group()
    rng = np.random.default_rng([q, m])
    count = 2 * G + 3
    Y = rng.uniform(-1.0, 1.0, (count, m))
    Y[0] = rng.integers(-2, 3, m)
    D = rng.integers(-3, 4, (q, m)).astype(np.float64) if q else None
    c = None
    if q:
        c = D @ Y[0] + np.array([(0.75, 0.0, -0.5)[r % 3] for r in range(q)])
    blocks, _ = family([3], m, "feasible", 1)
    s = load(gpu, blocks, m, "dense", D, c)
    _, lpviol, _ = s.check_y_many(Y)
    one = [s.check_y_many(Y[j:j + 1])[1][0] for j in range(count)]
    s.close()
    assert lpviol.shape == (count,)
    if q == 0:
        assert np.all(lpviol == 0.0)
        return
    slack0 = c - D @ Y[0]
    assert np.any(slack0 > 0) and (q < 3 or (np.any(slack0 == 0.0) and np.any(slack0 < 0)))
    for j in range(count):
        ref = max(0.0, float(np.max(c - D @ Y[j])))
        bound = 4 * (m + 1) * U * float(np.max(np.abs(c) + np.abs(D) @ np.abs(Y[j])))
        print("q = %d, m = %d, point %d: lpviol %.17g, numpy %.17g, bound %.3g" % (q, m, j, lpviol[j], ref, bound))
        assert abs(lpviol[j] - ref) <= bound, (j, lpviol[j], ref)
        assert float(lpviol[j]).hex() == float(one[j]).hex()
    assert lpviol[0] == 0.75                 # (integers: exact)
    if q >= 3:
        # a point every row has slack at: the violation is exactly 0
        s = load(gpu, blocks, m, "dense", D, c - 1.0)
        assert s.check_y_many(Y[:1])[1][0] == 0.0
        s.close()


# ---- 3. independence, bit for bit --------------------------------------------------------------------------------------------------------

IND_NS = [3, 17, 65, 130]


def _ind_problem(gpu):
    G = gpu.check_many_group()
    m = 5
    blocks, Y = family(IND_NS, m, "negative", 2 * G + 3, seed=3)
    rng = np.random.default_rng(11)
    D = rng.standard_normal((3, m))
    c = rng.standard_normal(3)
    return blocks, Y, m, D, c


@pytest.mark.parametrize("form", ["dense", "sparse"])
def test_the_bits_of_a_candidate_depend_on_its_row_and_the_block_alone(gpu, form, monkeypatch):
    monkeypatch.delenv("HIPSDP_CHECK_MANY_CHUNK", raising=False)
    blocks, Y, m, D, c = _ind_problem(gpu)
    count = len(Y)
    s = load(gpu, blocks, m, form, D, c)
    lmin, lpviol, _ = s.check_y_many(Y)
    again = s.check_y_many(Y)
    assert hexes(again[0]) == hexes(lmin) and hexes(again[1]) == hexes(lpviol)                   # two identical calls
    for j in range(count):                                                                         # the same row alone
        l1, v1, _ = s.check_y_many(Y[j:j + 1])
        assert hexes(l1[0]) == hexes(lmin[j]) and hexes(v1) == hexes(lpviol[j:j + 1]), j
    perm = np.random.default_rng(5).permutation(count)                                             # at another position
    lp_, vp_, _ = s.check_y_many(Y[perm])
    assert hexes(lp_) == hexes(lmin[perm]) and hexes(vp_) == hexes(lpviol[perm])
    for chunk in (1, 3):                                                                           # in other chunks
        monkeypatch.setenv("HIPSDP_CHECK_MANY_CHUNK", str(chunk))
        st0 = gpu.check_y_many_stats()
        lc, vc, _ = s.check_y_many(Y)
        st1 = gpu.check_y_many_stats()
        assert hexes(lc) == hexes(lmin) and hexes(vc) == hexes(lpviol), chunk
        assert st1[0] - st0[0] == 1 and st1[2] - st0[2] == (count + chunk - 1) // chunk
        assert st1[1] - st0[1] == ((count + chunk - 1) // chunk) * (1 + 1 + 1 + (130 + 3) + 1)
    monkeypatch.delenv("HIPSDP_CHECK_MANY_CHUNK")
    s.close()
    # a second solver with an extra block in front
    extra, _ = family([12], m, "feasible", 1, seed=9)
    s2 = load(gpu, extra + blocks, m, form, D, c)
    l2, v2, served = s2.check_y_many(Y)
    s2.close()
    assert list(served) == [0] * 5 and hexes(l2[:, 1:]) == hexes(lmin) and hexes(v2) == hexes(lpviol)


# ---- 4. the unit entry: k_cm_form_z alone ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["dense", "sparse"])
@pytest.mark.parametrize("m", [2, 37])
def test_form_z_many_unit(gpu, m, form):
    """dense rows (3, 17, 64 rows), packed triangles (65, 128, 130) and nonzeros: every candidate's Z in a batch is, bit for bit, the
    unit's output for that candidate alone, for count across the group edges; it is symmetric; it is numpy's Z within the rounding
    bound of a sum of m + 1 terms; one launch whatever the count"""
    G = gpu.check_many_group()
    ns = [3, 17, 64, 65, 128, 130]
    blocks, Y = family(ns, m, "negative", 2 * G + 3, seed=1)
    s = load(gpu, blocks, m, form, units=True)
    alone = []
    for j in range(len(Y)):
        Z, launches = s.form_z_many_unit(Y[j:j + 1])
        assert launches == 1
        alone.append(Z)
    for count in (1, G - 1, G, G + 1, 2 * G + 3):
        Z, launches = s.form_z_many_unit(Y[:count])
        assert launches == 1 and len(Z) == len(ns)
        for k, A in enumerate(blocks):
            assert Z[k].shape == (count, ns[k], ns[k])
            for j in range(count):
                assert np.array_equal(Z[k][j], alone[j][k][0]), (count, k, j)
    worst = 0.0
    for k, A in enumerate(blocks):
        for j in range(len(Y)):
            Zd = alone[j][k][0]
            assert np.array_equal(Zd, Zd.T), (k, j)
            bound = 4 * (m + 1) * U * (np.abs(A[0]) + np.tensordot(np.abs(Y[j]), np.abs(A[1:]), axes=(0, 0)))
            diff = np.abs(Zd - zmat(A, Y[j]))
            assert np.all(diff <= bound), (k, j, float(diff.max()))
            worst = max(worst, float(np.max(diff / np.maximum(bound, 1e-300))))
    print("m = %d %s: largest |Z - numpy| / bound = %.3g" % (m, form, worst))
    s.close()


# ---- 5. agreement with the calls that serve one point ------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["negative", "lowrank"])
def test_lmin_agrees_with_the_one_point_calls(gpu, kind):
    G = gpu.check_many_group()
    m = 7
    blocks, Y = family(EDGES, m, kind, G + 1, seed=2)
    s = load(gpu, blocks, m, "dense")
    lmin, _, _ = s.check_y_many(Y)
    _, top = spectra(blocks, Y)
    for j, y in enumerate(Y):
        small = s.eigencuts_all(y, 1e-6, 0)
        large = s.eigencuts_all_large(y, 1e-6, 0)
        for k, n in enumerate(EDGES):
            other = small[k][0] if n <= 128 else large[k][0]
            assert (large[k] is None) == (n <= 128)
            assert abs(lmin[j, k] - other) <= 2e-12 * top[j, k], (j, n, lmin[j, k], other)
    s.close()


# ---- 6. served / not served, argument errors with a solver -------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [[513, 12], [12, 513]])
def test_a_block_of_513_rows_is_turned_away_and_the_other_is_served(gpu, ns):
    m = 1
    blocks, Y = family(ns, m, "negative", 3, seed=4)
    s = load(gpu, blocks, m, "dense")
    lmin, _, served = s.check_y_many(Y, lmin_fill=-777.25)
    s.close()
    big, small = ns.index(513), ns.index(12)
    assert list(served) == [(-1 if n == 513 else 0) for n in ns]
    assert np.all(lmin[:, big] == -777.25)
    check_lmin(lmin[:, small:small + 1], [blocks[small]], Y, "beside 513 rows")


def test_argument_errors_with_a_solver(gpu):
    lib = gpu.lib()
    blocks, Y = family([3], 2, "feasible", 2)
    s = load(gpu, blocks, 2, "dense")
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    lm, lp = np.full(2, 7.0), np.full(2, 7.0)
    sv = np.full(1, 77, dtype=np.int32)
    ip = sv.ctypes.data_as(C.POINTER(C.c_int))
    st0 = gpu.check_y_many_stats()
    assert lib.hipsdp_check_y_many(s.h, -1, dp(Y), dp(lm), dp(lp), ip) == ERR_ARG
    assert lib.hipsdp_check_y_many(s.h, 2, None, dp(lm), dp(lp), ip) == ERR_ARG
    assert lib.hipsdp_check_y_many(s.h, 2, dp(Y), None, dp(lp), ip) == ERR_ARG
    assert lib.hipsdp_check_y_many(s.h, 0, None, None, None, None) == 0                 # count == 0: nothing happens
    assert lib.hipsdp_check_y_many(s.h, 0, dp(Y), dp(lm), dp(lp), ip) == 0
    assert list(lm) == [7.0, 7.0] and list(lp) == [7.0, 7.0] and list(sv) == [77]
    assert gpu.check_y_many_stats() == st0
    assert lib.hipsdp_check_y_many(s.h, 2, dp(Y), dp(lm), None, None) == 0              # lpviol and served may be NULL
    assert np.all(lm > 0.0)
    s.close()
    fresh = gpu.Solver(0)                                                                # a solver without a shape
    assert lib.hipsdp_check_y_many(fresh.h, 2, dp(Y), dp(lm), dp(lp), ip) == ERR_ARG
    fresh.close()


# ---- 7. launches and read-backs ----------------------------------------------------------------------------------------------------------

def formula(ns):
    small = any(n <= 64 for n in ns)
    mid = any(64 < n <= 128 for n in ns)
    nmax = max([n for n in ns if 128 < n <= 512], default=0)
    return (1 if ns else 0) + int(small) + int(mid) + (nmax + 3 if nmax else 0) + 1


@pytest.mark.parametrize("ns", [[12], [100], [12, 12, 30, 100, 70], [17, 65, 130], [129, 200, 150]])
def test_launches_and_readbacks_are_the_formula(gpu, ns, monkeypatch):
    monkeypatch.delenv("HIPSDP_CHECK_MANY_CHUNK", raising=False)
    G = gpu.check_many_group()
    blocks, Y = family(ns, 2, "negative", 2 * G + 3, seed=6)
    s = load(gpu, blocks, 2, "dense")
    others = (gpu.eigencuts_all_stats(), gpu.eigencuts_all_large_stats(), gpu.sparsecuts_all_stats(), gpu.onevar_bounds_all_stats())
    deltas = []
    for count in (1, 2 * G + 3):
        st0 = gpu.check_y_many_stats()
        s.check_y_many(Y[:count])
        st1 = gpu.check_y_many_stats()
        deltas.append(tuple(b - a for a, b in zip(st0, st1)))
    print("blocks %s: (calls, launches, read-backs) %s" % (ns, deltas))
    assert deltas[0] == deltas[1] == (1, formula(ns), 1)
    st0 = gpu.check_y_many_stats()
    s.check_y_many(Y[:0])
    assert gpu.check_y_many_stats() == st0                                               # count == 0 moves nothing
    assert others == (gpu.eigencuts_all_stats(), gpu.eigencuts_all_large_stats(), gpu.sparsecuts_all_stats(), gpu.onevar_bounds_all_stats())
    # ... and the reverse
    st0 = gpu.check_y_many_stats()
    s.eigencuts_all(Y[0], 1e-6, 0)
    assert gpu.check_y_many_stats() == st0
    s.close()


# ---- 8. two host threads -----------------------------------------------------------------------------------------------------------------

def test_two_host_threads_on_two_solvers_reproduce_the_single_thread_bits(gpu):
    G = gpu.check_many_group()
    data = [family([3, 17, 65, 130], 5, "negative", 2 * G + 3, seed=7), family([40, 100, 129], 3, "lowrank", G + 1, seed=8)]
    solvers = [load(gpu, d[0], d[1].shape[1], "dense") for d in data]
    single = [s.check_y_many(d[1]) for s, d in zip(solvers, data)]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                got[i].append(solvers[i].check_y_many(data[i][1]))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 3
        for r in got[i]:
            assert hexes(r[0]) == hexes(single[i][0]) and hexes(r[1]) == hexes(single[i][1])
    for s in solvers:
        s.close()


# ---- 9. end to end: the roundings of example_TT's root -----------------------------------------------------------------------------------

TT_COUNT = 64
# The seed was chosen on the CPU, with the numpy oracle's root solution (oracle/ipm_ref.py) and numpy alone.  The root's integer variables
# are at 0 or at fractions of 0.004 .. 0.024, and a rounding is feasible only if it raises one bar in each of five groups (243 of the
# 2^15 supports of the fractional variables are): a rounding of the root is feasible with probability 3.2e-8.  226626 is the FIRST seed of
# a scan from 0 whose 64 roundings hold a feasible point - candidate 3, the bars 9, 10, 13, 19, 25: Z has three zero eigenvalues there
# whatever the continuous variable is, against max |lambda| = 398.7, and no LP row is violated - beside 63 infeasible ones (lmin <=
# -0.178, ten distinct points), none within 1e-9 of a threshold.  No draw of the seed lies within 8.8e-4 of a fraction, so the 1e-6 by
# which the device's root solution differs from the oracle's changes no rounding.
TT_SEED = 226626


def test_roundings_of_the_root_of_example_tt(gpu):
    """The root relaxation of example_TT (the golden instance the other suites load: a 10 x 10 block, 85 LP rows, 37 variables, 36 of
    them binary) solved on the device, TT_COUNT randomized roundings of its solution (tests/harness/rounding.py), ONE check_y_many call:
    the candidates it accepts - lmin >= -1e-6 and lpviol <= 1e-6 - are the ones numpy accepts.  A candidate whose numpy lmin or LP slack
    lies within 1e-9 of the threshold is not compared; at most 2 of the 64 may be left out that way.

    The seed: see the note above TT_SEED."""
    import bnb
    import sdpa_io
    import sdpi_prepare
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", "example_TT.dat-s.gz"))
    P = sdpi_prepare.prepare(bnb.instance_to_sdpi(inst))
    b, blk, D, c, maps = sdpi_prepare.to_core(P)
    blocks = [np.asarray(A) for A in blk]
    D, c = np.asarray(D), np.asarray(c)
    s = gpu.Solver(0)
    s.load_core(ipm_ref.CoreProblem(b, blocks, D, c))
    info = s.solve(gaptol=1e-6, feastol=1e-6)
    assert info.status == 0
    y = s.y()
    act = maps["active"]
    ints = set(inst.intvars)
    isint = [a in ints for a in act]
    lb, ub = [P.lb[a] for a in act], [P.ub[a] for a in act]
    Y, keep = rounding.roundings(y, isint, lb, ub, TT_COUNT, TT_SEED)
    assert keep.all() and Y.shape == (TT_COUNT, len(b))
    st0 = gpu.check_y_many_stats()
    order, lmin, lpviol = rounding.check_roundings(s, Y, -np.asarray(b))
    st1 = gpu.check_y_many_stats()
    s.close()
    assert tuple(q - p for p, q in zip(st0, st1)) == (1, 3, 1)                           # one call: Z, the eigenvalues, the result
    lam1, top = spectra(blocks, Y)
    slack = np.array([float(np.max(c - D @ yy)) for yy in Y])
    ref_ok = (lam1[:, 0] >= -1e-6) & (slack <= 1e-6)
    near = (np.abs(lam1[:, 0] + 1e-6) <= 1e-9) | (np.abs(slack - 1e-6) <= 1e-9)
    dev_ok = np.zeros(TT_COUNT, dtype=bool)
    dev_ok[order] = True
    print("example_TT root: %d roundings, %d distinct, numpy accepts %d, the device %d, %d near a threshold; lmin in [%.6g, %.6g]" %
          (TT_COUNT, len({tuple(v) for v in Y}), int(ref_ok.sum()), int(dev_ok.sum()), int(near.sum()), lmin.min(), lmin.max()))
    assert near.sum() <= 2
    assert np.array_equal(dev_ok[~near], ref_ok[~near])
    assert np.any(ref_ok[~near]) and np.any(~ref_ok[~near])
    assert np.all(np.abs(lmin[:, 0] - lam1[:, 0]) <= 1e-12 * top[:, 0])
    vals = [float(-np.asarray(b) @ Y[j]) for j in order]
    assert vals == sorted(vals)
