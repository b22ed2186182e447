"""The case table of the small-path kernel tests (tests/small_path_cases.py) against the constants of the sources, and its references
(tests/harness/small_path_ref.py) against a second, independent float64 formulation.  No device."""
import numpy as np
import pytest

import small_path_cases as spc
import small_path_ref as ref


@pytest.fixture(scope="module")
def K():
    return spc.constants()


def test_constants_are_read_from_the_sources(K):
    assert set(K) == set(spc.NAMES) and all(isinstance(v, int) and v > 0 for v in K.values())
    # the straight-line branches of RB_LPROWS / RB_APPLYA and the group rule of the reductions are written with these numbers
    assert K["RB_ROWS"] * 65 <= K["RB_MATS"] * 4 * 65 <= 4 * K["HS_SMALL_N"] * (K["HS_SMALL_N"] + 1)


@pytest.mark.parametrize("c", spc.CASES, ids=[c["id"] for c in spc.CASES])
def test_case_reaches_the_branch_it_names(K, c):
    assert c["pred"](K) is True, "%s no longer reaches %s with %s" % (c["id"], c["branch"], K)
    assert c["records"] in (">=1", 0)


def test_every_named_branch_has_a_case(K):
    have = {c["branch"] for c in spc.CASES}
    missing = [b for b in spc.BRANCHES if b not in have]
    assert not missing, missing
    assert len({c["id"] for c in spc.CASES}) == len(spc.CASES)
    assert spc.DIR_BLOCK_TOO_LARGE == K["HS_SMALL_N"] + 1
    for op in ("dir_block", "lp_rows", "apply_A", "gemv_t", "reductions", "solve", "gemv_t3", "pass_a"):
        assert spc.cases(op), op


def test_declining_cases_are_the_ones_above_the_limits(K):
    """records = 0 exactly where the host-side rule of the operation says so"""
    for c in spc.CASES:
        if c["op"] == "lp_rows":
            assert (c["records"] == 0) == (c["q"] * c["m1"] > K["RB_MAXWORK"]), c["id"]
        elif c["op"] == "apply_A":
            assert (c["records"] == 0) == (len(c["n2"]) > 2 or (sum(c["n2"]) + c["q"]) * c["m1"] > K["RB_MAXWORK"]), c["id"]
        elif c["op"] == "gemv_t":
            assert (c["records"] == 0) == (c["E"] > K["RB_MAXN"] or c["R"] * c["E"] > K["RB_MAXWORK"]), c["id"]
        elif c["op"] == "reductions":
            assert (c["records"] == 0) == (c["lens"][-1] > K["RB_MAXN"]), c["id"]


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


@pytest.mark.parametrize("n,seed", [(3, 1), (7, 2), (16, 3)])
def test_references_against_a_second_formulation(n, seed):
    rng = np.random.default_rng(seed)
    X, R, E, Zi = (rng.standard_normal((n, n)) for _ in range(4))
    c, s1 = 0.73, 0.4
    # direction block through einsum, index by index
    G = c * np.einsum("ik,kj->ij", X, R) + E
    GZ = np.einsum("ik,kj->ij", G, Zi)
    H = s1 * Zi - X - 0.5 * (GZ + np.einsum("ij->ji", GZ))
    got, S = ref.dir_block(c, s1, X, R, E, Zi)
    assert _close(got, H) and np.all(S >= np.abs(got) * (1 - 1e-12))
    got0, _ = ref.dir_block(c, s1, X, R, None, Zi)
    assert _close(got0, H + 0.5 * (E @ Zi + (E @ Zi).T))
    # the passes through reshape / matmul
    m1, q = n + 2, 2 * n + 1
    A0, A1 = rng.standard_normal((m1, n, n)), rng.standard_normal((m1, 2, 2))
    V0, V1 = rng.standard_normal((n, n)), rng.standard_normal((2, 2))
    D, vlp, vin = rng.standard_normal((q, m1)), rng.standard_normal(q), rng.standard_normal(m1 - 1)
    want = A0.reshape(m1, -1) @ V0.ravel() + A1.reshape(m1, -1) @ V1.ravel() + vlp @ D
    for epi, wv in ((0, None), (1, want[1:] - 0.3 * vin), (2, 0.3 * vin - want[1:])):
        out, S, vout, Sv = ref.apply_A([A0.reshape(m1, -1), A1.reshape(m1, -1)], [V0, V1], D, vlp, epi, 0.3, vin)
        assert _close(out, want) and np.all(S >= np.abs(out) * (1 - 1e-12))
        assert (vout is None) if wv is None else _close(vout, wv)
    v, x, z, rd, elp = rng.standard_normal(m1), rng.uniform(0.5, 2, q), rng.uniform(0.5, 2, q), rng.standard_normal(q), rng.standard_normal(q)
    t = np.array([np.dot(D[r], v) for r in range(q)])
    o1, _, o2, _ = ref.lp_rows(D, v, 0, 0.9, 0.2, x, z, rd, elp)
    assert _close(o1, t - z) and o2 is None
    o1, _, o2, S2 = ref.lp_rows(D, v, 1, 0.9, 0.2, x, z, rd, elp)
    dz = t + 0.9 * rd
    assert _close(o1, dz) and _close(o2, (0.2 - x * z - x * dz - elp) / z) and np.all(S2 >= np.abs(o2) * (1 - 1e-12))
    o1n, _, o2n, _ = ref.lp_rows(D, v, 1, 0.9, 0.2, x, z, rd, None)
    assert _close(o2n, (0.2 - x * z - x * dz) / z)
    # lp_dir is lp_rows' second output with eta r in the place of out1
    assert _close(ref.lp_dir(0.2, 0.9, x, z, rd, elp)[0], (0.2 - x * z - 0.9 * x * rd - elp) / z)
    assert _close(ref.gemv_t(D, m1 - 1, vlp, 0.5, v[:m1 - 1])[0], (D.T @ vlp)[:m1 - 1] + 0.5 * v[:m1 - 1])
    assert _close(ref.gemv_n(D, m1 - 1, np.stack([v[:m1 - 1], v[1:]]))[0], np.stack([D[:, :m1 - 1] @ v[:m1 - 1], D[:, :m1 - 1] @ v[1:]]))
    assert _close(ref.make_ext(1.0, -2.0, v)[0], np.r_[1.0, -2.0 * v]) and _close(ref.axpy(0.5, v, 2 * v)[0], 2.5 * v)
    # the reductions
    a, b, cc = rng.standard_normal(q), rng.standard_normal(q), rng.standard_normal(q)
    assert _close(ref.reduction(0, a, b, cc)[0], np.einsum("i,i->", a, b))
    assert ref.reduction(1, a, b, cc)[0] == np.abs(a).max()
    assert ref.reduction(2, a, b, cc)[0] == min(-a[i] / b[i] for i in range(q) if b[i] < 0)
    assert ref.reduction(2, a, np.abs(b), cc)[0] == 1e300
    assert _close(ref.reduction(3, x, z, cc)[0], sum(x[i] / z[i] * cc[i] ** 2 for i in range(q)))
    assert ref.combine(1, 3.0, 2.0) == 3.0 and ref.combine(2, 3.0, 2.0) == 2.0 and ref.combine(0, 3.0, 2.0) == 5.0


def test_group_rule_of_the_reductions(K):
    assert spc._red_groups(K, (5, 5, 5, 5, 5), (0, 1, 2, 3, 4)) == [4, 1]
    assert spc._red_groups(K, (5, 5), (0, 0)) == [1, 1]
    assert spc._red_groups(K, (5, 1025, 5, 5), (0, 1, 2, 3)) == [1, 1, 2]
    assert spc.gemvn_plan(37, 16384, 16384, 1, 0, 74) == (2, True, [8192, 8192])
    assert spc.gemvn_plan(37, 16384, 16384, 1, 0, 73)[0] == 1
