"""The references of tests/test_gpu_schur_forms.py held alone to everything the GPU tests assume of them (tests/harness/schur_cases.py):
the 2^53 premise of the exact family, float64 numpy against integer arithmetic, float64 numpy in two summation orders against the
extended-precision reference of the iterate family, and the restated sharding and dispatch rules."""
import ctypes as C
import numpy as np
import pytest

import schur_cases as sc
import shard_ref

ALL_EXACT = sorted(set(sc.LADDER + [s[:2] for s in sc.FORM1 + sc.FORM2 + sc.FORM4] + sc.FORM3))


@pytest.mark.parametrize("m1,n", ALL_EXACT, ids=["%dx%d" % s for s in ALL_EXACT])
def test_exact_premise_every_partial_sum_is_an_integer_below_2_to_53(m1, n):
    A, R, G, X, Zi = sc.exact(m1, n)
    assert set(np.unique(A)) <= {-1.0, 0.0, 1.0} and np.array_equal(A, A.transpose(0, 2, 1))
    for L in (R, G):
        assert set(np.unique(L)) <= {-1.0, 0.0, 1.0} and np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) != 0)
    assert np.array_equal(X, X.T) and np.array_equal(Zi, Zi.T)
    p = sc.exact_premise(m1, n)
    print("(m1, n) = (%d, %d): largest entry of the abs-value chains %.3e = 2^%.1f" % (m1, n, p, np.log2(max(p, 1))))
    assert p < 2.0 ** 53
    # both formulations give the same integers in float64
    if m1 * n * n <= 2000000:
        assert np.array_equal(sc.u_matrix(A, X, Zi), sc.exact_ref(m1, n))


@pytest.mark.parametrize("m1,ns,q", sc.SMALL + sc.SMALL_REFUSED + [sc.SMALL_EDGE_TAKEN], ids=lambda v: str(v).replace(" ", ""))
def test_exact_small_premise_and_admission(m1, ns, q):
    As, Xs, Zs, D, x, z = sc.exact_small(m1, ns, q)
    assert sc.exact_small_premise(m1, ns, q) < 2.0 ** 53
    if q:
        assert np.array_equal(x / z, np.round(x / z)) and np.all(np.log2(z) == np.round(np.log2(z)))
    assert sc.small_admitted(m1, ns, q) == ((m1, ns, q) not in sc.SMALL_REFUSED)
    # float64 numpy against Python integers
    if m1 <= 13:
        M = sc.small_matrix(As, Xs, Zs, D, x, z)
        ref = np.zeros((m1, m1), dtype=object)
        for A, X, Zi in zip(As, Xs, Zs):
            Ai, Xi, Zii = (a.astype(np.int64).astype(object) for a in (A, X, Zi))
            U = [Xi @ (a @ Zii) for a in Ai]
            ref += np.array([[np.sum(Ai[i] * U[j]) for j in range(m1)] for i in range(m1)], dtype=object)
        if q:
            Di, w = D.astype(np.int64).astype(object), (x / z).astype(np.int64).astype(object)
            ref += Di.T @ (w[:, None] * Di)
        assert all(int(M[i, j]) == ref[i, j] and M[i, j] == int(M[i, j]) for i in range(m1) for j in range(m1))


@pytest.mark.parametrize("m1,n", [(20, 24), (9, 17), (41, 20), (33, 130)])
def test_float64_numpy_equals_int64_arithmetic_on_exact_cases(m1, n):
    A, R, G, X, Zi = (a.astype(np.int64) for a in sc.exact(m1, n))
    assert np.array_equal(R @ R.T, X) and np.array_equal(G.T @ G, Zi)
    W = np.matmul(G, np.matmul(A, R)).reshape(m1, -1)
    ref = W @ W.T
    U = np.matmul(X, np.matmul(A, Zi)).reshape(m1, -1)
    assert np.array_equal(A.reshape(m1, -1) @ U.T, ref)                  # tr(A_i X A_j Zinv) in both formulations
    assert np.array_equal(sc.exact_ref(m1, n).astype(np.int64), ref) and np.array_equal(sc.exact_ref(m1, n), ref.astype(np.float64))
    # the strictly sequential float64 loops of the iterate family are the same sums: the same bits here
    Af, Rf, Gf, Xf, Zf = sc.exact(m1, n)
    assert np.array_equal(sc.w_matrix_seq(Af, Rf, Gf), sc.exact_ref(m1, n)) and np.array_equal(sc.u_matrix_seq(Af, Xf, Zf), sc.exact_ref(m1, n))


@pytest.mark.parametrize("m1,n", sc.ITERATE, ids=["%dx%d" % s for s in sc.ITERATE])
def test_iterate_references_hold_float64_numpy_in_two_orders(m1, n):
    """F of float64 numpy (BLAS order) and of a strictly sequential float64 accumulation over k of the same three products: both below
    the worst-case bound (asserted), and the sequential one against the margin (10 x) the GPU test grants the device over numpy.

    That last comparison is an expected-value RECORD, not an assertion.  The sequential loops are correct - on the exact family they
    give numpy's bits (test_float64_numpy_equals_int64_arithmetic_on_exact_cases) - yet they miss the margin, in the U formulation by a
    few per cent from n = 33 on and in both at the longest sums: with OpenBLAS (AVX-512 kernels, 1 to 64 threads:
    the figures do not move) numpy's F at n = 130 is 5.8e-4 .. 8.6e-4 (W) and 4.8e-3 .. 1.1e-2 (U), the sequential order's 3.7e-3 ..
    6.3e-3 and 8.1e-2 .. 2.4e-1: ratios up to 10.6 (W, cond 1e8) and 21.5 (U, cond 1e4).  Up to n = 65 the W ratios are 0.8 .. 4.7 and
    the U ratios 2.5 .. 10.7.  One chain of K = n^2 additions against BLAS's dozens of interleaved partial sums is a factor of about
    sqrt(32) in the random-walk estimate, and the maximum over m1^2 entries scatters around it; a device kernel sums in MFMA steps of
    4, K blocks and split-K slabs, which is BLAS's side of that comparison.  Every figure is six decades below where a lost term shows
    (asserted at the end)."""
    if not sc.longdouble_ok():
        pytest.skip("numpy.longdouble has no 64-bit mantissa here: no reference for the iterate family")
    bad = []
    for cond in sc.CONDS:
        A, R, G, X, Zi = sc.iterate(m1, n, cond)
        assert np.all(np.triu(R, 1) == 0) and np.all(np.triu(G, 1) == 0) and np.array_equal(X, X.T) and np.array_equal(Zi, Zi.T)
        Mw, Bw, Mu, Bu = sc.iterate_ref(m1, n, cond)
        # the pair is what the family claims: complementary to the rounding of a condition-cond factorisation, graded entries
        mu = cond ** -0.5
        assert np.max(np.abs(R @ R.T @ np.linalg.inv(G.T @ G) - mu * np.eye(n))) <= 1e-3 * mu
        sm = np.abs(np.asarray(Mw, dtype=np.float64))
        print("n=%d cond=%.0e: |M| from %.2e to %.2e of the largest" % (n, cond, sm.min() / sm.max(), 1.0))
        fw, fu = sc.numpy_figures(m1, n, cond)
        fws = sc.figure(sc.w_matrix_seq(A, R, G), Mw, Bw)
        fus = sc.figure(sc.u_matrix_seq(A, X, Zi), Mu, Bu)
        what = "n=%d m1=%d cond=%.0e" % (n, m1, cond)
        sc.check("cpu numpy W / cap", what, fw, sc.cap(n), bad=bad)
        sc.check("cpu numpy U / cap", what, fu, sc.cap(n), bad=bad)
        sc.check("cpu sequential W / cap", what, fws, sc.cap(n), bad=bad)
        sc.check("cpu sequential U / cap", what, fus, sc.cap(n), bad=bad)
        sc.check("cpu sequential W / numpy", what, fws, sc.MARGIN * fw, ref=fw, bad=bad, asserted=False)
        sc.check("cpu sequential U / numpy", what, fus, sc.MARGIN * fu, ref=fu, bad=bad, asserted=False)
        # the figure sees one lost term: drop the largest term of one entry's last sum
        Wd = sc.w_matrix(A, R, G)
        T = np.matmul(G, np.matmul(A, R)).reshape(m1, -1)
        Wd[0, 0] -= np.max(T[0] * T[0])
        assert sc.figure(Wd, Mw, Bw) > 1e3 * sc.cap(n)
    assert not bad, bad


def test_scaling_is_exact_in_float64():
    k, s = sc.scaling(33)
    assert k.min() >= -10 and k.max() <= 10 and np.array_equal(s, 2.0 ** k) and len(set(k)) > 5
    A, R, G, X, Zi = sc.iterate(9, 17, 1e8)
    k, s = sc.scaling(9)
    for M0, M1 in ((sc.w_matrix_seq(A, R, G), sc.w_matrix_seq(A * s[:, None, None], R, G)),
                   (sc.u_matrix_seq(A, X, Zi), sc.u_matrix_seq(A * s[:, None, None], X, Zi))):
        assert np.array_equal(M1, M0 * s[:, None] * s[None, :])


def test_restated_sharding_agrees_with_the_distributed_tests(hb):
    """the slices and chunks the harness predicts are those of oracle/shard_ref.py (what tests/test_dist_cpu.py checks against the
    engine's host code, asked here as well), and they cover every column and every row once"""
    lib = hb.lib()
    for m1, n, parts in sc.FORM1 + [(120, 300, 64), (9, 1, 5), (9, 2, 3)]:
        sl = sc.col_slices(m1, n, parts)
        b = (C.c_int * (parts + 1))()
        assert lib.hipsdp_shard_columns(m1, n, parts, b) == 0
        assert [(b[g], b[g + 1] - b[g]) for g in range(parts)] == sl
        assert list(b) == shard_ref.shard_cols(m1, n, parts)
        assert sl[0][0] == 0 and all(a[0] + a[1] == c[0] for a, c in zip(sl, sl[1:])) and sl[-1][0] + sl[-1][1] == n
    widths = [cw for _, cw in sc.col_slices(*sc.FORM1[0])]
    assert len(set(widths)) > 1 and 0 < max(widths) <= 64                               # uneven and narrow
    assert 0 in [cw for _, cw in sc.col_slices(*sc.FORM1[1])]                           # empty slices
    assert max(cw for _, cw in sc.col_slices(*sc.FORM1[2])) > 64                        # 128-wide tiles
    for m1, n, parts in sc.FORM2 + [(5, 3, 8), (1, 4, 1)]:
        seen = np.zeros(m1, dtype=int)
        for g in range(parts):
            c, b1, b2 = shard_ref.shard_rows(m1, parts, g)
            assert sc.row_chunks(m1, parts)[2 * g:2 * g + 2] == [(b1, min(b1 + c, m1)), (b2, min(b2 + c, m1))]
        for r0, r1 in sc.row_chunks(m1, parts):
            seen[r0:max(r0, r1)] += 1
        assert np.all(seen == 1)


def test_restated_dispatch_on_the_shapes_of_the_ladder():
    """the rungs the shapes were chosen for, as the restated rules give them without a Gram plan and with one"""
    no, yes = (lambda M, K: False), (lambda M, K: True)
    assert sc.predict_used(0, 20, 24) == (0, 0, 0) and sc.predict_used(0, 9, 17) == (0, 0, 0)
    assert sc.predict_used(0, 192, 131) == (0, 0, 0)                    # odd n
    assert sc.predict_used(0, 192, 130) == (2, 2, 0)                    # both triangular products on the paired-band kernel
    assert sc.predict_used(0, 300, 140, has_plan=no)[:2] == (2, 2) and sc.predict_used(0, 300, 140, has_plan=yes) == (2, 2, 1)
    assert sc.predict_used(0, 401, 300, has_plan=yes) == (2, 2, 1)
    assert sc.predict_used(0, 401, 300, has_plan=no) == (3, 2, 0)       # 10 tiles in XCD-walked slices: the persistent tile kernel
    assert sc.predict_used(2, 150, 64, parts=2)[1:] == (0, 0)
    for m1, n, parts in sc.FORM4:
        assert sc.predict_used(4, m1, n, parts=parts) == (0, 0, 0)
    assert sc.pick_splitk(192, 192, 16900, 1) == 64 and sc.pick_splitk(4000, 4000, 250000, 0) == 1
