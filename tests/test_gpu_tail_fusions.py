"""The merged launches between two Schur assemblies on the general path (scip-sdp_amd/csrc/ipm.hip: general_tail), each
against the launches it replaces, on random inputs, bit for bit - through the hipsdp_tail_*_unit entries (include/hipsdp_units.h).

Sizes: m = 1, 63, 65, 255, 257, 1000 and n = 65, 130, 500 - the edges of the 256-thread workgroups, of the m <= 64 branch, and of the
vectors a batch of deferred reductions records (16 384 entries: the dots over n^2 = 4225 entries are recorded whole, those over 16 900
and 250 000 have their first stage launched and their second stage recorded, 9 and 123 partial sums).

  1 k_after_solve2 + hs_make_ext twice                 -> one launch: u2, wt, [1; u2], [0; u1]
  2 hs_unpack_sym three times (the three-vector sweep) -> one launch
  3 hs_unpack_sym + k_dz_combine (the corrector's dZ)  -> one launch
  4 hs_dirmat + hs_pack_weighted of its result         -> one launch: H and its packed, weighted copy
  5 the scalars of a direction and its closing kernel (fill, two stages of <B, H>, the dots over m, k_finish_dir: five launches)
    -> the first stage + one batch launch: the whole scalar block, dy and dyt
  6 the reductions of the solves with M and of the residual pass (several long dots into one slot and into slots of their own, a dot
    over m): hs_dot against hs_dot_deferred inside one batch"""
import numpy as np
import pytest

from chol_cases import same_bits

pytestmark = pytest.mark.gpu

MS = (1, 63, 65, 255, 257, 1000)
NS = (65, 130, 500)


def _mixed(rng, shape):
    """normal values over twelve decades: the roundings of a sum depend on every term"""
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 7, shape)


def _packed_len(n):
    t = n * (n + 1) // 2
    return t + (t & 1)


@pytest.mark.parametrize("m", MS)
def test_after_solve2_with_the_coefficient_vectors(gpu, m):
    bad = []
    rng = np.random.default_rng([m, 1])
    rhs2, u1 = _mixed(rng, 2 * m), _mixed(rng, m)
    ref = gpu.tail_after_solve2_unit(rhs2, u1, fused=False)
    got = gpu.tail_after_solve2_unit(rhs2, u1, fused=True)
    for nm, a, b in zip(("u2", "wt", "[1; u2]", "[0; u1]"), got, ref):
        same_bits("m=%d %s" % (m, nm), a, b, bad)
    assert np.array_equal(ref[0], rhs2[m:] - rhs2[:m]) and ref[2][0] == 1.0 and ref[3][0] == 0.0 and np.array_equal(ref[3][1:], u1)
    assert not bad, bad


@pytest.mark.parametrize("n", NS)
def test_three_unpacks_in_one_launch(gpu, n):
    bad = []
    rng = np.random.default_rng([n, 2])
    pk = _mixed(rng, (3, _packed_len(n)))
    ref = gpu.tail_unpack3_unit(pk, n, fused=False)
    got = gpu.tail_unpack3_unit(pk, n, fused=True)
    same_bits("n=%d unpacked" % n, got, ref, bad)
    r, c = np.tril_indices(n)
    assert np.array_equal(ref[1][r, c], pk[1][r * (r + 1) // 2 + c]) and np.array_equal(ref[2], ref[2].T)
    assert not bad, bad


@pytest.mark.parametrize("n", NS)
def test_unpack_and_dz_combine_in_one_launch(gpu, n):
    bad = []
    rng = np.random.default_rng([n, 3])
    pk, P2, Rd = _mixed(rng, _packed_len(n)), _mixed(rng, (n, n)), _mixed(rng, (n, n))
    for dtau, eta in ((-0.731, 0.9), (3.0e-7, 1.0), (12.5, 1e-8)):
        ref = gpu.tail_dz_unit(pk, P2, Rd, dtau, eta, fused=False)
        got = gpu.tail_dz_unit(pk, P2, Rd, dtau, eta, fused=True)
        same_bits("n=%d dtau=%g eta=%g dZ" % (n, dtau, eta), got, ref, bad)
        assert np.all(np.isfinite(ref))
    assert not bad, bad


@pytest.mark.parametrize("n", NS)
def test_dirmat_with_its_packed_copy(gpu, n):
    bad = []
    rng = np.random.default_rng([n, 4])
    Zinv, X, GZ = _mixed(rng, (n, n)), _mixed(rng, (n, n)), _mixed(rng, (n, n))
    for s1 in (0.0, 0.37, 4.2e-9):
        Hr, pr = gpu.tail_dirmat_unit(s1, Zinv, X, GZ, fused=False)
        Hg, pg = gpu.tail_dirmat_unit(s1, Zinv, X, GZ, fused=True)
        same_bits("n=%d s1=%g H" % (n, s1), Hg, Hr, bad)
        same_bits("n=%d s1=%g packed copy" % (n, s1), pg, pr, bad)        # (the padding entry of an odd length is NaN on both sides)
        r, c = np.tril_indices(n)
        assert np.array_equal(pr[r * (r + 1) // 2 + c], np.where(r == c, 1.0, 2.0) * Hr[r, c])
    assert not bad, bad


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_direction_scalars_and_closing_kernel(gpu, m, n):
    bad = []
    rng = np.random.default_rng([m, n, 5])
    B, H = _mixed(rng, (n, n)), _mixed(rng, (n, n))
    rhs2, rp, b, u1, u2 = (_mixed(rng, m) for _ in range(5))
    par = np.array([0.73, -0.021, 3.1e-3, 0.88, 0.052, 1.7e-4])           # eta, rg, sigmu, tau, kappa, etk
    sc = rng.standard_normal(gpu.tail_sc_len())                            # S0, b^T M^-1 b and every slot the run leaves alone
    ref = gpu.tail_dir_unit(B, H, rhs2, rp, b, u1, u2, par, sc, fused=False)
    got = gpu.tail_dir_unit(B, H, rhs2, rp, b, u1, u2, par, sc, fused=True)
    for nm, a, r in zip(("scalar block", "dy", "dyt"), got, ref):
        same_bits("m=%d n=%d %s" % (m, n, nm), a, r, bad)
    assert np.all(np.isfinite(ref[1])) and np.array_equal(ref[2][1:], ref[1]) and np.sum(ref[0] != sc) >= 6
    assert not bad, bad


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_deferred_dots_of_a_batch(gpu, m, n):
    bad = []
    rng = np.random.default_rng([m, n, 6])
    a, v = _mixed(rng, (3, n * n)), _mixed(rng, (2, m))
    ref = gpu.tail_dots_unit(a, v, fused=False)
    got = gpu.tail_dots_unit(a, v, fused=True)
    same_bits("m=%d n=%d sums" % (m, n), got, ref, bad)
    exact = np.array([float(np.dot(a[0].astype(np.longdouble), (a[1] + a[2]).astype(np.longdouble))),
                      float(np.dot(a[2].astype(np.longdouble), a[2].astype(np.longdouble))),
                      float(np.dot(v[0].astype(np.longdouble), v[1].astype(np.longdouble)))])
    scale = np.array([np.abs(a[0]) @ (np.abs(a[1]) + np.abs(a[2])), a[2] @ a[2], np.abs(v[0]) @ np.abs(v[1])])
    print("m=%d n=%d: sums against extended precision, relative to sum |.|: %s" % (m, n, np.abs(ref - exact) / scale))
    assert np.all(np.abs(ref - exact) <= 1e-12 * scale)
    assert not bad, bad
