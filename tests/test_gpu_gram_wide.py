"""The wide instance of the Gram kernel (scip-sdp_amd/csrc/gram.hip: hs_gram_kernel<1> - tile rows of 256 on eight wavefronts, one
workgroup per CU; an off-diagonal item is a column half of a tile, 256 x 128, a diagonal item the lower triangle of 256 x 256 with
seventeen accumulators per wavefront), forced through hipsdp_gram_product_unit (the caller's W, alpha, beta and leading dimension) and,
once, through hipsdp_schur_form_unit with the hook hipsdp_gram_instance_force set.

C (lower triangle) = alpha W W^T + beta C, W m1 x K.  Shapes: m1 = 255 (one ragged diagonal tile), 256 (one diagonal tile exactly), 257
(a second tile row of ONE valid row), 300, 513 (three tile rows, the third ragged: both column halves of an off-diagonal tile and a
diagonal tile of one row); K = 24 (three stages: fewer than the ring of four holds), 36 (no multiple of the stage's 8), 256, 4100
(several K slices per tile, summed by the second kernel).

  figure  random operands in [-0.5, 0.5): F = max over the lower triangle of |C - C_ref| / (eps B), C_ref in extended precision on the
          operands handed to the device, B = |alpha| |W| |W|^T + |beta| |C_0| the abs-value chain that bounds every partial sum; the
          device's F against 10 x the F of float64 numpy on the same case (figure and margin of tests/test_gpu_schur_forms.py).  Two
          runs must give the same bits.
  exact   entries in {-2 .. 2}: every partial sum is an integer of at most 4 K <= 16400, so the wide instance, the 128 x 128 instance
          and numpy must agree bit for bit.  C starts as a sentinel everywhere (beta = 0): the lower triangle must be written
          completely, and nothing above the diagonal may be touched.
The plan test needs no device: it reads the lists the host builds for either instance."""
import numpy as np
import pytest

import schur_cases as sc

gpu_test = pytest.mark.gpu

SENTINEL = -7.25e300
M1S = (255, 256, 257, 300, 513)
KS = (24, 36, 256, 4100)
SHAPES = [(m1, K) for m1 in M1S for K in KS]
IDS = ["%dx%d" % s for s in SHAPES]
XD = sc.XD

_CASES = {}


def _low(M):
    return np.tril_indices(M)


def xd_gram(W):
    """lower triangle of W W^T in extended precision, by row blocks (the upper triangle stays zero)"""
    M = W.shape[0]
    Wx = W.astype(XD)
    out = np.zeros((M, M), dtype=XD)
    for r0 in range(0, M, 128):
        r1 = min(r0 + 128, M)
        out[r0:r1, :r1] = Wx[r0:r1] @ Wx[:r1].T
    return out


def case(m1, K, fam, alpha=1.0, beta=0.0, ldw=None):
    """(W as handed to the device (m1 x ldw, NaN behind column K), C_0, and for the random family C_ref, B, numpy's F; for the exact
    family numpy's result), made once"""
    key = (m1, K, fam, alpha, beta, ldw)
    if key not in _CASES:
        rng = np.random.default_rng([m1, K, fam == "exact", int(alpha * 4), int(beta * 4)])
        ld = K if ldw is None else ldw
        W = np.full((m1, ld), np.nan)
        W[:, :K] = rng.integers(-2, 3, (m1, K)).astype(np.float64) if fam == "exact" else rng.random((m1, K)) - 0.5
        if beta == 0.0:
            C0 = np.full((m1, m1), SENTINEL)
            prior = np.zeros((m1, m1))
        else:
            C0 = rng.integers(-9, 10, (m1, m1)).astype(np.float64) if fam == "exact" else rng.random((m1, m1)) - 0.5
            prior = C0
        Wk = np.ascontiguousarray(W[:, :K])
        npy = alpha * (Wk @ Wk.T) + beta * prior
        out = {"W": W, "C0": C0, "numpy": npy}
        if fam != "exact":
            ref = XD(alpha) * xd_gram(Wk) + XD(beta) * prior.astype(XD)
            B = abs(alpha) * (np.abs(Wk) @ np.abs(Wk).T) + abs(beta) * np.abs(prior)
            out["ref"], out["B"] = ref, B
            out["numpy_F"] = low_figure(npy, ref, B)
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[key] = out
    return _CASES[key]


def low_figure(C, ref, B):
    i = _low(C.shape[0])
    return sc.figure(C[i], ref[i], B[i])


def run(gpu, c, K, mode, alpha=1.0, beta=0.0):
    """the product with the instance forced -> (C, counters); what lies above the diagonal must come back as it went in"""
    C, used = gpu.gram_product_unit(c["W"], K, mode, alpha=alpha, beta=beta, Cin=c["C0"])
    up = np.triu_indices(C.shape[0], 1)
    assert np.array_equal(C[up], c["C0"][up]), "written above the diagonal"
    return C, used


@gpu_test
@pytest.mark.parametrize("m1,K", SHAPES, ids=IDS)
def test_wide_instance_against_extended_precision(gpu, m1, K):
    assert sc.longdouble_ok()
    c = case(m1, K, "random")
    C, used = run(gpu, c, K, 1)
    C2, used2 = run(gpu, c, K, 1)
    assert used == used2 == (1, 1)
    assert not np.any(C[_low(m1)] == SENTINEL), "lower triangle not written completely"
    sc.check("gram wide", "m1 %d K %d" % (m1, K), low_figure(C, c["ref"], c["B"]), sc.MARGIN * c["numpy_F"], ref=c["numpy_F"])
    assert np.array_equal(C, C2), "two runs of the forced wide instance differ"


@gpu_test
@pytest.mark.parametrize("m1,K", SHAPES, ids=IDS)
def test_exact_operands_three_ways(gpu, m1, K):
    c = case(m1, K, "exact")
    Cw, uw = run(gpu, c, K, 1)
    Cn, un = run(gpu, c, K, 0)
    i = _low(m1)
    print("m1 %d K %d: counters wide %s narrow %s; wide == numpy %s, narrow == numpy %s" % (
        m1, K, uw, un, np.array_equal(Cw[i], c["numpy"][i]), np.array_equal(Cn[i], c["numpy"][i])))
    assert uw == (1, 1) and un == (1, 0)
    assert np.array_equal(Cw[i], c["numpy"][i]), sc.first_difference(np.tril(Cw), np.tril(c["numpy"]))
    assert np.array_equal(Cn[i], c["numpy"][i]), sc.first_difference(np.tril(Cn), np.tril(c["numpy"]))
    assert np.array_equal(Cw, Cn)


@gpu_test
@pytest.mark.parametrize("m1,K", [(257, 36), (300, 4100)], ids=["257x36", "300x4100"])
def test_alpha_beta_and_leading_dimension(gpu, m1, K):
    """the cold start's packed caller: alpha = 2, on top of what Mx holds (beta = 1), rows longer than K (NaN behind column K)"""
    ldw = K + 6
    e = case(m1, K, "exact", alpha=2.0, beta=1.0, ldw=ldw)
    Ce, ue = run(gpu, e, K, 1, alpha=2.0, beta=1.0)
    i = _low(m1)
    assert ue == (1, 1)
    assert np.array_equal(Ce[i], e["numpy"][i]), sc.first_difference(np.tril(Ce), np.tril(e["numpy"]))
    c = case(m1, K, "random", alpha=2.0, beta=1.0, ldw=ldw)
    C, used = run(gpu, c, K, 1, alpha=2.0, beta=1.0)
    assert used == (1, 1)
    sc.check("gram wide", "m1 %d K %d alpha 2 beta 1 ldw %d" % (m1, K, ldw), low_figure(C, c["ref"], c["B"]), sc.MARGIN * c["numpy_F"],
             ref=c["numpy_F"])


@gpu_test
def test_unforced_small_product_is_declined(gpu):
    """chosen per shape, neither instance takes a product below the kernel's size: the counters stay, C comes back whole"""
    c = case(300, 256, "exact")
    C, used = gpu.gram_product_unit(c["W"], 256, -1, Cin=c["C0"])
    assert used == (0, 0)
    assert np.all(C == SENTINEL)


@gpu_test
def test_assembly_with_the_wide_instance_forced(gpu):
    """hs_schur_W at m1 = 300, n = 140 (K = 19600, a shape the Gram kernel takes by itself) with the hook set: the Gram product runs on
    the wide instance, the counter of test_gpu_schur_forms.py counts it, and Mx equals numpy's bits (the exact family)"""
    m1, n = 300, 140
    assert sc.exact_premise(m1, n) < 2.0 ** 53
    A, R, G, _, _ = sc.exact(m1, n)
    got = {}
    try:
        for mode in (1, 0):
            w0 = gpu.gram_instance_force(mode)
            M, used = gpu.schur_form_unit(0, A, R, G)
            got[mode] = (M, used, gpu.gram_instance_force(mode) - w0)
    finally:
        gpu.gram_instance_force(-1)
    print("used (persistent, paired band, Gram), wide Gram products: wide", got[1][1:], "narrow", got[0][1:])
    assert got[1][1][2] == 1 and got[1][2] == 1
    assert got[0][1][2] == 1 and got[0][2] == 0
    assert np.array_equal(got[1][0], got[0][0])
    assert np.array_equal(got[1][0], sc.exact_ref(m1, n))


# ---- the plan, on the host ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inst", (0, 1), ids=("128", "wide"))
@pytest.mark.parametrize("K", (24, 250000))
@pytest.mark.parametrize("m1", (256, 257, 1001, 2001))
def test_plan_covers_the_lower_triangle_once(hb, inst, m1, K):
    u = hb.ulib()
    import ctypes as C
    for forced, nslab in ((1, 64), (1, 5), (0, 64)):
        info = (C.c_int * 4)()
        off = np.zeros(513, dtype=np.int32)
        items = np.zeros((8192, 6), dtype=np.int32)
        rc = u.hipsdp_gram_plan_unit(inst, forced, m1, C.c_longlong(K), nslab, items.shape[0], items.ctypes.data_as(C.POINTER(C.c_int)),
                                     off.ctypes.data_as(C.POINTER(C.c_int)), info)
        if not forced and rc != 0:
            continue                                    # chosen per shape, a product may have no plan: the tile kernels take it
        assert rc == 0, "a forced instance has a plan for every shape"
        nit, nwg, no, nd = info[0], info[1], info[2], info[3]
        assert nwg == (256 if inst else 512) and 0 < nit <= items.shape[0]
        assert 1 <= no <= nslab and 1 <= nd <= nslab, "more partial tiles than slabs granted"
        off = off[:nwg + 1]
        assert off[0] == 0 and off[-1] == nit and np.all(np.diff(off) >= 0)
        if not forced:
            assert np.all(np.diff(off) <= 1), "one item per workgroup by default"
        bt = 256 if inst else 128
        tm = -(-m1 // bt)
        tiles = {}
        for ti, tj, k0, k1, slab, half in items[:nit]:
            assert 0 <= tj <= ti < tm and half in ((0, 1) if inst and tj < ti else (0,))
            assert 0 <= k0 < k1 <= K, "empty item or outside K"
            assert 0 <= slab < (nd if ti == tj else no)
            tiles.setdefault((ti, tj, half), []).append((k0, k1, slab))
        want = [(ti, tj, h) for ti in range(tm) for tj in range(ti + 1) for h in range(2 if inst and tj < ti else 1)]
        assert sorted(tiles) == want
        for key, rs in tiles.items():
            rs.sort()
            assert len(rs) == (nd if key[0] == key[1] else no)
            assert rs[0][0] == 0 and rs[-1][1] == K and all(a[1] == b[0] for a, b in zip(rs, rs[1:])), "gap or overlap in K: %r" % (key,)
            assert sorted(r[2] for r in rs) == list(range(len(rs))), "two items of a tile share a slab"
        for w in range(nwg):                            # a workgroup walks its list in K order
            k0s = items[off[w]:off[w + 1], 2]
            assert np.all(np.diff(k0s) >= 0)
        print("inst %d m1 %d K %d forced %d slabs %d: %d items, %d / %d partial tiles" % (inst, m1, K, forced, nslab, nit, no, nd))
