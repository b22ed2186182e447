"""GPU: the kernels of csrc/sparse.hip entry by entry against extended-precision references (tests/sparse_kernel_cases.py), under the
bound 2 K u S that module derives - nothing here is a measured tolerance.

hipsdp_schur_sparse_unit2 runs k_sp_trows and then, by the caller's choice, k_sp_schur_t (one thread per pair of variables) or
k_sp_schur (one wavefront per pair, 64-lane split of the entries, six-step shuffle sum): both kernels see every family, whatever
hs_sp_schur's rule (fewer than 24 full entries per matrix on average: one thread) would pick, and the rule itself is restated.
hipsdp_sparse_ops_unit runs k_sp_apply (<A_v, V>) and k_sp_apply_t (base + sum coef_v A_v).  Where the exact result is a structural
zero (a variable that does not occur in the block, a position no triplet touches) the device must return exactly 0.0 / the bits of
base.  All three operations promise the same bits whatever the order of the caller's triplets (the header of sparse.hip: the copies
of an SPMD run agree to the last bit), so that is demanded too.

Grid-stride loops: the ones of k_sp_apply (cap 4096 workgroups of 4 wavefronts), k_sp_apply_t (4096 x 256 threads) and k_sp_schur
(65536 x 4 wavefronts) are entered below.  The one of k_sp_schur_t (65536 x 256 threads) needs m >= 5793 variables and a result of
268 MB: it is deliberately left out."""
import functools
import numpy as np
import pytest

import ipm_ref
import sparse_kernel_cases as skc

pytestmark = pytest.mark.gpu

LD = skc.LD


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(dev, ref, bound, what):
    """prints the worst error in units of the bound, then asserts"""
    err = np.abs(dev.astype(LD) - ref).astype(np.float64)
    worst = float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))
    exact = bool(np.all(err[bound == 0] == 0.0))
    print("%s: worst |device - ref| / bound = %.3g over %d results" % (what, worst, err.size))
    assert np.all(np.isfinite(dev)), what
    assert exact, what + ": a result whose magnitude S is zero is not exactly the reference"
    assert np.all(err <= bound), (what, worst)


@functools.lru_cache(maxsize=None)
def _schur_reference(name, kind):
    n, m, coo = skc.case(name)
    X, Zi = skc.schur_operands(n, kind)
    ref, S = skc.schur_ref(n, m, coo, X, Zi)
    bound = skc.schur_bound(n, m, coo, S)
    for a in (ref, bound):
        a.flags.writeable = False
    return ref, bound


def _schur_checked(gpu, name, kind, kernel):
    """(lower triangle m x m of the device result, took) after the checks every call must pass: the kernel is the forced one, row and
    column 0 and the upper triangle are untouched"""
    n, m, coo = skc.case(name)
    X, Zi = skc.schur_operands(n, kind)
    Mx, took = gpu.schur_sparse_unit2(n, m, coo, X, Zi, kernel=kernel)
    if kernel >= 0:
        assert took == kernel
    assert np.all(_bits(Mx[0, :]) == 0) and np.all(_bits(Mx[:, 0]) == 0)
    assert np.all(_bits(Mx[np.triu_indices(m + 1, 1)]) == 0)
    return Mx[1:, 1:], took


@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("name", skc.NAMES)
def test_schur_entries_of_both_kernels_against_the_reference(gpu, name, kind):
    n, m, coo = skc.case(name)
    ref, bound = _schur_reference(name, kind)
    il = np.tril_indices(m)
    zero = skc.schur_structural_zero(n, m, coo)[il]
    M = {}
    for kernel in (0, 1):
        M[kernel], _ = _schur_checked(gpu, name, kind, kernel)
        _check(M[kernel][il], ref[il], bound[il], "%s/%s kernel %d" % (name, kind, kernel))
        assert np.all(M[kernel][il][zero] == 0.0)          # a variable that does not occur in the block: exactly zero
    # the two kernels sum the entries of A_i in different orders: apart by at most the two bounds
    assert np.all(np.abs(M[0][il] - M[1][il]) <= 2.0 * bound[il])
    # the engine's rule, restated from the deduplicated list, and its result: the bits of the forced call of that kernel
    Ma, took = _schur_checked(gpu, name, kind, -1)
    assert took == skc.rule_kernel(n, m, coo) == skc.intended_kernel(name)
    assert np.array_equal(_bits(Ma), _bits(M[took]))
    X, Zi = skc.schur_operands(n, kind)
    assert np.array_equal(_bits(gpu.schur_sparse_unit(n, m, coo, X, Zi)[1:, 1:]), _bits(Ma))       # hs_sp_schur as the engine calls it


@pytest.mark.parametrize("name", skc.NAMES)
def test_apply_A_against_the_reference(gpu, name):
    n, m, coo = skc.case(name)
    Vs, Vn, coef, base, zero = skc.pass_operands(n, m)
    empty = skc.counts(n, m, coo)[0] == 0
    for tag, V in (("symmetric V", Vs), ("non-symmetric V", Vn)):
        ref, S = skc.apply_ref(n, m, coo, V)
        out, _ = gpu.sparse_ops_unit(n, m, coo, V=V)
        _check(out, ref, skc.apply_bound(n, m, coo, S), "%s A(V), %s" % (name, tag))
        assert np.all(_bits(out[empty]) == 0)               # a variable that does not occur in the block: exactly zero


@pytest.mark.parametrize("name", skc.NAMES)
def test_apply_AT_against_the_reference(gpu, name):
    n, m, coo = skc.case(name)
    Vs, Vn, coef, base, zero = skc.pass_operands(n, m)
    untouched = skc.position_counts(n, m, coo) == 0
    for tag, b in (("random base", base), ("zero base", zero)):
        ref, S = skc.apply_t_ref(n, m, coo, coef, b)
        _, out = gpu.sparse_ops_unit(n, m, coo, coef=coef, base=b)
        _check(out, ref, skc.apply_t_bound(n, m, coo, S), "%s A^T(coef), %s" % (name, tag))
        assert np.array_equal(_bits(out[untouched]), _bits(b[untouched]))            # positions no triplet touches: the bits of base
        if b is zero:
            assert np.array_equal(_bits(out), _bits(out.T))                          # both triangles get the same sum
        # coef[0] belongs to the constant matrix (k_sp_base): the sparse pass must not read it into the result
        c2 = coef.copy(); c2[0] = -17.0
        assert np.array_equal(_bits(gpu.sparse_ops_unit(n, m, coo, coef=c2, base=b)[1]), _bits(out))


def _all_three(gpu, n, m, coo):
    X, Zi = skc.schur_operands(n, "ill")
    Vs, Vn, coef, base, zero = skc.pass_operands(n, m)
    outA, outAT = gpu.sparse_ops_unit(n, m, coo, V=Vn, coef=coef, base=base)
    return [_bits(gpu.schur_sparse_unit2(n, m, coo, X, Zi, kernel=0)[0]), _bits(gpu.schur_sparse_unit2(n, m, coo, X, Zi, kernel=1)[0]),
            _bits(outA), _bits(outAT)]


@pytest.mark.parametrize("name", skc.NAMES)
def test_bits_do_not_depend_on_the_call_or_the_order_of_the_triplets(gpu, name):
    n, m, coo = skc.case(name)
    cl = skc.clean(n, m, coo)
    first = _all_three(gpu, n, m, cl)
    for other in (_all_three(gpu, n, m, cl), _all_three(gpu, n, m, skc.shuffled(cl)), _all_three(gpu, n, m, skc.shuffled(cl, seed=8))):
        for a, b in zip(first, other):
            assert np.array_equal(a, b)
    if name == "messy_input":
        # either triangle, duplicates (the last one counts): the bits of the cleaned list
        assert len(coo[3]) > len(cl[3])
        for a, b in zip(first, _all_three(gpu, n, m, coo)):
            assert np.array_equal(a, b)


# ---- the grid-stride loops -----------------------------------------------------------------------------------------------------------

def test_apply_A_beyond_4096_workgroups(gpu):
    """m = 16 500 variables of one or two entries in an 8 x 8 block: more than 4096 x 4 wavefronts, so the first 116 wavefronts take a
    second variable"""
    rng = np.random.default_rng(60)
    n, m = 8, 16500
    two = rng.random(m) < 0.5
    var = np.concatenate([np.arange(1, m + 1), np.flatnonzero(two) + 1]).astype(np.int32)
    ii, jj = np.tril_indices(n)
    p1 = rng.integers(0, len(ii), m)
    p2 = (p1[two] + rng.integers(1, len(ii), int(two.sum()))) % len(ii)                   # another position of the same variable
    pos = np.concatenate([p1, p2])
    row, col = ii[pos].astype(np.int32), jj[pos].astype(np.int32)
    val = rng.standard_normal(len(var))
    V = rng.standard_normal((n, n))
    Vl = V.astype(LD)
    w = np.where(row != col, Vl[row, col] + Vl[col, row], Vl[row, col])
    ref = np.zeros(m, dtype=LD); S = np.zeros(m, dtype=LD)
    np.add.at(ref, var - 1, val.astype(LD) * w)
    np.add.at(S, var - 1, np.abs(val).astype(LD) * np.where(row != col, np.abs(Vl[row, col]) + np.abs(Vl[col, row]), np.abs(Vl[row, col])))
    K = np.bincount(var - 1, minlength=m) + 7
    out, _ = gpu.sparse_ops_unit(n, m, (var, row, col, val), V=V)
    _check(out, ref, 2.0 * K * skc.U * S.astype(np.float64) * (1.0 + 2.0 ** -40), "A(V), m = 16500")
    assert np.all(out[16384:] != 0.0)


def test_apply_AT_beyond_4096_workgroups(gpu):
    """n = 1450, m = 2, both variables on all 1 051 975 lower positions: more than 4096 x 256 threads"""
    rng = np.random.default_rng(61)
    n, m = 1450, 2
    ii, jj = np.tril_indices(n)
    L = len(ii)
    assert L == 1051975 > 4096 * 256
    var = np.repeat(np.array([1, 2], dtype=np.int32), L)
    row = np.tile(ii, 2).astype(np.int32); col = np.tile(jj, 2).astype(np.int32)
    val = rng.standard_normal(2 * L)
    coef = np.array([5.0, 0.75, -1.5])
    base = rng.standard_normal((n, n))
    _, out = gpu.sparse_ops_unit(n, m, (var, row, col, val), coef=coef, base=base)
    T = np.zeros((n, n), dtype=LD); Sa = np.zeros((n, n), dtype=LD)
    for v in (1, 2):
        A = np.zeros((n, n), dtype=LD)
        A[ii, jj] = val[(v - 1) * L:v * L]
        A[jj, ii] = val[(v - 1) * L:v * L]
        T += LD(coef[v]) * A
        Sa += np.abs(LD(coef[v]) * A)
    ref = base.astype(LD) + T
    S = np.abs(base).astype(LD) + Sa
    _check(out, ref, 2.0 * 3 * skc.U * S.astype(np.float64) * (1.0 + 2.0 ** -40), "A^T(coef), n = 1450")


def test_wavefront_schur_kernel_beyond_65536_workgroups(gpu):
    """k_sp_schur forced on m = 730 matrices of 13 lower entries, n = 70: 266 815 pairs, more than 65536 x 4 wavefronts.  The full
    matrix against the float64 dense formula on the expansion (at twice the bound: that formula has a rounding error of its own),
    2000 pairs - the last ones and the ones either side of the stride among them - against the extended-precision reference"""
    n, m, k = 70, 730, 13
    n_, m_, coo = skc.uniform(n, m, k, seed=62)
    npairs = m * (m + 1) // 2
    assert npairs == 266815 > 65536 * 4
    X, Zi = skc.schur_operands(n, "well")
    Mx, took = gpu.schur_sparse_unit2(n, m, coo, X, Zi, kernel=1)
    assert took == 1
    M = Mx[1:, 1:]
    il = np.tril_indices(m)
    A = np.zeros((m + 1, n, n))
    A[1:] = skc.expand(n, m, coo, dtype=np.float64)
    Md = ipm_ref.schur_block(A, X, Zi)[1:, 1:]
    Sd = ipm_ref.schur_block(np.abs(A), np.abs(X), np.abs(Zi))[1:, 1:]
    Kmat = skc.schur_K(n, m, coo)
    bound = 2.0 * Kmat * skc.U * Sd * (1.0 + 1e-9)                         # (S itself from float64 products)
    _check(M[il], Md[il].astype(LD), 2.0 * bound[il], "k_sp_schur, 266815 pairs, against the dense formula")
    assert np.all(_bits(Mx[np.triu_indices(m + 1, 1)]) == 0) and np.all(_bits(Mx[:, 0]) == 0)
    rng = np.random.default_rng(63)
    pr = np.unique(np.concatenate([rng.integers(0, npairs, 1500), npairs - 1 - rng.integers(0, 5000, 700),
                                   np.array([0, 65536 * 4 - 1, 65536 * 4, 65536 * 4 + 1, npairs - 4, npairs - 3, npairs - 2, npairs - 1])]))
    assert len(pr) >= 2000 and np.sum(pr >= npairs - 5000) >= 500
    i = ((np.sqrt(8.0 * pr + 1.0) - 1.0) / 2.0).astype(np.int64)
    i = np.where((i + 1) * (i + 2) // 2 <= pr, i + 1, i)
    i = np.where(i * (i + 1) // 2 > pr, i - 1, i)
    j = pr - i * (i + 1) // 2
    assert np.all((0 <= j) & (j <= i) & (i < m))
    ref, S = skc.schur_ref_pairs(n, m, coo, X, Zi, list(zip(i.tolist(), j.tolist())))
    _check(M[i, j], ref, 2.0 * Kmat[i, j] * skc.U * S.astype(np.float64) * (1.0 + 2.0 ** -40), "k_sp_schur, %d sampled pairs" % len(pr))
