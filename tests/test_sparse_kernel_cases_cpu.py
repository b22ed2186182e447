"""CPU: the inputs, references and bounds of tests/sparse_kernel_cases.py are sound before a GPU sees them.  For every family the
float64 restatements of the kernels of csrc/sparse.hip (ipm_ref.schur_rows_sparse for the Schur matrix, sparse_kernel_cases.apply_f64
and apply_t_f64 for the two passes) meet the extended-precision references under the derived bound 2 K u S, every family lands on the
side of hs_sp_schur's 24-entries rule it is meant for, and the two unit entries the GPU tests call are symbols of the units library
alone."""
import os
import re
import numpy as np
import pytest

import ipm_ref
import sparse_kernel_cases as skc
from conftest import ROOT

LD_TINY = np.longdouble(1e-300)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _within(dev, ref, bound):
    err = np.abs(dev.astype(skc.LD) - ref).astype(np.float64)
    return bool(np.all(err <= bound)), float(np.max(err / np.where(bound > 0, bound, 1.0), initial=0.0))


@pytest.mark.parametrize("name", skc.NAMES)
def test_family_lands_on_the_intended_side_of_the_rule(name):
    n, m, coo = skc.case(name)
    nnz, nfull = skc.counts(n, m, coo)
    assert skc.rule_kernel(n, m, coo) == skc.intended_kernel(name), (name, float(nfull.sum()) / m)
    assert n <= 130 and m <= 60


def test_the_families_have_the_shapes_they_are_named_for():
    n, m, coo = skc.case("lane_edges")
    assert n == 70 and skc.counts(n, m, coo)[1].tolist() == [63, 64, 65, 128, 129]
    for name in ("with_empty_below_24", "with_empty_above_24"):
        n, m, coo = skc.case(name)
        nnz = skc.counts(n, m, coo)[0]
        assert nnz[0] == 0 and nnz[-1] == 0 and np.all((nnz == 0) == (np.arange(m) % 3 == 0))
    assert skc.counts(*skc.case("single_empty"))[0].tolist() == [0] and len(skc.case("single_empty")[2][3]) == 0
    assert skc.counts(*skc.case("single_nonempty"))[0].tolist() == [30]
    nnz = skc.counts(*skc.case("skewed"))[0]
    assert nnz.max() == 600 and np.sum(nnz == 1) == len(nnz) - 1
    var, row, col, val = skc.case("diagonal_only")[2]
    assert np.all(row == col)
    var, row, col, val = skc.case("offdiag_only")[2]
    assert np.all(row != col)
    for name, n in (("tiny_n1", 1), ("tiny_n2", 2)):
        nn, m, coo = skc.case(name)
        assert nn == n and np.all(skc.position_counts(nn, m, coo) == m)
    n, m, coo = skc.case("shared_positions")
    cnt = skc.position_counts(n, m, coo)
    assert set(np.unique(cnt).tolist()) == {0, m} and np.sum(cnt == m) == 6
    # messy_input: both triangles, duplicates with other values, and the dense scatter agrees with the cleaned list
    n, m, coo = skc.case("messy_input")
    var, row, col, val = coo
    assert np.any(row < col) and np.any(row > col)
    cl = skc.clean(n, m, coo)
    assert len(cl[3]) == 5 * m and len(val) == 6 * m
    assert np.array_equal(skc.expand(n, m, coo), skc.expand(n, m, cl))
    A = skc.expand(n, m, coo, dtype=np.float64)
    assert np.array_equal(A, A.transpose(0, 2, 1))
    keys = list(zip(var.tolist(), np.maximum(row, col).tolist(), np.minimum(row, col).tolist()))
    assert len(set(keys)) == 5 * m
    first = {}
    for k, x in zip(keys, val.tolist()):
        first.setdefault(k, x)
    assert any(first[(v, r, c)] != x for v, r, c, x in zip(*[a.tolist() for a in cl]))     # first-wins would differ


@pytest.mark.parametrize("kind", ["well", "ill"])
@pytest.mark.parametrize("name", skc.NAMES)
def test_schur_restatement_meets_the_reference_under_the_bound(name, kind):
    n, m, coo = skc.case(name)
    X, Zi = skc.schur_operands(n, kind)
    ref, S = skc.schur_ref(n, m, coo, X, Zi)
    bound = skc.schur_bound(n, m, coo, S)
    M = ipm_ref.schur_rows_sparse(m, n, skc.clean(n, m, coo), X, Zi)
    ok, worst = _within(M, ref, bound)
    print("%s/%s: worst error / bound %.3g, max S / |ref| %.3g" % (name, kind, worst,
          float(np.max(S.astype(np.float64) / np.maximum(np.abs(ref).astype(np.float64), 1e-300), initial=0.0))))
    assert ok, worst
    zero = skc.schur_structural_zero(n, m, coo)
    assert np.all(M[zero] == 0.0) and np.all(ref[zero] == 0) and np.all(S[zero] == 0)
    # the second, independent form of the reference (pair by pair) agrees to extended precision
    rng = np.random.default_rng(3)
    pairs = [(int(i), int(j)) for i, j in zip(rng.integers(0, m, 40), rng.integers(0, m, 40))]
    Mp, Sp = skc.schur_ref_pairs(n, m, coo, X, Zi, pairs)
    ii, jj = np.array(pairs).T
    assert np.all(np.abs(Mp - ref[ii, jj]) <= 2.0 ** -58 * skc.schur_K(n, m, coo)[ii, jj] * Sp)
    assert np.all(np.abs(Sp - S[ii, jj]) <= 2.0 ** -58 * skc.schur_K(n, m, coo)[ii, jj] * Sp)


def test_the_ill_conditioned_pair_cancels():
    """what the 'ill' operands are for: S far above |ref|, so an absolute tolerance scaled by max |M| would not see a wrong entry"""
    n, m, coo = skc.case("uniform_k4")
    X, Zi = skc.schur_operands(n, "ill")
    assert np.linalg.cond(Zi) > 5e7
    ref, S = skc.schur_ref(n, m, coo, X, Zi)
    il = np.tril_indices(m)
    ratio = (S[il] / np.maximum(np.abs(ref[il]), LD_TINY)).astype(np.float64)
    assert np.median(ratio) > 3.0 and np.max(ratio) > 100.0


@pytest.mark.parametrize("name", skc.NAMES)
def test_pass_restatements_meet_the_references_under_the_bounds(name):
    n, m, coo = skc.case(name)
    Vs, Vn, coef, base, zero = skc.pass_operands(n, m)
    assert coef[0] != 0.0 and (m < 8 or np.any(coef[1:] == 0.0))
    for V in (Vs, Vn):
        ref, S = skc.apply_ref(n, m, coo, V)
        ok, worst = _within(skc.apply_f64(n, m, coo, V), ref, skc.apply_bound(n, m, coo, S))
        assert ok, worst
        empty = skc.counts(n, m, coo)[0] == 0
        assert np.all(ref[empty] == 0)
    for b in (base, zero):
        ref, S = skc.apply_t_ref(n, m, coo, coef, b)
        out = skc.apply_t_f64(n, m, coo, coef, b)
        ok, worst = _within(out, ref, skc.apply_t_bound(n, m, coo, S))
        assert ok, worst
        untouched = skc.position_counts(n, m, coo) == 0
        assert np.array_equal(out[untouched].view(np.uint64), b[untouched].view(np.uint64))
        assert np.all(ref[untouched] == b[untouched])


def test_the_two_unit_entries_are_symbols_of_the_units_library_alone(hb):
    units = _read("include", "hipsdp_units.h")
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_sparse_ops_unit\s*\(\s*int\s+device\s*,\s*int\s+n\s*,\s*int\s+m\s*,\s*long\s+long\s+nnz\s*,", units)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_schur_sparse_unit2\s*\([^;]*\bint\s+kernel\s*,\s*int\s*\*\s*took\s*\)\s*;", units)
    product = _read("include", "hipsdp.h")
    lib = hb.lib()
    for name in ("hipsdp_sparse_ops_unit", "hipsdp_schur_sparse_unit2"):
        assert name not in product
        assert not hasattr(lib, name), name
        assert hasattr(hb.ulib(), name), name
    assert callable(hb.sparse_ops_unit) and callable(hb.schur_sparse_unit2)
    # refused before any device work
    assert hb.ulib().hipsdp_schur_sparse_unit2(0, 0, 0, 0, None, None, None, None, None, None, None, 2, None) != 0
