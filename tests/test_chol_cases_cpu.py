"""CPU: tests/harness/chol_cases.py - the input families, the oracle's pivot loop and the error figures of tests/test_gpu_chol.py -
held to everything the GPU tests assume of them, with LAPACK and the oracle alone (no device)."""
import ctypes as C
import os
import re
import numpy as np
import pytest

import ipm_ref
import chol_cases as cc
from chol_cases import (graded, graded_all, indefinite_at, fail_columns, lead, spread, psd_all, psd_ranks, spread_shapes, spread_seed,
                        chol_psd_pivots, psd_oracle, clear_columns, lapack_chol, comp_backward, recon, check, same_bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extended_precision_is_there_for_the_error_figures():
    assert np.finfo(cc.XD).eps <= 2.0 ** -63


def test_graded_has_the_condition_it_states_and_rowscale_is_exact():
    for cond in cc.CONDS:
        S = graded(64, cond)
        ev = np.linalg.eigvalsh(S)
        assert np.array_equal(S, S.T) and abs(ev[-1] / ev[0] / cond - 1.0) <= 1e-3, (cond, ev[-1] / ev[0])
        T = graded(64, cond, rowscale=True)
        dg = np.diag(T)
        assert np.array_equal(T, T.T) and lapack_chol(T)[1] == 0 and dg.max() / dg.min() > 2.0 ** 20, cond
    assert not graded(17, 1e8).flags.writeable and graded(17, 1e8) is graded(17, 1e8)
    assert graded(1, 1e12).shape == (1, 1) and graded(1, 1e12)[0, 0] == 1.0


def test_lapack_componentwise_backward_error_on_graded():
    """LAPACK's |L L^T - S|_ij <= 0.12 (n + 1) eps (|L||L^T|)_ij at every size of 15 rows and more that the GPU tests use (measured:
    0.111 at most).  At 2 rows an entry is two or three roundings over 3 eps: 0.161 here with seed 0 (0.19 - 0.26 with seeds 1 - 3), so
    there the figure is held to what Higham's gamma_{n+1} gives with unit roundoff eps / 2 for any correctly rounded factorization: 0.5.
    The device's bound in test_gpu_chol.py is 2, four times that."""
    worst = 0.0
    for n in sorted(set(cc.SINGLE + cc.BLOCKED + cc.SEQ_SIZES)):
        for name, S in graded_all(n):
            L, info = lapack_chol(S)
            assert info == 0, name
            f = comp_backward(L, S)
            worst = max(worst, f)
            assert f <= (0.12 if n >= 15 else 0.5), (name, f)
    print("LAPACK componentwise: worst %.3f (n + 1) eps" % worst)


def test_comp_backward_sees_one_wrong_entry():
    S = graded(33, 1e8)
    L, _ = lapack_chol(S)
    assert comp_backward(L, S) <= 0.12
    L[20, 7] *= 1.0 + 1e-11
    assert comp_backward(L, S) > 2.0


def test_indefinite_at_is_reported_at_its_pivot_by_lapack():
    for n in cc.FAIL_SIZES:
        S = graded(n, 1e2)
        for k in fail_columns(n, cc.FAIL_AT):
            assert lapack_chol(indefinite_at(S, k))[1] == k + 1, (n, k)
    for n in cc.SINGLE:
        S = graded(n, 1e2)
        for k in fail_columns(n, cc.SMALL_FAIL_AT):
            T = indefinite_at(S, k)
            assert lapack_chol(T)[1] == k + 1, (n, k)
            assert np.array_equal(np.delete(T.ravel(), k * n + k), np.delete(S.ravel(), k * n + k))


def _takes_its_loop(M):
    try:
        L = np.linalg.cholesky(M)
        return not np.all(np.diag(L) ** 2 > 1e-13 * np.diag(M))
    except np.linalg.LinAlgError:
        return True


def test_chol_psd_pivots_returns_the_bits_of_the_oracle():
    assert ipm_ref.PIVOT_RULE == 3
    loops = 0
    for m in cc.PSD_SIZES:
        for fam, name, M in psd_all(m):
            L, piv, forced, zeroed = chol_psd_pivots(M)
            assert np.all(zeroed <= forced)
            assert all(not np.any(L[k + 1:, k]) for k in np.flatnonzero(zeroed)), name
            if _takes_its_loop(M):
                loops += 1
                assert np.array_equal(ipm_ref.chol_psd(M), L), name
    assert loops >= 100
    S = graded(33, 1e2)                                    # a definite matrix: nothing forced, the plain factor
    L, piv, forced, zeroed = chol_psd_pivots(S)
    assert not forced.any() and np.abs(L - np.linalg.cholesky(S)).max() <= 1e-14


def test_lead_every_column_is_clear():
    """rank r exactly: the oracle zeroes the columns r .. m - 1 and no others, every noise pivot far below the zeroing threshold (0.06 of
    it at most), every kept pivot far above the forcing threshold, the oracle's reconstruction at 4e-14"""
    noise = 0.0
    kept = np.inf
    rec = 0.0
    for m in cc.PSD_SIZES:
        for r in psd_ranks(m):
            M = lead(m, r)
            L, piv, forced, zeroed = psd_oracle(M)
            assert clear_columns(M).all(), (m, r)
            assert np.array_equal(np.flatnonzero(zeroed), np.arange(r, m)) and np.array_equal(forced, zeroed), (m, r)
            k1 = np.arange(1, m + 1)
            if zeroed.any():
                noise = max(noise, np.max(np.abs(piv[zeroed]) / (cc.NOISE * k1[zeroed] * np.diag(M)[zeroed])))
            kept = min(kept, np.min(piv[~zeroed] / (cc.REGTOL * np.diag(M)[~zeroed])))
            rec = max(rec, recon(L, M))
    print("lead: noise pivots at most %.3f of the zeroing threshold, kept pivots at least %.1e of the forcing threshold, oracle's "
          "reconstruction %.1e" % (noise, kept, rec))
    assert noise <= 0.125 and kept >= 1e9 and rec <= 1e-13


def test_forced_kept_at_is_forced_and_kept_by_the_oracle_with_room_on_both_sides():
    for n in cc.KEPT_SIZES:
        for k in cc.KEPT_AT:
            M = cc.forced_kept_at(graded(n, 1e2), k)
            L, piv, forced, zeroed = chol_psd_pivots(M)
            assert np.array_equal(L, ipm_ref.chol_psd(M))
            assert not forced[:k].any() and forced[k] and not zeroed[k], (n, k)
            up, down = cc.REGTOL * M[k, k] / piv[k], piv[k] / (cc.NOISE * (k + 1) * M[k, k])
            assert up >= 1.25 and down >= 1.25, (n, k, up, down)
            assert np.abs(L[k + 1:, k]).max() > 1.0                         # the column is there, and large
            later = np.arange(k + 1, n)
            assert np.all((np.abs(piv[later]) > 8 * cc.REGTOL * np.diag(M)[later]) | ~forced[later]), (n, k)


def test_spread_stays_out_of_the_mask_comparison_as_a_whole():
    """a fact about the family: with seed 0 throughout, up to 41 % of the columns of a spread matrix have a pivot within a factor 8 of a
    threshold in the oracle alone, and twelve of the 68 matrices more than 30 %, so two correct implementations may decide them
    differently and the GPU test compares the mask on clear_columns only.  The seeds fixed in SPREAD_SEEDS for those twelve bring every
    matrix to 30 % or less (the GPU test asks for 35 % with the device's own undecided columns counted in); the narrower factor-4 band
    still leaves columns out; forced pivots that keep their column are there, every one of them inside the band"""
    worst0 = worst8 = worst4 = 0.0
    over0 = set()
    forced_kept = 0
    for m in cc.PSD_SIZES:
        for r, s in spread_shapes(m):
            share0 = 1.0 - clear_columns(spread(m, r, s, 0)).mean()
            worst0 = max(worst0, share0)
            if share0 > 0.30:
                over0.add((m, r, s))
            M = spread(m, r, s, spread_seed(m, r, s))
            clear = clear_columns(M)
            worst8 = max(worst8, 1.0 - clear.mean())
            worst4 = max(worst4, 1.0 - clear_columns(M, band=4.0).mean())
            _, piv, forced, zeroed = psd_oracle(M)
            forced_kept += int(np.sum(forced & ~zeroed))
            assert not np.any(forced & ~zeroed & clear), (m, r, s)
    print("spread: seed 0 leaves up to %.0f %% of a matrix's columns not clear; the fixed seeds %.0f %% (factor 8), %.0f %% (factor 4); "
          "%d forced pivots keep their column" % (100 * worst0, 100 * worst8, 100 * worst4, forced_kept))
    assert over0 == set(cc.SPREAD_SEEDS) and 0.40 < worst0 < 0.42
    assert 0.10 < worst8 <= 0.30 and worst4 > 0.05 and forced_kept > 0


def test_check_collects_and_asserts():
    bad = []
    check("unit", "fine", 1.0, 2.0, ref=0.5, bad=bad)
    check("unit", "recorded only", 5.0, 2.0, bad=bad, asserted=False)
    assert not bad and cc.LEVELS["unit"][1] == 5.0
    check("unit", "miss", 3.0, 2.0, bad=bad)
    check("unit", "nan", float("nan"), 2.0, bad=bad)
    assert len(bad) == 2 and cc.LEVELS["unit"][4] == "nan"
    with pytest.raises(AssertionError):
        check("unit", "miss", 3.0, 2.0)
    same_bits("zeros", np.array([0.0]), np.array([-0.0]), bad)
    same_bits("nan", np.array([np.nan, 1.0]), np.array([np.nan, 1.0]), bad)
    assert len(bad) == 3
    del cc.LEVELS["unit"]


def test_unit_entries_refuse_bad_arguments_before_they_touch_a_device(hb):
    """HIPSDP_ERR_ARG comes back before the device is chosen, so this runs without one"""
    u = hb.ulib()
    ERR_ARG = int(re.search(r"#define\s+HIPSDP_ERR_ARG\s+(\d+)", open(os.path.join(ROOT, "include", "hipsdp.h")).read()).group(1))
    A = np.eye(4)
    rhs = np.zeros((1, 4, 4))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    fail = C.c_int(0)
    for nr, md, psd, n in ((0, 7, 0, 4), (5, 7, 0, 4), (1, 4, 0, 4), (1, 1, 0, 4), (1, 2, 0, 4), (1, 0, 0, 4), (1, 7, 2, 4), (1, 7, 0, 0)):
        rc = u.hipsdp_potrs_seq(0, n, dp(A), psd, 1, ip(np.array([nr], dtype=np.int32)), ip(np.array([md], dtype=np.int32)), dp(rhs), None,
                                C.byref(fail))
        assert rc == ERR_ARG, (nr, md, psd, n, rc)
    out = [np.zeros(4096) for _ in range(5)]
    flag = np.zeros(2, dtype=np.int32)
    B = np.eye(40)
    for n, pair, want in ((0, 0, 0), (65, 0, 0), (40, 2, 0), (40, 0, 1), (33, 1, 1)):
        rc = u.hipsdp_potrf_small_unit(0, n, pair, dp(B), None, C.c_double(0.0), 0, want, dp(out[0]), dp(out[1]), dp(out[2]), dp(out[3]),
                                       dp(out[4]), ip(flag))
        assert rc == ERR_ARG, (n, pair, want, rc)
