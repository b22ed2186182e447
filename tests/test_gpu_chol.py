"""GPU: the Cholesky kernels of scip-sdp_amd/csrc/chol.hip against LAPACK (numpy / scipy) and against the oracle's pivot rule
(ipm_ref.chol_psd) on the input families of tests/harness/chol_cases.py: graded spectra up to condition 1e12 with rows scaled by
2^-10 .. 2^10, matrices made indefinite at one chosen pivot, exactly rank-deficient and spread Gram matrices.  tests/test_chol_cases_cpu.py
holds the references alone to what is assumed of them here.

  1 single block, n <= 64 (hipsdp_potrf and the fused hipsdp_potrf_small_unit): componentwise |L L^T - S| <= 2 (n + 1) eps |L||L^T|
    - Higham's gamma_{n+1} for any order of summation, doubled for v_rcp_f64 / v_rsq_f64 with their Newton steps, which are good to
    about 1 ulp instead of correctly rounded (eps = 2^-52; LAPACK stays at 0.12, 0.16 at 2 rows); zero upper triangle, identity-padded
    dinv, Linv = dinv
  2 the factor of 4^k S, k = +-50, is 2^k times the factor of S bit for bit (Linv: 2^-k, Gram: 4^-k): every operation of the pivot
    chain is exact under that scaling
  3 fused outputs: Mout = base + alpha dir bit for bit, |Linv L - I| and |Gram M - I| within 10 x scipy's dtrtri / numpy's inv + n eps,
    the pair form returns the bits of the single form, the failure flag with set_flag 0 and 1
  4 blocked, 65 .. 321 rows (last blocks of 1, 16, 17, 32, 33, 64, 22, 8 rows: every launch_potrf_step instantiation and its edges):
    both forms bit for bit; ||L L^T - S||_F / ||S||_F <= 10 R + 64 eps kappa, R = LAPACK's figure, kappa = the largest condition number
    of a 64 x 64 diagonal block of LAPACK's factor - the panel is A21 inv(L_bb)^T with an explicit inverse, not a substitution, which
    costs 64 eps kappa(L_bb) relative to the panel.  The componentwise figure is recorded, not asserted
  5 the failure index equals the info of LAPACK's dpotrf at panel and block edges, both forms
  6 semidefinite mode: mask = the oracle's zeroed set, forced diagonal entries sqrt(1e-13 M_kk) to 2 ulp, exact zeros below; the
    reconstruction and the residual of a consistent system through hipsdp_potrs_seq(psd) within 10 x the oracle's + 1e-15 (both are
    amplified rounding noise: the oracle's own values range over two to six decades between seeds; a wrong or unzeroed column shows
    at 1e-3 and above).  On `lead` all of this holds for every column of every matrix.  On `spread` two things were found on the
    device and are restated, each from the pivots:
    (a) spread m=96 r=96 s=12: the columns 56 .. 64 keep pivots of 2e-13 .. 7e-13 M_kk on both sides - rounding noise that neither
    threshold catches - which differ by up to 50 % between device and oracle (2.87e-13 against 4.46e-13 at column 64); every later
    pivot inherits that, and column 80, clear by the oracle's pivot (-4.3e-15 M_kk, zeroed), has 1.32e-13 M_kk on the device and is
    kept.  So a column is also left out of the mask comparison when the device kept it with a pivot of ITS OWN within a factor 8 of
    the forcing threshold (L_kk^2 tells); a zeroed column never is.  The share left out, now per form, still has to stay <= 35 %.
    (b) spread m=64 r=32 s=0: pivot 32, the first dependent column, is 6.76e-14 M_kk in the oracle, 15 % above the zeroing threshold
    5.87e-14 M_kk: the oracle keeps the column, the device zeroes it (and column 34).  The column is noise of 4e-12 |M| (pivot 31 is
    7e-6 M_kk); kept, it is reproduced by L L^T, zeroed, it is what L L^T misses: 7.2e-12 against 4.8e-14, residual 8.8e-9 against
    8.8e-14.  Factor 10 compares two runs of the same decisions, so it is asserted when the device's mask equals the oracle's
    zeroed set in EVERY column (all of `lead`, all but these few of `spread`).  Otherwise the bound is what rule 3 guarantees for
    either decision: a zeroed column k of the Schur complement C has c_kk <= tau M_kk, tau = max(1e-13, 1.78e-15 m), and
    |c_ik| <= sqrt(c_ii c_kk) <= sqrt(tau M_ii M_kk), so ||L L^T - M||_F <= sqrt(2 tau) trace(M), and the residual of a consistent
    system is at most that times |x| / |b|, |x| that of the oracle's solution
  7 solves in sequence on ONE workspace with 3, 1, 2, 4, 1, 3 right-hand sides: residual within 20 x scipy's cho_solve + 1e-15 (the
    criterion of test_corrected_solves_on_an_ill_conditioned_factor) and the bits of each call alone on a fresh workspace, also with
    the parity of the exchange vectors flipped by single-mode calls in between; modes 5 then 6 give the bits of mode 7; mode 3 (no
    correction) within 20 kappa(L_bb) x.  Up to 128 rows hs_trsv_sync hands over to the one-workgroup kernels k_trsv<1..4>, which
    use no workspace: there the comparison with a fresh workspace says only that a call does not depend on the one before

Every figure is printed before it is judged; a test collects what missed and asserts once.  tests/devtools/chol_levels.py runs the
same functions and writes the worst figure of every group to profiles/r13_chol_levels.txt."""
import numpy as np
import pytest
import scipy.linalg as sla

import ipm_ref
import chol_cases as cc
from chol_cases import (EPS, graded, graded_all, indefinite_at, fail_columns, psd_all, psd_oracle, clear_columns, lapack_chol,
                        comp_backward, recon, backward_figures, lapack_figures, residual, inverse_defect, block_kappa, check, same_bits)

pytestmark = pytest.mark.gpu

SEQ = (3, 1, 2, 4, 1, 3)


def _dir_for(S, seed):
    """symmetric indefinite direction, small enough that S + alpha dir stays definite for alpha <= 0.5"""
    n = S.shape[0]
    rng = np.random.default_rng([seed, n, 77])
    G = rng.standard_normal((n, n))
    D = 0.5 * (G + G.T)
    D[0, 0] = -abs(D[0, 0]) - 1.0                               # a negative and (n > 1) a positive diagonal entry: indefinite
    if n > 1:
        D[n - 1, n - 1] = abs(D[n - 1, n - 1]) + 1.0
    D *= 0.5 * np.linalg.eigvalsh(S)[0] / np.linalg.norm(D, 2)
    return np.ascontiguousarray(0.5 * (D + D.T))


@pytest.mark.parametrize("n", cc.SINGLE)
def test_single_block_factorization_componentwise(gpu, n):
    bad = []
    for name, S in graded_all(n):
        ref = lapack_figures(S)[2]
        L, fail = gpu.potrf(S)
        check("1 potrf componentwise", name, comp_backward(L, S), 2.0, ref=ref, bad=bad)
        o = gpu.potrf_small_unit(S)
        if fail != 0 or o["flag"] != 0:
            bad.append((name, "flagged", fail, o["flag"]))
        Ls, dinv, Linv = o["L"], o["dinv"], o["Linv"]
        check("1 small_unit componentwise", name, comp_backward(np.tril(Ls), S), 2.0, ref=ref, bad=bad)
        if np.any(np.triu(Ls, 1) != 0.0):
            bad.append((name, "upper triangle of L not zero"))
        pad = np.eye(64)
        pad[:n, :n] = np.tril(dinv[:n, :n])
        if not np.array_equal(dinv, pad):
            bad.append((name, "dinv not identity-padded with a zero upper triangle"))
        same_bits(name + ": Linv against dinv", Linv, dinv[:n, :n], bad)
        same_bits(name + ": Mout against base", o["Mout"], S, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", cc.SINGLE)
def test_single_block_scales_exactly_with_powers_of_four(gpu, n):
    bad = []
    for name, S in graded_all(n):
        L0, _ = gpu.potrf(S)
        o0 = gpu.potrf_small_unit(S, want_gram=n <= 32)
        for k in (-50, 50):
            Sk = S * 4.0 ** k
            Lk, fail = gpu.potrf(Sk)
            ok = gpu.potrf_small_unit(Sk, want_gram=n <= 32)
            what = "%s 4^%d" % (name, k)
            if fail != 0 or ok["flag"] != 0:
                bad.append((what, "flagged"))
            same_bits(what + ": potrf L", Lk, L0 * 2.0 ** k, bad)
            same_bits(what + ": small_unit L", ok["L"], o0["L"] * 2.0 ** k, bad)
            same_bits(what + ": Linv", ok["Linv"], o0["Linv"] * 2.0 ** -k, bad)
            same_bits(what + ": dinv", ok["dinv"][:n, :n], o0["dinv"][:n, :n] * 2.0 ** -k, bad)
            if n <= 32:
                same_bits(what + ": Gram", ok["Gram"], o0["Gram"] * 4.0 ** -k, bad)
    assert not bad, bad


@pytest.mark.parametrize("n", cc.SINGLE)
def test_fused_outputs_of_the_small_block_kernel(gpu, n):
    bad = []
    gram = n <= 32
    singles = []
    for cond, alpha in ((1e2, 0.5), (1e8, 0.25)):
        S = graded(n, cond)
        D = _dir_for(S, int(np.log10(cond)))
        M = S + alpha * D                                       # alpha dir is exact, one rounding in the sum: what fma gives
        name = "n=%d cond=%.0e alpha=%g" % (n, cond, alpha)
        if n > 1 and not (np.linalg.eigvalsh(D)[0] < 0 < np.linalg.eigvalsh(D)[-1]):
            bad.append((name, "dir is not indefinite"))
        o = gpu.potrf_small_unit(S, D, alpha, want_gram=gram)
        singles.append((S, D, alpha, o))
        if o["flag"] != 0:
            bad.append((name, "flagged", o["flag"]))
        same_bits(name + ": Mout", o["Mout"], M, bad)
        L = np.tril(o["L"])
        check("3 factor of base + alpha dir", name, comp_backward(L, M), 2.0, ref=comp_backward(lapack_chol(M)[0], M), bad=bad)
        ti, info = sla.lapack.dtrtri(L, lower=1)
        ref = inverse_defect(np.tril(ti), L)
        check("3 |Linv L - I|", name, inverse_defect(o["Linv"], L), 10.0 * ref + n * EPS, ref=ref, bad=bad)
        if gram:
            ref = inverse_defect(np.linalg.inv(M), M)
            check("3 |Gram M - I|", name, inverse_defect(o["Gram"], M), 10.0 * ref + n * EPS, ref=ref, bad=bad)
            same_bits(name + ": Gram symmetric", o["Gram"], o["Gram"].T, bad)
    # the pair form: the two problems above in one launch (same alpha: the second one once more with the first one's)
    for al in (0.5, 0.25):
        a = gpu.potrf_small_unit(singles[0][0], singles[0][1], al, want_gram=gram)
        b = gpu.potrf_small_unit(singles[1][0], singles[1][1], al, want_gram=gram)
        p = gpu.potrf_small_unit(np.stack([singles[0][0], singles[1][0]]), np.stack([singles[0][1], singles[1][1]]), al, pair=True,
                                 want_gram=gram)
        for j, o in enumerate((a, b)):
            for key in ("L", "dinv", "Mout", "Linv") + (("Gram",) if gram else ()):
                same_bits("n=%d alpha=%g pair problem %d: %s" % (n, al, j, key), p[key][j], o[key], bad)
            if p["flag"][j] != o["flag"]:
                bad.append((n, al, "pair flag", j, int(p["flag"][j]), o["flag"]))
    # the failure flag, written (set_flag = 1) or recorded into the cleared word (0), alone and beside a definite problem
    S = graded(n, 1e2)
    for k in fail_columns(n, cc.SMALL_FAIL_AT):
        T = indefinite_at(S, k)
        for sf in (False, True):
            f1 = gpu.potrf_small_unit(T, set_flag=sf)["flag"]
            f2 = gpu.potrf_small_unit(np.stack([S, T]), pair=True, set_flag=sf)["flag"]
            print("n=%d pivot %d set_flag %d: flag %d, pair flags %s" % (n, k, sf, f1, f2))
            if f1 != k + 1 or list(f2) != [0, k + 1]:
                bad.append((n, k, sf, "failure flag", f1, list(f2)))
    assert not bad, bad


@pytest.mark.parametrize("n", cc.BLOCKED)
def test_blocked_factorization_both_forms(gpu, n):
    bad = []
    for name, S in graded_all(n):
        Lr, info, cref, R, kappa = lapack_figures(S)
        L1, d1, _, f1 = gpu.potrf_ex(S, psd=False, v1=True)
        L0, d0, _, f0 = gpu.potrf_ex(S, psd=False, v1=False)
        if info != 0 or f0 != 0 or f1 != 0:
            bad.append((name, "flagged", info, f0, f1))
        same_bits(name + ": L of the two forms", np.tril(L0), np.tril(L1), bad)
        same_bits(name + ": dinv of the two forms", d0, d1, bad)
        L = np.tril(L0)
        comp, nrm = backward_figures(L, S)
        check("4 blocked norm-wise", name, nrm, 10.0 * R + 64.0 * EPS * kappa, ref=R, bad=bad)
        check("4 blocked componentwise", name, comp, 2.0, ref=cref, bad=bad, asserted=False)
    assert not bad, bad


@pytest.mark.parametrize("n", cc.FAIL_SIZES)
def test_failure_index_is_lapacks_info(gpu, n):
    bad = []
    S = graded(n, 1e2)
    for k in fail_columns(n, cc.FAIL_AT):
        T = indefinite_at(S, k)
        info = lapack_chol(T)[1]
        f1 = gpu.potrf_ex(T, v1=True)[3]
        f0 = gpu.potrf_ex(T, v1=False)[3]
        print("n=%d pivot %d: dpotrf info %d, four-launch form %d, one launch per block column %d" % (n, k, info, f1, f0))
        if not (f0 == f1 == info == k + 1):
            bad.append((n, k, info, f1, f0))
    assert not bad, bad


@pytest.mark.parametrize("m", cc.PSD_SIZES)
def test_semidefinite_mode_against_the_oracle(gpu, m):
    bad = []
    rng = np.random.default_rng(9000 + m)
    for fam, name, M in psd_all(m):
        _, piv, forced, zeroed = psd_oracle(M)
        Lo = ipm_ref.chol_psd(M)
        b = M @ rng.standard_normal(m)
        xo = sla.solve_triangular(Lo.T, sla.solve_triangular(Lo, b, lower=True, check_finite=False), lower=False, check_finite=False)
        rec_o, res_o = recon(Lo, M), residual(M, xo, b)
        clear = clear_columns(M)
        if fam == "lead" and not clear.all():
            bad.append((name, "reference: a column of lead is not clear"))
        dg = np.diag(M)
        # what rule 3 itself guarantees, whichever way the columns near a threshold go: see the docstring of the module
        tau = max(cc.REGTOL, cc.NOISE * m)
        rule_bound = np.sqrt(2.0 * tau) * np.trace(M) / np.linalg.norm(M)
        forms = ((False, "one launch per column"), (True, "four launches")) if m > 64 else ((False, "single block"),)
        first = None
        for v1, form in forms:
            Lg, dinv, mask, fail = gpu.potrf_ex(M, psd=True, v1=v1)
            Lg = np.tril(Lg)
            what = "%s, %s" % (name, form)
            mask = mask.astype(bool)
            if first is None:
                first = (Lg, mask)
            else:
                same_bits(what + ": L against the other form", Lg, first[0], bad)
                if not np.array_equal(mask, first[1]):
                    bad.append((what, "mask differs from the other form's"))
            compare = clear
            if fam == "spread":
                # a column the device kept with a pivot of its own within the band of the forcing threshold is as undecided as one
                # where the oracle's pivot is (a zeroed column has lost its pivot and is never taken out here)
                pd = np.diag(Lg) ** 2
                compare = clear & ~(~mask & (pd >= cc.REGTOL * dg / 8.0) & (pd <= cc.REGTOL * dg * 8.0))
            check("6 %s share of columns left out" % fam, what, 1.0 - compare.mean(), 0.35, bad=bad)
            if not np.array_equal(mask[compare], zeroed[compare]):
                k = np.flatnonzero((mask != zeroed) & compare)
                print("%s: mask differs at %s: oracle pivots %s, thresholds %s" % (what, k[:8], piv[k[:8]], cc.NOISE * (k[:8] + 1) * dg[k[:8]]))
                bad.append((what, "mask differs from the oracle's zeroed set at", list(k[:8])))
            z = np.flatnonzero(mask)
            if len(z):
                want = np.sqrt(cc.REGTOL * dg[z])
                ulps = np.max(np.abs(Lg[z, z] - want) / np.spacing(want))
                check("6 %s forced diagonal, ulp" % fam, what, ulps, 2.0, bad=bad)
                below = max(float(np.max(np.abs(Lg[k + 1:, k]), initial=0.0)) for k in z)
                if below != 0.0:
                    bad.append((what, "entries below a zeroed pivot", below))
            same = fam == "lead" or np.array_equal(mask, zeroed)
            if same:
                check("6 %s reconstruction" % fam, what, recon(Lg, M), 10.0 * rec_o + 1e-15, ref=rec_o, bad=bad)
            else:
                k = np.flatnonzero(mask != zeroed)
                print("%s: decided unlike the oracle at the undecided columns %s (oracle pivots / M_kk %s)" % (what, k[:8], (piv / dg)[k[:8]]))
                check("6 spread reconstruction, other decisions", what, recon(Lg, M), rule_bound, ref=rec_o, bad=bad)
        # the solve factors for itself (one launch per block column): judged by the decisions of ITS factorization
        xs, mask2, fail = gpu.potrs_seq(M, [(7, b)], psd=True)
        mask2 = mask2.astype(bool)
        if not np.array_equal(mask2, first[1]):
            bad.append((name, "mask of hipsdp_potrs_seq differs from hipsdp_potrf_ex"))
        if fam == "lead" or np.array_equal(mask2, zeroed):
            check("6 %s residual" % fam, name, residual(M, xs[0], b), 10.0 * res_o + 1e-15, ref=res_o, bad=bad)
        else:
            # M x - b = (M - L L^T) x; |x| taken from the oracle's solution, so that nothing of the device enters the bound
            check("6 spread residual, other decisions", name, residual(M, xs[0], b),
                  rule_bound * np.linalg.norm(M) * np.linalg.norm(xo) / np.linalg.norm(b), ref=res_o, bad=bad)
    assert not bad, bad


@pytest.mark.parametrize("n", cc.KEPT_SIZES)
def test_a_forced_pivot_above_the_noise_level_keeps_its_column(gpu, n):
    """the decision between the two thresholds of rule 3, on a pivot made to sit between them (chol_cases.forced_kept_at): forced to
    1e-13 M_kk, its column divided by the forced pivot and kept - the mask is the oracle's zeroed set in every column (the later pivots
    are large negative numbers on both sides: forced and zeroed).  The columns 0 .. k are the oracle's to 8 (k + 1) eps kappa relative to
    their largest entry, kappa = 1e2 the condition of the matrix the leading block is cut from: the first-order bound on the factor of a
    block of k + 1 rows under backward errors of (k + 1) eps (column k is the Schur column over the forced pivot, which is the same
    number on both sides, so it carries the same relative error).  `spread` cannot show this decision: a forced pivot that keeps its
    column lies within a factor 8 of one of the two thresholds at every k.  (Not in the issue: added because turning 1.78e-15 into
    1.78e-13 in pd_panel, which zeroes every forced column, passes every other test of this file.)"""
    bad = []
    S = graded(n, 1e2)
    for k in cc.KEPT_AT:
        M = cc.forced_kept_at(S, k)
        Lo, piv, forced, zeroed = cc.chol_psd_pivots(M)
        for v1 in ((False, True) if n > 64 else (False,)):
            Lg, dinv, mask, fail = gpu.potrf_ex(M, psd=True, v1=v1)
            Lg = np.tril(Lg)
            what = "n=%d pivot %d v1=%d" % (n, k, v1)
            if not np.array_equal(mask.astype(bool), zeroed):
                bad.append((what, "mask differs from the oracle's zeroed set at", list(np.flatnonzero(mask.astype(bool) != zeroed)[:8])))
            want = np.sqrt(cc.REGTOL * M[k, k])
            check("6 kept forced diagonal, ulp", what, abs(Lg[k, k] - want) / np.spacing(want), 2.0, bad=bad)
            check("6 kept columns against the oracle", what, np.abs(Lg[:, :k + 1] - Lo[:, :k + 1]).max() / np.abs(Lo[:, :k + 1]).max(), 8.0 * (k + 1) * EPS * 1e2, bad=bad)
    assert not bad, bad


@pytest.mark.parametrize("n", cc.SEQ_SIZES)
def test_solves_in_sequence_on_one_workspace(gpu, n):
    bad = []
    M = graded(n, 1e8)
    rng = np.random.default_rng(7000 + n)
    bs = [(M @ rng.standard_normal((n, k))).T.copy() for k in SEQ]
    c, low = sla.cho_factor(M, lower=True)
    seq, _, fail = gpu.potrs_seq(M, [(7, b) for b in bs])
    assert fail == 0
    for i, b in enumerate(bs):
        ref = residual(M, sla.cho_solve((c, low), b.T).T, b)
        what = "n=%d call %d (%d rhs)" % (n, i, b.shape[0])
        check("7 corrected solves in sequence", what, residual(M, seq[i], b), 20.0 * ref + 1e-15, ref=ref, bad=bad)
        alone = gpu.potrs_seq(M, [(7, b)])[0][0]
        same_bits(what + ": against the same call alone on a fresh workspace", seq[i], alone, bad)
    # an odd number of single-mode calls in front flips the parity: the forward sweeps then run on the exchange vector the backward
    # sweeps had, and back again after the second one
    flip = gpu.potrs_seq(M, [(5, bs[1]), (7, bs[0]), (7, bs[3]), (6, bs[4]), (7, bs[2])])[0]
    for j, i in ((1, 0), (2, 3), (4, 2)):
        same_bits("n=%d call %d of the sequence with the parity flipped" % (n, j), flip[j], seq[i], bad)
    # forward alone, then backward alone on its result: the bits of mode 7; the forward result against the device's own factor
    L = np.tril(gpu.potrf_ex(M)[0])
    kappa = lapack_figures(M)[4]
    for i in (0, 3):
        b = bs[i]
        what = "n=%d %d rhs" % (n, b.shape[0])
        y = gpu.potrs_seq(M, [(5, b)])[0][0]
        x = gpu.potrs_seq(M, [(5, b), (6, y)])[0][1]
        same_bits(what + ": modes 5 then 6 against mode 7", x, seq[i], bad)
        yr = sla.solve_triangular(L, b.T, lower=True, check_finite=False).T
        ref = residual(L, yr, b)
        check("7 forward solve alone", what, residual(L, y, b), 20.0 * ref + 1e-15, ref=ref, bad=bad)
        x3 = gpu.potrs_seq(M, [(3, bs[1]), (3, b)])[0][1]
        ref = residual(M, sla.cho_solve((c, low), b.T).T, b)
        check("7 uncorrected solves (mode 3)", what, residual(M, x3, b), 20.0 * kappa * ref + 1e-15, ref=ref, bad=bad)
    assert not bad, bad
