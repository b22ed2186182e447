"""The small-problem passes of the general path (scip-sdp_amd/csrc/kernels.hip: hs_dir_block_small, hs_lp_rows_small, hs_apply_A_small,
hs_lp_dir, hs_vec_mul, hs_axpy3, hs_make_ext, hs_gemv_t, the four reductions, the m <= 64 solves) and their recorded forms inside the
single-workgroup batch kernel k_red_batch, one operation at a time through the unit entries of include/hipsdp_units.h, at the shapes
of tests/small_path_cases.py (every case names the branch of the kernel it is there for).  For every case:

  (a) the recorded form and the launch give the same bits;
  (b) the launch is within its first-order rounding bound of an extended-precision reference (tests/harness/small_path_ref.py:
      (N + k + 4) 2^-52 times the same expression on absolute values; the direction block (2 n + 8) 2^-52 B), or exactly equal where
      the operation is exact (absmax, ratio_min);
  (c) the number of records pending before the batch is launched says that the recorded form ran (>= 1), or that the call declined (0);
  (d) what an operation does not write is still NaN (reductions: still the preset value).

Inputs are normal values over twelve decades, seeded from the case.  Each test prints its largest error / bound.

Also here: hs_gemv_t3 against three hs_gemv_t calls (bit for bit, and against the reference), and hs_gemv_n (pass A) with a free row
pitch, one to four vectors, a vector base that is not 16-byte aligned, and the split forms.  k_gemv_n_rows4 is deliberately left out:
it needs R >= 1024 rows of E >= 2^18 entries, 2 GiB of A."""
import os

import numpy as np
import pytest

import small_path_cases as spc
import small_path_ref as ref
from chol_cases import same_bits

pytestmark = pytest.mark.gpu


def _mixed(rng, shape):
    """normal values over twelve decades: the roundings of a sum depend on every term"""
    return rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 7, shape)


def _seed(c, salt):
    return [salt] + [int(v) for k in sorted(c) if k not in ("op", "branch", "pred", "records", "id") for v in np.ravel(c[k])]


def _pending(c, pend_rec, pend_launch, what, bad):
    """(c)"""
    if pend_launch != 0:
        bad.append((what, "records pending without a batch", pend_launch))
    if (c["records"] == 0 and pend_rec != 0) or (c["records"] != 0 and pend_rec < 1):
        bad.append((what, "records pending: %d, the case says %s" % (pend_rec, c["records"])))


def _within(what, got, want, bnd, bad, worst):
    """(b)"""
    r = ref.worst_ratio(got, want, bnd)
    worst[0] = max(worst[0], r)
    if not (r <= 1.0) or not np.all(np.isfinite(got)):
        bad.append((what, "error / bound", r))


def _par(op):
    return pytest.mark.parametrize("c", spc.cases(op), ids=spc.ids(op))


@_par("dir_block")
def test_direction_block(gpu, c):
    n = c["n"]
    bad, worst = [], [0.0]
    rng = np.random.default_rng(_seed(c, 1))
    X, R, E, Zi = (_mixed(rng, (n, n)) for _ in range(4))
    for Ee in (None, E):
        for cc in (1.0, 0.73):
            for s1 in (0.0, 4.2e-9):
                what = "n=%d E=%s c=%g s1=%g" % (n, Ee is not None, cc, s1)
                lau, p0 = gpu.small_dir_block_unit(cc, s1, X, R, Ee, Zi, recorded=False)
                rec, p1 = gpu.small_dir_block_unit(cc, s1, X, R, Ee, Zi, recorded=True)
                same_bits(what, rec, lau, bad)
                _pending(c, p1, p0, what, bad)
                want, B = ref.dir_block(cc, s1, X, R, Ee, Zi)
                _within(what, lau, want, (2 * n + 8) * ref.EPS * B, bad, worst)
    # symmetric X and Zinv: the result is its own transpose, bit for bit
    Xs, Zs = X + X.T, Zi + Zi.T
    for recorded in (False, True):
        out, _ = gpu.small_dir_block_unit(0.73, 4.2e-9, Xs, R, E, Zs, recorded=recorded)
        same_bits("n=%d symmetric operands, recorded=%s: out against its transpose" % (n, recorded), out, out.T, bad)
    print("direction block n=%d: largest error / bound %.3f" % (n, worst[0]))
    assert not bad, bad


def test_direction_block_above_the_small_size_is_an_argument_error(gpu):
    n = spc.DIR_BLOCK_TOO_LARGE
    Z = np.ones((n, n))
    for recorded in (False, True):
        with pytest.raises(RuntimeError, match="rc=3"):
            gpu.small_dir_block_unit(1.0, 0.0, Z, Z, None, Z, recorded=recorded)
    out, pend = gpu.small_dir_block_unit(1.0, 0.0, Z[:2, :2], Z[:2, :2], None, Z[:2, :2], recorded=True)      # nothing is left behind
    assert pend == 1 and np.array_equal(out, -5.0 * np.ones((2, 2)))


@_par("lp_rows")
def test_lp_rows(gpu, c):
    q, m1 = c["q"], c["m1"]
    bad, worst = [], [0.0]
    rng = np.random.default_rng(_seed(c, 2))
    D, v, rd, elp = _mixed(rng, (q, m1)), _mixed(rng, m1), _mixed(rng, q), _mixed(rng, q)
    x, z = np.abs(_mixed(rng, q)), np.abs(_mixed(rng, q))
    eta, sigmu = 0.73, 3.1e-3
    for mode in (0, 1):
        for ee in (None, elp):
            what = "q=%d m1=%d mode=%d elp=%s" % (q, m1, mode, ee is not None)
            l1, l2, p0 = gpu.small_lp_rows_unit(D, v, mode, eta, sigmu, x, z, rd, ee, recorded=False)
            r1, r2, p1 = gpu.small_lp_rows_unit(D, v, mode, eta, sigmu, x, z, rd, ee, recorded=True)
            same_bits(what + " out1", r1, l1, bad)
            same_bits(what + " out2", r2, l2, bad)
            _pending(c, p1, p0, what, bad)
            w1, S1, w2, S2 = ref.lp_rows(D, v, mode, eta, sigmu, x, z, rd, ee)
            _within(what + " out1", l1, w1, ref.bound(m1, 1 if mode == 0 else 2, S1), bad, worst)
            if mode == 0:
                if not np.all(np.isnan(l2)):
                    bad.append((what, "mode 0 wrote out2"))
            else:
                _within(what + " out2", l2, w2, ref.bound(m1, 8, S2), bad, worst)
    print("lp rows q=%d m1=%d: largest error / bound %.3f" % (q, m1, worst[0]))
    assert not bad, bad


@_par("apply_A")
def test_apply_A(gpu, c):
    n2, q, m1 = c["n2"], c["q"], c["m1"]
    bad, worst = [], [0.0]
    rng = np.random.default_rng(_seed(c, 3))
    As, Vs = [_mixed(rng, (m1, k)) for k in n2], [_mixed(rng, k) for k in n2]
    D, vlp, vin = _mixed(rng, (q, m1)), _mixed(rng, q), _mixed(rng, m1 - 1)
    scal = 0.88
    N = sum(n2) + q
    for epi in (0, 1, 2):
        what = "n2=%s q=%d m1=%d epi=%d" % (n2, q, m1, epi)
        lo, lv, p0 = gpu.small_apply_A_unit(As, Vs, D, vlp, epi, scal, vin, recorded=False)
        ro, rv, p1 = gpu.small_apply_A_unit(As, Vs, D, vlp, epi, scal, vin, recorded=True)
        same_bits(what + " out", ro, lo, bad)
        same_bits(what + " vout", rv, lv, bad)
        _pending(c, p1, p0, what, bad)
        wo, S, wv, Sv = ref.apply_A(As, Vs, D, vlp, epi, scal, vin)
        _within(what + " out", lo, wo, ref.bound(N, 0, S), bad, worst)
        if epi == 0:
            if not np.all(np.isnan(lv)):
                bad.append((what, "epi 0 wrote vout"))
        else:
            _within(what + " vout", lv, wv, ref.bound(N, 2, Sv), bad, worst)
    print("apply_A n2=%s q=%d m1=%d: largest error / bound %.3f" % (n2, q, m1, worst[0]))
    assert not bad, bad


@pytest.mark.parametrize("n,nn,records", [(1, (1, 0, 0), 4), (255, (3, 0, 256), 4), (257, (257, 5, 1), 4), (16384, (16384, 300, 7), 4),
                                          (16385, (16385, 3, 3), 0)])
def test_elementwise_kernels(gpu, n, nn, records):
    """hs_lp_dir, hs_vec_mul, hs_make_ext, hs_axpy3: recorded up to RB_MAXN entries (four records), above it launched"""
    K = spc.constants()
    assert (records == 0) == (n > K["RB_MAXN"]) and (max(nn) > K["RB_MAXN"]) == (n > K["RB_MAXN"])
    bad, worst = [], [0.0]
    rng = np.random.default_rng([4, n])
    vecs = _mixed(rng, (6, n))
    vecs[1] = np.abs(vecs[1])
    xs, ys = _mixed(rng, sum(nn)), _mixed(rng, sum(nn))
    par = np.array([3.1e-3, 0.73, -0.21, 1.0, -0.6])                       # sigmu, eta, alpha, s0, s1
    for use_elp in (0, 1):
        lau = gpu.small_elementwise_unit(vecs, par, xs, ys, nn, use_elp, recorded=False)
        rec = gpu.small_elementwise_unit(vecs, par, xs, ys, nn, use_elp, recorded=True)
        for nm, a, b in zip(("lp_dir", "vec_mul", "make_ext", "axpy3"), rec[:4], lau[:4]):
            same_bits("n=%d %s" % (n, nm), a, b, bad)
        if lau[4] != 0 or rec[4] != records:
            bad.append(("n=%d" % n, "records pending", lau[4], rec[4]))
        x, z, r, elp, a, b = vecs
        w, S = ref.lp_dir(par[0], par[1], x, z, r, elp if use_elp else None)
        _within("lp_dir", lau[0], w, ref.bound(0, 7, S), bad, worst)
        w, S = ref.vec_mul(a, b)
        _within("vec_mul", lau[1], w, ref.bound(0, 1, S), bad, worst)
        w, S = ref.make_ext(par[3], par[4], a)
        _within("make_ext", lau[2], w, ref.bound(0, 1, S), bad, worst)
        assert lau[2][0] == par[3]
        w, S = ref.axpy(par[2], xs, ys)
        _within("axpy3", lau[3], w, ref.bound(0, 2, S), bad, worst)
    print("element-wise n=%d: largest error / bound %.3f" % (n, worst[0]))
    assert not bad, bad


@_par("gemv_t")
def test_recorded_gemv_t(gpu, c):
    R, E = c["R"], c["E"]
    bad, worst = [], [0.0]
    rng = np.random.default_rng(_seed(c, 5))
    for lda in (E, E + 3):
        A, coef, add = _mixed(rng, (R, lda)), _mixed(rng, R), _mixed(rng, E)
        for mode in (0, 1, 2):
            what = "R=%d E=%d lda=%d add=%s" % (R, E, lda, ("none", "separate", "the output")[mode])
            lau, p0 = gpu.small_gemv_t_unit(A, E, coef, 0.9, None if mode == 0 else add, mode, recorded=False)
            rec, p1 = gpu.small_gemv_t_unit(A, E, coef, 0.9, None if mode == 0 else add, mode, recorded=True)
            same_bits(what, rec, lau, bad)
            _pending(c, p1, p0, what, bad)
            w, S = ref.gemv_t(A, E, coef, 0.9, None if mode == 0 else add)
            _within(what, lau, w, ref.bound(R, 0 if mode == 0 else 2, S), bad, worst)
    print("gemv_t R=%d E=%d: largest error / bound %.3f" % (R, E, worst[0]))
    assert not bad, bad


def _reduction_operands(rng, kind, c):
    tot = sum(c["lens"])
    a, b, cc = _mixed(rng, tot), _mixed(rng, tot), _mixed(rng, tot)
    if kind == 3 or (kind == 2 and c["positive_d"]):
        b = np.abs(b)
    if kind == 2:
        a = np.abs(a)
    return a, b, cc


@pytest.mark.parametrize("kind", range(4), ids=ref.KINDS)
@_par("reductions")
def test_reductions(gpu, c, kind):
    """A launched reduction of more than RED_STAGE_N = 2048 entries runs in two stages (k_reduce_stage1 on ceil(n / 2048) workgroups,
    each thread striding by 256 ceil(n / 2048), then k_reduce_stage2 over the partial results), and its record has to combine the same
    terms in the same association: the cases red_two_stage_form (2049, 5000, 16 384 entries) and red_longest_recorded failed (a) for dot
    and lp_s0 while the record summed as one workgroup striding by 256."""
    lens, slots, acc, ns = c["lens"], c["slots"], c["acc"], c["nslots"]
    bad, worst = [], [0.0]
    rng = np.random.default_rng(_seed(c, 6) + [kind])
    a, b, cc = _reduction_operands(rng, kind, c)
    preset = np.abs(_mixed(rng, ns))
    lau, p0 = gpu.reductions_unit(kind, lens, slots, acc, a, b, cc, preset, recorded=False)
    rec, p1 = gpu.reductions_unit(kind, lens, slots, acc, a, b, cc, preset, recorded=True)
    what = "%s lens=%s slots=%s acc=%s" % (ref.KINDS[kind], lens, slots, acc)
    same_bits(what, rec, lau, bad)
    _pending(c, p1, p0, what, bad)
    # the slots in the order of the calls, exact and as a bound
    val = ref.ld(preset).copy()
    S = np.abs(ref.ld(preset))
    nterms = np.zeros(ns)
    exact = np.ones(ns, dtype=bool)
    off = 0
    for L, s, ac in zip(lens, slots, acc):
        v, Sv, k = ref.reduction(kind, a[off:off + L], b[off:off + L], cc[off:off + L])
        off += L
        if Sv is None:
            val[s] = ref.combine(kind, val[s], v) if ac else v
        else:
            exact[s] = False
            val[s], S[s], nterms[s] = (val[s] + v, S[s] + Sv, nterms[s] + L + k + 1) if ac else (v, Sv, L + k)
    for s in range(ns):
        if exact[s]:
            if lau[s] != float(val[s]):
                bad.append((what, "slot %d: %r, exactly %r expected" % (s, lau[s], float(val[s]))))
        else:
            _within(what + " slot %d" % s, lau[s:s + 1], val[s:s + 1], ref.bound(nterms[s], 0, S[s:s + 1]), bad, worst)
    untouched = [s for s in range(ns) if s not in slots]
    if not np.array_equal(lau[untouched], preset[untouched]) or not np.array_equal(rec[untouched], preset[untouched]):
        bad.append((what, "a slot no reduction writes lost its preset value"))
    if kind == 2 and c["positive_d"]:
        assert lau[0] == 1e300
    print("%s: largest error / bound %.3g" % (what, worst[0]))
    assert not bad, bad


@pytest.mark.parametrize("subst", (False, True), ids=("inverse", "subst"))
@_par("solve")
def test_small_solves(gpu, c, subst):
    import scipy.linalg as sla
    m = c["m"]
    rng = np.random.default_rng(_seed(c, 7))
    M = ref.ill_conditioned_spd(rng, m)
    b = M @ rng.standard_normal((m, 3))
    fac = sla.cho_factor(M, lower=True)

    def check(what, x, rhs):
        res = np.linalg.norm(M @ x - rhs) / np.linalg.norm(rhs)
        res_ref = np.linalg.norm(M @ sla.cho_solve(fac, rhs) - rhs) / np.linalg.norm(rhs)
        print("m=%d %s %s: residual %.3g, LAPACK %.3g" % (m, "subst" if subst else "inverse", what, res, res_ref))
        assert res <= 20.0 * res_ref + 1e-15, (what, res, res_ref)

    old = os.environ.get("HIPSDP_SMALL_SOLVE")
    try:
        if subst:
            os.environ["HIPSDP_SMALL_SOLVE"] = "subst"
        else:
            os.environ.pop("HIPSDP_SMALL_SOLVE", None)
        for nrhs in (1, 3):
            slab = np.full((nrhs, m + 3), np.nan)
            slab[:, :m] = b[:, :nrhs].T
            out, pend, fail = gpu.small_solve_unit(M, slab, form=0)
            assert pend == 1 and fail == 0
            assert np.all(np.isnan(out[:, m:])) and np.all(np.isfinite(out[:, :m]))
            check("recorded solve, %d right-hand side(s)" % nrhs, out[:, :m].T, b[:, :nrhs])
        rhs2, u2, wt, fail = gpu.small_solve_unit(M, np.concatenate([b[:, 0], b[:, 1]]), form=1)
        assert fail == 0
        check("k_solve2_small", rhs2.reshape(2, m).T, b[:, :2])
        assert np.array_equal(u2, rhs2[m:] - rhs2[:m]) and wt[0] == 1.0 and np.array_equal(wt[1:], -rhs2[:m])
    finally:
        if old is None:
            os.environ.pop("HIPSDP_SMALL_SOLVE", None)
        else:
            os.environ["HIPSDP_SMALL_SOLVE"] = old


@_par("gemv_t3")
def test_gemv_t3_against_three_calls(gpu, c):
    R, E = c["R"], c["E"]
    bad, worst = [], [0.0]
    rng = np.random.default_rng(_seed(c, 8))
    for lda in ((c["lda"],) if "lda" in c else (E, E + 2)):
        A, cf = _mixed(rng, (R, lda)), _mixed(rng, (3, R))
        what = "R=%d E=%d lda=%d" % (R, E, lda)
        three, t0 = gpu.gemv_t3_unit(A, E, cf, fused=False)
        one, t1 = gpu.gemv_t3_unit(A, E, cf, fused=True)
        same_bits(what, one, three, bad)
        if t0 != 0 or t1 != (0 if c["records"] == 0 else 1):
            bad.append((what, "fused kernel took the shape: %d / %d" % (t0, t1)))
        for v in range(3):
            w, S = ref.gemv_t(A, E, cf[v], 0.0, None)
            _within(what + " vector %d" % v, three[v], w, ref.bound(R, 0, S), bad, worst)
    print("gemv_t3 R=%d E=%d: largest error / bound %.3f" % (R, E, worst[0]))
    assert not bad, bad


@_par("pass_a")
def test_pass_A(gpu, c):
    R, E, lda, nv = c["R"], c["E"], c["lda"], c["nv"]
    rng = np.random.default_rng(_seed(c, 9))
    A, V = _mixed(rng, (R, lda)), _mixed(rng, (nv, E))
    out, slices, vec = gpu.pass_a_unit(A, E, V, voff=c["voff"], wsdoubles=c["ws"])
    plan = spc.gemvn_plan(R, E, lda, nv, c["voff"], c["ws"])
    assert (slices, vec) == plan[:2], (slices, vec, plan)
    want, _ = ref.gemv_n(A, E, V)
    want = np.asarray(want, dtype=np.float64)
    err = np.abs(out - want).max() / max(1e-300, np.abs(want).max())
    print("pass A R=%d E=%d lda=%d nv=%d voff=%d: %d slice(s), vector loads %s, relative error %.3g (allowed %.3g)"
          % (R, E, lda, nv, c["voff"], slices, vec, err, 1e-13 * E ** 0.5))
    assert np.all(np.isfinite(out)) and err <= 1e-13 * E ** 0.5
