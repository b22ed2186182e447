"""GPU: hipsdp_onevar_bounds_large - the one-variable SDPs of blocks of 129 .. 512 rows as rounds of batched launches - against the
numpy restatement of tests/onevar_cases.py, against hipsdp_onevar_bounds_all's kernels at the sizes both serve (unit entries), and
against itself bit for bit under everything its bits must not depend on: the other jobs, their order, the workgroups per job, the
chunking.

The bounds are those of tests/test_gpu_onevar_all.py: on decidable jobs status and evaluation count equal the restatement's, a bound
is returned exactly, and
    |optval - ref| <= 0.8 feastol / g        (onevar_cases.inner_bound: derived from concavity, not measured);
an EXTREMES job is held to |lambda - numpy| <= 1e-12 max|ev(A_i)|, the bound of the eigenvalue entry points."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import numpy as np
import pytest
import ipm_ref
import sdpi_driver
from conftest import ROOT, GOLDEN
import onevar_cases as K
import onevar_all_cases as KA
import onevar_large_cases as KL
from test_gpu_onevar_all import load_dense, load_sparse, _bits, _take, _check_properties, _check_against_ref

pytestmark = pytest.mark.gpu


def _solver(gpu, blocks, how):
    b = np.ones(blocks[0].shape[0] - 1)
    s = (load_dense if how == "dense" else load_sparse)(gpu, list(blocks), b)
    if how == "sparse":
        assert all(s.is_sparse(k) for k in range(len(blocks)))
    return s


def _delta(c0, c1):
    return tuple(c1[k] - c0[k] for k in range(3))


_worst = {}


@pytest.mark.parametrize("how,size", [("dense", s) for s in KL.SIZES] + [("sparse", s) for s in KL.SPARSE_SIZES],
                         ids=lambda v: v if isinstance(v, str) else "n%d" % v[0])
def test_family_matches_the_restatement(gpu, how, size):
    """1: the 18 instances of a size, u = ub, every variable in one call.  The worst |optval - ref| g / feastol of the INNER jobs is
    printed before it is checked against 0.8.  Measured on an MI355X (dense): see DESIGN.md 6.10."""
    n, m, rank = size
    worst, jobs, und = 0.0, 0, 0
    for fl, sd, A, lb, ub, refs in KL.instances(size):
        s = _solver(gpu, [A], how)
        c0 = gpu.onevar_bounds_large_stats()
        st, ov, lmin, grad, ne = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL)
        c1 = gpu.onevar_bounds_large_stats()
        s.close()
        R = int(max(ne))
        assert _delta(c0, c1) == (1, KL.launches(n, R, 1), R + 1), (fl, sd, _delta(c0, c1), R)
        for i, r in enumerate(refs):
            jobs += 1
            tag = (how, n, fl, sd, i)
            _check_properties(A, ub, i, lb[i], ub[i], int(st[i]), float(ov[i]), K.FEASTOL)
            if st[i] == K.LB:
                assert grad[i] == 0.0, tag
            if not K.decidable(K.NEWTON, r[5]):
                und += 1
                continue
            worst = max(worst, _check_against_ref(A, ub, i, r, int(st[i]), float(ov[i]), int(ne[i]), K.FEASTOL, lb[i], ub[i], tag))
    print("%s, n = %3d: worst |optval - ref| g / feastol = %.3g (bound 0.8); %d jobs, %d undecidable" % (how, n, worst, jobs, und))
    assert worst <= 0.8
    assert jobs == 18 * m and und == KL.UNDECIDABLE[n]


def _two_blocks():
    """blocks of 130 and 257 rows that share six variables (the generator of tests/onevar_all_cases.py at these sizes)"""
    return KA.multi_family(1, 0.6, 0.0, 0, blocks=[(130, 10), (257, 12)])


def test_bits_second_call_subset_alone_and_two_blocks(gpu):
    """2a: a second call; a shuffled subset; one job alone against the same job among six; two blocks in one call against each block in
    a call of its own - all bit for bit"""
    blocks, lb, ub = _two_blocks()
    m = len(ub)
    s = _solver(gpu, blocks, "dense")
    lbj, ubj = np.tile(lb, 2), np.tile(ub, 2)
    jb, jv = np.repeat(np.arange(2, dtype=np.int32), m), np.tile(np.arange(m, dtype=np.int32), 2)
    full = s.onevar_bounds_large(ub, lbj, ubj, K.FEASTOL)
    assert set(int(x) for x in full[0]) <= {K.LB, K.INNER, K.INFEASIBLE} and K.INNER in set(int(x) for x in full[0])
    assert _bits(s.onevar_bounds_large(ub, lbj, ubj, K.FEASTOL)) == _bits(full)
    assert _bits(s.onevar_bounds_large(ub, lbj, ubj, K.FEASTOL, blocks=jb, vars=jv)) == _bits(full)
    sub = np.random.default_rng(24).permutation(2 * m)[:7]
    part = s.onevar_bounds_large(ub, lbj[sub], ubj[sub], K.FEASTOL, blocks=jb[sub], vars=jv[sub])
    assert _bits(part) == _bits(_take(full, sub))
    for j in (2, m + 3):
        one = s.onevar_bounds_large(ub, lbj[j:j + 1], ubj[j:j + 1], K.FEASTOL, blocks=jb[j:j + 1], vars=jv[j:j + 1])
        assert _bits(one) == _bits(_take(full, [j])), j
    for b in range(2):
        own = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL, blocks=np.full(m, b, dtype=np.int32), vars=np.arange(m, dtype=np.int32))
        assert _bits(own) == _bits(_take(full, np.arange(b * m, (b + 1) * m))), b
    s.close()
    # ... and a solver that holds one of the blocks alone
    for b in range(2):
        s1 = _solver(gpu, [blocks[b]], "dense")
        assert _bits(s1.onevar_bounds_large(ub, lb, ub, K.FEASTOL)) == _bits(_take(full, np.arange(b * m, (b + 1) * m))), b
        s1.close()


_CHILD = r"""
import sys, json
import numpy as np
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(harness)r); sys.path.insert(0, %(oracle)r)
import importlib.util
spec = importlib.util.spec_from_file_location("hb_child", %(binding)r)
hb = importlib.util.module_from_spec(spec); spec.loader.exec_module(hb)
import onevar_cases as K
import onevar_all_cases as KA
import test_gpu_onevar_all as T
blocks, lb, ub = KA.multi_family(1, 0.6, 0.0, 0, blocks=[(130, 10), (257, 12)])
s = T.load_dense(hb, list(blocks), np.ones(len(ub)))
c0 = hb.onevar_bounds_large_stats()
res = s.onevar_bounds_large(ub, np.tile(lb, 2), np.tile(ub, 2), K.FEASTOL)
c1 = hb.onevar_bounds_large_stats()
s.close()
print(json.dumps({"bits": [np.asarray(a).tobytes().hex() for a in res], "stats": [c1[k] - c0[k] for k in range(3)]}))
"""


def _child(chunk):
    env = dict(os.environ)
    env.pop("HIPSDP_ONEVAR_LARGE_CHUNK", None)
    if chunk:
        env["HIPSDP_ONEVAR_LARGE_CHUNK"] = str(chunk)
    code = _CHILD % {"tests": os.path.join(ROOT, "tests"), "harness": os.path.join(ROOT, "tests", "harness"),
                     "oracle": os.path.join(ROOT, "oracle"), "binding": os.path.join(ROOT, "scip-sdp_amd", "binding.py")}
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bits_do_not_depend_on_the_chunking(gpu):
    """2b: HIPSDP_ONEVAR_LARGE_CHUNK=2 against one chunk, each in a fresh child process: twelve jobs in six chunks of two (ordered by
    descending n: three chunks per block), the same bits, more launches and read-backs"""
    one, six = _child(0), _child(2)
    assert one["bits"] == six["bits"]
    assert one["stats"][0] == six["stats"][0] == 1
    assert six["stats"][2] > one["stats"][2] and six["stats"][1] > one["stats"][1]


def _unit_jobs(ns, seed0=3):
    Z, A, sh, lo, hi = [], [], [], [], []
    for k, n in enumerate(ns):
        Ab, lb, ub = K.family(n, 3, max(1, min(6, n // 2)), seed0 + k, 0.6, 0.0, 0)
        i = k % 3
        Z.append(K.z_of(Ab, ub)); A.append(Ab[i + 1]); sh.append(ub[i]); lo.append(lb[i]); hi.append(ub[i])
    return Z, A, sh, lo, hi


def test_bits_do_not_depend_on_the_workgroups_per_job(gpu):
    """2c: through the unit entry, a workgroup cap of 1 (every row of a job in one workgroup), of 3 and the default; and two chunks
    against one"""
    ns = [200, 129, 257, 64]
    Z, A, sh, lo, hi = _unit_jobs(ns)
    kind = [K.NEWTON, K.NEWTON, K.TWOPOINT, K.NEWTON]
    base = gpu.onevar_large_unit(Z, A, sh, lo, hi, K.FEASTOL, kind=kind)
    assert all(int(x) in (K.LB, K.INNER, K.INFEASIBLE, K.UBONLY) for x in base[0]) and K.INNER in [int(x) for x in base[0]]
    for cap in (1, 3):
        assert _bits(gpu.onevar_large_unit(Z, A, sh, lo, hi, K.FEASTOL, kind=kind, wg_cap=cap)) == _bits(base), cap
    assert _bits(gpu.onevar_large_unit(Z, A, sh, lo, hi, K.FEASTOL, kind=kind, chunk=2)) == _bits(base)
    assert _bits(gpu.onevar_large_unit(Z, A, sh, lo, hi, K.FEASTOL, kind=kind, chunk=1, wg_cap=2)) == _bits(base)


def test_small_and_mixed_sizes_through_the_unit_entry(gpu):
    """3: n = 2, 3, 64, 65, 128, 129 in ONE call: every job agrees with the restatement and with the kernels of hipsdp_onevar_bounds /
    hipsdp_onevar_bounds_all on the same matrices (status and evaluations equal on decidable jobs, optval within the concavity bound);
    and a 2 x 2 case by hand"""
    ns = [2, 3, 64, 65, 128, 129]
    seen = set()
    for seed0, t in ((3, 0.6), (11, 0.3), (19, 0.9)):
        Z, A, sh, lo, hi = [], [], [], [], []
        for k, n in enumerate(ns):
            Ab, lb, ub = K.family(n, 3, max(1, min(6, n // 2)), seed0 + k, t, 0.0, 0)
            i = k % 3
            Z.append(K.z_of(Ab, ub)); A.append(Ab[i + 1]); sh.append(ub[i]); lo.append(lb[i]); hi.append(ub[i])
        st, ov, lmin, grad, ne, rounds = gpu.onevar_large_unit(Z, A, sh, lo, hi, K.FEASTOL, with_rounds=True)
        assert rounds == max(ne)
        small = gpu.onevar_all_unit(Z[:5], A[:5], sh[:5], lo[:5], hi[:5], K.FEASTOL)
        for k, n in enumerate(ns):
            ref = K.onevar_ref(Z[k], A[k], sh[k], K.NEWTON, lo[k], hi[k], K.FEASTOL)
            tag = (seed0, n)
            seen.add(ref[0])
            if not K.decidable(K.NEWTON, ref[5]):
                continue
            assert (int(st[k]), int(ne[k])) == (ref[0], ref[4]), (tag, st[k], ne[k], ref[0], ref[4])
            if ref[1] == lo[k] or ref[1] == hi[k]:
                assert ov[k] == ref[1], tag
            else:
                assert abs(ov[k] - ref[1]) <= K.inner_bound(Z[k], A[k], sh[k], ov[k], ref[1], K.FEASTOL)[0], tag
            if k < 5:
                assert (int(small[0][k]), int(small[4][k])) == (int(st[k]), int(ne[k])), tag
                if ref[1] == lo[k] or ref[1] == hi[k]:
                    assert small[1][k] == ov[k], tag
                else:
                    assert abs(small[1][k] - ov[k]) <= K.inner_bound(Z[k], A[k], sh[k], ov[k], small[1][k], K.FEASTOL)[0], tag
                old = gpu.onevar_unit(n, Z[k], [A[k]], [sh[k]], [lo[k]], [hi[k]], K.FEASTOL)
                assert (int(old[0][0]), int(old[4][0])) == (int(st[k]), int(ne[k])), tag
    assert K.INNER in seen
    # by hand: A = I, Z = -I / 2 (2 x 2): M(mu) = (mu - 0.5) I
    Z2, A2 = [-0.5 * np.eye(2)] * 5, [np.eye(2)] * 5
    kind = [K.TWOPOINT, K.TWOPOINT, K.TWOPOINT, K.NEWTON, K.NEWTON]
    lo, hi = [0.6, 0.0, 0.0, 0.0, 0.0], [1.0, 1.0, 0.25, 1.0, 0.25]
    st, ov, lmin, grad, ne = gpu.onevar_large_unit(Z2, A2, [0.0] * 5, lo, hi, 1e-6, kind=kind)
    assert list(st) == [K.LB, K.UBONLY, K.INFEASIBLE, K.INNER, K.INFEASIBLE] and list(ne) == [1, 2, 2, 3, 1]
    assert list(ov[:3]) == [0.6, 1.0, 0.25] and np.max(np.abs(lmin[:3] - np.array([0.1, 0.5, -0.25]))) <= 1e-14
    assert abs(ov[3] - (0.5 - 0.5e-6)) <= 1e-14 and ov[4] == 0.25
    assert abs(grad[3] - 1.0) <= 1e-12 and abs(grad[4] - 1.0) <= 1e-12 and list(grad[:3]) == [0.0, 0.0, 0.0]


def test_known_answers_embedded_in_a_block_of_129_rows(gpu):
    """4: the five known answers of the reference's unit test (tests/golden/onevar_cases.json) in the leading rows of a 129-row block:
    A_1 padded with zeros, A_0 with -c I (c = 1000), so Z = -A_0 has +c on the padding and lambda_min is the small problem's"""
    with open(os.path.join(GOLDEN, "onevar_cases.json")) as f:
        G = json.load(f)
    n, c = 129, 1000.0
    for case in G["cases"]:
        k = case["n"]
        A = np.zeros((2, n, n))
        A[0] = -c * np.eye(n)
        A[0][:k, :k] = sdpi_driver._dense(k, case["const"])
        A[1][:k, :k] = sdpi_driver._dense(k, case["var"])
        for how in ("dense", "sparse"):
            s = _solver(gpu, [A], how)
            st, ov, lmin, grad, ne = s.onevar_bounds_large([0.0], [case["lb"]], [case["ub"]], G["eps"], infinity=G["infinity"])
            s.close()
            ref = K.onevar_ref(-A[0], A[1], 0.0, K.NEWTON, case["lb"], case["ub"], G["eps"], infinity=G["infinity"])
            if case["infeasible"]:
                assert st[0] == K.INFEASIBLE, (case["name"], how)
                continue
            assert st[0] in (K.LB, K.INNER) and abs(ov[0] - case["optval"]) <= G["eps"], (case["name"], how, ov[0])
            assert (int(st[0]), int(ne[0])) == (ref[0], ref[4]), (case["name"], how)
            if ref[1] == case["lb"] or ref[1] == case["ub"]:
                assert ov[0] == ref[1]
            else:
                assert abs(ov[0] - ref[1]) <= K.inner_bound(-A[0], A[1], 0.0, ov[0], ref[1], G["eps"])[0], (case["name"], how)


@pytest.mark.parametrize("how,size", [("dense", KL.SIZES[0]), ("sparse", KL.SIZES[0]), ("dense", KL.SIZES[5])],
                         ids=lambda v: v if isinstance(v, str) else "n%d" % v[0])
def test_kinds(gpu, how, size):
    """5: TWOPOINT mixed with NEWTON; u = 0; EXTREMES alone (no Z(u) launch), with maxevals = 1, and mixed in without touching the
    other jobs' bits; a zero A_i; DECLINED beside served jobs; maxevals = 2 -> GAVEUP"""
    n, m, rank = size
    A, lb, ub, refs = KL.instance(size, K.FLAVOURS[6], 2)             # the indefinite flavour: the last A_i has both signs
    A = np.array(A)
    A[2] = 0.0                                                        # variable 1 has no entry
    s = _solver(gpu, [A], how)
    newton = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL)
    kind = np.array([i % 2 for i in range(m)], dtype=np.int32)
    mixed = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL, kind=kind)
    nw = np.nonzero(kind == K.NEWTON)[0]
    assert _bits(_take(mixed, nw)) == _bits(_take(newton, nw))
    Z = K.z_of(A, ub)
    for i in range(m):
        ref = K.onevar_ref(Z, A[i + 1], ub[i], int(kind[i]), lb[i], ub[i], K.FEASTOL)
        if K.decidable(int(kind[i]), ref[5]):
            assert (int(mixed[0][i]), int(mixed[4][i])) == (ref[0], ref[4]), (i, kind[i])
        if kind[i] == K.TWOPOINT:
            assert mixed[3][i] == 0.0 and mixed[1][i] in (lb[i], ub[i])
    # u = 0 (tightenMatrices): Z(0) = -A_0, bounds 0 .. 1
    zero = np.zeros(m)
    t0 = s.onevar_bounds_large(zero, zero, np.ones(m), K.FEASTOL)
    for i in range(m):
        ref = K.onevar_ref(-A[0], A[i + 1], 0.0, K.NEWTON, 0.0, 1.0, K.FEASTOL)
        if K.decidable(K.NEWTON, ref[5]):
            assert (int(t0[0][i]), int(t0[4][i])) == (ref[0], ref[4]), i
            if ref[1] in (0.0, 1.0):
                assert t0[1][i] == ref[1]
            else:
                assert abs(t0[1][i] - ref[1]) <= K.inner_bound(-A[0], A[i + 1], 0.0, t0[1][i], ref[1], K.FEASTOL)[0], i
    # EXTREMES
    ex = np.full(m, KA.EXTREMES, dtype=np.int32)
    c0 = gpu.onevar_bounds_large_stats()
    st, ov, lmin, grad, ne = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL, kind=ex)
    c1 = gpu.onevar_bounds_large_stats()
    assert _delta(c0, c1) == (1, KL.launches(n, 1, 0), 2)                       # no Z(u) launch, one round
    st1, ov1, lmin1, grad1, ne1 = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL, kind=ex, maxevals=1)
    inf = s.onevar_bounds_large(ub, np.full(m, -1e20), np.full(m, 1e20), K.FEASTOL, kind=ex)
    assert _bits(inf) == _bits((st, ov, lmin, grad, ne))                        # the bounds are not read: nothing is declined
    worst = 0.0
    for i in range(m):
        lo, hi = KA.extremes_ref(A[i + 1])
        scale = max(abs(lo), abs(hi))
        assert (st[i], ne[i], grad[i]) == (KA.DONE, 2, 0.0), i
        assert (st1[i], ne1[i], grad1[i]) == (KA.DONE, 1, 0.0) and ov1[i] == lmin1[i] and lmin1[i] == lmin[i], i
        if scale == 0.0:
            assert abs(lmin[i]) < 1e-200 and abs(ov[i]) < 1e-200, (i, lmin[i], ov[i])
            continue
        worst = max(worst, abs(lmin[i] - lo) / scale, abs(ov[i] - hi) / scale)
        assert abs(lmin[i] - lo) <= 1e-12 * scale and abs(ov[i] - hi) <= 1e-12 * scale, (i, lmin[i], lo, ov[i], hi)
    print("%s, n = %d: worst |lambda - numpy| / max|ev| = %.3g (bound 1e-12)" % (how, n, worst))
    assert KA.extremes_ref(A[m])[0] < 0.0 < KA.extremes_ref(A[m])[1]
    mk = np.array([KA.EXTREMES if i % 3 == 0 else i % 2 for i in range(m)], dtype=np.int32)
    mx = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL, kind=mk)
    keep, exj = np.nonzero(mk != KA.EXTREMES)[0], np.nonzero(mk == KA.EXTREMES)[0]
    assert _bits(_take(mx, keep)) == _bits(_take(mixed, keep))
    assert _bits(_take(mx, exj)) == _bits(_take((st, ov, lmin, grad, ne), exj))
    # a declined job beside served ones
    ub2 = np.array(ub)
    ub2[0] = 1e20
    dec = s.onevar_bounds_large(ub, lb, ub2, K.FEASTOL)
    assert dec[0][0] == K.DECLINED and dec[4][0] == 0 and dec[1][0] == 0.0 and dec[2][0] == 0.0 and dec[3][0] == 0.0
    assert _bits(_take(dec, np.arange(1, m))) == _bits(_take(newton, np.arange(1, m)))
    c0 = gpu.onevar_bounds_large_stats()
    alldec = s.onevar_bounds_large(ub, np.full(m, -1e20), ub, K.FEASTOL)
    c1 = gpu.onevar_bounds_large_stats()
    assert list(alldec[0]) == [K.DECLINED] * m and _delta(c0, c1) == (1, 0, 0)   # decided before anything is read or launched
    s.close()
    # a bounded loop: two evaluations are not enough for an INNER job of the plain flavour
    A, lb, ub, refs = KL.instance(size, K.FLAVOURS[1], 1)
    inner = [i for i in range(m) if refs[i][0] == K.INNER and refs[i][4] > 2]
    assert inner
    i = inner[0]
    s = _solver(gpu, [A], how)
    c0 = gpu.onevar_bounds_large_stats()
    g = s.onevar_bounds_large(ub, lb[i:i + 1], ub[i:i + 1], K.FEASTOL, blocks=[0], vars=[i], maxevals=2)
    c1 = gpu.onevar_bounds_large_stats()
    s.close()
    assert g[0][0] == K.GAVEUP and g[4][0] == 2 and g[1][0] == lb[i]
    assert _delta(c0, c1) == (1, KL.launches(n, 2, 1), 2)             # R = maxevals: the result rows come with the last count
    r2 = K.onevar_ref(K.z_of(A, ub), A[i + 1], ub[i], K.NEWTON, lb[i], ub[i], K.FEASTOL, maxevals=2)
    assert r2[0] == K.GAVEUP and r2[1] == lb[i]


def test_blocks_of_128_and_513_rows_are_turned_away(gpu):
    """6: their jobs get -1 with nothing written, the 129-row block's jobs the bits they get alone"""
    A, lb, ub, refs = KL.instance(KL.SIZES[0], K.FLAVOURS[1], 1)
    m = len(ub)
    rng = np.random.default_rng(513)
    others = []
    for n in (128, 513):
        B = np.zeros((m + 1, n, n))
        for i in range(m + 1):
            F = rng.standard_normal((n, 2))
            B[i] = F @ F.T + np.eye(n)
        others.append(B)
    s1 = _solver(gpu, [A], "dense")
    alone = s1.onevar_bounds_large(ub, lb, ub, K.FEASTOL)
    s1.close()
    s = _solver(gpu, [others[0], A, others[1]], "dense")
    st, ov, lmin, grad, ne = s.onevar_bounds_large(ub, np.tile(lb, 3), np.tile(ub, 3), K.FEASTOL)
    small = s.onevar_bounds_all(ub, np.tile(lb, 3), np.tile(ub, 3), K.FEASTOL)
    s.close()
    for part in (slice(0, m), slice(2 * m, 3 * m)):
        assert list(st[part]) == [-1] * m and list(ne[part]) == [0] * m
        assert np.all(np.isnan(ov[part])) and np.all(np.isnan(lmin[part])) and np.all(np.isnan(grad[part]))
    mid = slice(m, 2 * m)
    assert _bits([a[mid] for a in (st, ov, lmin, grad, ne)]) == _bits(alone)
    # the two calls split the blocks between them: the 128-row block is the other call's, the 513-row block nobody's
    assert all(x >= 0 for x in small[0][:m]) and list(small[0][m:]) == [-1] * (2 * m)


def test_counts(gpu):
    """7: (calls, launches, read-backs) follow  z + R (nmax + 5)  and  R + 1  for one job and for six jobs of the same block - equal
    when R is -, and for two blocks; the totals of the two other one-variable calls do not move"""
    blocks, lb, ub = _two_blocks()
    m = len(ub)
    s = _solver(gpu, blocks, "dense")
    o0, a0 = gpu.onevar_bounds_stats(), gpu.onevar_bounds_all_stats()
    zb, vb = np.zeros(m, dtype=np.int32), np.arange(m, dtype=np.int32)
    c0 = gpu.onevar_bounds_large_stats()
    six = s.onevar_bounds_large(ub, lb, ub, K.FEASTOL, blocks=zb, vars=vb)
    c1 = gpu.onevar_bounds_large_stats()
    R6 = int(max(six[4]))
    assert _delta(c0, c1) == (1, KL.launches(130, R6, 1), R6 + 1)
    j = int(np.argmax(six[4]))                                                    # the longest job alone: the same R, the same counts
    one = s.onevar_bounds_large(ub, lb[j:j + 1], ub[j:j + 1], K.FEASTOL, blocks=[0], vars=[j])
    c2 = gpu.onevar_bounds_large_stats()
    assert _delta(c1, c2) == _delta(c0, c1) and int(one[4][0]) == R6
    both = s.onevar_bounds_large(ub, np.tile(lb, 2), np.tile(ub, 2), K.FEASTOL)
    c3 = gpu.onevar_bounds_large_stats()
    R12 = int(max(both[4]))
    assert _delta(c2, c3) == (1, KL.launches(257, R12, 1), R12 + 1)
    assert gpu.onevar_bounds_stats() == o0 and gpu.onevar_bounds_all_stats() == a0
    s.onevar_bounds_all(ub, np.tile(lb, 2), np.tile(ub, 2), K.FEASTOL)            # serves nothing here, and moves no total of this call
    assert gpu.onevar_bounds_large_stats() == c3
    s.close()


def test_two_host_threads_on_different_solvers(gpu):
    """8a: one solver per thread, three calls each, the single-thread bits"""
    data = [KL.instance(KL.SIZES[0], K.FLAVOURS[3], sd) for sd in (1, 2)]
    solvers = [_solver(gpu, [d[0]], "dense") for d in data]

    def call(i):
        A, lb, ub, refs = data[i]
        return _bits(solvers[i].onevar_bounds_large(ub, lb, ub, K.FEASTOL))
    single = [call(i) for i in range(2)]
    got, errs = [[], []], []

    def work(i):
        try:
            for _ in range(3):
                got[i].append(call(i))
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for s in solvers:
        s.close()
    assert not errs, errs
    for i in range(2):
        assert got[i] == [single[i]] * 3


def test_argument_errors_the_implicit_list_and_an_empty_call(gpu):
    """8b: a solver with one 129-row and one 12-row block: every argument error returns HIPSDP_ERR_ARG (3) with nothing launched and
    status untouched; count == 0 returns 0; the implicit block-major list equals the explicit one, the 12-row block's jobs get -1"""
    blocks, lb, ub = KA.multi_family(1, 0.6, 0.0, 0, blocks=[(129, 10), (12, 2)])
    nb, m = 2, len(ub)
    cnt = nb * m
    s = _solver(gpu, blocks, "dense")
    f = gpu.lib().hipsdp_onevar_bounds_large
    dp, ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    u, l, h = np.array(ub), np.tile(lb, nb), np.tile(ub, nb)
    st, ov = np.full(cnt, 7, dtype=np.int32), np.zeros(cnt)
    jb, jv = np.repeat(np.arange(nb, dtype=np.int32), m), np.tile(np.arange(m, dtype=np.int32), nb)
    kind = np.zeros(cnt, dtype=np.int32)
    opts = gpu.OnevarOpts(1e-6, 1e20, 0)
    o = C.byref(opts)
    c0 = gpu.onevar_bounds_large_stats()
    fresh = gpu.Solver(0)                                                         # no shape
    assert f(fresh.h, dp(u), cnt, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    fresh.close()
    assert f(None, dp(u), cnt, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, None, cnt, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, None, dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), None, o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), None, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), o, None, dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), o, ip(st), None, None, None, None) == 3
    assert f(s.h, dp(u), -1, ip(jb), ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt - 1, None, None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, ip(jb), None, None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), cnt, None, ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    for bad in (-1, nb):
        b2 = jb.copy()
        b2[5] = bad
        assert f(s.h, dp(u), cnt, ip(b2), ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    for bad in (-1, m):
        v2 = jv.copy()
        v2[2] = bad
        assert f(s.h, dp(u), cnt, ip(jb), ip(v2), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    for bad in (-1, 3):
        k2 = kind.copy()
        k2[3] = bad
        assert f(s.h, dp(u), cnt, ip(jb), ip(jv), ip(k2), dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 3
    neg = gpu.OnevarOpts(-1e-6, 1e20, 0)
    assert f(s.h, dp(u), cnt, None, None, None, dp(l), dp(h), C.byref(neg), ip(st), dp(ov), None, None, None) == 3
    assert f(s.h, dp(u), 0, ip(jb), ip(jv), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 0        # count == 0
    assert list(st) == [7] * cnt and gpu.onevar_bounds_large_stats() == c0
    # only the small block's jobs: no served job, nothing launched
    assert f(s.h, dp(u), m, ip(jb[m:].copy()), ip(jv[m:].copy()), None, dp(l), dp(h), o, ip(st), dp(ov), None, None, None) == 0
    assert list(st[:m]) == [-1] * m and gpu.onevar_bounds_large_stats() == c0
    implicit = s.onevar_bounds_large(ub, l, h, K.FEASTOL)
    explicit = s.onevar_bounds_large(ub, l, h, K.FEASTOL, blocks=jb, vars=jv)
    assert _bits(implicit) == _bits(explicit)
    assert list(implicit[0][m:]) == [-1] * m and all(x in (K.LB, K.INNER, K.INFEASIBLE) for x in implicit[0][:m])
    # ... and the optional outputs missing
    st2 = np.full(cnt, 7, dtype=np.int32)
    assert f(s.h, dp(u), cnt, ip(jb), ip(jv), None, dp(l), dp(h), o, ip(st2), dp(ov), None, None, None) == 0
    assert list(st2) == list(implicit[0])
    s.close()
