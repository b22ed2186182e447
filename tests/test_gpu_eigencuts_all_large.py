"""GPU: hipsdp_eigencuts_all_large - the dense eigenvector cuts and the feasibility eigenvalue of ALL blocks of 129 .. 512 rows in one
call (csrc/eigcuts_large.hip, the batched selection of csrc/syevx.hip) - against the numpy restatement oracle/eigcuts_ref.cuts_dense on
the cases of tests/harness/eigencuts_all_large_cases.py, against the per-block hipsdp_eigencuts, in the storage forms of a block, and
for what makes it a batch: the blocks it turns away, bits that do not depend on the other blocks, their order, the chunks or the
calling thread, and a launch count that is a function of the largest block and of maxcuts > 0 alone.

Tolerances are those tests/test_gpu_eigencuts_all.py applies to hipsdp_eigencuts_all; counts and vectors are compared because the
cases keep their margins (tests/test_eigencuts_all_large_cpu.py recomputes them).  The families are loaded as dense matrices: the
engine sweeps a block of more than 64 rows as packed lower triangles, and a solver with the sparse policy keeps it as nonzeros; full
dense rows are the form of blocks of at most 64 rows, which this call turns away."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import numpy as np
import pytest
from conftest import ROOT
import instances
import eig_cases
import eigencuts_all_large_cases as E
from test_gpu_eigencuts_all import load_dense, load_sparse, same_bits

pytestmark = pytest.mark.gpu

TOL, MAXCUTS, WIDE = E.TOL, E.MAXCUTS, E.WIDE
ERR_ARG = 3
_dev = {}


def device(gpu, name, maxcuts=MAXCUTS):
    """the call on the family loaded as dense matrices, once per (family, maxcuts)"""
    key = (name, maxcuts)
    if key not in _dev:
        blocks, ys, y, b = E.family(name)
        s = load_dense(gpu, blocks, b)
        _dev[key] = s.eigencuts_all_large(y, TOL, maxcuts)
        s.close()
    return _dev[key]


def formula(maxcuts, nmax):
    return 2 + (nmax - 1) + 1 + (2 if maxcuts > 0 else 0) + 1


def check_block(res, name, k, maxcuts, what):
    """counts, lmin, ev[0] == lmin and the six tolerances of tests/test_gpu_eigencuts_all.py for one served block"""
    blocks, ys, y, b = E.family(name)
    rl, rev, rco, rlh, rve = E.reference(name, k, maxcuts)
    lmin, ev, co, lh, ve = res
    print("%s %s block %d (n = %d): ncuts %d / oracle %d, lmin %.12g / %.12g" % (what, name, k, blocks[k].shape[1], len(ev), len(rev), lmin, rl))
    assert len(ev) == len(rev) == maxcuts, (what, name, k)
    assert abs(lmin - rl) <= 1e-9 * max(1.0, abs(rl)), (what, name, k, lmin, rl)
    assert np.max(np.abs(ev - rev)) <= 1e-9 * max(1.0, np.max(np.abs(rev))), (what, name, k)
    assert ev[0] == lmin
    fig = [0.0] * 6
    for c in range(len(ev)):
        v = ve[c]
        f = (abs(np.linalg.norm(v) - 1.0), abs(abs(v @ rve[c]) - 1.0), np.max(np.abs(co[c] - rco[c])) / max(1.0, np.max(np.abs(rco[c]))),
             abs(lh[c] - rlh[c]) / max(1.0, abs(rlh[c])), abs((co[c] @ y - lh[c]) - ev[c]) / max(1.0, abs(ev[c])), -min(0.0, co[c] @ ys - lh[c]))
        fig = [max(a, g) for a, g in zip(fig, f)]
    print("   | |v| - 1 | %.2e, | |v.v_ref| - 1 | %.2e, coefs %.2e, lhs %.2e, cut identity %.2e, violation at ys %.2e" % tuple(fig))
    assert fig[0] <= 1e-10 and fig[1] <= 1e-6 and fig[2] <= 1e-6 and fig[3] <= 1e-6 and fig[4] <= 1e-8 and fig[5] <= 1e-9, (what, name, k, fig)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,maxcuts", [("f3", MAXCUTS), ("n129", MAXCUTS), ("n257", MAXCUTS), ("n512", MAXCUTS), ("n257", WIDE)])
def test_every_served_block_matches_the_oracle(gpu, name, maxcuts):
    blocks, ys, y, b = E.family(name)
    res = device(gpu, name, maxcuts)
    assert len(res) == len(blocks)
    for k in range(len(blocks)):
        if k in E.large_blocks(name):
            check_block(res[k], name, k, maxcuts, "oracle, maxcuts %d:" % maxcuts)
        else:
            assert res[k] is None, k


# ---- 2. against the per-block call -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["f3", "n129"])
def test_served_blocks_agree_with_the_per_block_call(gpu, name):
    blocks, ys, y, b = E.family(name)
    res = device(gpu, name)
    s = load_dense(gpu, blocks, b)
    lchk, _ = s.check_y(y)
    for k in E.large_blocks(name):
        lmin, ev, co, lh, ve = res[k]
        pev, pco, plh, pve = s.eigencuts(k, y, TOL, MAXCUTS)
        assert len(ev) == len(pev) == MAXCUTS
        assert abs(lmin - lchk[k]) <= 1e-8 * max(1.0, abs(lmin)), (k, lmin, lchk[k])
        assert np.max(np.abs(ev - pev)) <= 1e-9 * max(1.0, np.max(np.abs(pev)))
        for c in range(len(ev)):
            assert np.max(np.abs(co[c] - pco[c])) <= 1e-6 * max(1.0, np.max(np.abs(pco[c])))
            assert abs(lh[c] - plh[c]) <= 1e-6 * max(1.0, abs(plh[c]))
            assert abs(abs(ve[c] @ pve[c]) - 1.0) <= 1e-6
    s.close()


# ---- 3. / 4. / 5. sentinels: a feasible point, maxcuts = 0, the blocks turned away -------------------------------------------------------

def _raw(gpu, s, y, maxcuts, fill, nullcuts=False, nullvec=False):
    lib = gpu.lib()
    nb, m = len(s.ns), len(y)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    mc = max(1, maxcuts)
    arr = dict(ncuts=np.full(nb, 77, dtype=np.int32), lmin=np.full(nb, fill), eigvals=np.full(nb * mc, fill),
               coefs=np.full(nb * mc * m, fill), lhs=np.full(nb * mc, fill), vecs=np.full(mc * sum(s.ns), fill))
    y = np.ascontiguousarray(y, dtype=np.float64)
    rc = lib.hipsdp_eigencuts_all_large(s.h, dp(y), C.c_double(TOL), maxcuts, ip(arr["ncuts"]), dp(arr["lmin"]),
                                        None if nullcuts else dp(arr["eigvals"]), None if nullcuts else dp(arr["coefs"]),
                                        None if nullcuts else dp(arr["lhs"]), None if (nullcuts or nullvec) else dp(arr["vecs"]))
    return rc, arr


def _untouched(a, k, n, off, m, fill, first=0, maxcuts=MAXCUTS):
    """slots first .. maxcuts - 1 of block k hold the sentinel"""
    lo, hi = k * maxcuts + first, (k + 1) * maxcuts
    return (np.all(a["eigvals"][lo:hi] == fill) and np.all(a["lhs"][lo:hi] == fill) and np.all(a["coefs"][lo * m:hi * m] == fill)
            and np.all(a["vecs"][off + first * n:off + maxcuts * n] == fill))


def test_a_feasible_point_has_nothing_to_cut_and_no_slot_is_written(gpu):
    ns, m, fill = [16, 150, 48, 200, 10], E.M, 777.0
    blocks, ys, y, b = E.family("f3")
    s = load_dense(gpu, blocks, b)
    rc, a = _raw(gpu, s, ys, MAXCUTS, fill)
    assert rc == 0 and list(a["ncuts"]) == [-1, 0, -1, 0, -1]
    l0, _ = s.check_y(ys)
    off = 0
    for k, n in enumerate(ns):
        assert _untouched(a, k, n, off, m, fill), k
        if k in (1, 3):
            assert a["lmin"][k] >= -1e-9 and abs(a["lmin"][k] - l0[k]) <= 1e-8 * max(1.0, abs(l0[k])), (k, a["lmin"][k], l0[k])
        else:
            assert a["lmin"][k] == fill
        off += MAXCUTS * n
    res = s.eigencuts_all_large(ys, TOL, MAXCUTS)
    assert res[0] is None and len(res[1][1]) == 0 and res[1][2].shape == (0, m) and res[3][4].shape == (0, 200)
    s.close()


def test_no_cuts_wanted_is_a_feasibility_check(gpu):
    """lmin only, with eigvals, coefs, lhs and vecs NULL; the launches are the formula's maxcuts == 0 value"""
    blocks, ys, y, b = E.family("f3")
    s = load_dense(gpu, blocks, b)
    s.eigencuts_all_large(y, TOL, 0)                    # first use (workspace, job table)
    c0, l0, r0 = gpu.eigencuts_all_large_stats()
    rc, a = _raw(gpu, s, y, 0, 777.0, nullcuts=True)
    c1, l1, r1 = gpu.eigencuts_all_large_stats()
    assert rc == 0 and list(a["ncuts"]) == [-1, 0, -1, 0, -1]
    assert (c1 - c0, l1 - l0, r1 - r0) == (1, formula(0, 200), 1) == (1, 203, 1)
    full = device(gpu, "f3")
    for k in (1, 3):
        want = E.reference("f3", k, MAXCUTS)[0]
        assert abs(a["lmin"][k] - want) <= 1e-9 * max(1.0, abs(want)) and a["lmin"][k] < -TOL
        # (eigenvalue 1 by index and slot 0 of the selection are two multisections of the same matrix: they need not round alike)
        assert abs(a["lmin"][k] - full[k][0]) <= 1e-9 * max(1.0, abs(want)), (k, a["lmin"][k], full[k][0])
    assert a["lmin"][0] == 777.0 and a["lmin"][2] == 777.0 and a["lmin"][4] == 777.0
    r = s.eigencuts_all_large(y, TOL, 0)
    assert r[0] is None and r[1][0] == a["lmin"][1] and len(r[1][1]) == 0 and r[3][4].shape == (0, 200)
    s.close()


def test_blocks_the_call_turns_away_get_minus_one_and_nothing_else(gpu):
    ns, m, fill = [16, 150, 48, 200, 10], E.M, 777.0
    blocks, ys, y, b = E.family("f3")
    s = load_dense(gpu, blocks, b)
    for mc in (MAXCUTS, 2):
        rc, a = _raw(gpu, s, y, mc, fill)
        assert rc == 0 and list(a["ncuts"]) == [-1, mc, -1, mc, -1]
        off = 0
        for k, n in enumerate(ns):
            if k in (1, 3):
                assert a["lmin"][k] != fill and a["lmin"][k] == a["eigvals"][k * mc]
                assert np.all(a["eigvals"][k * mc:(k + 1) * mc] != fill) and np.all(a["vecs"][off:off + mc * n] != fill)
            else:
                assert a["lmin"][k] == fill and _untouched(a, k, n, off, m, fill, maxcuts=mc), (mc, k)
            off += mc * n
    # vecs may be NULL: the rest is what the full call writes
    rc5, a5 = _raw(gpu, s, y, MAXCUTS, fill)
    rc, a2 = _raw(gpu, s, y, MAXCUTS, fill, nullvec=True)
    assert rc == rc5 == 0 and np.all(a2["vecs"] == fill)
    for key in ("ncuts", "lmin", "eigvals", "coefs", "lhs"):
        assert np.array_equal(a2[key], a5[key]), key
    s.close()


def test_a_call_without_a_served_block_launches_nothing_and_argument_errors_with_a_solver(gpu):
    """blocks of 128 and 513 rows alone: both -1, nothing launched, the totals stay; the argument errors with a live solver"""
    m = 2
    blocks = []
    for n, seed in ((128, 51), (513, 53)):
        b, A, ys, Xs, Zs = instances.planted_dense(n, m, seed)
        blocks.append(A)
    y = np.array([0.3, -0.2])
    s = load_dense(gpu, blocks, np.ones(m))
    before = gpu.eigencuts_all_large_stats()
    rc, a = _raw(gpu, s, y, MAXCUTS, 777.0)
    assert rc == 0 and list(a["ncuts"]) == [-1, -1] and np.all(a["lmin"] == 777.0) and np.all(a["vecs"] == 777.0)
    assert np.all(a["eigvals"] == 777.0) and np.all(a["coefs"] == 777.0) and np.all(a["lhs"] == 777.0)
    assert s.eigencuts_all_large(y, TOL, MAXCUTS) == [None, None]
    assert gpu.eigencuts_all_large_stats() == before
    # argument errors: nothing written, nothing counted
    L = gpu.lib()
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    k = (C.c_int * 2)(77, 77)
    buf = np.zeros(4096)
    tol = C.c_double(TOL)
    unshaped = gpu.Solver(0)
    assert L.hipsdp_eigencuts_all_large(None, dp(y), tol, MAXCUTS, k, dp(buf), dp(buf), dp(buf), dp(buf), None) == ERR_ARG
    assert L.hipsdp_eigencuts_all_large(unshaped.h, dp(y), tol, MAXCUTS, k, dp(buf), dp(buf), dp(buf), dp(buf), None) == ERR_ARG
    unshaped.close()
    assert L.hipsdp_eigencuts_all_large(s.h, None, tol, MAXCUTS, k, dp(buf), dp(buf), dp(buf), dp(buf), None) == ERR_ARG
    assert L.hipsdp_eigencuts_all_large(s.h, dp(y), tol, MAXCUTS, None, dp(buf), dp(buf), dp(buf), dp(buf), None) == ERR_ARG
    assert L.hipsdp_eigencuts_all_large(s.h, dp(y), tol, -1, k, dp(buf), dp(buf), dp(buf), dp(buf), None) == ERR_ARG
    assert L.hipsdp_eigencuts_all_large(s.h, dp(y), tol, 33, k, dp(buf), dp(buf), dp(buf), dp(buf), None) == ERR_ARG
    assert L.hipsdp_eigencuts_all_large(s.h, dp(y), tol, MAXCUTS, k, dp(buf), None, dp(buf), dp(buf), None) == ERR_ARG
    assert L.hipsdp_eigencuts_all_large(s.h, dp(y), tol, MAXCUTS, k, dp(buf), dp(buf), None, dp(buf), None) == ERR_ARG
    assert L.hipsdp_eigencuts_all_large(s.h, dp(y), tol, MAXCUTS, k, dp(buf), dp(buf), dp(buf), None, None) == ERR_ARG
    assert list(k) == [77, 77] and gpu.eigencuts_all_large_stats() == before
    assert L.hipsdp_eigencuts_all_large(s.h, dp(y), tol, 32, k, dp(buf), dp(buf), dp(buf), dp(buf), None) == 0 and list(k) == [-1, -1]
    s.close()


# ---- 6. bits ---------------------------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_a_block_alone_and_the_reversed_order_give_the_same_bits(gpu):
    blocks, ys, y, b = E.family("f3")
    full = device(gpu, "f3")
    served = lambda r: [x for x in r if x is not None]
    s = load_dense(gpu, blocks, b)
    for _ in range(2):                                  # (the second one on a used workspace)
        again = s.eigencuts_all_large(y, TOL, MAXCUTS)
        assert [x is None for x in again] == [x is None for x in full] and same_bits(served(again), served(full))
    s.close()
    s1 = load_dense(gpu, [blocks[3]], b)
    assert same_bits(s1.eigencuts_all_large(y, TOL, MAXCUTS), [full[3]])
    s1.close()
    sr = load_dense(gpu, blocks[::-1], b)
    rev = sr.eigencuts_all_large(y, TOL, MAXCUTS)
    sr.close()
    assert [x is None for x in rev[::-1]] == [x is None for x in full] and same_bits(served(rev[::-1]), served(full))


_CHILD = r"""
import sys, json
import numpy as np
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(harness)r); sys.path.insert(0, %(oracle)r)
import importlib.util
spec = importlib.util.spec_from_file_location("hb_child", %(binding)r)
hb = importlib.util.module_from_spec(spec); spec.loader.exec_module(hb)
import eigencuts_all_large_cases as E
import test_gpu_eigencuts_all as T
blocks, ys, y, b = E.family(%(family)r)
s = T.load_dense(hb, blocks, b)
c0 = hb.eigencuts_all_large_stats()
res = s.eigencuts_all_large(y, E.TOL, E.MAXCUTS)
c1 = hb.eigencuts_all_large_stats()
s.close()
print(json.dumps({"bits": [None if r is None else [np.asarray(a).tobytes().hex() for a in r] for r in res],
                  "stats": [c1[k] - c0[k] for k in range(3)]}))
"""


def _child(chunk, family="f3"):
    env = dict(os.environ)
    env.pop("HIPSDP_EIGENCUTS_LARGE_CHUNK", None)
    if chunk:
        env["HIPSDP_EIGENCUTS_LARGE_CHUNK"] = str(chunk)
    code = _CHILD % {"family": family, "tests": os.path.join(ROOT, "tests"), "harness": os.path.join(ROOT, "tests", "harness"),
                     "oracle": os.path.join(ROOT, "oracle"), "binding": os.path.join(ROOT, "scip-sdp_amd", "binding.py")}
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bits_do_not_depend_on_the_chunking(gpu):
    """HIPSDP_EIGENCUTS_LARGE_CHUNK=1 against the default, each in a fresh child process: the two large blocks of f3 in two chunks (200
    rows first) - the same bits as the unchunked call of this process, one read-back per chunk, the launches of a chunk those of its own
    largest block"""
    one, two = _child(0), _child(1)
    assert one["bits"] == two["bits"]
    here = [None if r is None else [np.asarray(a).tobytes().hex() for a in r] for r in device(gpu, "f3")]
    assert one["bits"] == here
    assert one["stats"] == [1, formula(MAXCUTS, 200), 1]
    assert two["stats"] == [1, formula(MAXCUTS, 200) + formula(MAXCUTS, 150), 2]


def test_a_chunk_of_several_blocks_that_is_not_the_whole_call(gpu):
    """family f4 - blocks of 130, 12, 129, 131 rows, served by descending rows as 3, 0, 2 - with the chunk variable unset (one chunk
    of three), 2 (blocks 3 and 0, then block 2: a chunk whose own vector offsets differ from the caller's) and 1, each in a fresh
    child process: the same bits, the 12-row block turned away, one read-back per chunk, the launches of a chunk those of its own
    largest block"""
    whole, pair, single = (_child(c, E.CHUNKED) for c in (0, 2, 1))
    print("stats %s / %s / %s" % (whole["stats"], pair["stats"], single["stats"]))
    assert whole["bits"] == pair["bits"] == single["bits"]
    assert whole["bits"][1] is None and all(whole["bits"][k] is not None for k in (0, 2, 3))      # (None: ncuts = -1)
    f = lambda n: formula(MAXCUTS, n)
    assert whole["stats"] == [1, f(131), 1]
    assert pair["stats"] == [1, f(131) + f(129), 2]
    assert single["stats"] == [1, f(131) + f(130) + f(129), 3]


def test_two_host_threads_reproduce_the_single_thread_bits(gpu):
    names = ["f3", "n129"]
    data = [E.family(f) for f in names]
    solvers = [load_dense(gpu, d[0], d[3]) for d in data]
    single = [[x for x in device(gpu, f) if x is not None] for f in names]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                got[i].append([x for x in solvers[i].eigencuts_all_large(data[i][2], TOL, MAXCUTS) if x is not None])
        except Exception as e:          # noqa: BLE001 - reported by the assertion below
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for i in range(2):
        assert len(got[i]) == 3
        for r in got[i]:
            assert same_bits(r, single[i])
    for s in solvers:
        s.close()


# ---- 7. storage forms ------------------------------------------------------------------------------------------------------------------

def test_the_storage_forms_give_the_same_cuts(gpu):
    """f3 loaded as dense input (its large blocks swept as packed lower triangles) and as triplets under sparse_policy(2) (kept as
    nonzeros): both match the oracle, and each other to the coefficient tolerance"""
    blocks, ys, y, b = E.family("f3")
    sd, ss = load_dense(gpu, blocks, b), load_sparse(gpu, blocks, b)
    for k in (1, 3):
        assert ss.is_sparse(k) and not sd.is_sparse(k), k
    rd, rs = sd.eigencuts_all_large(y, TOL, MAXCUTS), ss.eigencuts_all_large(y, TOL, MAXCUTS)
    assert [x is None for x in rd] == [x is None for x in rs] == [True, False, True, False, True]
    for k in (1, 3):
        check_block(rd[k], "f3", k, MAXCUTS, "packed:")
        check_block(rs[k], "f3", k, MAXCUTS, "nonzeros:")
        (ld, ed, cd, hd, vd), (ls, es, cs, hs, vs) = rd[k], rs[k]
        assert abs(ld - ls) <= 1e-9 * max(1.0, abs(ld))
        assert np.max(np.abs(ed - es)) <= 1e-9 * max(1.0, np.max(np.abs(ed)))
        for c in range(MAXCUTS):
            assert abs(abs(vd[c] @ vs[c]) - 1.0) <= 1e-6
            assert np.max(np.abs(cd[c] - cs[c])) <= 1e-6 * max(1.0, np.max(np.abs(cd[c])))
            assert abs(hd[c] - hs[c]) <= 1e-6 * max(1.0, abs(hd[c]))
    sd.close()
    ss.close()


# ---- 8. launches and read-backs --------------------------------------------------------------------------------------------------------

def _other_totals(gpu):
    return (gpu.eigencuts_all_stats(), gpu.sparsecuts_all_stats(), gpu.sparsecuts_stats(), gpu.sparsecuts_ex_stats(),
            gpu.sparsecuts_all_large_stats())


def test_launches_and_readbacks_are_the_formula(gpu):
    """one block (129 rows) and the two large blocks of f3 (nmax = 200), maxcuts 5, 1, 32, 0: the formula of the header, one read-back;
    the totals of hipsdp_eigencuts_all and of the four sparse-cut calls do not move"""
    others = _other_totals(gpu)
    for name, nmax in (("n129", 129), ("f3", 200)):
        blocks, ys, y, b = E.family(name)
        s = load_dense(gpu, blocks, b)
        for mc in (MAXCUTS, 1, WIDE, 0):
            c0, l0, r0 = gpu.eigencuts_all_large_stats()
            res = s.eigencuts_all_large(y, TOL, mc)
            c1, l1, r1 = gpu.eigencuts_all_large_stats()
            print("%s maxcuts %d: %d launches (formula %d), %d read-backs" % (name, mc, l1 - l0, formula(mc, nmax), r1 - r0))
            assert (c1 - c0, l1 - l0, r1 - r0) == (1, formula(mc, nmax), 1), (name, mc)
            assert l1 - l0 <= nmax + 6
            assert all(len(res[k][1]) == mc for k in E.large_blocks(name))
        s.close()
    assert _other_totals(gpu) == others


def test_launches_do_not_depend_on_the_number_of_blocks_and_the_totals_are_separate(gpu):
    """one 200-row block and four of them: the same launches and read-backs; the other cut calls on the same solver do not move this
    call's totals"""
    blocks, ys, y, b = E.family("f3")
    deltas = {}
    for label, cnt in (("one", 1), ("four", 4)):
        s = load_dense(gpu, [blocks[3]] * cnt, b)
        for mc in (MAXCUTS, 0):
            c0, l0, r0 = gpu.eigencuts_all_large_stats()
            res = s.eigencuts_all_large(y, TOL, mc)
            c1, l1, r1 = gpu.eigencuts_all_large_stats()
            deltas[(label, mc)] = (c1 - c0, l1 - l0, r1 - r0)
            assert same_bits(res, [res[0]] * cnt)             # (every copy of the block has the block's bits)
        mine = gpu.eigencuts_all_large_stats()
        before = _other_totals(gpu)
        s.eigencuts_all(y, TOL, 1)
        s.sparsecuts_all(y, [10] * cnt, TOL, 1e-6, 1)
        s.sparsecuts(0, y, 10, TOL, 1e-6, 1)
        s.sparsecuts_all_ex(y, [10] * cnt, TOL, 1e-6, 1, 1)
        s.sparsecuts_all_large(y, [10] * cnt, TOL, 1e-6, 1, 0)
        after = _other_totals(gpu)
        assert all(a[0] == p[0] + 1 for a, p in zip(after, before)), (before, after)
        assert gpu.eigencuts_all_large_stats() == mine
        s.close()
    for mc in (MAXCUTS, 0):
        assert deltas[("one", mc)] == deltas[("four", mc)] == (1, formula(mc, 200), 1), mc


# ---- 9. / 10. the unit entry of the batched selection ------------------------------------------------------------------------------------

@pytest.mark.parametrize("cap", [1, 128])
def test_the_batched_selection_has_the_bits_of_syevx_below(gpu, cap):
    """mixed sizes 129, 200, 257 through the staging, the column launches with `cap` workgroups per matrix and the batched selection:
    count, values and vectors of every matrix are those of hipsdp_syevx_below called on it alone"""
    ns = (129, 200, 257)
    mats, bounds = [], []
    for n in ns:
        W, ev, scale = eig_cases.spectra(n)["random"]
        mats.append(np.array(W))
        bounds.append(0.5 * (ev[2] + ev[3]))
    # one bound for the launch: the midpoint between eigenvalues 3 and 4 of the FIRST matrix; what it selects of the others is whatever
    # hipsdp_syevx_below selects of them at the same bound
    for bound in (bounds[0], bounds[2]):
        got = gpu.syevx_many_below_unit(mats, bound, 32, cap)
        total = 0
        for n, W, (cnt, lam, V) in zip(ns, mats, got):
            lam1, V1, nbelow = gpu.syevx_below(W, bound, 32)
            print("n = %d cap %d bound %.6g: %d pairs (alone %d of %d below)" % (n, cap, bound, cnt, len(lam1), nbelow))
            assert cnt == len(lam1) == min(nbelow, 32)
            assert lam.tobytes() == lam1.tobytes() and V.tobytes() == V1.tobytes(), (n, cap)
            total += cnt
        assert total >= 3
    # ... and each matrix at its own midpoint: exactly 3 pairs, accurate (a batch of one)
    for n, W, bound in zip(ns, mats, bounds):
        (cnt, lam, V), = gpu.syevx_many_below_unit([W], bound, 32, cap)
        lam1, V1, nbelow = gpu.syevx_below(W, bound, 32)
        assert cnt == 3 == nbelow and lam.tobytes() == lam1.tobytes() and V.tobytes() == V1.tobytes(), (n, cap)
        Wc, ev, scale = eig_cases.spectra(n)["random"]
        eig_cases.check_pairs("random", Wc, ev, scale, 1, lam, V)


def test_the_batched_selection_on_a_multiple_eigenvalue(gpu):
    """the 117 eigenvalues -0.01 of the shifted low-rank matrix of 129 rows, bound -1e-6, maxk 5: residual and orthonormality inside the
    cluster to the figures of check_pairs"""
    W, ev, scale = eig_cases.spectra(129)["low_rank_shifted"]
    (cnt, lam, V), = gpu.syevx_many_below_unit([np.array(W)], -1e-6, 5, 128)
    assert cnt == 5
    eig_cases.check_pairs("low_rank_shifted", W, ev, scale, 1, lam, V)


# ---- 11. a multiple negative eigenvalue through the public call ------------------------------------------------------------------------

def test_a_multiple_negative_eigenvalue_through_the_call(gpu):
    """one block of 129 rows, m = 1, A_0 = -W, y = 0: 5 cuts of eigenvalue -0.01; the vectors are any orthonormal basis of a
    5-dimensional part of the eigenspace, so they are checked as pairs of Z (check_pairs), not against the oracle's vectors"""
    blocks, y, b, W, ev = E.multiple_case()
    s = load_dense(gpu, blocks, b)
    (lmin, lam, co, lh, ve), = s.eigencuts_all_large(y, TOL, MAXCUTS)
    s.close()
    assert len(lam) == 5 and lam[0] == lmin
    eig_cases.check_pairs("low_rank_shifted, the call", W, ev, max(1.0, np.abs(ev).max()), 1, lam, ve)
    A = blocks[0]
    for c in range(5):
        assert abs((co[c] @ y - lh[c]) - lam[c]) <= 1e-8 * max(1.0, abs(lam[c])), c
        assert abs(co[c][0] - ve[c] @ A[1] @ ve[c]) <= 1e-6 * max(1.0, abs(co[c][0])), c
