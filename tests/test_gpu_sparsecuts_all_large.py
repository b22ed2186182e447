"""GPU: hipsdp_sparsecuts_all_large - the sparse eigenvector cuts of ALL blocks of 129 .. 512 rows in one call, with the reference's
switches recomputesparseev, recomputeinitial and exacttrans as a bit mask, zero included (csrc/sparsecuts_large_rounds.hip) - against
the numpy restatement tests/harness/sparsecuts_variants_ref.py on the cases of tests/harness/sparsecuts_all_large_cases.py, with
variant 0 against hipsdp_sparsecuts block by block, for the properties that need no oracle, and for what makes it a batch: the blocks
it turns away, bits that do not depend on the other blocks, their order, the chunks or the calling thread, and a launch count that is
a function of (variant, maxcuts, nmax) alone.

Counts, supports and iteration numbers are compared only after the restatement has shown the case stable (check_margins of the cases
file; tests/test_sparsecuts_all_large_cpu.py runs it for every case).  Tolerances are those of tests/test_gpu_sparsecuts_variants.py.
The families are loaded as dense matrices: the engine sweeps a block of more than 64 rows as packed lower triangles, and a solver
with the sparse policy keeps it as nonzeros; full dense rows are the form of blocks of at most 64 rows, which this call turns away."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading
import numpy as np
import pytest
from conftest import ROOT
import sparsecuts_all_large_cases as L
from test_gpu_sparsecuts_all import load_dense, load_sparse, same_bits, support

pytestmark = pytest.mark.gpu

TOL, FEASTOL, MAXCUTS = L.TOL, L.FEASTOL, L.MAXCUTS
ERR_ARG = 3
_dev, _one = {}, {}


def device(gpu, name, size, variant):
    """the call on the family loaded as dense matrices, once per case"""
    key = (name, size, variant)
    if key not in _dev:
        blocks, ys, y, b = L.family(name)
        s = load_dense(gpu, blocks, b)
        _dev[key] = s.sparsecuts_all_large(y, [size] * len(blocks), TOL, FEASTOL, MAXCUTS, variant)
        s.close()
    return _dev[key]


def formula(variant, maxcuts, nmax):
    s, d = int(bool(variant & 1)), int(bool(variant & 6))
    rounds = maxcuts if variant else 0
    return 1 + (nmax + 3) + rounds * (1 + 4 * s + d * (nmax + 3)) + 1 + (1 if maxcuts > 0 else 0)


# ---- 1. against the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,k,size,variant", L.CASES + L.CASES0)
def test_every_row_matches_the_restatement(gpu, name, k, size, variant):
    L.check_margins(name, k, size, variant)
    blocks, ys, y, b = L.family(name)
    rn, rl, rev, rco, rlh, rve, rsup, rit, rfl, mg, runs = L.reference(name, k, size, variant)
    res = device(gpu, name, size, variant)
    assert len(res) == len(blocks)
    nc, lmin, ev, co, lh, ve, iters, flags = res[k]
    print("%s block %d (n = %d) size %d variant %d: ncuts %d / %d, iterations %d / %d, flags %d / %d, lmin %.12g / %.12g"
          % (name, k, blocks[k].shape[1], size, variant, nc, rn, iters, rit, flags, rfl, lmin, rl))
    assert nc == rn >= 1 and iters == rit and flags == rfl
    assert abs(lmin - rl) <= 1e-9 * max(1.0, abs(rl))
    for c in range(nc):
        assert support(ve[c]) == list(rsup[c]), c
        assert abs(ev[c] - rev[c]) <= 1e-9 * max(1.0, abs(rev[c])), c
        assert abs(abs(ve[c] @ rve[c]) - 1.0) <= 1e-6, c
        assert np.max(np.abs(co[c] - rco[c])) <= 1e-6 * max(1.0, np.max(np.abs(rco[c]))), c
        assert abs(lh[c] - rlh[c]) <= 1e-6 * max(1.0, abs(rlh[c])), c


@pytest.mark.parametrize("variant", [0, 1, 2, 4, 7])
def test_the_loop_that_ends_at_once(gpu, variant):
    """the 200-row block of f3 at size 4: no cut under any mask, the iterations of its one run counted"""
    name, k, size = L.QUIET
    r = L.reference(name, k, size, variant)
    nc, lmin, ev, co, lh, ve, iters, flags = device(gpu, name, size, variant)[k]
    assert (nc, iters, flags) == (0, r[7], 0) == (0, 73, 0) and abs(lmin - r[1]) <= 1e-9 * abs(r[1])


# ---- 2. variant 0 against hipsdp_sparsecuts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,size", [("f3", 4), ("f3", 10), ("n129", 24), ("n257", 10), ("n512", 24)])
def test_variant_0_against_the_per_block_call(gpu, name, size):
    """counts, iterations, supports and flags equal, values to 1e-9 relative; whether the bits agree is printed (they need not: the
    tridiagonal form comes from the batched kernels)"""
    blocks, ys, y, b = L.family(name)
    res = device(gpu, name, size, 0)
    s = load_dense(gpu, blocks, b)
    for k in L.large_blocks(name):
        one = s.sparsecuts(k, y, size, TOL, FEASTOL, MAXCUTS)
        nc, lmin, ev, co, lh, ve, iters, flags = res[k]
        print("%s block %d size %d: same bits as hipsdp_sparsecuts: %s (ncuts %d, iterations %d)" % (name, k, size, same_bits([one], [res[k]]), nc, iters))
        assert (one[0], one[6], one[7]) == (nc, iters, flags) and nc >= 0
        assert abs(one[1] - lmin) <= 1e-9 * max(1.0, abs(lmin))
        for c in range(nc):
            assert support(one[5][c]) == support(ve[c]), (k, c)
            assert abs(one[2][c] - ev[c]) <= 1e-9 * max(1.0, abs(ev[c])), (k, c)
            assert np.max(np.abs(one[5][c] - ve[c])) <= 1e-9, (k, c)
            assert np.max(np.abs(one[3][c] - co[c])) <= 1e-9 * max(1.0, np.max(np.abs(co[c]))), (k, c)
            assert abs(one[4][c] - lh[c]) <= 1e-9 * max(1.0, abs(lh[c])), (k, c)
    s.close()
    assert sum(max(res[k][0], 0) for k in L.large_blocks(name)) >= 1


# ---- 3. properties that need no oracle -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,size,variant", sorted(set((f, sz, v) for f, k, sz, v in L.CASES + L.CASES0)) + [("f3", 10, 0), ("f3", 4, 0)])
def test_properties_that_need_no_oracle(gpu, name, size, variant):
    """Z_c is the matrix after the deflations the outputs themselves describe; the cut is built from the A_i, so coefs @ y - lhs is
    x^T Z(y) x, and the value of the cut is x^T Z_c x (the forms tests/test_gpu_sparsecuts_variants.py checks)"""
    blocks, ys, y, b = L.family(name)
    res = device(gpu, name, size, variant)
    for k in L.large_blocks(name):
        A = blocks[k]
        nc, lmin, ev, co, lh, ve, iters, flags = res[k]
        assert nc >= 0
        Z0 = np.tensordot(y, A[1:], axes=(0, 0)) - A[0]
        Zc = Z0.copy()
        znorm = np.linalg.norm(Z0, 2)
        for c in range(nc):
            x = ve[c]
            S = support(x)
            assert abs(np.linalg.norm(x) - 1.0) <= 1e-10, (k, c)
            assert len(S) <= size and np.all(x[np.setdiff1d(np.arange(len(x)), S)] == 0.0), (k, c)
            viol = co[c] @ y - lh[c]
            assert abs(viol - x @ Z0 @ x) <= 1e-8, (k, c, viol)
            assert abs(viol - sum(ev[j] * (ve[j] @ x) ** 2 for j in range(c)) - x @ Zc @ x) <= 1e-8, (k, c, viol)
            assert abs(ev[c] - x @ Zc @ x) <= 1e-8, (k, c, ev[c])
            if c == 0:                                                             # (no deflation yet: coefs . y - lhs = eigvals)
                assert abs(viol - ev[0]) <= 1e-9, (k, viol, ev[0])
            assert viol <= ev[c] + 1e-8 and viol < -FEASTOL, (k, c, viol)
            assert co[c] @ ys - lh[c] >= -1e-9, (k, c)
            if variant & 1:
                sub = Zc[np.ix_(S, S)]
                assert abs(ev[c] - np.linalg.eigvalsh(sub)[0]) <= 1e-8 * znorm, (k, c)
                assert np.linalg.norm(sub @ x[S] - ev[c] * x[S]) <= 1e-8 * znorm, (k, c)
            Zc = Zc - ev[c] * np.outer(x, x)


# ---- 4. turned away ------------------------------------------------------------------------------------------------------------------

def _raw(gpu, s, y, sizes, maxcuts, variant, fill, nullcuts=False):
    lib = gpu.lib()
    nb, m = len(s.ns), len(y)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    mc = max(1, maxcuts)
    arr = dict(ncuts=np.full(nb, 77, dtype=np.int32), lmin=np.full(nb, fill), eigvals=np.full(nb * mc, fill),
               coefs=np.full(nb * mc * m, fill), lhs=np.full(nb * mc, fill), vecs=np.full(mc * sum(s.ns), fill),
               iters=np.full(nb, 77, dtype=np.int32), flags=np.full(nb, 77, dtype=np.int32))
    y = np.ascontiguousarray(y, dtype=np.float64)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    opts = gpu.SparsecutOpts(TOL, FEASTOL, 0.0, maxcuts, 0)
    rc = lib.hipsdp_sparsecuts_all_large(s.h, dp(y), ip(sizes), C.byref(opts), C.c_uint(variant), ip(arr["ncuts"]), dp(arr["lmin"]),
                                         None if nullcuts else dp(arr["eigvals"]), None if nullcuts else dp(arr["coefs"]),
                                         None if nullcuts else dp(arr["lhs"]), dp(arr["vecs"]), ip(arr["iters"]), ip(arr["flags"]))
    return rc, arr


def _untouched(a, k, n, off, m, fill, first=0):
    """slots first .. MAXCUTS - 1 of block k hold the sentinel"""
    lo, hi = k * MAXCUTS + first, (k + 1) * MAXCUTS
    return (np.all(a["eigvals"][lo:hi] == fill) and np.all(a["lhs"][lo:hi] == fill) and np.all(a["coefs"][lo * m:hi * m] == fill)
            and np.all(a["vecs"][off + first * n:off + MAXCUTS * n] == fill))


def test_blocks_the_call_turns_away_get_minus_one_and_nothing_else(gpu):
    ns, m = [16, 150, 48, 200, 10], 25
    blocks, ys, y, b = L.family("f3")
    s = load_dense(gpu, blocks, b)
    fill = 777.0
    for variant, sizes in ((0, [4] * 5), (1, [4] * 5), (7, [10] * 5), (1, [4, 129, 4, 10, 4]), (2, [4, 129, 4, 10, 4])):
        rc, a = _raw(gpu, s, y, sizes, MAXCUTS, variant, fill)
        assert rc == 0
        off = 0
        for k, n in enumerate(ns):
            away = n <= 128 or (variant & 1 and sizes[k] > 128)
            if away:
                assert a["ncuts"][k] == -1 and a["lmin"][k] == fill and a["iters"][k] == 77 and a["flags"][k] == 77, (variant, k)
                assert _untouched(a, k, n, off, m, fill), (variant, k)
            else:
                kept = int(a["ncuts"][k])
                assert kept >= 0 and a["lmin"][k] != fill and a["iters"][k] != 77 and a["flags"][k] != 77, (variant, k)
                assert _untouched(a, k, n, off, m, fill, first=kept), (variant, k)          # slots c >= ncuts: not written
                assert np.all(a["eigvals"][k * MAXCUTS:k * MAXCUTS + kept] != fill), (variant, k)
            off += MAXCUTS * n
        # the 200-row block is served in every one of them (at size 4 its loop ends at once: 0 cuts, its run counted)
        assert a["ncuts"][3] >= (1 if sizes[3] == 10 else 0) and a["iters"][3] >= 73
    # the served block's bits do not depend on what happens to the other one
    rc, a1 = _raw(gpu, s, y, [4, 129, 4, 10, 4], MAXCUTS, 1, fill)
    rc, a2 = _raw(gpu, s, y, [10] * 5, MAXCUTS, 1, fill)
    lo, hi = 3 * MAXCUTS, 4 * MAXCUTS
    assert a1["ncuts"][3] == a2["ncuts"][3] and np.array_equal(a1["eigvals"][lo:hi], a2["eigvals"][lo:hi])
    # a size above 128 WITHOUT recomputesparseev is served (mask 2 above), and size 129 on the 129-row block is size == n
    s.close()
    blocks1, ys1, y1, b1 = L.family("n129")
    s1 = load_dense(gpu, blocks1, b1)
    r = s1.sparsecuts_all_large(y1, [129], TOL, FEASTOL, MAXCUTS, 2)[0]
    assert r[0] >= 1 and len(support(r[5][0])) <= 129
    assert s1.sparsecuts_all_large(y1, [130], TOL, FEASTOL, MAXCUTS, 2)[0][0] == 0          # size > n: no cut (cons_sdp.c:1403)
    assert s1.sparsecuts_all_large(y1, [129], TOL, FEASTOL, MAXCUTS, 3)[0][0] == -1
    s1.close()


def test_a_call_without_a_served_block_launches_nothing_and_argument_errors_with_a_solver(gpu):
    blocks, ys, y, b = L.family("f3")
    small = [blocks[0], blocks[2], blocks[4]]
    s = load_dense(gpu, small, b)
    before = gpu.sparsecuts_all_large_stats()
    res = s.sparsecuts_all_large(y, [4] * 3, TOL, FEASTOL, MAXCUTS, 7)
    assert [r[0] for r in res] == [-1, -1, -1] and gpu.sparsecuts_all_large_stats() == before
    for variant, sizes, mc in ((8, [4] * 3, MAXCUTS), (1, [4, 0, 4], MAXCUTS), (0, [4] * 3, -1)):
        rc, a = _raw(gpu, s, y, sizes, mc, variant, 777.0)
        assert rc == ERR_ARG and list(a["ncuts"]) == [77] * 3, (variant, sizes, mc)
    rc, a = _raw(gpu, s, y, [4] * 3, MAXCUTS, 0, 777.0, nullcuts=True)
    assert rc == ERR_ARG and list(a["ncuts"]) == [77] * 3
    assert gpu.sparsecuts_all_large_stats() == before
    s.close()


# ---- 5. bits ---------------------------------------------------------------------------------------------------------------------------

def test_the_same_call_twice_a_block_alone_and_the_reversed_order_give_the_same_bits(gpu):
    name = "f3"
    blocks, ys, y, b = L.family(name)
    nb = len(blocks)
    for size, variant in ((10, 0), (10, 7), (4, 1), (10, 2)):
        full = device(gpu, name, size, variant)
        s = load_dense(gpu, blocks, b)
        assert same_bits(s.sparsecuts_all_large(y, [size] * nb, TOL, FEASTOL, MAXCUTS, variant), full)
        assert same_bits(s.sparsecuts_all_large(y, [size] * nb, TOL, FEASTOL, MAXCUTS, variant), full)       # (a used workspace)
        s.close()
        for k in (1, 3):
            s1 = load_dense(gpu, [blocks[k]], b)
            assert same_bits(s1.sparsecuts_all_large(y, [size], TOL, FEASTOL, MAXCUTS, variant), [full[k]]), (size, variant, k)
            s1.close()
        sr = load_dense(gpu, blocks[::-1], b)
        rev = sr.sparsecuts_all_large(y, [size] * nb, TOL, FEASTOL, MAXCUTS, variant)
        sr.close()
        assert same_bits(rev[::-1], full), (size, variant)


_CHILD = r"""
import sys, json
import numpy as np
sys.path.insert(0, %(tests)r); sys.path.insert(0, %(harness)r); sys.path.insert(0, %(oracle)r)
import importlib.util
spec = importlib.util.spec_from_file_location("hb_child", %(binding)r)
hb = importlib.util.module_from_spec(spec); spec.loader.exec_module(hb)
import sparsecuts_all_large_cases as L
import test_gpu_sparsecuts_all as T
blocks, ys, y, b = L.family(%(family)r)
s = T.load_dense(hb, blocks, b)
out = {}
for variant in (0, 7):
    c0 = hb.sparsecuts_all_large_stats()
    res = s.sparsecuts_all_large(y, [%(size)d] * len(blocks), L.TOL, L.FEASTOL, L.MAXCUTS, variant)
    c1 = hb.sparsecuts_all_large_stats()
    out[str(variant)] = {"bits": [[r[0], r[6], r[7]] + [np.asarray(a).tobytes().hex() for a in r[1:6]] for r in res],
                         "stats": [c1[k] - c0[k] for k in range(3)]}
s.close()
print(json.dumps(out))
"""


def _child(chunk, family="f3", size=10):
    env = dict(os.environ)
    env.pop("HIPSDP_SPARSECUTS_LARGE_CHUNK", None)
    if chunk:
        env["HIPSDP_SPARSECUTS_LARGE_CHUNK"] = str(chunk)
    code = _CHILD % {"family": family, "size": size, "tests": os.path.join(ROOT, "tests"), "harness": os.path.join(ROOT, "tests", "harness"),
                     "oracle": os.path.join(ROOT, "oracle"), "binding": os.path.join(ROOT, "scip-sdp_amd", "binding.py")}
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bits_do_not_depend_on_the_chunking(gpu):
    """HIPSDP_SPARSECUTS_LARGE_CHUNK=1 against the default, each in a fresh child process: the two large blocks of f3 in two chunks
    (200 rows first) - the same bits, one read-back per chunk, the launches of a chunk those of its own largest block"""
    one, two = _child(0), _child(1)
    for v in ("0", "7"):
        assert one[v]["bits"] == two[v]["bits"], v
        assert one[v]["stats"] == [1, formula(int(v), MAXCUTS, 200), 1], v
        assert two[v]["stats"] == [1, formula(int(v), MAXCUTS, 200) + formula(int(v), MAXCUTS, 150), 2], v


def test_a_chunk_of_several_blocks_that_is_not_the_whole_call(gpu):
    """family f4 - blocks of 130, 12, 129, 131 rows, served by descending rows as 3, 0, 2 - at size 4 with the chunk variable unset
    (one chunk of three), 2 (blocks 3 and 0, then block 2: a chunk whose own vector offsets differ from the caller's) and 1, each in
    a fresh child process: the same bits, the 12-row block turned away, one read-back per chunk, the launches of a chunk those of
    its own largest block"""
    assert L.CHUNKED_MASKS == (0, 7)
    runs = [_child(c, L.CHUNKED, L.CHUNKED_SIZE) for c in (0, 2, 1)]
    for v in ("0", "7"):
        f = lambda n: formula(int(v), MAXCUTS, n)
        whole, pair, single = (r[v] for r in runs)
        print("variant %s: stats %s / %s / %s, ncuts %s" % (v, whole["stats"], pair["stats"], single["stats"], [r[0] for r in whole["bits"]]))
        assert whole["bits"] == pair["bits"] == single["bits"], v
        assert whole["bits"][1][0] == -1 and all(whole["bits"][k][0] >= 1 for k in (0, 2, 3)), v
        assert whole["stats"] == [1, f(131), 1], v
        assert pair["stats"] == [1, f(131) + f(129), 2], v
        assert single["stats"] == [1, f(131) + f(130) + f(129), 3], v


def test_two_host_threads_reproduce_the_single_thread_bits(gpu):
    cases = [("f3", 10, 7), ("n129", 10, 2)]
    data = [L.family(f) for f, _, _ in cases]
    solvers = [load_dense(gpu, d[0], d[3]) for d in data]
    single = [device(gpu, *c) for c in cases]
    got = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(3):
                got[i].append(solvers[i].sparsecuts_all_large(data[i][2], [cases[i][1]] * len(data[i][0]), TOL, FEASTOL, MAXCUTS, cases[i][2]))
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


# ---- 6. storage forms ------------------------------------------------------------------------------------------------------------------

def test_the_storage_forms_give_the_same_cuts(gpu):
    """the 150-row block loaded dense (swept as packed lower triangles) and kept as nonzeros: counts and supports equal, values to
    1e-9.  (Full dense rows are the form of blocks of at most 64 rows; no solver keeps a block of 150 rows that way.)"""
    blocks, ys, y, b = L.family("f3")
    A = blocks[1]
    sd, ss = load_dense(gpu, [A], b), load_sparse(gpu, [A], b)
    assert ss.is_sparse(0) and not sd.is_sparse(0)
    for size, variant in ((10, 0), (10, 1), (10, 7), (4, 2)):
        rd = sd.sparsecuts_all_large(y, [size], TOL, FEASTOL, MAXCUTS, variant)[0]
        rs = ss.sparsecuts_all_large(y, [size], TOL, FEASTOL, MAXCUTS, variant)[0]
        (nd, ld, ed, cd, hd, vd, itd, fd), (n_s, ls, es, cs, hs, vs, its, fs) = rd, rs
        assert nd == n_s >= 1 and itd == its and fd == fs, (size, variant)
        assert same_bits([rd], [device(gpu, "f3", size, variant)[1]])
        assert abs(ld - ls) <= 1e-9 * max(1.0, abs(ld))
        for c in range(nd):
            assert support(vd[c]) == support(vs[c]), (size, variant, c)
            assert abs(ed[c] - es[c]) <= 1e-9 * max(1.0, abs(ed[c])), (size, variant, c)
            assert np.max(np.abs(vd[c] - vs[c])) <= 1e-9, (size, variant, c)
            assert np.max(np.abs(cd[c] - cs[c])) <= 1e-9 * max(1.0, np.max(np.abs(cd[c]))), (size, variant, c)
            assert abs(hd[c] - hs[c]) <= 1e-9 * max(1.0, abs(hd[c])), (size, variant, c)
    sd.close()
    ss.close()


# ---- 7. launches and read-backs --------------------------------------------------------------------------------------------------------

def test_launches_and_readbacks_are_the_formula(gpu):
    """one block (129 rows) and the two large blocks of f3 (nmax = 200), maxcuts 5, 1, 0, masks 0, 1, 2, 7: the formula of the header,
    one read-back; the other sparse-cut totals do not move"""
    others = (gpu.sparsecuts_all_stats(), gpu.sparsecuts_stats(), gpu.sparsecuts_ex_stats())
    for name, nmax in (("n129", 129), ("f3", 200)):
        blocks, ys, y, b = L.family(name)
        s = load_dense(gpu, blocks, b)
        for variant in (0, 1, 2, 7):
            for mc in (MAXCUTS, 1, 0):
                c0, l0, r0 = gpu.sparsecuts_all_large_stats()
                res = s.sparsecuts_all_large(y, [10] * len(blocks), TOL, FEASTOL, mc, variant)
                c1, l1, r1 = gpu.sparsecuts_all_large_stats()
                print("%s variant %d maxcuts %d: %d launches (formula %d), %d read-backs, %d cuts" %
                      (name, variant, mc, l1 - l0, formula(variant, mc, nmax), r1 - r0, sum(max(r[0], 0) for r in res)))
                assert (c1 - c0, l1 - l0, r1 - r0) == (1, formula(variant, mc, nmax), 1), (name, variant, mc)
                if mc == 0:
                    assert all(res[k][0] == 0 and res[k][6] == 0 and res[k][7] == 0 for k in L.large_blocks(name))
        s.close()
    assert (gpu.sparsecuts_all_stats(), gpu.sparsecuts_stats(), gpu.sparsecuts_ex_stats()) == others


def test_launches_do_not_depend_on_the_number_of_blocks_and_the_other_totals_stay(gpu):
    """two solvers whose largest block has 200 rows: that block alone, and with the 150-row block beside it"""
    blocks, ys, y, b = L.family("f3")
    deltas = {}
    for label, sel in (("one", [3]), ("two", [1, 3])):
        s = load_dense(gpu, [blocks[k] for k in sel], b)
        for variant in (0, 1, 2, 7):
            for mc in (MAXCUTS, 1, 0):
                c0, l0, r0 = gpu.sparsecuts_all_large_stats()
                s.sparsecuts_all_large(y, [10] * len(sel), TOL, FEASTOL, mc, variant)
                c1, l1, r1 = gpu.sparsecuts_all_large_stats()
                deltas[(label, variant, mc)] = (c1 - c0, l1 - l0, r1 - r0)
        # the other calls on the same solver do not move these totals, and the reverse
        mine = gpu.sparsecuts_all_large_stats()
        one0, ex0, all0 = gpu.sparsecuts_stats(), gpu.sparsecuts_ex_stats(), gpu.sparsecuts_all_stats()
        s.sparsecuts(0, y, 10, TOL, FEASTOL, MAXCUTS)
        s.sparsecuts_all_ex(y, [10] * len(sel), TOL, FEASTOL, MAXCUTS, 1)
        s.sparsecuts_all(y, [10] * len(sel), TOL, FEASTOL, MAXCUTS)
        assert gpu.sparsecuts_all_large_stats() == mine
        assert gpu.sparsecuts_stats()[0] == one0[0] + 1 and gpu.sparsecuts_ex_stats()[0] == ex0[0] + 1 and gpu.sparsecuts_all_stats()[0] == all0[0] + 1
        s.close()
    for variant in (0, 1, 2, 7):
        for mc in (MAXCUTS, 1, 0):
            assert deltas[("one", variant, mc)] == deltas[("two", variant, mc)] == (1, formula(variant, mc, 200), 1), (variant, mc)


# ---- 8. maxcuts = 0 --------------------------------------------------------------------------------------------------------------------

def test_no_cuts_wanted_is_a_feasibility_check(gpu):
    """lmin only, with eigvals, coefs and lhs NULL"""
    blocks, ys, y, b = L.family("f3")
    s = load_dense(gpu, blocks, b)
    for variant in (0, 7):
        rc, a = _raw(gpu, s, y, [10] * 5, 0, variant, 777.0, nullcuts=True)
        assert rc == 0 and list(a["ncuts"]) == [-1, 0, -1, 0, -1]
        for k in (1, 3):
            want = device(gpu, "f3", 10, variant)[k][1]
            assert a["lmin"][k] == want < -TOL and a["iters"][k] == 0 and a["flags"][k] == 0, (variant, k)
        assert np.all(a["vecs"] == 777.0) and a["lmin"][0] == 777.0
    s.close()
