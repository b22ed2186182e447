"""hipsdp_psd_project_many_large: the PSD projections of many blocks of 129 .. 512 rows in one call (csrc/psd_large.hip) against the
oracle, against hipsdp_syevr, against the single call and against itself.  Inputs: tests/harness/psd_large_cases.py; the CPU test
checks on every one of them that no entry of the spectral form lies between 1e-10 and 1e-8 (epsilon is 1e-9) and that no
eigenvalue lies near minev - epsilon, so kept / dropped entries are compared as LISTS.  scale = max(1, max|M| sqrt(n)).
Bounds: mode 0 against the literal chain on hipsdp_syevr's vectors 1e-10 scale; mode 1 against the spectral form 1e-9 scale; the
smallest eigenvalue of a mode 1 result >= minev - 1e-8 scale."""
import ctypes as C
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from conftest import ROOT
import psd_project_ref as ref
import psd_large_cases as cases
import psd_large_chunk_child as child

pytestmark = pytest.mark.gpu
PD = C.POINTER(C.c_double)
PI = C.POINTER(C.c_int)
EPS = cases.EPSILON


def launches_of(nmax):
    return nmax + 8 + 6 * -(-nmax // 32)


def run_large(hb, jobs, mode, caps=None, epsilon=EPS):
    """raw call: (rc, [(row, col, val), or None where nothing was written], [nnz_out]); asserts that a job that got nothing written
    has its output arrays untouched"""
    tab = (hb.PsdJob * max(len(jobs), 1))()
    keep = []
    for j, job in enumerate(jobs):
        row = np.ascontiguousarray(job.row, dtype=np.int32)
        col = np.ascontiguousarray(job.col, dtype=np.int32)
        val = np.ascontiguousarray(job.val, dtype=np.float64)
        cap = job.n * (job.n + 1) // 2 if caps is None or caps[j] is None else caps[j]
        ro = np.full(max(cap, 1), -7, dtype=np.int32)
        co = np.full(max(cap, 1), -7, dtype=np.int32)
        vo = np.full(max(cap, 1), -7.0)
        keep.append((row, col, val, ro, co, vo))
        tab[j].n, tab[j].nnz, tab[j].minev, tab[j].cap, tab[j].nnz_out = job.n, len(val), job.minev, cap, -3
        tab[j].row, tab[j].col, tab[j].val = row.ctypes.data_as(PI), col.ctypes.data_as(PI), val.ctypes.data_as(PD)
        tab[j].rowout, tab[j].colout, tab[j].valout = ro.ctypes.data_as(PI), co.ctypes.data_as(PI), vo.ctypes.data_as(PD)
    rc = hb.lib().hipsdp_psd_project_many_large(0, len(jobs), tab, C.c_double(epsilon), mode)
    out, need = [], []
    for j, k in enumerate(keep):
        t = tab[j].nnz_out
        need.append(t)
        if t > tab[j].cap or t < 0:
            assert np.all(k[3] == -7) and np.all(k[4] == -7) and np.all(k[5] == -7.0)          # nothing written
            out.append(None)
        else:
            assert np.all(k[3][t:] == -7) and np.all(k[5][t:] == -7.0)
            out.append((k[3][:t].copy(), k[4][:t].copy(), k[5][:t].copy()))
    return rc, out, need


def same_bits(a, b):
    return a is not None and b is not None and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def dense(n, r, c, v):
    D = np.zeros((n, n))
    D[r, c] = v
    return D


def syevr_eig(hb, n):
    def eig(full_flat):
        lam, V = hb.syevr(np.array(full_flat, dtype=np.float64).reshape(n, n))
        return lam, V.reshape(-1)
    return eig


def check_mode0(hb, job, res):
    r2, c2, v2, R2 = ref.chain(job.n, job.row, job.col, job.val, job.minev, eig=syevr_eig(hb, job.n))
    assert cases.band_is_empty(R2), job.name
    diff = np.max(np.abs(res[2] - v2)) if len(v2) == len(res[2]) and len(v2) else 0.0
    print("%s mode 0: %d entries, max |diff| %.3e (bound %.3e)" % (job.name, len(v2), diff, 1e-10 * job.scale))
    assert list(res[0]) == list(r2) and list(res[1]) == list(c2), job.name
    assert np.all(np.abs(res[2] - v2) <= 1e-10 * job.scale), job.name


def check_mode1(job, res):
    n = job.n
    S = ref.spectral(n, job.row, job.col, job.val, job.minev)
    assert cases.band_is_empty(S), job.name
    rs, cs = np.nonzero(np.abs(np.triu(S)) > EPS)
    diff = np.max(np.abs(res[2] - S[rs, cs])) if len(rs) == len(res[2]) and len(rs) else 0.0
    D1 = dense(n, *res)
    lmin = np.linalg.eigvalsh(D1 + np.triu(D1, 1).T).min()
    print("%s mode 1: %d entries, max |diff| %.3e (bound %.3e), lmin - minev %.3e (bound %.3e)"
          % (job.name, len(rs), diff, 1e-9 * job.scale, lmin - job.minev, -1e-8 * job.scale))
    assert list(res[0]) == list(rs) and list(res[1]) == list(cs), job.name
    assert np.all(np.abs(res[2] - S[rs, cs]) <= 1e-9 * job.scale), job.name
    assert lmin >= job.minev - 1e-8 * job.scale, job.name
    assert np.all(res[0] <= res[1]) and np.all(np.diff(res[0].astype(np.int64) * n + res[1]) > 0)
    return S


@pytest.fixture(scope="module")
def mixed(gpu):
    """the mixed batch and what one call returns for it in either mode (shared, never changed)"""
    jobs = cases.mixed_jobs()
    res = []
    for mode in (0, 1):
        before = gpu.psd_project_many_large_stats()
        rc, out, need = run_large(gpu, jobs, mode)
        after = gpu.psd_project_many_large_stats()
        assert rc == 0 and all(o is not None for o in out)
        assert tuple(a - b for a, b in zip(after, before)) == (1, launches_of(257), 1)
        res.append(out)
    return jobs, res


def test_batched_decomposition_equals_syevr_bit_for_bit(gpu):
    mats = cases.decomposition_table()
    assert [M.shape[0] for M in mats] == [129, 160, 200, 257, 129]
    alone = [gpu.syevr(M) for M in mats]
    for lam, V in alone:
        assert np.all(np.diff(lam) >= 0) and np.abs(V @ V.T - np.eye(len(lam))).max() < 1e-10
    for table, cap in ((mats, 8), (mats[::-1], 8), (mats, 1), (mats, 4)):
        got = gpu.syevr_many_unit(table, cap)
        if table is not mats:
            got = got[::-1]
        for k, ((lam, V), (l1, V1)) in enumerate(zip(got, alone)):
            assert lam.tobytes() == l1.tobytes(), (k, cap)
            assert V.tobytes() == V1.tobytes(), (k, cap)


def test_one_mixed_call_mode0_against_chain_on_syevr_vectors(gpu, mixed):
    jobs, res = mixed
    assert len(jobs) == 4 * 2 * 2 + 3 + 2 and max(j.n for j in jobs) == 257
    for k, job in enumerate(jobs):
        check_mode0(gpu, job, res[0][k])


def test_one_mixed_call_mode1_against_spectral_form(gpu, mixed):
    jobs, res = mixed
    dropped = 0
    for k, job in enumerate(jobs):
        check_mode1(job, res[1][k])
        if job.name.startswith("blocks"):
            dropped += job.n * (job.n + 1) // 2 - len(res[1][k][2])
            r, c, _ = res[1][k]
            assert any(c[r == i].min() < 64 <= c[r == i].max() for i in range(job.n) if np.any(r == i))       # kept columns on both sides of a tile boundary
    assert dropped > 0


def test_mode1_against_the_per_job_call(gpu, mixed):
    jobs, res = mixed
    for name in ("random_n129_d1_m0.0001", "random_n200_d0.05_m0.5"):
        k = [j.name for j in jobs].index(name)
        job = jobs[k]
        r, c, v = gpu.psd_project(job.n, job.row, job.col, job.val, job.minev, EPS, 1)
        S = ref.spectral(job.n, job.row, job.col, job.val, job.minev)
        print("%s: per-job call against the spectral form %.3e, large call %.3e (bound %.3e each)"
              % (name, np.max(np.abs(v - S[r, c])), np.max(np.abs(res[1][k][2] - S[r, c])), 1e-9 * job.scale))
        assert list(r) == list(res[1][k][0]) and list(c) == list(res[1][k][1]), name
        assert np.all(np.abs(v - res[1][k][2]) <= 2e-9 * job.scale), name


def test_512_rows_once(gpu):
    job = cases.job_512()
    before = gpu.psd_project_many_large_stats()
    rc, out, _ = run_large(gpu, [job], 1)
    after = gpu.psd_project_many_large_stats()
    assert rc == 0
    check_mode1(job, out[0])
    assert tuple(a - b for a, b in zip(after, before)) == (1, launches_of(512), 1) and launches_of(512) == 616


def test_edge_cases(gpu):
    empty, diag, psd = cases.edge_jobs()
    n = 129
    for mode in (0, 1):
        rc, out, need = run_large(gpu, [empty, diag, psd], mode)
        assert rc == 0
        # no triplets, minev 0.5: exactly the diagonal at 0.5
        assert list(out[0][0]) == list(range(n)) and list(out[0][1]) == list(range(n)) and np.all(out[0][2] == 0.5)
        # a diagonal matrix: the raised diagonal, nothing else
        want = np.where(diag.val - diag.minev < -EPS, diag.minev, diag.val)
        assert np.sum(want == diag.minev) > 10
        assert list(out[1][0]) == list(range(n)) and list(out[1][1]) == list(range(n))
        assert np.all(np.abs(out[1][2] - want) <= 1e-10 * diag.scale)
        # already >= minev: the input's upper triangle (mode 1; the literal chain of mode 0 is no projection in a general basis)
        if mode == 0:
            continue
        rs, cs = np.nonzero(np.abs(np.triu(psd.M)) > EPS)
        assert list(out[2][0]) == list(rs) and list(out[2][1]) == list(cs)
        print("edge_psd mode %d: max |diff| to the input %.3e (bound %.3e)" % (mode, np.max(np.abs(out[2][2] - psd.M[rs, cs])), 1e-10 * psd.scale))
        assert np.all(np.abs(out[2][2] - psd.M[rs, cs]) <= 1e-10 * psd.scale)


def test_turned_away_jobs(gpu, mixed):
    jobs, res = mixed
    names = [j.name for j in jobs]
    served = [jobs[names.index(nm)] for nm in ("random_n129_d0.05_m0.0001", "low_rank_n200_r20_s0.25", "blocks_100_29")]
    intruders = []
    for n in (1, 64, 128, 513):
        row, col, val, M = cases.random_sparse_sym(n, 950 + n, 1.0 if n < 200 else 0.01)
        intruders.append(cases.Job("intruder_n%d" % n, n, row, col, val, M, 1e-4))
    batch = [intruders[0], served[0], intruders[1], intruders[2], served[1], intruders[3], served[2]]
    for mode in (0, 1):
        rc, out, need = run_large(gpu, batch, mode)
        assert rc == 0
        for pos in (0, 2, 3, 5):
            assert need[pos] == -1 and out[pos] is None                    # (run_large checked that nothing was written)
        for pos, job in zip((1, 4, 6), served):
            assert same_bits(out[pos], res[mode][names.index(job.name)]), (job.name, mode)
    before = gpu.psd_project_many_large_stats()
    rc, out, need = run_large(gpu, intruders, 1)
    after = gpu.psd_project_many_large_stats()
    assert rc == 0 and need == [-1] * 4 and after[1:] == before[1:]        # nothing launched, nothing waited on


def test_bits_do_not_depend_on_the_batch(gpu, mixed):
    jobs, res = mixed
    names = [j.name for j in jobs]
    k = names.index("low_rank_n257_r30_s-0.01")
    others = [jobs[i] for i in range(len(jobs)) if i != k][:8]
    for mode in (0, 1):
        for batch, pos in (([jobs[k]], 0), ([jobs[k]] + others, 0), (others + [jobs[k]], 8)):
            rc, out, _ = run_large(gpu, batch, mode)
            assert rc == 0 and len(batch) in (1, 9) and same_bits(out[pos], res[mode][k]), (mode, len(batch), pos)
    # two host threads at once, each with half of the mixed batch
    parts = [list(range(0, len(jobs), 2)), list(range(1, len(jobs), 2))[::-1]]
    got = [None, None]

    def work(t):
        got[t] = [run_large(gpu, [jobs[i] for i in parts[t]], mode) for mode in (0, 1)]

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(2):
        for mode in (0, 1):
            rc, out, _ = got[t][mode]
            assert rc == 0
            for pos, i in enumerate(parts[t]):
                assert same_bits(out[pos], res[mode][i]), (t, jobs[i].name, mode)


def test_bits_do_not_depend_on_the_chunking(gpu):
    """a fresh child process with HIPSDP_PSD_LARGE_CHUNK = 1 MiB: every one of the three jobs is a chunk of its own"""
    cj = child.chunk_jobs()
    assert sorted(j.n for j in cj) == [129, 160, 200]
    here = {}
    for mode in (0, 1):
        before = gpu.psd_project_many_large_stats()
        res = gpu.psd_project_many_large([j.args() for j in cj], EPS, mode)
        after = gpu.psd_project_many_large_stats()
        assert tuple(a - b for a, b in zip(after, before)) == (1, launches_of(200), 1)
        here[mode] = [child.digest(r) for r in res]
    env = dict(os.environ, HIPSDP_PSD_LARGE_CHUNK="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "harness", "psd_large_chunk_child.py")], env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    for mode in (0, 1):
        g = got["mode%d" % mode]
        assert g["sha"] == here[mode], mode
        assert g["calls"] == 1 and g["readbacks"] == 3                     # one read-back per chunk
        assert g["launches"] == launches_of(200) + launches_of(160) + launches_of(129)


def test_cap_one_short(gpu, mixed):
    jobs, res = mixed
    names = [j.name for j in jobs]
    pick = [names.index(nm) for nm in ("random_n160_d1_m0.5", "blocks_150_107", "random_n129_d1_m0.0001")]
    for mode in (0, 1):
        full = len(res[mode][pick[1]][2])
        rc, out, need = run_large(gpu, [jobs[i] for i in pick], mode, caps=[None, full - 1, None])
        assert rc == 3                                                     # HIPSDP_ERR_ARG: one job did not fit
        assert need[1] == full and out[1] is None                          # it reports its need and got nothing written
        assert same_bits(out[0], res[mode][pick[0]]) and same_bits(out[2], res[mode][pick[2]])
        rc, out, need = run_large(gpu, [jobs[i] for i in pick], mode, caps=[None, full, None])
        assert rc == 0 and same_bits(out[1], res[mode][pick[1]])


def test_launch_counts(gpu):
    lib = gpu.lib()
    for nmax, name in ((129, None), (257, None)):
        big = cases.random_job(nmax, 0.05, 0.5)
        small = cases.random_job(129, 0.05, 0.5)
        for count in (1, 3, 9):
            before = gpu.psd_project_many_large_stats()
            out = gpu.psd_project_many_large([small.args()] * (count - 1) + [big.args()], EPS, 1)
            after = gpu.psd_project_many_large_stats()
            assert len(out) == count and all(o is not None for o in out)
            calls, launches, readbacks = (a - b for a, b in zip(after, before))
            print("nmax %d, %d jobs: %d call, %d launches, %d read-back" % (nmax, count, calls, launches, readbacks))
            assert (calls, launches, readbacks) == (1, launches_of(nmax), 1)
    # calls counts only calls that passed the checks
    before = gpu.psd_project_many_large_stats()
    tab = (gpu.PsdJob * 1)()
    eps = C.c_double(EPS)
    assert lib.hipsdp_psd_project_many_large(0, -1, tab, eps, 0) == 3
    assert lib.hipsdp_psd_project_many_large(0, 1025, tab, eps, 0) == 3
    assert lib.hipsdp_psd_project_many_large(0, 1, None, eps, 0) == 3
    assert run_large(gpu, [cases.random_job(129, 0.05, 0.5)], 2)[0] == 3
    tab[0].n = 0
    assert lib.hipsdp_psd_project_many_large(0, 1, tab, eps, 0) == 3
    assert gpu.psd_project_many_large_stats() == before
    assert lib.hipsdp_psd_project_many_large(0, 0, None, eps, 0) == 0      # nothing to do
    assert gpu.psd_project_many_large_stats()[1:] == before[1:]
