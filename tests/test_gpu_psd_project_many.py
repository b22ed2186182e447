"""hipsdp_psd_project_many: the PSD projections of many blocks in one call (csrc/psd_many.hip) against the oracle, against the single
call and against itself.  Inputs: tests/harness/psd_many_cases.py (every size at which the batched path changes, two densities, two
minev).  Kept / dropped entries are compared as LISTS, which is meaningful because no entry of an oracle result lies between 1e-10
and 1e-8 in absolute value (epsilon is 1e-9): every test asserts that on the oracle's result first."""
import ctypes as C
import threading
import numpy as np
import pytest

import psd_project_ref as ref
import psd_many_cases as cases

pytestmark = pytest.mark.gpu
PD = C.POINTER(C.c_double)
PI = C.POINTER(C.c_int)
EPS = cases.EPSILON


def _pd(a):
    return a.ctypes.data_as(PD)


def _pi(a):
    return a.ctypes.data_as(PI)


def run_many(hb, jobs, mode, caps=None, epsilon=EPS):
    """raw call: returns (rc, [(row, col, val) or None where the job did not fit], [nnz_out])"""
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
        tab[j].n, tab[j].nnz, tab[j].minev, tab[j].cap, tab[j].nnz_out = job.n, len(val), job.minev, cap, -1
        tab[j].row, tab[j].col, tab[j].val = _pi(row), _pi(col), _pd(val)
        tab[j].rowout, tab[j].colout, tab[j].valout = _pi(ro), _pi(co), _pd(vo)
    rc = hb.lib().hipsdp_psd_project_many(0, len(jobs), tab, C.c_double(epsilon), mode)
    out, need = [], []
    for j, k in enumerate(keep):
        t = tab[j].nnz_out
        need.append(t)
        cap = tab[j].cap
        if t > cap or t < 0:
            assert np.all(k[3] == -7) and np.all(k[4] == -7) and np.all(k[5] == -7.0)          # nothing written
            out.append(None)
        else:
            out.append((k[3][:t].copy(), k[4][:t].copy(), k[5][:t].copy()))
    return rc, out, need


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def device_eig(lib, n):
    def eig(full_flat):
        a = np.array(full_flat, dtype=np.float64).copy()
        lam = np.zeros(n)
        V = np.zeros(n * n)
        assert lib.SCIPlapackComputeEigenvectorDecomposition(None, n, _pd(a), _pd(lam), _pd(V)) == 1
        return lam, V
    return eig


def dense(n, r, c, v):
    D = np.zeros((n, n))
    D[r, c] = v
    return D


def check_against_oracle(lib, job, res0, res1):
    """mode 0 against the literal chain on the device's eigenvectors, mode 1 against the spectral form"""
    n = job.n
    r2, c2, v2, R2 = ref.chain(n, job.row, job.col, job.val, job.minev, eig=device_eig(lib, n))
    assert cases.band_is_empty(R2), job.name
    print("%s mode 0: %d entries, max |diff| %.3e (bound %.3e)" % (job.name, len(v2), np.max(np.abs(res0[2] - v2)) if len(v2) == len(res0[2]) and len(v2) else 0.0, 1e-10 * job.scale))
    assert list(res0[0]) == list(r2) and list(res0[1]) == list(c2), job.name
    assert np.all(np.abs(res0[2] - v2) <= 1e-10 * job.scale), job.name
    S = ref.spectral(n, job.row, job.col, job.val, job.minev)
    assert cases.band_is_empty(S), job.name
    keep = np.abs(np.triu(S)) > EPS
    rs, cs = np.nonzero(keep)
    assert list(res1[0]) == list(rs) and list(res1[1]) == list(cs), job.name
    print("%s mode 1: %d entries, max |diff| %.3e (bound %.3e)" % (job.name, len(rs), np.max(np.abs(res1[2] - S[rs, cs])) if len(rs) else 0.0, 1e-9 * job.scale))
    assert np.all(np.abs(res1[2] - S[rs, cs]) <= 1e-9 * job.scale), job.name
    D1 = dense(n, *res1)
    assert np.linalg.eigvalsh(D1 + np.triu(D1, 1).T).min() >= job.minev - 1e-8 * job.scale, job.name


@pytest.fixture(scope="module")
def mixed(gpu):
    """the mixed batch and what one call returns for it in either mode (shared, never changed)"""
    jobs = cases.mixed_jobs()
    res = []
    for mode in (0, 1):
        rc, out, need = run_many(gpu, jobs, mode)
        assert rc == 0 and all(o is not None for o in out)
        res.append(out)
    return jobs, res


def test_one_mixed_call_against_oracle_and_single_call(gpu, mixed):
    jobs, res = mixed
    lib = gpu.lib()
    assert sorted(set(j.n for j in jobs)) == list(cases.SIZES) and len(jobs) == len(cases.SIZES) * 4
    dropped = 0
    for k, job in enumerate(jobs):
        check_against_oracle(lib, job, res[0][k], res[1][k])
        dropped += job.n * (job.n + 1) // 2 - len(res[0][k][2])
        for mode in (0, 1):
            r, c, v = gpu.psd_project(job.n, job.row, job.col, job.val, job.minev, EPS, mode)
            assert list(r) == list(res[mode][k][0]) and list(c) == list(res[mode][k][1]), (job.name, mode)
            assert np.all(np.abs(v - res[mode][k][2]) <= 1e-10 * job.scale), (job.name, mode)
            assert np.all(r <= c) and np.all(np.diff(r.astype(np.int64) * job.n + c) > 0)
    assert dropped > 0                                        # (n = 17, density 0.3 keeps 137 of 153: the drop path is exercised)


def test_position_independence(gpu, mixed):
    jobs, res = mixed
    for mode in (0, 1):
        for k, job in enumerate(jobs):
            rc, out, _ = run_many(gpu, [job], mode)
            assert rc == 0 and same_bits(out[0], res[mode][k]), (job.name, mode)
        rc, out, _ = run_many(gpu, jobs[::-1], mode)
        assert rc == 0
        for k in range(len(jobs)):
            assert same_bits(out[len(jobs) - 1 - k], res[mode][k]), (jobs[k].name, mode)


def test_sparse_results(gpu):
    lib = gpu.lib()
    jobs = cases.sparse_result_jobs()
    assert [j.n for j in jobs] == [65, 128]
    blocks = [(40, 25), (70, 58)]
    rc0, out0, _ = run_many(gpu, jobs, 0)
    rc1, out1, _ = run_many(gpu, jobs, 1)
    assert rc0 == 0 and rc1 == 0
    for k, job in enumerate(jobs):
        check_against_oracle(lib, job, out0[k], out1[k])
        n1, n2 = blocks[k]
        for r, c, v in (out0[k], out1[k]):
            # the projection has the two dense blocks of the input and nothing else: the rest of every row is dropped ...
            assert len(v) == n1 * (n1 + 1) // 2 + n2 * (n2 + 1) // 2 < job.n * (job.n + 1) // 2
            # ... and some row keeps entries on both sides of the 64-column boundary
            assert any(c[r == i].min() < 64 <= c[r == i].max() for i in range(job.n) if np.any(r == i))


def test_edge_jobs_in_one_call(gpu):
    lib = gpu.lib()
    n = 6
    idx = np.arange(n, dtype=np.int32)
    d = np.arange(1, n + 1, dtype=np.float64)
    none_i, none_d = np.zeros(0, np.int32), np.zeros(0)
    diag = cases.Job("diag", n, idx, idx, d, np.diag(d), 1e-3)
    empty_half = cases.Job("empty_half", n, none_i, none_i, none_d, np.zeros((n, n)), 0.5)
    empty_zero = cases.Job("empty_zero", n, none_i, none_i, none_d, np.zeros((n, n)), 0.0)
    short = cases.Job("short", n, idx, idx, d, np.diag(d), 1e-3)
    jobs = [diag, short, empty_half, empty_zero, diag]
    for mode in (0, 1):
        rc, out, need = run_many(gpu, jobs, mode, caps=[None, 2, None, None, None])
        assert rc == 3                                                     # HIPSDP_ERR_ARG: one job did not fit
        assert need == [n, n, n, 0, n] and out[1] is None                  # the short job reports its need and got nothing written
        for k in (0, 4):
            assert list(out[k][0]) == list(range(n)) and list(out[k][1]) == list(range(n)) and np.allclose(out[k][2], d, atol=1e-12)
        assert list(out[2][0]) == list(range(n)) and list(out[2][1]) == list(range(n)) and np.allclose(out[2][2], 0.5, atol=1e-15)
        assert len(out[3][2]) == 0
    # argument errors: HIPSDP_ERR_ARG and nothing launched
    before = gpu.psd_project_many_stats()
    good = cases.Job("good", 3, np.array([0, 1, 2], np.int32), np.array([0, 0, 2], np.int32), np.array([1.0, 2.0, 3.0]), np.eye(3), 1e-4)
    eps = C.c_double(EPS)
    tab = (gpu.PsdJob * 1)()
    assert lib.hipsdp_psd_project_many(0, -1, tab, eps, 0) == 3
    assert lib.hipsdp_psd_project_many(0, 1025, tab, eps, 0) == 3
    assert lib.hipsdp_psd_project_many(0, 1, None, eps, 0) == 3
    assert run_many(gpu, [good], 2)[0] == 3 and run_many(gpu, [good], -1)[0] == 3
    bad_n = cases.Job("bad_n", 0, none_i, none_i, none_d, np.zeros((0, 0)), 1e-4)
    assert run_many(gpu, [good, bad_n], 0)[0] == 3
    for r_, c_ in (([0, 1, 3], [0, 0, 2]), ([0, 1, 2], [0, -1, 2])):
        bad = cases.Job("bad_index", 3, np.array(r_, np.int32), np.array(c_, np.int32), good.val, np.eye(3), 1e-4)
        assert run_many(gpu, [good, bad], 0)[0] == 3
    row, col, val = good.row.copy(), good.col.copy(), good.val.copy()
    ro, co, vo = np.zeros(6, np.int32), np.zeros(6, np.int32), np.zeros(6)
    for null in ("row", "col", "val", "rowout", "colout", "valout"):
        tab[0].n, tab[0].nnz, tab[0].minev, tab[0].cap = 3, 3, 1e-4, 6
        tab[0].row, tab[0].col, tab[0].val, tab[0].rowout, tab[0].colout, tab[0].valout = _pi(row), _pi(col), _pd(val), _pi(ro), _pi(co), _pd(vo)
        setattr(tab[0], null, None)
        assert lib.hipsdp_psd_project_many(0, 1, tab, eps, 0) == 3, null
    assert gpu.psd_project_many_stats() == before
    assert lib.hipsdp_psd_project_many(0, 0, None, eps, 0) == 0            # nothing to do
    assert gpu.psd_project_many_stats()[1:] == before[1:]                  # ... and nothing launched, nothing waited on


def test_launch_counts(gpu):
    row, col, val, M = cases.random_sparse_sym(12, 712, 1.0)
    job = cases.Job("n12", 12, row, col, val, M, 1e-4)
    for count in (64, 1):
        before = gpu.psd_project_many_stats()
        out = gpu.psd_project_many([job.args()] * count)
        after = gpu.psd_project_many_stats()
        assert len(out) == count
        calls, launches, readbacks = (a - b for a, b in zip(after, before))
        print("count %d: %d call, %d launches, %d read-back" % (count, calls, launches, readbacks))
        assert calls == 1 and 1 <= launches <= 6 and readbacks == 1


def test_job_of_129_rows_inside_a_batch(gpu, mixed):
    jobs, res = mixed
    row, col, val, M = cases.random_sparse_sym(129, 700 + 129, 0.3)
    big = cases.Job("n129", 129, row, col, val, M, 1e-4)
    pick = [k for k, j in enumerate(jobs) if j.n in (9, 64, 128)][:6]
    for mode in (0, 1):
        single = gpu.psd_project(big.n, big.row, big.col, big.val, big.minev, EPS, mode)
        batch = [jobs[k] for k in pick[:3]] + [big] + [jobs[k] for k in pick[3:]]
        rc, out, _ = run_many(gpu, batch, mode)
        assert rc == 0 and same_bits(out[3], single)
        for pos, k in zip((0, 1, 2, 4, 5, 6), pick):
            assert same_bits(out[pos], res[mode][k]), (jobs[k].name, mode)


def test_two_host_threads(gpu, mixed):
    jobs, res = mixed
    parts = [list(range(0, len(jobs), 2)), list(range(1, len(jobs), 2))[::-1]]
    got = [None, None]

    def work(t):
        got[t] = [run_many(gpu, [jobs[k] for k in parts[t]], mode) for mode in (0, 1)]

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for t in range(2):
        for mode in (0, 1):
            rc, out, _ = got[t][mode]
            assert rc == 0
            for pos, k in enumerate(parts[t]):
                assert same_bits(out[pos], res[mode][k]), (t, jobs[k].name, mode)
