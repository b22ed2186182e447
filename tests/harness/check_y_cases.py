"""Problems whose Z(y) is known on the host, for the tests of hipsdp_check_y_many (tests/test_gpu_check_y_many.py) and of hipsdp_check_y
(tests/test_gpu_check_y_routes.py): families of blocks with points, the solver loaded in either storage form, numpy's Z(y) and its
spectrum, and the eigenvalue bound of the header's contract."""
import numpy as np
import ipm_ref

KINDS = ["feasible", "negative", "lowrank"]


def sym(rng, n):
    R = rng.standard_normal((n, n))
    return (R + R.T) / 2.0


def family(ns, m, kind, count, seed=0):
    """blocks [m + 1, n, n] and count points: `feasible` - Z(y) positive definite at every point; `negative` - indefinite; `lowrank` - rank
    one matrices of a few variables plus a shift: n - r copies of the shift at the bottom of the spectrum"""
    rng = np.random.default_rng([seed, m, KINDS.index(kind), len(ns), count])
    Y = rng.uniform(0.5, 1.5, (count, m)) if kind == "lowrank" else rng.uniform(-1.0, 1.0, (count, m))
    blocks = []
    for n in ns:
        A = np.zeros((m + 1, n, n))
        if kind == "lowrank":
            r = max(1, min(m, n // 3))
            for i in range(1, r + 1):
                u = rng.choice([-1.0, 1.0], n)
                A[i] = np.outer(u, u)
            A[0] = -0.75 * np.eye(n)
        else:
            for i in range(1, m + 1):
                A[i] = sym(rng, n) / np.sqrt(n)
            A[0] = sym(rng, n) / np.sqrt(n)
            if kind == "feasible":
                A[0] -= (2.0 * np.sqrt(m) + 2.0) * np.eye(n)
        blocks.append(A)
    return blocks, Y


def zmat(A, y):
    return (np.tensordot(y, A[1:], axes=(0, 0)) if len(y) else 0.0) - A[0]


def spectra(blocks, Y):
    """numpy: lam1[count, nb] and the largest |lambda| [count, nb]"""
    lam1 = np.zeros((len(Y), len(blocks)))
    top = np.zeros_like(lam1)
    for j, y in enumerate(Y):
        for k, A in enumerate(blocks):
            w = np.linalg.eigvalsh(zmat(A, y))
            lam1[j, k], top[j, k] = w[0], max(abs(w[0]), abs(w[-1]))
    return lam1, top


def load(hb, blocks, m, form, D=None, c=None, units=False):
    """form 'dense': dense input (dense rows up to 64 rows, packed triangles above); 'sparse': triplets, every block kept as nonzeros"""
    q = 0 if D is None else len(c)
    s = hb.Solver(0, units=units)
    if form == "dense":
        s.load_core(ipm_ref.CoreProblem(np.zeros(m), blocks, D, c))
        return s
    s.sparse_policy(2)
    trip = []
    for A in blocks:
        n = A.shape[1]
        il = np.tril_indices(n)
        var = np.repeat(np.arange(m + 1, dtype=np.int32), len(il[0]))
        row = np.tile(il[0].astype(np.int32), m + 1)
        col = np.tile(il[1].astype(np.int32), m + 1)
        val = np.concatenate([A[i][il] for i in range(m + 1)])
        keep = val != 0.0
        trip.append((var[keep], row[keep], col[keep], val[keep]))
    s.set_shape(m, [A.shape[1] for A in blocks], q, nnz=[len(t[3]) for t in trip])
    s.set_obj(np.zeros(m))
    for k, t in enumerate(trip):
        s.add_entries(k, *t)
    if q:
        s.set_lp(np.concatenate([np.asarray(c).reshape(-1, 1), D], axis=1))
    for k in range(len(blocks)):
        assert s.is_sparse(k), k
    return s


def check_lmin(lmin, blocks, Y, what):
    lam1, top = spectra(blocks, Y)
    err = np.abs(lmin - lam1) / top
    for k, A in enumerate(blocks):
        print("%s n = %3d: lambda_1 in [%.6g, %.6g], largest |lmin - lambda_1| / max |lambda| = %.3g" %
              (what, A.shape[1], lam1[:, k].min(), lam1[:, k].max(), err[:, k].max()))
    assert np.all(err <= 1e-12), (what, float(err.max()))
    return lam1
