"""binding.py - ctypes view of libhipsdp.so's C ABI (include/hipsdp.h) for the test-suite, bench.py and
__graft_entry__.py.  This is plumbing only: no arithmetic happens here, and nothing in this file imports oracle/.
If the shared library is missing or there is no GPU, calls fail loudly (RuntimeError) - there is no fallback path."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.environ.get("HIPSDP_LIB", os.path.join(_HERE, "lib", "libhipsdp.so"))     # HIPSDP_LIB: developer experiments with kernel variants

STATUS_NAMES = {0: "optimal", 1: "dual_infeasible", 2: "dual_unbounded", 3: "both_infeasible", 4: "iterlimit",
                5: "numeric", 6: "timelimit", 7: "objlimit", -1: "unsolved"}


class Params(C.Structure):
    _fields_ = [("gaptol", C.c_double), ("feastol", C.c_double), ("infeastol", C.c_double), ("objlimit", C.c_double),
                ("timelimit", C.c_double), ("gamma", C.c_double), ("ws_gbytes", C.c_double), ("maxiter", C.c_int),
                ("verbose", C.c_int), ("lanczos_steps", C.c_int), ("settings", C.c_int), ("pabstol", C.c_double), ("preoptgap", C.c_double)]


class Info(C.Structure):
    _fields_ = [("status", C.c_int), ("iterations", C.c_int), ("pobj", C.c_double), ("dobj", C.c_double),
                ("pinf", C.c_double), ("dinf", C.c_double), ("dabs", C.c_double), ("gap", C.c_double), ("mu", C.c_double),
                ("tau", C.c_double), ("kappa", C.c_double), ("solve_seconds", C.c_double), ("schur_seconds", C.c_double),
                ("schur_flops", C.c_double), ("schur_calls", C.c_int), ("chol_fail", C.c_int), ("warm_started", C.c_int),
                ("settings_used", C.c_int), ("schur_flops_executed", C.c_double)]


_lib = None


def lib():
    """loads libhipsdp.so (raises if it was not built: run `python -c 'import __graft_entry__ as g; g.build()'`)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIBPATH):
            raise RuntimeError("libhipsdp.so not built (%s); run __graft_entry__.build()" % LIBPATH)
        eng = C.CDLL(LIBPATH, mode=C.RTLD_GLOBAL)
        # the solver-interface backend (SCIPsdpiSolver*, SCIPlapack*) is a library of its own that needs the engine: symbol lookups
        # on its handle also find the engine's (dlsym searches the dependencies)
        sdpi = os.path.join(os.path.dirname(LIBPATH), os.path.basename(LIBPATH).replace("libhipsdp", "libhipsdp_sdpi", 1))
        _lib = C.CDLL(sdpi, mode=C.RTLD_GLOBAL) if os.path.exists(sdpi) else eng
        _lib.hipsdp_last_error.restype = C.c_char_p
        _lib.hipsdp_version.restype = C.c_char_p
    return _lib


_ulib = None


def ulib():
    """libhipsdp_units.so: the engine's objects plus the TEST / BENCH entry points of csrc/units.hip (include/hipsdp_units.h) - a library
    of its own, loaded beside the product libraries with local symbol scope (its copy of the engine is self-contained)"""
    global _ulib
    if _ulib is None:
        path = os.path.join(os.path.dirname(LIBPATH), "libhipsdp_units.so")
        if not os.path.exists(path):
            raise RuntimeError("libhipsdp_units.so not built (%s); run __graft_entry__.build()" % path)
        _ulib = C.CDLL(path, mode=C.RTLD_LOCAL)
        _ulib.hipsdp_last_error.restype = C.c_char_p
    return _ulib


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: rc=%d (%s)" % (what, rc, lib().hipsdp_last_error().decode()))


def _stats3(name, which=None):
    """the process totals (calls, launches, read-backs) of the C getter `name`; which: the library loader that is asked (None: lib)"""
    calls, launches, readbacks = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
    _chk(getattr((which or lib)(), name)(C.byref(calls), C.byref(launches), C.byref(readbacks)), name)
    return calls.value, launches.value, readbacks.value


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def device_count():
    return lib().hipsdp_device_count()


class Solver:
    """thin RAII wrapper of hipsdp_solver"""

    def __init__(self, device=0, units=False):
        """units: the solver lives in libhipsdp_units.so's copy of the engine (what the unit entries that take a solver need:
        sparse_dump)"""
        self._l = ulib if units else lib
        self.h = C.c_void_p()
        _chk(self._l().hipsdp_create(C.byref(self.h), device), "hipsdp_create")
        self.m = 0
        self.ns = []
        self.q = 0

    def close(self):
        if self.h:
            self._l().hipsdp_free(C.byref(self.h))
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_shape(self, m, blocksizes, q, nnz=None):
        """nnz: lower-triangular triplets the caller is going to add per block (hipsdp_set_shape2: a block whose count makes the
        pair formula the cheaper Schur assembly is kept as nonzeros)"""
        bs = np.asarray(blocksizes, dtype=np.int32)
        if nnz is None:
            _chk(self._l().hipsdp_set_shape(self.h, m, len(bs), _ip(bs), q), "hipsdp_set_shape")
        else:
            cnt = np.ascontiguousarray(nnz, dtype=np.int64)
            assert len(cnt) == len(bs)
            _chk(self._l().hipsdp_set_shape2(self.h, m, len(bs), _ip(bs), q, cnt.ctypes.data_as(C.POINTER(C.c_longlong))), "hipsdp_set_shape2")
        self.m, self.ns, self.q = m, [int(v) for v in bs], q

    def sparse_policy(self, mode):
        _chk(self._l().hipsdp_sparse_policy(self.h, mode), "hipsdp_sparse_policy")

    def is_sparse(self, k):
        return bool(self._l().hipsdp_block_is_sparse(self.h, k))

    def load_sparse(self, m, n, b, coo, A0):
        """one block given as triplets of the variables' matrices (var 1 .. m, row >= col) and a dense constant matrix"""
        var, row, col, val = coo
        il = np.tril_indices(n)
        c0 = A0[il]
        keep = c0 != 0.0
        self.set_shape(m, [n], 0, nnz=[len(val) + int(keep.sum())])
        self.set_obj(b)
        self.add_entries(0, np.concatenate([np.zeros(int(keep.sum()), dtype=np.int32), var]),
                         np.concatenate([il[0][keep].astype(np.int32), row]), np.concatenate([il[1][keep].astype(np.int32), col]),
                         np.concatenate([c0[keep], val]))

    def set_obj(self, b):
        b = _f64(b)
        _chk(self._l().hipsdp_set_obj(self.h, _dp(b)), "hipsdp_set_obj")

    # ---- master copy (hipsdp_master_*): matrices of all variables in original indices, gathered per node on the device ----

    def master_define(self, nvars, blocksizes, nblockvars=None, nnz=None):
        """nnz: None - every block a dense slots x N x N array (hipsdp_master_define); a list - block b is kept as triplets where
        nnz[b] >= 0 (hipsdp_master_define2)"""
        bs = np.ascontiguousarray(blocksizes, dtype=np.int32)
        bv = None if nblockvars is None else np.ascontiguousarray(nblockvars, dtype=np.int32)
        if nnz is None:
            _chk(self._l().hipsdp_master_define(self.h, nvars, len(bs), _ip(bs), None if bv is None else _ip(bv)), "hipsdp_master_define")
        else:
            cnt = np.ascontiguousarray(nnz, dtype=np.int64)
            assert len(cnt) == len(bs)
            _chk(self._l().hipsdp_master_define2(self.h, nvars, len(bs), _ip(bs), None if bv is None else _ip(bv),
                                                 cnt.ctypes.data_as(C.POINTER(C.c_longlong))), "hipsdp_master_define2")

    def master_block_is_sparse(self, b):
        return bool(self._l().hipsdp_master_block_is_sparse(self.h, b))

    def master_add_entries(self, b, slot, row, col, val):
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        row = np.ascontiguousarray(row, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = _f64(val)
        return self._l().hipsdp_master_add_entries(self.h, b, C.c_longlong(len(val)), _ip(slot), _ip(row), _ip(col), _dp(val))

    def master_add_vars(self, b, rows, cols, vals):
        """per-slot arrays: slot k has rows[k], cols[k], vals[k]"""
        rs = [np.ascontiguousarray(r, dtype=np.int32) for r in rows]
        cs = [np.ascontiguousarray(c, dtype=np.int32) for c in cols]
        vs = [_f64(v) for v in vals]
        k = len(vs)
        nnz = np.array([len(v) for v in vs], dtype=np.int32)
        PR = (C.POINTER(C.c_int) * max(k, 1))(*[_ip(r) for r in rs])
        PC = (C.POINTER(C.c_int) * max(k, 1))(*[_ip(c) for c in cs])
        PV = (C.POINTER(C.c_double) * max(k, 1))(*[_dp(v) for v in vs])
        return self._l().hipsdp_master_add_vars(self.h, b, k, _ip(nnz), PR, PC, PV)

    def master_gather(self, engine_block, master_block, slots, kept):
        """return code of hipsdp_master_gather (0: done): slots[a] = slot of the a-th active variable or -1, kept = original rows"""
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        kept = np.ascontiguousarray(kept, dtype=np.int32)
        return self._l().hipsdp_master_gather(self.h, engine_block, master_block, len(slots), _ip(slots), len(kept), _ip(kept))

    def master_gather_stats(self):
        """(device_builds, host_builds, launches, readbacks) of this solver"""
        v = [C.c_longlong(0) for _ in range(4)]
        _chk(self._l().hipsdp_master_gather_stats(self.h, *[C.byref(x) for x in v]), "hipsdp_master_gather_stats")
        return tuple(x.value for x in v)

    def last_error(self):
        return self._l().hipsdp_last_error().decode()

    def sparse_dump(self, k):
        """the device structure of block k, a block kept as nonzeros (hipsdp_sparse_dump_unit; the solver must have been created with
        units=True): dict of the counts n, m, nnz, npos, nfull, nslots and the seventeen arrays"""
        assert self._l is ulib
        cnt = np.zeros(6, dtype=np.int64)
        pc = cnt.ctypes.data_as(C.POINTER(C.c_longlong))
        _chk(ulib().hipsdp_sparse_dump_unit(self.h, k, pc, *([None] * 16)), "hipsdp_sparse_dump_unit")
        n, m, nnz, npos, nfull, nslots = [int(x) for x in cnt]
        shape = [("voff", m + 1, 'i'), ("vrow", nnz, 'i'), ("vcol", nnz, 'i'), ("vval", nnz, 'd'), ("poff", npos + 1, 'i'), ("prow", npos, 'i'),
                 ("pcol", npos, 'i'), ("pvar", nnz, 'i'), ("pval", nnz, 'd'), ("foff", m + 1, 'i'), ("frow", nfull, 'i'), ("fcol", nfull, 'i'),
                 ("fval", nfull, 'd'), ("soff", m + 1, 'i'), ("srow", nslots, 'i'), ("sent", nslots + 1, 'i')]
        arrs = [np.full(max(ln, 1), -7, dtype=np.int32 if t == 'i' else np.float64) for _, ln, t in shape]
        _chk(ulib().hipsdp_sparse_dump_unit(self.h, k, pc, *[_ip(a) if a.dtype == np.int32 else _dp(a) for a in arrs]), "hipsdp_sparse_dump_unit")
        out = dict(n=n, m=m, nnz=nnz, npos=npos, nfull=nfull, nslots=nslots)
        for (name, ln, _), a in zip(shape, arrs):
            out[name] = a[:ln].copy()
        return out

    def set_block_dense(self, k, A):
        A = _f64(A)
        assert A.size == (self.m + 1) * self.ns[k] ** 2
        _chk(self._l().hipsdp_set_block_dense(self.h, k, _dp(A)), "hipsdp_set_block_dense")

    def add_entries(self, k, var, row, col, val):
        var = np.ascontiguousarray(var, dtype=np.int32)
        row = np.ascontiguousarray(row, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = _f64(val)
        _chk(self._l().hipsdp_add_entries(self.h, k, C.c_longlong(len(val)), _ip(var), _ip(row), _ip(col), _dp(val)),
             "hipsdp_add_entries")

    def set_lp(self, Dext):
        Dext = _f64(Dext)
        _chk(self._l().hipsdp_set_lp(self.h, _dp(Dext)), "hipsdp_set_lp")

    def block_device_ptr(self, k):
        p = C.POINTER(C.c_double)()
        _chk(self._l().hipsdp_block_device_ptr(self.h, k, C.byref(p)), "hipsdp_block_device_ptr")
        return C.cast(p, C.c_void_p).value

    def gen_planted(self, n, m, seed, Xstar, Zstar, ystar):
        """device-side synthetic instance (see hipsdp_gen_planted); returns b"""
        Xstar, Zstar, ystar = _f64(Xstar), _f64(Zstar), _f64(ystar)
        b = np.zeros(m)
        _chk(self._l().hipsdp_gen_planted(self.h, n, m, C.c_longlong(seed), _dp(Xstar), _dp(Zstar), _dp(ystar), _dp(b)),
             "hipsdp_gen_planted")
        return b

    def gen_planted_density(self, n, m, seed, density, Xstar, Zstar, ystar):
        Xstar, Zstar, ystar = _f64(Xstar), _f64(Zstar), _f64(ystar)
        b = np.zeros(m)
        _chk(self._l().hipsdp_gen_planted_density(self.h, n, m, C.c_longlong(seed), C.c_double(density), _dp(Xstar), _dp(Zstar), _dp(ystar),
                                              _dp(b)), "hipsdp_gen_planted_density")
        return b

    def get_block_dense(self, k):
        A = np.zeros((self.m + 1, self.ns[k], self.ns[k]))
        _chk(self._l().hipsdp_get_block_dense(self.h, k, _dp(A)), "hipsdp_get_block_dense")
        return A

    def load_core(self, prob):
        """prob: object with m, b, blocks (list of [m+1, n, n]), D [q, m], c [q] (the oracle's CoreProblem layout)"""
        self.set_shape(prob.m, [A.shape[1] for A in prob.blocks], prob.q)
        self.set_obj(prob.b)
        for k, A in enumerate(prob.blocks):
            self.set_block_dense(k, A)
        if prob.q:
            self.set_lp(np.concatenate([np.asarray(prob.c).reshape(-1, 1), prob.D], axis=1))

    def set_start(self, y, X, Z, x=None, z=None):
        """start point of the next solve (used by the engine only if strictly interior: Info.warm_started)"""
        y = _f64(y)
        Xs = [_f64(M) for M in X]
        Zs = [_f64(M) for M in Z]
        PX = (C.POINTER(C.c_double) * max(len(Xs), 1))(*[_dp(M) for M in Xs])
        PZ = (C.POINTER(C.c_double) * max(len(Zs), 1))(*[_dp(M) for M in Zs])
        xx = _f64(x if x is not None else np.zeros(max(self.q, 1)))
        zz = _f64(z if z is not None else np.zeros(max(self.q, 1)))
        _chk(self._l().hipsdp_set_start(self.h, _dp(y), PX, PZ, _dp(xx), _dp(zz)), "hipsdp_set_start")

    def solve(self, **kw):
        p = Params()
        self._l().hipsdp_default_params(C.byref(p))
        for k, v in kw.items():
            setattr(p, k, v)
        info = Info()
        _chk(self._l().hipsdp_solve(self.h, C.byref(p), C.byref(info)), "hipsdp_solve")
        return info

    def solve_objectives(self, B, **kw):
        """hipsdp_solve_objectives: the loaded problem under every row of B (count x m) as objective, in one call; the keywords are
        Solver.solve's, one set for all jobs.  Returns (list of Info, Y) with Y[j] = y of job j; raises RuntimeError with the per-job
        return codes when the call failed."""
        B = _f64(B)
        if B.ndim != 2 or B.shape[1] != self.m:
            raise ValueError("solve_objectives: B must be count x %d" % self.m)
        n = B.shape[0]
        p = _params(kw)
        infos = (Info * max(n, 1))()
        rcs = (C.c_int * max(n, 1))()
        Y = np.zeros((n, self.m))
        rc = self._l().hipsdp_solve_objectives(self.h, n, _dp(B), C.byref(p), infos, _dp(Y), rcs)
        if rc != 0:
            raise RuntimeError("hipsdp_solve_objectives failed: rc=%d, per job %s (%s)" %
                               (rc, list(rcs)[:n], self._l().hipsdp_last_error().decode()))
        return [infos[i] for i in range(n)], Y

    def solve_path(self):
        """1: the last solve ran in the one-launch kernel of csrc/solve1.hip, 0: the general path"""
        return self._l().hipsdp_solve_path(self.h)

    def gram_cache_stats(self):
        """(hits, misses) of this solver's cold-start store: cold solves that copied the first Schur matrix / computed and stored it"""
        hits = C.c_longlong(0)
        misses = C.c_longlong(0)
        _chk(self._l().hipsdp_gram_cache_stats(self.h, C.byref(hits), C.byref(misses)), "hipsdp_gram_cache_stats")
        return hits.value, misses.value

    def solve1_trace(self, rows=0):
        out = np.zeros(64)
        hist = np.zeros((max(rows, 1), 16))
        _chk(self._l().hipsdp_solve1_trace(self.h, _dp(out), rows, _dp(hist) if rows else None), "hipsdp_solve1_trace")
        return out, hist[:rows]

    def y(self):
        out = np.zeros(self.m)
        _chk(self._l().hipsdp_get_y(self.h, _dp(out)), "hipsdp_get_y")
        return out

    def X(self, k):
        out = np.zeros((self.ns[k], self.ns[k]))
        _chk(self._l().hipsdp_get_X(self.h, k, _dp(out)), "hipsdp_get_X")
        return out

    def Z(self, k):
        out = np.zeros((self.ns[k], self.ns[k]))
        _chk(self._l().hipsdp_get_Z(self.h, k, _dp(out)), "hipsdp_get_Z")
        return out

    def lp(self):
        x = np.zeros(self.q)
        z = np.zeros(self.q)
        _chk(self._l().hipsdp_get_lp(self.h, _dp(x), _dp(z)), "hipsdp_get_lp")
        return x, z

    def preoptimal(self):
        """(y, [X_k], x) of the preoptimal iterate of the last solve (params preoptgap > 0) or None"""
        avail = C.c_int(0)
        y = np.zeros(max(1, self.m))
        x = np.zeros(max(1, self.q))
        _chk(self._l().hipsdp_get_preoptimal(self.h, C.byref(avail), _dp(y), _dp(x)), "hipsdp_get_preoptimal")
        if not avail.value:
            return None
        Xs = []
        for k, n in enumerate(self.ns):
            X = np.zeros((n, n))
            _chk(self._l().hipsdp_get_preoptimal_X(self.h, k, _dp(X)), "hipsdp_get_preoptimal_X")
            Xs.append(X)
        return y[:self.m], Xs, x[:self.q]

    def check_y(self, y, tol=0.0):
        """lambda_min of Z(y) per block (tol > 0: blocks above 64 rows report the certified bound -0.999 tol when it holds)"""
        y = _f64(y)
        lmin = np.zeros(max(1, len(self.ns)))
        viol = C.c_double(0.0)
        if tol > 0.0:
            _chk(self._l().hipsdp_check_y_tol(self.h, _dp(y), C.c_double(tol), _dp(lmin), C.byref(viol)), "hipsdp_check_y_tol")
        else:
            _chk(self._l().hipsdp_check_y(self.h, _dp(y), _dp(lmin), C.byref(viol)), "hipsdp_check_y")
        return lmin[:len(self.ns)], viol.value

    def eigencuts(self, block, y, tol, maxcuts):
        """eigenvector cuts of one block at y: (eigvals[k], coefs[k, m], lhs[k], vecs[k, n]); cut c: coefs[c] @ y >= lhs[c]"""
        y = _f64(y)
        m, n = len(y), self.ns[block]
        k = C.c_int(0)
        ev = np.zeros(max(1, maxcuts))
        co = np.zeros((max(1, maxcuts), max(1, m)))
        lh = np.zeros(max(1, maxcuts))
        ve = np.zeros((max(1, maxcuts), n))
        _chk(self._l().hipsdp_eigencuts(self.h, block, _dp(y), C.c_double(tol), maxcuts, C.byref(k), _dp(ev), _dp(co), _dp(lh), _dp(ve)),
             "hipsdp_eigencuts")
        return ev[:k.value], co[:k.value, :m], lh[:k.value], ve[:k.value]

    def eigencuts_all(self, y, tol, maxcuts):
        """the separation round of all blocks in one call (hipsdp_eigencuts_all): per block a tuple (lmin, eigvals[k], coefs[k, m],
        lhs[k], vecs[k, n]) with lmin the smallest eigenvalue of Z_b(y); cut c of a block: coefs[c] @ y >= lhs[c]"""
        y = _f64(y)
        m, nb, mc = len(y), len(self.ns), max(1, maxcuts)
        k = np.zeros(max(1, nb), dtype=np.int32)
        lmin = np.zeros(max(1, nb))
        ev = np.zeros((max(1, nb), mc))
        co = np.zeros((max(1, nb), mc, max(1, m)))
        lh = np.zeros((max(1, nb), mc))
        ve = np.zeros(max(1, maxcuts * sum(self.ns)))
        if m > 0 and maxcuts > 0:
            co = np.zeros((max(1, nb), maxcuts, m))
        _chk(self._l().hipsdp_eigencuts_all(self.h, _dp(y), C.c_double(tol), maxcuts, _ip(k), _dp(lmin), _dp(ev), _dp(co), _dp(lh), _dp(ve)),
             "hipsdp_eigencuts_all")
        out, off = [], 0
        for b, n in enumerate(self.ns):
            kb = int(k[b])
            if maxcuts > 0:
                evb, lhb = ev.reshape(-1)[b * maxcuts:b * maxcuts + kb], lh.reshape(-1)[b * maxcuts:b * maxcuts + kb]
                cob = co.reshape(-1)[b * maxcuts * m:(b * maxcuts + kb) * m].reshape(kb, m)
            else:
                evb, lhb, cob = np.zeros(0), np.zeros(0), np.zeros((0, m))
            out.append((float(lmin[b]), evb.copy(), cob.copy(), lhb.copy(), ve[off:off + kb * n].reshape(kb, n).copy()))
            off += maxcuts * n
        return out

    @staticmethod
    def eigencuts_all_stats():
        """process totals (calls, launches, read-backs): the module's eigencuts_all_stats()"""
        return eigencuts_all_stats()

    def eigencuts_all_large(self, y, tol, maxcuts):
        """the partner of eigencuts_all for the blocks of 129 .. 512 rows (hipsdp_eigencuts_all_large): their dense eigenvector cuts
        and feasibility eigenvalues in one call; per block a tuple (lmin, eigvals[k], coefs[k, m], lhs[k], vecs[k, n]) as
        eigencuts_all returns it, or None for a block that came back with -1 (at most 128 or more than 512 rows)"""
        y = _f64(y)
        m, nb, mc = len(y), len(self.ns), max(1, maxcuts)
        k = np.zeros(max(1, nb), dtype=np.int32)
        lmin = np.full(max(1, nb), np.nan)
        ev = np.zeros(max(1, nb) * mc)
        co = np.zeros(max(1, nb) * mc * max(1, m))
        lh = np.zeros(max(1, nb) * mc)
        ve = np.zeros(max(1, maxcuts * sum(self.ns)))
        _chk(self._l().hipsdp_eigencuts_all_large(self.h, _dp(y), C.c_double(tol), int(maxcuts), _ip(k), _dp(lmin), _dp(ev), _dp(co), _dp(lh),
                                                  _dp(ve)), "hipsdp_eigencuts_all_large")
        out, off = [], 0
        for b, n in enumerate(self.ns):
            kb = int(k[b])
            if kb < 0:
                out.append(None)
            else:
                s0 = b * maxcuts
                out.append((float(lmin[b]), ev[s0:s0 + kb].copy(), co[s0 * m:(s0 + kb) * m].reshape(kb, m).copy(), lh[s0:s0 + kb].copy(),
                            ve[off:off + kb * n].reshape(kb, n).copy()))
            off += maxcuts * n
        return out

    @staticmethod
    def eigencuts_all_large_stats():
        """process totals (calls, launches, read-backs): the module's eigencuts_all_large_stats()"""
        return eigencuts_all_large_stats()

    def check_y_many(self, Y, lmin_fill=np.nan):
        """the feasibility check of many candidate points in one call (hipsdp_check_y_many): Y is count x m; returns
        (lmin[count, nblocks], lpviol[count], served[nblocks]) - served[b] = -1: block b is not served and column b of lmin keeps
        lmin_fill"""
        Y = _f64(Y).reshape(-1, self.m) if self.m > 0 else np.zeros((len(Y), 0))
        count, nb = Y.shape[0], len(self.ns)
        lmin = np.full((max(1, count), max(1, nb)), lmin_fill, dtype=np.float64)
        viol = np.zeros(max(1, count))
        served = np.full(max(1, nb), -1, dtype=np.int32)
        _chk(self._l().hipsdp_check_y_many(self.h, count, _dp(Y), _dp(lmin), _dp(viol), _ip(served)), "hipsdp_check_y_many")
        return lmin[:count, :nb], viol[:count], served[:nb]

    def check_y_many_stats(self):
        """process totals (calls, launches, read-backs) of hipsdp_check_y_many in the library this solver lives in"""
        return check_y_many_stats(self._l)

    def rank1_check_many(self, Y, feastol, fill=np.nan, minors=True, dets=True):
        """the rank-1 constraints of many candidate points in one call (hipsdp_rank1_check_many): Y is count x m; returns
        (lam[count, nblocks, 3], minorev[count, nblocks], minorind[count, nblocks, 2], minordet[count, nblocks],
        detind[count, nblocks, 2], served[nblocks]) - served[b] = -1: block b is not served and its columns keep `fill` (the index
        arrays -7); minors / dets = False: that pair is passed as NULL and returned as None"""
        Y = _f64(Y).reshape(-1, self.m) if self.m > 0 else np.zeros((len(Y), 0))
        count, nb = Y.shape[0], len(self.ns)
        c1, b1 = max(1, count), max(1, nb)
        lam = np.full((c1, b1, 3), fill, dtype=np.float64)
        mev, mdet = np.full((c1, b1), fill, dtype=np.float64), np.full((c1, b1), fill, dtype=np.float64)
        mind, dind = np.full((c1, b1, 2), -7, dtype=np.int32), np.full((c1, b1, 2), -7, dtype=np.int32)
        served = np.full(b1, -1, dtype=np.int32)
        _chk(self._l().hipsdp_rank1_check_many(self.h, count, _dp(Y), C.c_double(feastol), _dp(lam), _dp(mev) if minors else None,
                                               _ip(mind) if minors else None, _dp(mdet) if dets else None, _ip(dind) if dets else None,
                                               _ip(served)), "hipsdp_rank1_check_many")
        return (lam[:count, :nb], mev[:count, :nb] if minors else None, mind[:count, :nb] if minors else None,
                mdet[:count, :nb] if dets else None, dind[:count, :nb] if dets else None, served[:nb])

    def rank1_approx(self, y, want=None, fill=np.nan, raw=False):
        """the device part of the rank-1 approximation heuristic (hipsdp_rank1_approx): per block (lmax, v[n], rhs[n (n + 1) / 2]) or None
        for a block that is not asked for or not served; returns (list, served[nblocks]); raw: the call's own arrays (lmax[nblocks], vec,
        rhs, served) instead, the slices it did not write still holding `fill`"""
        y = _f64(y)
        nb = len(self.ns)
        lmax = np.full(max(1, nb), fill)
        vec = np.full(max(1, int(sum(self.ns))), fill)
        rhs = np.full(max(1, sum(n * (n + 1) // 2 for n in self.ns)), fill)
        served = np.full(max(1, nb), -7, dtype=np.int32)
        w = None if want is None else np.ascontiguousarray(want, dtype=np.int32)
        _chk(self._l().hipsdp_rank1_approx(self.h, _dp(y), None if w is None else _ip(w), _dp(lmax), _dp(vec), _dp(rhs), _ip(served)),
             "hipsdp_rank1_approx")
        if raw:
            return lmax[:nb], vec, rhs, served[:nb]
        out, vo, ro = [], 0, 0
        for b, n in enumerate(self.ns):
            t = n * (n + 1) // 2
            out.append((float(lmax[b]), vec[vo:vo + n].copy(), rhs[ro:ro + t].copy()) if served[b] == 0 else None)
            vo += n
            ro += t
        return out, served[:nb]

    def rank1_approx_stats(self):
        """process totals (calls, launches, read-backs) of hipsdp_rank1_approx in the library this solver lives in"""
        return rank1_approx_stats(self._l)

    def rank1_check_many_stats(self):
        """process totals (calls, launches, read-backs) of hipsdp_rank1_check_many in the library this solver lives in"""
        return rank1_check_many_stats(self._l)

    def rounding_frame(self, X, want_vecs=True, fill=np.nan, raw=False):
        """stage 1 of the primal rounding problem (hipsdp_rounding_frame): X is a list with one entry per block - a dense symmetric
        n_b x n_b array (its nonzeros of both triangles become the triplets), a tuple (row, col, val) of triplets, or None (the zero
        matrix).  Returns (eigvals[N], obj[N], coefs[N, m], vecs[sum n_b^2] or None, served[nblocks]); the slots of a block that is not
        served keep `fill`.  raw: the status is returned in front instead of raised"""
        nb, N = len(self.ns), int(sum(self.ns))
        assert len(X) == nb
        keep, cnt = [], np.zeros(max(1, nb), dtype=np.int32)
        rows, cols, vals = (C.POINTER(C.c_int) * max(1, nb))(), (C.POINTER(C.c_int) * max(1, nb))(), (C.POINTER(C.c_double) * max(1, nb))()
        for b, Xb in enumerate(X):
            if Xb is None:
                continue
            if isinstance(Xb, tuple):
                r, c, v = Xb
            else:
                Xb = np.asarray(Xb, dtype=np.float64)
                r, c = np.nonzero(Xb)
                v = Xb[r, c]
            r, c, v = np.ascontiguousarray(r, dtype=np.int32), np.ascontiguousarray(c, dtype=np.int32), _f64(v)
            keep.append((r, c, v))
            cnt[b] = len(v)
            if len(v):
                rows[b], cols[b], vals[b] = _ip(r), _ip(c), _dp(v)
        eig, obj = np.full(max(1, N), fill), np.full(max(1, N), fill)
        coefs = np.full((max(1, N), max(1, self.m)), fill)
        vecs = np.full(max(1, sum(n * n for n in self.ns)), fill) if want_vecs else None
        served = np.full(max(1, nb), -1, dtype=np.int32)
        rc = self._l().hipsdp_rounding_frame(self.h, _ip(cnt), rows, cols, vals, _dp(eig), _dp(obj), _dp(coefs),
                                             _dp(vecs) if want_vecs else None, _ip(served))
        res = (eig[:N], obj[:N], coefs[:N, :self.m], vecs, served[:nb])
        if raw:
            return (rc,) + res
        _chk(rc, "hipsdp_rounding_frame")
        return res

    def rounding_recombine(self, lam, epsilon=1e-9, mode=0, caps=None, raw=False):
        """stage 2 (hipsdp_rounding_recombine) on the frame of the last rounding_frame: lam[N]; per block (row, col, val) of the kept
        upper-triangle entries, None for a block the frame does not hold, or the int needed length for a block over its cap
        (caps[b]; default n (n + 1) / 2).  raw: (status, list) instead of raising on a status other than 0"""
        nb = len(self.ns)
        lam = _f64(lam)
        assert lam.shape == (int(sum(self.ns)),)
        tab = (RoundingOut * max(1, nb))()
        keep = []
        for b, n in enumerate(self.ns):
            cap = n * (n + 1) // 2 if caps is None else int(caps[b])
            ro, co, vo = np.zeros(max(1, cap), dtype=np.int32), np.zeros(max(1, cap), dtype=np.int32), np.zeros(max(1, cap))
            keep.append((ro, co, vo))
            tab[b].cap, tab[b].nnz_out = cap, -7
            tab[b].rowout, tab[b].colout, tab[b].valout = _ip(ro), _ip(co), _dp(vo)
        rc = self._l().hipsdp_rounding_recombine(self.h, _dp(lam), C.c_double(epsilon), int(mode), tab)
        out = []
        for b in range(nb):
            k = tab[b].nnz_out
            out.append(None if k < 0 else (k if k > tab[b].cap else (keep[b][0][:k].copy(), keep[b][1][:k].copy(), keep[b][2][:k].copy())))
        if raw:
            return rc, out
        _chk(rc, "hipsdp_rounding_recombine")
        return out

    def rounding_stats(self):
        """process totals (calls, launches, read-backs) of both rounding stages in the library this solver lives in"""
        return rounding_stats(self._l)

    def form_z_many_unit(self, Y):
        """k_cm_form_z alone (hipsdp_form_z_many_unit; the solver must have been created with units=True): Y is count x m; returns
        ([per block b: Z[count, n_b, n_b] or None for a block that is not served], launches)"""
        assert self._l is ulib
        Y = _f64(Y).reshape(-1, self.m) if self.m > 0 else np.zeros((len(Y), 0))
        count, nb = Y.shape[0], len(self.ns)
        per = sum(n * n for n in self.ns)
        Z = np.full((count, max(1, per)), np.nan)
        served = np.full(max(1, nb), -1, dtype=np.int32)
        launches = C.c_int(-1)
        rc = ulib().hipsdp_form_z_many_unit(self.h, count, _dp(Y), _dp(Z), _ip(served), C.byref(launches))
        if rc != 0:
            raise RuntimeError("hipsdp_form_z_many_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
        out, off = [], 0
        for b, n in enumerate(self.ns):
            out.append(Z[:, off:off + n * n].reshape(count, n, n).copy() if served[b] == 0 else None)
            off += n * n
        return out, launches.value

    def sparsecuts_all(self, y, sizes, tol, feastol, maxcuts, convtol=0, maxit=0):
        """sparse eigenvector cuts of all blocks in one call (hipsdp_sparsecuts_all; sizes[b]: target sparsity of block b): per block
        a tuple (ncuts, lmin, eigvals[k], coefs[k, m], lhs[k], vecs[k, n], iters, flags); ncuts = -1: the block is not served (then
        lmin is nan and the rest empty / 0); cut c of a block: coefs[c] @ y >= lhs[c], violated at y by -eigvals[c]"""
        y = _f64(y)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        m, nb, mc = len(y), len(self.ns), max(1, maxcuts)
        assert len(sizes) == nb
        opts = SparsecutOpts(tol, feastol, convtol, maxcuts, maxit)
        k = np.zeros(max(1, nb), dtype=np.int32)
        it = np.zeros(max(1, nb), dtype=np.int32)
        fl = np.zeros(max(1, nb), dtype=np.int32)
        lmin = np.full(max(1, nb), np.nan)
        ev = np.zeros(max(1, nb) * mc)
        co = np.zeros(max(1, nb) * mc * max(1, m))
        lh = np.zeros(max(1, nb) * mc)
        ve = np.zeros(max(1, maxcuts * sum(self.ns)))
        _chk(self._l().hipsdp_sparsecuts_all(self.h, _dp(y), _ip(sizes), C.byref(opts), _ip(k), _dp(lmin), _dp(ev), _dp(co), _dp(lh),
                                             _dp(ve), _ip(it), _ip(fl)), "hipsdp_sparsecuts_all")
        out, off = [], 0
        for b, n in enumerate(self.ns):
            kb = max(0, int(k[b]))
            s0 = b * maxcuts
            out.append((int(k[b]), float(lmin[b]), ev[s0:s0 + kb].copy(), co[s0 * m:(s0 + kb) * m].reshape(kb, m).copy(),
                        lh[s0:s0 + kb].copy(), ve[off:off + kb * n].reshape(kb, n).copy(), int(it[b]), int(fl[b])))
            off += maxcuts * n
        return out

    @staticmethod
    def sparsecuts_all_stats():
        """process totals (calls, launches, read-backs): the module's sparsecuts_all_stats()"""
        return sparsecuts_all_stats()

    def sparsecuts(self, block, y, size, tol, feastol, maxcuts, convtol=0.0, maxit=0):
        """sparse eigenvector cuts of ONE block of up to 512 rows (hipsdp_sparsecuts; size: its target sparsity): the tuple one block
        of sparsecuts_all has, (ncuts, lmin, eigvals[k], coefs[k, m], lhs[k], vecs[k, n], iters, flags); ncuts = -1: the block is
        not served (more than 512 rows, a communicator or sharded matrices; then lmin is nan and the rest empty / 0)"""
        y = _f64(y)
        m, n, mc = len(y), self.ns[block], max(1, maxcuts)
        opts = SparsecutOpts(tol, feastol, convtol, maxcuts, maxit)
        k, it, fl = C.c_int(0), C.c_int(0), C.c_int(0)
        lmin = C.c_double(np.nan)
        ev, lh = np.zeros(mc), np.zeros(mc)
        co = np.zeros(mc * max(1, m))
        ve = np.zeros(mc * n)
        _chk(self._l().hipsdp_sparsecuts(self.h, int(block), _dp(y), int(size), C.byref(opts), C.byref(k), C.byref(lmin), _dp(ev), _dp(co),
                                         _dp(lh), _dp(ve), C.byref(it), C.byref(fl)), "hipsdp_sparsecuts")
        kb = max(0, k.value)
        return (k.value, lmin.value, ev[:kb].copy(), co[:kb * m].reshape(kb, m).copy(), lh[:kb].copy(), ve[:kb * n].reshape(kb, n).copy(),
                it.value, fl.value)

    @staticmethod
    def sparsecuts_stats():
        """process totals (calls, launches, read-backs): the module's sparsecuts_stats()"""
        return sparsecuts_stats()

    def sparsecuts_all_ex(self, y, sizes, tol, feastol, maxcuts, variant, convtol=0, maxit=0):
        """sparsecuts_all with the reference's switches as a bit mask (hipsdp_sparsecuts_all_ex; variant: SC_RECOMPUTE_SPARSEEV |
        SC_RECOMPUTE_INITIAL | SC_EXACTTRANS, 0: the call is sparsecuts_all): the same list of tuples; with a switch set a block of
        more than 128 rows is not served (ncuts = -1), and flags bit 2 says that the loop ended at lambda >= -tol"""
        y = _f64(y)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        m, nb, mc = len(y), len(self.ns), max(1, maxcuts)
        assert len(sizes) == nb
        opts = SparsecutOpts(tol, feastol, convtol, maxcuts, maxit)
        k = np.zeros(max(1, nb), dtype=np.int32)
        it = np.zeros(max(1, nb), dtype=np.int32)
        fl = np.zeros(max(1, nb), dtype=np.int32)
        lmin = np.full(max(1, nb), np.nan)
        ev = np.zeros(max(1, nb) * mc)
        co = np.zeros(max(1, nb) * mc * max(1, m))
        lh = np.zeros(max(1, nb) * mc)
        ve = np.zeros(max(1, maxcuts * sum(self.ns)))
        _chk(self._l().hipsdp_sparsecuts_all_ex(self.h, _dp(y), _ip(sizes), C.byref(opts), C.c_uint(variant), _ip(k), _dp(lmin), _dp(ev),
                                                _dp(co), _dp(lh), _dp(ve), _ip(it), _ip(fl)), "hipsdp_sparsecuts_all_ex")
        out, off = [], 0
        for b, n in enumerate(self.ns):
            kb = max(0, int(k[b]))
            s0 = b * maxcuts
            out.append((int(k[b]), float(lmin[b]), ev[s0:s0 + kb].copy(), co[s0 * m:(s0 + kb) * m].reshape(kb, m).copy(),
                        lh[s0:s0 + kb].copy(), ve[off:off + kb * n].reshape(kb, n).copy(), int(it[b]), int(fl[b])))
            off += maxcuts * n
        return out

    def sparsecuts_ex(self, block, y, size, tol, feastol, maxcuts, variant, convtol=0.0, maxit=0):
        """sparsecuts with the reference's switches as a bit mask (hipsdp_sparsecuts_ex): the tuple one block of sparsecuts_all_ex has"""
        y = _f64(y)
        m, n, mc = len(y), self.ns[block], max(1, maxcuts)
        opts = SparsecutOpts(tol, feastol, convtol, maxcuts, maxit)
        k, it, fl = C.c_int(0), C.c_int(0), C.c_int(0)
        lmin = C.c_double(np.nan)
        ev, lh = np.zeros(mc), np.zeros(mc)
        co = np.zeros(mc * max(1, m))
        ve = np.zeros(mc * n)
        _chk(self._l().hipsdp_sparsecuts_ex(self.h, int(block), _dp(y), int(size), C.byref(opts), C.c_uint(variant), C.byref(k),
                                            C.byref(lmin), _dp(ev), _dp(co), _dp(lh), _dp(ve), C.byref(it), C.byref(fl)),
             "hipsdp_sparsecuts_ex")
        kb = max(0, k.value)
        return (k.value, lmin.value, ev[:kb].copy(), co[:kb * m].reshape(kb, m).copy(), lh[:kb].copy(), ve[:kb * n].reshape(kb, n).copy(),
                it.value, fl.value)

    @staticmethod
    def sparsecuts_ex_stats():
        """process totals (calls, launches, read-backs): the module's sparsecuts_ex_stats()"""
        return sparsecuts_ex_stats()

    def sparsecuts_all_large(self, y, sizes, tol, feastol, maxcuts, variant, convtol=0, maxit=0):
        """the partner of sparsecuts_all_ex for the blocks it turns away (hipsdp_sparsecuts_all_large): the sparse cuts of all blocks
        of 129 .. 512 rows in one call, variant 0 .. 7; the same list of tuples - ncuts = -1 for a block of at most 128 or more than
        512 rows, and for a block whose sizes[b] exceeds 128 while SC_RECOMPUTE_SPARSEEV is set"""
        y = _f64(y)
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        m, nb, mc = len(y), len(self.ns), max(1, maxcuts)
        assert len(sizes) == nb
        opts = SparsecutOpts(tol, feastol, convtol, maxcuts, maxit)
        k = np.zeros(max(1, nb), dtype=np.int32)
        it = np.zeros(max(1, nb), dtype=np.int32)
        fl = np.zeros(max(1, nb), dtype=np.int32)
        lmin = np.full(max(1, nb), np.nan)
        ev = np.zeros(max(1, nb) * mc)
        co = np.zeros(max(1, nb) * mc * max(1, m))
        lh = np.zeros(max(1, nb) * mc)
        ve = np.zeros(max(1, maxcuts * sum(self.ns)))
        _chk(self._l().hipsdp_sparsecuts_all_large(self.h, _dp(y), _ip(sizes), C.byref(opts), C.c_uint(variant), _ip(k), _dp(lmin), _dp(ev),
                                                   _dp(co), _dp(lh), _dp(ve), _ip(it), _ip(fl)), "hipsdp_sparsecuts_all_large")
        out, off = [], 0
        for b, n in enumerate(self.ns):
            kb = max(0, int(k[b]))
            s0 = b * maxcuts
            out.append((int(k[b]), float(lmin[b]), ev[s0:s0 + kb].copy(), co[s0 * m:(s0 + kb) * m].reshape(kb, m).copy(),
                        lh[s0:s0 + kb].copy(), ve[off:off + kb * n].reshape(kb, n).copy(), int(it[b]), int(fl[b])))
            off += maxcuts * n
        return out

    @staticmethod
    def sparsecuts_all_large_stats():
        """process totals (calls, launches, read-backs): the module's sparsecuts_all_large_stats()"""
        return sparsecuts_all_large_stats()

    def onevar_bounds(self, block, u, lb, ub, feastol, vars=None, kind=None, infinity=1e20, maxevals=0):
        """all one-variable SDPs of a block in one call (hipsdp_onevar_bounds): job j works on Z_block(u) + (mu - u_i) A_i with
        i = vars[j] (None: all variables in index order), kind[j] ONEVAR_NEWTON (None: all) or ONEVAR_TWOPOINT, bounds lb[j], ub[j].
        Returns the arrays (status, optval, lmin, grad, evals); every status -1: the block is not served"""
        u, lb, ub = _f64(u), _f64(lb), _f64(ub)
        count = len(lb)
        assert len(ub) == count
        cv = None if vars is None else np.ascontiguousarray(vars, dtype=np.int32)
        ck = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
        assert cv is None or len(cv) == count
        assert ck is None or len(ck) == count
        opts = OnevarOpts(feastol, infinity, maxevals)
        status = np.full(max(1, count), -1, dtype=np.int32)
        evals = np.zeros(max(1, count), dtype=np.int32)
        optval, lmin, grad = (np.full(max(1, count), np.nan) for _ in range(3))
        _chk(self._l().hipsdp_onevar_bounds(self.h, int(block), _dp(u), count, None if cv is None else _ip(cv),
                                            None if ck is None else _ip(ck), _dp(lb), _dp(ub), C.byref(opts), _ip(status), _dp(optval),
                                            _dp(lmin), _dp(grad), _ip(evals)), "hipsdp_onevar_bounds")
        return status[:count], optval[:count], lmin[:count], grad[:count], evals[:count]

    @staticmethod
    def onevar_bounds_stats():
        """process totals (calls, launches, read-backs): the module's onevar_bounds_stats()"""
        return onevar_bounds_stats()

    def onevar_bounds_all(self, u, lb, ub, feastol, blocks=None, vars=None, kind=None, infinity=1e20, maxevals=0):
        """the one-variable SDPs of ALL blocks in one call (hipsdp_onevar_bounds_all): job j is (blocks[j], vars[j]) with kind[j]
        (None: all ONEVAR_NEWTON; ONEVAR_TWOPOINT; ONEVAR_EXTREMES: lmin / optval = the smallest / largest eigenvalue of A_i alone) and
        the bounds lb[j], ub[j]; blocks and vars both None: every (block, variable) pair in block-major order.  Returns the arrays
        (status, optval, lmin, grad, evals); status -1 and NaN: the job's block is not served"""
        u, lb, ub = _f64(u), _f64(lb), _f64(ub)
        count = len(lb)
        assert len(ub) == count
        cb = None if blocks is None else np.ascontiguousarray(blocks, dtype=np.int32)
        cv = None if vars is None else np.ascontiguousarray(vars, dtype=np.int32)
        ck = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
        assert all(c is None or len(c) == count for c in (cb, cv, ck))
        opts = OnevarOpts(feastol, infinity, maxevals)
        status = np.full(max(1, count), -1, dtype=np.int32)
        evals = np.zeros(max(1, count), dtype=np.int32)
        optval, lmin, grad = (np.full(max(1, count), np.nan) for _ in range(3))
        _chk(self._l().hipsdp_onevar_bounds_all(self.h, _dp(u), count, None if cb is None else _ip(cb), None if cv is None else _ip(cv),
                                                None if ck is None else _ip(ck), _dp(lb), _dp(ub), C.byref(opts), _ip(status),
                                                _dp(optval), _dp(lmin), _dp(grad), _ip(evals)), "hipsdp_onevar_bounds_all")
        return status[:count], optval[:count], lmin[:count], grad[:count], evals[:count]

    @staticmethod
    def onevar_bounds_all_stats():
        """process totals (calls, launches, read-backs): the module's onevar_bounds_all_stats()"""
        return onevar_bounds_all_stats()

    def onevar_bounds_large(self, u, lb, ub, feastol, blocks=None, vars=None, kind=None, infinity=1e20, maxevals=0):
        """the one-variable SDPs of the blocks of 129 .. 512 rows (hipsdp_onevar_bounds_large): arguments and results of
        onevar_bounds_all; status -1 and NaN: the job's block is not served here (at most 128 rows: onevar_bounds_all serves it)"""
        u, lb, ub = _f64(u), _f64(lb), _f64(ub)
        count = len(lb)
        assert len(ub) == count
        cb = None if blocks is None else np.ascontiguousarray(blocks, dtype=np.int32)
        cv = None if vars is None else np.ascontiguousarray(vars, dtype=np.int32)
        ck = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
        assert all(c is None or len(c) == count for c in (cb, cv, ck))
        opts = OnevarOpts(feastol, infinity, maxevals)
        status = np.full(max(1, count), -1, dtype=np.int32)
        evals = np.zeros(max(1, count), dtype=np.int32)
        optval, lmin, grad = (np.full(max(1, count), np.nan) for _ in range(3))
        _chk(self._l().hipsdp_onevar_bounds_large(self.h, _dp(u), count, None if cb is None else _ip(cb), None if cv is None else _ip(cv),
                                                  None if ck is None else _ip(ck), _dp(lb), _dp(ub), C.byref(opts), _ip(status),
                                                  _dp(optval), _dp(lmin), _dp(grad), _ip(evals)), "hipsdp_onevar_bounds_large")
        return status[:count], optval[:count], lmin[:count], grad[:count], evals[:count]

    @staticmethod
    def onevar_bounds_large_stats():
        """process totals (calls, launches, read-backs): the module's onevar_bounds_large_stats()"""
        return onevar_bounds_large_stats()


class OnevarOpts(C.Structure):
    """hipsdp_onevar_opts"""
    _fields_ = [("feastol", C.c_double), ("infinity", C.c_double), ("maxevals", C.c_int)]


ONEVAR_NEWTON, ONEVAR_TWOPOINT = 0, 1                                                                          # HIPSDP_ONEVAR_* kinds
ONEVAR_LB, ONEVAR_INNER, ONEVAR_INFEASIBLE, ONEVAR_UBONLY, ONEVAR_DECLINED, ONEVAR_GAVEUP = 0, 1, 2, 3, 4, 5    # ... and statuses
ONEVAR_EXTREMES, ONEVAR_DONE = 2, 6                                                  # kind and status of hipsdp_onevar_bounds_all alone


def onevar_bounds_stats():
    """process totals of hipsdp_onevar_bounds: (calls that served their block, kernel launches issued, device->host synchronisations)"""
    return _stats3("hipsdp_onevar_bounds_stats")


def onevar_bounds_all_stats():
    """process totals of hipsdp_onevar_bounds_all: (calls that served a job, kernel launches issued, device->host synchronisations)"""
    return _stats3("hipsdp_onevar_bounds_all_stats")


def onevar_all_unit(Z, A, shift, lb, ub, feastol, kind=None, maxevals=0, mid_cap=256, device=0):
    """the launches of hipsdp_onevar_bounds_all alone on host matrices per job (hipsdp_onevar_all_unit of the units library): Z[j] and
    A[j] are n_j x n_j, shift[j] = u_i; mid_cap: the cap on the grid of the 65-128 launch; returns the arrays (status, optval, lmin,
    grad, evals)"""
    Z = [np.asarray(z, dtype=np.float64) for z in Z]
    A = [np.asarray(a, dtype=np.float64) for a in A]
    count = len(Z)
    ns = np.ascontiguousarray([z.shape[0] for z in Z], dtype=np.int32)
    assert len(A) == count and all(Z[j].shape == A[j].shape == (ns[j], ns[j]) for j in range(count))
    zf = _f64(np.concatenate([z.reshape(-1) for z in Z]))
    af = _f64(np.concatenate([a.reshape(-1) for a in A]))
    shift, lb, ub = _f64(np.atleast_1d(shift)), _f64(np.atleast_1d(lb)), _f64(np.atleast_1d(ub))
    assert len(lb) == count and len(ub) == count and len(shift) == count
    ck = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
    status = np.full(count, -1, dtype=np.int32)
    evals = np.zeros(count, dtype=np.int32)
    optval, lmin, grad = (np.full(count, np.nan) for _ in range(3))
    rc = ulib().hipsdp_onevar_all_unit(device, count, _ip(ns), _dp(zf), _dp(af), _dp(shift), None if ck is None else _ip(ck), _dp(lb),
                                       _dp(ub), C.c_double(feastol), int(maxevals), int(mid_cap), _ip(status), _dp(optval), _dp(lmin),
                                       _dp(grad), _ip(evals))
    if rc != 0:
        raise RuntimeError("hipsdp_onevar_all_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    return status, optval, lmin, grad, evals


def onevar_bounds_large_stats():
    """process totals of hipsdp_onevar_bounds_large: (calls that served a job, kernel launches issued, device->host synchronisations)"""
    return _stats3("hipsdp_onevar_bounds_large_stats")


def onevar_large_unit(Z, A, shift, lb, ub, feastol, kind=None, maxevals=0, wg_cap=0, chunk=0, device=0, with_rounds=False):
    """the rounds of hipsdp_onevar_bounds_large alone on host matrices per job (hipsdp_onevar_large_unit of the units library): Z[j] and
    A[j] are n_j x n_j, 2 <= n_j <= 512, shift[j] = u_i; wg_cap: workgroups per job of a column launch at most (0: the product call's
    choice); chunk: jobs per chunk at most (0: one chunk); returns the arrays (status, optval, lmin, grad, evals), with_rounds: and the
    number of rounds"""
    Z = [np.asarray(z, dtype=np.float64) for z in Z]
    A = [np.asarray(a, dtype=np.float64) for a in A]
    count = len(Z)
    ns = np.ascontiguousarray([z.shape[0] for z in Z], dtype=np.int32)
    assert len(A) == count and all(Z[j].shape == A[j].shape == (ns[j], ns[j]) for j in range(count))
    zf = _f64(np.concatenate([z.reshape(-1) for z in Z]))
    af = _f64(np.concatenate([a.reshape(-1) for a in A]))
    shift, lb, ub = _f64(np.atleast_1d(shift)), _f64(np.atleast_1d(lb)), _f64(np.atleast_1d(ub))
    assert len(lb) == count and len(ub) == count and len(shift) == count
    ck = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
    status = np.full(count, -1, dtype=np.int32)
    evals = np.zeros(count, dtype=np.int32)
    optval, lmin, grad = (np.full(count, np.nan) for _ in range(3))
    rounds = C.c_int(0)
    rc = ulib().hipsdp_onevar_large_unit(device, count, _ip(ns), _dp(zf), _dp(af), _dp(shift), None if ck is None else _ip(ck), _dp(lb),
                                         _dp(ub), C.c_double(feastol), int(maxevals), int(wg_cap), int(chunk), _ip(status), _dp(optval),
                                         _dp(lmin), _dp(grad), _ip(evals), C.byref(rounds))
    if rc != 0:
        raise RuntimeError("hipsdp_onevar_large_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    res = (status, optval, lmin, grad, evals)
    return res + (rounds.value,) if with_rounds else res


def onevar_unit(n, Z, A, shift, lb, ub, feastol, kind=None, maxevals=0, device=0):
    """the Newton kernel of hipsdp_onevar_bounds alone on host matrices (hipsdp_onevar_unit of the units library): Z (n x n), A
    (count dense n x n), shift[j] = u_i; returns the arrays (status, optval, lmin, grad, evals)"""
    n = int(n)
    Z = _f64(np.asarray(Z, dtype=np.float64).reshape(-1))
    A = _f64(np.asarray(A, dtype=np.float64).reshape(-1))
    shift, lb, ub = _f64(np.atleast_1d(shift)), _f64(np.atleast_1d(lb)), _f64(np.atleast_1d(ub))
    count = len(lb)
    assert len(Z) == n * n and len(A) == count * n * n and len(ub) == count and len(shift) == count
    ck = None if kind is None else np.ascontiguousarray(kind, dtype=np.int32)
    status = np.full(count, -1, dtype=np.int32)
    evals = np.zeros(count, dtype=np.int32)
    optval, lmin, grad = (np.full(count, np.nan) for _ in range(3))
    rc = ulib().hipsdp_onevar_unit(device, n, count, _dp(Z), _dp(A), _dp(shift), None if ck is None else _ip(ck), _dp(lb), _dp(ub),
                                   C.c_double(feastol), int(maxevals), _ip(status), _dp(optval), _dp(lmin), _dp(grad), _ip(evals))
    if rc != 0:
        raise RuntimeError("hipsdp_onevar_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    return status, optval, lmin, grad, evals


class SparsecutOpts(C.Structure):
    """hipsdp_sparsecut_opts"""
    _fields_ = [("tol", C.c_double), ("feastol", C.c_double), ("convtol", C.c_double), ("maxcuts", C.c_int), ("maxit", C.c_int)]


def sparsecuts_all_stats():
    """process totals of hipsdp_sparsecuts_all: (calls, kernel launches issued, device->host synchronisations)"""
    return _stats3("hipsdp_sparsecuts_all_stats")


def sparsecuts_stats():
    """process totals of hipsdp_sparsecuts: (calls, kernel launches issued, device->host synchronisations)"""
    return _stats3("hipsdp_sparsecuts_stats")


SC_RECOMPUTE_SPARSEEV, SC_RECOMPUTE_INITIAL, SC_EXACTTRANS = 1, 2, 4      # HIPSDP_SC_*


def sparsecuts_ex_stats():
    """process totals of hipsdp_sparsecuts_all_ex / hipsdp_sparsecuts_ex with a switch set: (calls, kernel launches issued,
    device->host synchronisations)"""
    return _stats3("hipsdp_sparsecuts_ex_stats")


def sparsecuts_all_large_stats():
    """process totals of hipsdp_sparsecuts_all_large: (calls that served a block, kernel launches issued, device->host
    synchronisations)"""
    return _stats3("hipsdp_sparsecuts_all_large_stats")


def sparsecuts_large_unit(n, Z, v0, maxeig, size, feastol, maxcuts, convtol=0, maxit=0, device=0):
    """k_sc_tpower_large alone on one host matrix of 129 .. 512 rows (hipsdp_sparsecuts_large_unit of the units library): (ncuts,
    eigvals[k], vecs[k, n], iters, flags)"""
    n = int(n)
    Z = _f64(np.asarray(Z, dtype=np.float64).reshape(-1))
    v0 = _f64(np.asarray(v0, dtype=np.float64).reshape(-1))
    assert len(Z) == n * n and len(v0) == n
    opts = SparsecutOpts(0.0, feastol, convtol, maxcuts, maxit)
    k, it, fl = C.c_int(0), C.c_int(0), C.c_int(0)
    ev = np.zeros(max(1, maxcuts))
    ve = np.zeros(max(1, maxcuts) * n)
    rc = ulib().hipsdp_sparsecuts_large_unit(device, n, _dp(Z), _dp(v0), C.c_double(maxeig), int(size), C.byref(opts), C.byref(k), _dp(ev),
                                             _dp(ve), C.byref(it), C.byref(fl))
    if rc != 0:
        raise RuntimeError("hipsdp_sparsecuts_large_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    kk = k.value
    return kk, ev[:kk].copy(), ve[:kk * n].reshape(kk, n).copy(), it.value, fl.value


def sparsecuts_unit(ns, Zs, v0s, maxeig, sizes, feastol, maxcuts, convtol=0, maxit=0, device=0):
    """k_sc_tpower alone on host matrices (hipsdp_sparsecuts_unit of the units library): per matrix (ncuts, eigvals[k], vecs[k, n],
    iters, flags)"""
    ns = [int(n) for n in ns]
    cnt = len(ns)
    cns = np.asarray(ns, dtype=np.int32)
    Z = _f64(np.concatenate([np.asarray(z, dtype=np.float64).reshape(-1) for z in Zs]))
    v0 = _f64(np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for v in v0s]))
    me = _f64(maxeig)
    sizes = np.ascontiguousarray(sizes, dtype=np.int32)
    opts = SparsecutOpts(0.0, feastol, convtol, maxcuts, maxit)
    k, it, fl = (np.zeros(cnt, dtype=np.int32) for _ in range(3))
    ev = np.zeros(cnt * maxcuts)
    ve = np.zeros(maxcuts * sum(ns))
    rc = ulib().hipsdp_sparsecuts_unit(device, cnt, _ip(cns), _dp(Z), _dp(v0), _dp(me), _ip(sizes), C.byref(opts), _ip(k), _dp(ev), _dp(ve),
                                       _ip(it), _ip(fl))
    if rc != 0:
        raise RuntimeError("hipsdp_sparsecuts_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    out, off = [], 0
    for j, n in enumerate(ns):
        kj = int(k[j])
        out.append((kj, ev[j * maxcuts:j * maxcuts + kj].copy(), ve[off:off + kj * n].reshape(kj, n).copy(), int(it[j]), int(fl[j])))
        off += maxcuts * n
    return out


def eigencuts_all_stats():
    """process totals of hipsdp_eigencuts_all: (calls, kernel launches issued for batched blocks, device->host synchronisations)"""
    return _stats3("hipsdp_eigencuts_all_stats")


def eigencuts_all_large_stats():
    """process totals of hipsdp_eigencuts_all_large: (calls that served a block, kernel launches issued, device->host
    synchronisations)"""
    return _stats3("hipsdp_eigencuts_all_large_stats")


def check_y_many_stats(which=None):
    """process totals of hipsdp_check_y_many: (calls that launched something, kernel launches issued, device->host synchronisations);
    which: the library loader whose copy of the engine is asked (lib, the default, or ulib)"""
    return _stats3("hipsdp_check_y_many_stats", which)


def rank1_check_many_stats(which=None):
    """process totals of hipsdp_rank1_check_many: (calls that launched something, kernel launches issued, device->host
    synchronisations); which: the library loader whose copy of the engine is asked (lib, the default, or ulib)"""
    return _stats3("hipsdp_rank1_check_many_stats", which)


def rank1_approx_stats(which=None):
    """process totals of hipsdp_rank1_approx: (calls that launched something, kernel launches issued, device->host synchronisations)"""
    return _stats3("hipsdp_rank1_approx_stats", which)


def _mats_cat(mats):
    mats = [np.asarray(a, dtype=np.float64) for a in mats]
    ns = np.ascontiguousarray([a.shape[0] for a in mats], dtype=np.int32)
    assert all(a.shape == (n, n) for a, n in zip(mats, ns))
    return ns, _f64(np.concatenate([a.reshape(-1) for a in mats]))


def rank1_minors_unit(mats, feastol, device=0):
    """the two scans over the principal 2 x 2 minors on host matrices of mixed sizes (hipsdp_rank1_minors_unit of the units library):
    (minorev[count], minorind[count, 2], minordet[count], detind[count, 2])"""
    ns, cat = _mats_cat(mats)
    k = len(ns)
    mev, mdet = np.full(k, np.nan), np.full(k, np.nan)
    mind, dind = np.full((k, 2), -7, dtype=np.int32), np.full((k, 2), -7, dtype=np.int32)
    rc = ulib().hipsdp_rank1_minors_unit(device, k, _ip(ns), _dp(cat), C.c_double(feastol), _dp(mev), _ip(mind), _dp(mdet), _ip(dind))
    if rc != 0:
        raise RuntimeError("hipsdp_rank1_minors_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    return mev, mind, mdet, dind


def lsel_many_unit(mats, device=0):
    """eigenvalues 1, n - 1 and n of host matrices of mixed sizes by the three-index values kernels of hipsdp_rank1_check_many
    (hipsdp_lsel_many_unit of the units library): lam[count, 3]"""
    ns, cat = _mats_cat(mats)
    lam = np.full((len(ns), 3), np.nan)
    rc = ulib().hipsdp_lsel_many_unit(device, len(ns), _ip(ns), _dp(cat), _dp(lam))
    if rc != 0:
        raise RuntimeError("hipsdp_lsel_many_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    return lam


class RoundingOut(C.Structure):
    """hipsdp_rounding_out of include/hipsdp.h, field for field"""
    _fields_ = [("cap", C.c_int), ("nnz_out", C.c_int), ("rowout", C.POINTER(C.c_int)), ("colout", C.POINTER(C.c_int)),
                ("valout", C.POINTER(C.c_double))]


def rounding_stats(which=None):
    """process totals of hipsdp_rounding_frame and hipsdp_rounding_recombine together: (calls that launched something, kernel launches
    issued, device->host synchronisations); which: lib (default) or ulib"""
    return _stats3("hipsdp_rounding_stats", which)


def rounding_coefs_unit(V, A, form, nonzeros=None, device=0):
    """the coefficient launches of hipsdp_rounding_frame alone (hipsdp_rounding_coefs_unit of the units library) on one block: V (n x n,
    row j = v_j); form 0: A = [m + 1, n, n] dense; form 1: the same dense input, packed here into lower triangles; form 2: A = the
    dense constant matrix [n, n] and nonzeros = (m, var 1 .. m, row, col <= row, val).
    Returns (table[n, m + 1], route, slices)"""
    V = _f64(V)
    n = V.shape[0]
    A = np.asarray(A, dtype=np.float64)
    var = row = col = val = None
    nnz = 0
    if form == 2:
        m, mats = nonzeros[0], _f64(A.reshape(n, n))
        var, row, col, val = [np.asarray(x) for x in nonzeros[1:]]
        order = np.argsort(var, kind="stable")
        var, row, col = [np.ascontiguousarray(x[order], dtype=np.int32) for x in (var, row, col)]
        val = _f64(val[order])
        nnz = len(val)
    else:
        m = A.shape[0] - 1
        il = np.tril_indices(n)
        mats = _f64(A.reshape(m + 1, n * n) if form == 0 else np.stack([A[i][il] for i in range(m + 1)]))
    out = np.full((n, m + 1), np.nan)
    route, slices = C.c_int(-1), C.c_int(-1)
    rc = ulib().hipsdp_rounding_coefs_unit(device, n, int(m), int(form), _dp(V), _dp(mats), C.c_longlong(nnz),
                                           _ip(var) if nnz else None, _ip(row) if nnz else None, _ip(col) if nnz else None,
                                           _dp(val) if nnz else None, _dp(out), C.byref(route), C.byref(slices))
    if rc != 0:
        raise RuntimeError("hipsdp_rounding_coefs_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    return out, route.value, slices.value


def check_many_group():
    """the candidates k_cm_form_z serves per pass over a block's storage (hipsdp_check_many_group of the units library)"""
    return int(ulib().hipsdp_check_many_group())


def syevx_many_below_unit(mats, bound, maxk, cap, device=0):
    """the batched selection behind hipsdp_eigencuts_all_large on host matrices of mixed sizes (hipsdp_syevx_many_below_unit of the
    units library): the eigenvalues <= bound of every matrix, at most maxk, through column launches of at most cap workgroups per
    matrix; per matrix (count, lam[count], V[count, n])"""
    mats = [np.asarray(a, dtype=np.float64) for a in mats]
    ns = np.ascontiguousarray([a.shape[0] for a in mats], dtype=np.int32)
    assert all(a.shape == (n, n) for a, n in zip(mats, ns))
    cat = _f64(np.concatenate([a.reshape(-1) for a in mats]))
    cnt = np.full(len(mats), -1, dtype=np.int32)
    mk = max(1, int(maxk))
    lam = np.zeros(len(mats) * mk)
    V = np.zeros(mk * int(sum(ns)))
    rc = ulib().hipsdp_syevx_many_below_unit(device, len(mats), _ip(ns), _dp(cat), C.c_double(bound), int(maxk), int(cap), _ip(cnt), _dp(lam),
                                             _dp(V))
    if rc != 0:
        raise RuntimeError("hipsdp_syevx_many_below_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    out, off = [], 0
    for j, n in enumerate(ns):
        kj = int(cnt[j])
        out.append((kj, lam[j * maxk:j * maxk + kj].copy(), V[off:off + kj * n].reshape(kj, n).copy()))
        off += maxk * int(n)
    return out


# ---- unit-level host-buffer kernels ---------------------------------------------------------------------------------

def _params(kw):
    p = Params()
    lib().hipsdp_default_params(C.byref(p))
    for k, v in (kw or {}).items():
        setattr(p, k, v)
    return p


def solve_many(solvers, params=None):
    """hipsdp_solve_many: every Solver of the list (loaded, one device, each at most once) solved in one call - the one-launch
    kernel once per size class for all of them, the general path one after another for the rest.  params: None (defaults), one dict
    for all, or a list of dicts, one per solver (Solver.solve's keywords).  Returns the list of Info; raises RuntimeError with the
    per-solver return codes when any of them failed."""
    n = len(solvers)
    if isinstance(params, (list, tuple)):
        if len(params) != n:
            raise ValueError("solve_many: %d params for %d solvers" % (len(params), n))
        plist = [_params(kw) for kw in params]
    else:
        plist = [_params(params)] * n
    hs = (C.c_void_p * max(n, 1))(*[s.h for s in solvers])
    ps = (Params * max(n, 1))(*plist)
    infos = (Info * max(n, 1))()
    rcs = (C.c_int * max(n, 1))()
    rc = lib().hipsdp_solve_many(n, hs, ps, infos, rcs)
    if rc != 0:
        raise RuntimeError("hipsdp_solve_many failed: rc=%d, per solver %s (%s)" %
                           (rc, list(rcs)[:n], lib().hipsdp_last_error().decode()))
    return [infos[i] for i in range(n)]


def solve_many_stats():
    """(launches, problems): process totals of hipsdp_solve_many's one-launch part"""
    launches = C.c_longlong(0)
    problems = C.c_longlong(0)
    _chk(lib().hipsdp_solve_many_stats(C.byref(launches), C.byref(problems)), "hipsdp_solve_many_stats")
    return launches.value, problems.value


def solve_objectives_stats():
    """(calls, launches, problems): process totals of hipsdp_solve_objectives - calls, launches of its fan-out and of the one-launch
    kernel, jobs whose results that kernel delivered"""
    v = [C.c_longlong(0) for _ in range(3)]
    _chk(lib().hipsdp_solve_objectives_stats(*[C.byref(x) for x in v]), "hipsdp_solve_objectives_stats")
    return tuple(x.value for x in v)


def objs_fanout_unit(B, b_own, ns, q=0, start=None, gap=2, guard=-7.25):
    """hipsdp_objs_fanout_unit (libhipsdp_units.so): the fan-out kernel of hipsdp_solve_objectives alone.  B: count x m, b_own: m,
    start: None or (y, x, z, [X_k], [Z_k]).  Returns (lanes [(count + 1) x lane_len], offs, launches): lane 0 is the home lane, every
    array of a lane is followed by gap guard words."""
    B = _f64(B)
    count, m = B.shape
    b_own = _f64(b_own)
    nsa = (C.c_int * max(len(ns), 1))(*[int(n) for n in ns])
    offs = np.zeros(4 + 2 * len(ns), dtype=np.int64)
    po = offs.ctypes.data_as(C.POINTER(C.c_longlong))
    ln = C.c_longlong(0)
    launches = C.c_int(0)
    if start is not None:
        y, x, z, X, Z = start
        y, x, z = _f64(y), _f64(x if q else np.zeros(1)), _f64(z if q else np.zeros(1))
        XZ = _f64(np.concatenate([np.concatenate([_f64(X[k]).ravel(), _f64(Z[k]).ravel()]) for k in range(len(ns))]))
        ptrs = (_dp(y), _dp(x), _dp(z), _dp(XZ))
    else:
        ptrs = (None, None, None, None)
    hs = 1 if start is not None else 0
    rc = ulib().hipsdp_objs_fanout_unit(0, count, m, q, len(ns), nsa, _dp(B), _dp(b_own), hs, *ptrs, gap, C.c_double(guard), C.byref(ln),
                                        po, None, None)
    if rc != 0:
        raise RuntimeError("hipsdp_objs_fanout_unit failed: rc=%d" % rc)
    lanes = np.zeros((count + 1, ln.value))
    rc = ulib().hipsdp_objs_fanout_unit(0, count, m, q, len(ns), nsa, _dp(B), _dp(b_own), hs, *ptrs, gap, C.c_double(guard), C.byref(ln),
                                        po, _dp(lanes), C.byref(launches))
    if rc != 0:
        raise RuntimeError("hipsdp_objs_fanout_unit failed: rc=%d (%s)" % (rc, ulib().hipsdp_last_error().decode()))
    return lanes, offs.copy(), launches.value


def solve1_fits(m, q, ns):
    """the one-launch kernel's admission rule (hs_solve1_fits: its LDS layout fits) for m variables, q LP rows, blocks of ns rows"""
    a = (C.c_int * max(len(ns), 1))(*[int(n) for n in ns])
    return bool(ulib().hipsdp_solve1_fits(int(m), int(q), len(ns), a))


def solve1_class(m, ns):
    """the size class of the kernel instance that would serve the shape: 10, 16, 64, or 1064 (m > 64)"""
    a = (C.c_int * max(len(ns), 1))(*[int(n) for n in ns])
    return ulib().hipsdp_solve1_class(int(m), len(ns), a)


def dgemm(A, B, layA=0, layB=1, alpha=1.0, beta=0.0, Cin=None, lower_only=False, splitk=0, device=0):
    """row-major C = alpha op(A) op(B) + beta C.  layA = 0: A is [M, K]; 1: A is [K, M].  layB = 0: B is [N, K]; 1: [K, N]."""
    A = _f64(A)
    B = _f64(B)
    M, K = (A.shape if layA == 0 else A.shape[::-1])
    N = B.shape[0] if layB == 0 else B.shape[1]
    Cout = np.zeros((M, N)) if Cin is None else _f64(Cin).copy()
    _chk(lib().hipsdp_dgemm(device, layA, layB, M, N, K, C.c_double(alpha), _dp(A), C.c_longlong(A.shape[1]), _dp(B),
                            C.c_longlong(B.shape[1]), C.c_double(beta), _dp(Cout), C.c_longlong(N), int(lower_only), splitk),
         "hipsdp_dgemm")
    return Cout


def schur_dense(A, X, Zinv, ws_gbytes=0.0, device=0):
    A = _f64(A)
    m1, n = A.shape[0], A.shape[1]
    X = _f64(X)
    Zinv = _f64(Zinv)
    Mx = np.zeros((m1, m1))
    _chk(ulib().hipsdp_schur_dense(device, m1, n, _dp(A), _dp(X), _dp(Zinv), _dp(Mx), C.c_double(ws_gbytes)),
         "hipsdp_schur_dense")
    return Mx


def schur_sparse_unit(n, m, coo, X, Zinv, device=0):
    """(m + 1) x (m + 1) array whose lower triangle of rows / columns 1 .. m holds tr(A_i X A_j Zinv) as csrc/sparse.hip assembles it"""
    var, row, col, val = coo
    var = np.ascontiguousarray(var, dtype=np.int32); row = np.ascontiguousarray(row, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32); val = _f64(val)
    X = _f64(X); Zinv = _f64(Zinv)
    Mx = np.zeros((m + 1, m + 1))
    _chk(ulib().hipsdp_schur_sparse_unit(device, n, m, C.c_longlong(len(val)), _ip(var), _ip(row), _ip(col), _dp(val), _dp(X), _dp(Zinv), _dp(Mx)),
         "hipsdp_schur_sparse_unit")
    return Mx


def _coo_i32(coo):
    var, row, col, val = coo
    return (np.ascontiguousarray(var, dtype=np.int32), np.ascontiguousarray(row, dtype=np.int32),
            np.ascontiguousarray(col, dtype=np.int32), _f64(val))


def schur_sparse_unit2(n, m, coo, X, Zinv, kernel=-1, device=0):
    """schur_sparse_unit with the kernel in the caller's hand (hipsdp_schur_sparse_unit2: kernel -1 the engine's rule, 0 one thread
    per pair, 1 one wavefront per pair): (Mx, took) with took = the kernel that ran"""
    var, row, col, val = _coo_i32(coo)
    X = _f64(X); Zinv = _f64(Zinv)
    Mx = np.zeros((m + 1, m + 1))
    took = C.c_int(-7)
    _chk(ulib().hipsdp_schur_sparse_unit2(device, n, m, C.c_longlong(len(val)), _ip(var), _ip(row), _ip(col), _dp(val), _dp(X), _dp(Zinv),
                                          _dp(Mx), int(kernel), C.byref(took)), "hipsdp_schur_sparse_unit2")
    return Mx, took.value


def sparse_ops_unit(n, m, coo, V=None, coef=None, base=None, device=0):
    """the two passes of csrc/sparse.hip on the caller's triplets (hipsdp_sparse_ops_unit): (outA[m] = <A_v, V> or None when V is None,
    outAT[n, n] = base + sum_v coef[v] A_v or None when coef is None; coef has m + 1 entries, base defaults to zeros)"""
    var, row, col, val = _coo_i32(coo)
    outA = outAT = None
    pV = pc = pb = pA = pAT = None
    if V is not None:
        V = _f64(V)
        assert V.shape == (n, n)
        outA = np.full(m, np.nan)
        pV, pA = _dp(V), _dp(outA)
    if coef is not None:
        coef = _f64(coef)
        assert coef.shape == (m + 1,)
        base = np.zeros((n, n)) if base is None else _f64(base)
        assert base.shape == (n, n)
        outAT = np.full((n, n), np.nan)
        pc, pb, pAT = _dp(coef), _dp(base), _dp(outAT)
    _chk(ulib().hipsdp_sparse_ops_unit(device, n, m, C.c_longlong(len(val)), _ip(var), _ip(row), _ip(col), _dp(val), pV, pc, pb, pA, pAT),
         "hipsdp_sparse_ops_unit")
    return outA, outAT


def schur_w(A, X, Z, device=0):
    A = _f64(A)
    m1, n = A.shape[0], A.shape[1]
    X = _f64(X)
    Z = _f64(Z)
    Mx = np.zeros((m1, m1))
    _chk(ulib().hipsdp_schur_w(device, m1, n, _dp(A), _dp(X), _dp(Z), _dp(Mx)), "hipsdp_schur_w")
    return Mx


def schur_form_unit(form, A, P, Q, parts=1, ws_gbytes=0.0, device=0):
    """one dense block through ONE form of the assembly from the caller's operands (0 hs_schur_W, 1 hs_schur_Wcols in `parts` slices,
    2 hs_schur_Urows in 2 * parts chunks, 3 hs_schur_U, 4 hs_schur_Wvar in slices of `parts` columns; W forms: P = R, Q = G, U forms:
    P = X, Q = Zinv) -> (Mx with both triangles, (products of the persistent kernels, of these the paired-band kernel's, Gram kernel's))"""
    A = _f64(A)
    m1, n = A.shape[0], A.shape[1]
    P = _f64(P); Q = _f64(Q)
    assert A.shape == (m1, n, n) and P.shape == (n, n) and Q.shape == (n, n)
    Mx = np.zeros((m1, m1))
    used = (C.c_int * 3)(0, 0, 0)
    _chk(ulib().hipsdp_schur_form_unit(device, form, parts, m1, n, _dp(A), _dp(P), _dp(Q), C.c_double(ws_gbytes), _dp(Mx), used),
         "hipsdp_schur_form_unit")
    return Mx, tuple(used)


def schur_small_unit(As, Xs, Zinvs, Dext=None, x=None, z=None, fill=0.0, device=0):
    """hs_schur_small alone: block k has the matrices As[k] (m1 x n_k x n_k), Xs[k], Zinvs[k]; LP rows Dext (q x m1), x, z or None
    -> (taken, Mx, Lm, diagM); the outputs start as `fill`, which is what comes back where the kernel wrote nothing"""
    As = [_f64(a) for a in As]; Xs = [_f64(a) for a in Xs]; Zinvs = [_f64(a) for a in Zinvs]
    nblk, m1 = len(As), As[0].shape[0]
    ns = np.array([a.shape[1] for a in As], dtype=np.int32)
    for k in range(nblk):
        assert As[k].shape == (m1, ns[k], ns[k]) and Xs[k].shape == (ns[k], ns[k]) and Zinvs[k].shape == (ns[k], ns[k])
    q = 0 if Dext is None else int(np.shape(Dext)[0])
    if q > 0:
        Dext = _f64(Dext); x = _f64(x); z = _f64(z)
        assert Dext.shape == (q, m1) and x.shape == (q,) and z.shape == (q,)
    arr = C.POINTER(C.c_double) * nblk
    pA, pX, pZ = arr(*[_dp(a) for a in As]), arr(*[_dp(a) for a in Xs]), arr(*[_dp(a) for a in Zinvs])
    m = m1 - 1
    Mx = np.full((m1, m1), fill)
    Lm = np.full(max(m * m, 1), fill)
    dg = np.full(max(m, 1), fill)
    taken = C.c_int(-1)
    _chk(ulib().hipsdp_schur_small_unit(device, m1, nblk, _ip(ns), pA, pX, pZ, q, _dp(Dext) if q else None, _dp(x) if q else None,
                                        _dp(z) if q else None, _dp(Mx), _dp(Lm), _dp(dg), C.byref(taken)), "hipsdp_schur_small_unit")
    return taken.value, Mx, Lm[:m * m].reshape(m, m), dg[:m]


def gram_plan_info(M, K, nslab=64, device=0):
    """the plan csrc/gram.hip chooses for the Gram product of a shape -> (no, nd, items, span), or None when it takes none"""
    no, nd, ni = C.c_int(0), C.c_int(0), C.c_int(0)
    sp = C.c_double(0.0)
    rc = ulib().hipsdp_gram_plan_info(device, M, C.c_longlong(K), nslab, C.byref(no), C.byref(nd), C.byref(ni), C.byref(sp))
    return (no.value, nd.value, ni.value, sp.value) if rc == 0 else None


def dgemm_selfcheck(M, N, K, layB=1, batch=1, splitk=1, flags=0, beta=0.0, device=0):
    """both GEMM kernels on the same device-generated operands -> (used_v2, number of elements of C differing in any bit)"""
    used = C.c_int(0)
    nd = C.c_longlong(0)
    _chk(ulib().hipsdp_dgemm_selfcheck(device, M, N, K, layB, batch, splitk, flags, C.c_double(beta), C.byref(used), C.byref(nd)),
         "hipsdp_dgemm_selfcheck")
    return used.value, nd.value


def dgemm_selfcheck2(M, N, K, layB=1, batch=1, splitk=1, flags=0, alpha=1.0, beta=0.0, reps=0, device=0):
    """the tile kernel alone against the default dispatch (persistent tile kernel, strip kernel) on the same device-generated
    operands -> (used bits: 1 persistent tile kernel, 2 strip kernel; differing elements; ms tile; ms default)"""
    used = C.c_int(0)
    nd = C.c_longlong(0)
    t0, t1 = C.c_double(0.0), C.c_double(0.0)
    _chk(ulib().hipsdp_dgemm_selfcheck2(device, M, N, K, layB, batch, splitk, flags, C.c_double(alpha), C.c_double(beta), reps,
                                       C.byref(used), C.byref(nd), C.byref(t0), C.byref(t1)), "hipsdp_dgemm_selfcheck2")
    return used.value, nd.value, t0.value, t1.value


def dgemm_selfcheck3(M, N, K, layB=1, batch=1, splitk=1, flags=0, alpha=1.0, beta=0.0, reps=0, device=0):
    """as dgemm_selfcheck2, with the largest absolute difference of the two results and the number of elements that differ between
    two runs of the default dispatch -> (used bits, differing elements, max |difference|, not reproduced, ms tile, ms default)"""
    used = C.c_int(0)
    nd, nr = C.c_longlong(0), C.c_longlong(0)
    md, t0, t1 = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    _chk(ulib().hipsdp_dgemm_selfcheck3(device, M, N, K, layB, batch, splitk, flags, C.c_double(alpha), C.c_double(beta), reps,
                                       C.byref(used), C.byref(nd), C.byref(md), C.byref(nr), C.byref(t0), C.byref(t1)), "hipsdp_dgemm_selfcheck3")
    return used.value, nd.value, md.value, nr.value, t0.value, t1.value


def tri_product_unit(A, B, flags, mode, layB=1, sentinel=None, pad_rows=0, pad_cols=0, device=0):
    """one product with a triangular operand from the caller's operands, the paired-band kernel's instance forced (mode 0: 128 x 128,
    1: wide, -1: default dispatch): A (M x K), B (batch x K x N for layB = 1, batch x N x K for 0) -> (C as (batch, M + pad_rows,
    N + pad_cols) that started as `sentinel` everywhere, (products of the paired-band kernel, of these the wide instance's))"""
    A = _f64(A); B = _f64(B)
    M, K = A.shape
    batch = B.shape[0]
    N = B.shape[2] if layB == 1 else B.shape[1]
    assert B.shape == ((batch, K, N) if layB == 1 else (batch, N, K))
    Cio = np.full((batch, M + pad_rows, N + pad_cols), np.nan if sentinel is None else sentinel)
    used = (C.c_int * 2)(0, 0)
    _chk(ulib().hipsdp_tri_product_unit(device, mode, M, N, K, layB, batch, flags, _dp(A), _dp(B), _dp(Cio), M + pad_rows, N + pad_cols, used),
         "hipsdp_tri_product_unit")
    return Cio, tuple(used)


def tri_instance_force(mode):
    """forces the paired-band kernel's instance for products reached through other entries of the units library (0: 128 x 128, 1: wide,
    -1: chosen per shape again) -> products the wide instance has taken so far"""
    return ulib().hipsdp_tri_instance_force(mode)


def gram_product_unit(W, K, mode, alpha=1.0, beta=0.0, Cin=None, nslab=64, device=0):
    """one Gram product from the caller's operands, the Gram kernel's instance forced (mode 0: 128 x 128, 1: wide, -1: chosen per
    shape): W (M x ldw, the first K of every row are the operand) -> (C (M x M) that started as Cin with its lower triangle
    = alpha W W^T + beta Cin, (the Gram kernel took it, its wide instance did))"""
    W = _f64(W)
    M, ldw = W.shape
    Cio = np.zeros((M, M)) if Cin is None else _f64(Cin).copy()
    assert Cio.shape == (M, M)
    used = (C.c_int * 2)(0, 0)
    _chk(ulib().hipsdp_gram_product_unit(device, mode, M, C.c_longlong(K), _dp(W), C.c_longlong(ldw), C.c_double(alpha), C.c_double(beta),
                                         _dp(Cio), nslab, used), "hipsdp_gram_product_unit")
    return Cio, tuple(used)


def gram_instance_force(mode):
    """forces the Gram kernel's instance for products reached through other entries of the units library (0: 128 x 128, 1: wide,
    -1: chosen per shape again) -> products the wide instance has taken so far"""
    return ulib().hipsdp_gram_instance_force(mode)


def gram_plan_unit(inst, M, K, nslab=64, forced=False):
    """host only: the plan of one instance of the Gram kernel -> None, or (items as an (n, 5) array of ti, tj, k0, k1, slab; list
    offsets; partial tiles per off-diagonal tile; per diagonal tile)"""
    info = (C.c_int * 4)()
    off = np.zeros(513, dtype=np.int32)
    items = np.zeros((4096, 6), dtype=np.int32)
    if ulib().hipsdp_gram_plan_unit(inst, int(forced), M, C.c_longlong(K), nslab, items.shape[0], _ip(items), _ip(off), info) != 0:
        return None
    assert info[0] <= items.shape[0]
    return items[:info[0], :5].copy(), off[:info[1] + 1].copy(), info[2], info[3]


def gram_selfcheck(M, K, reps=0, device=0):
    """W W^T on the lower triangle through the K-sliced tile kernels and through the Gram kernel (csrc/gram.hip)
    -> (Gram kernel took it, max |difference| over the lower triangle, elements not reproduced by a second run, ms tile path, ms Gram kernel)"""
    used = C.c_int(0)
    nr = C.c_longlong(0)
    md, t0, t1 = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    _chk(ulib().hipsdp_gram_selfcheck(device, M, C.c_longlong(K), reps, C.byref(used), C.byref(md), C.byref(nr), C.byref(t0), C.byref(t1)),
         "hipsdp_gram_selfcheck")
    return used.value, md.value, nr.value, t0.value, t1.value


def schur_identity_unit(A, Mx=None, ws_gbytes=0.0, full_storage=False, device=0):
    """first assembly of a cold solve on its own: Mx (zeros when None) += <A_i, A_j> on the lower tiles, from the packed lower triangles
    (csrc/schur.hip: hs_schur_W_identity_packed) or, full_storage=True, from the full rows -> (Mx, executed matrix-core flops)"""
    A = _f64(A)
    m1, n = A.shape[0], A.shape[1]
    Mx = np.zeros((m1, m1)) if Mx is None else _f64(Mx).copy()
    fl = C.c_double(0.0)
    _chk(ulib().hipsdp_schur_identity_unit(device, m1, n, _dp(A), C.c_double(ws_gbytes), int(full_storage), _dp(Mx), C.byref(fl)),
         "hipsdp_schur_identity_unit")
    return Mx, fl.value


def potrf(A, device=0):
    L = _f64(A).copy()
    fail = C.c_int(0)
    _chk(ulib().hipsdp_potrf(device, L.shape[0], _dp(L), C.byref(fail)), "hipsdp_potrf")
    return np.tril(L), fail.value


def potrf_ex(A, psd=False, v1=False, device=0):
    """blocked Cholesky in either form -> (L with the untouched upper part as stored, dinv, regmask, fail)"""
    L = _f64(A).copy()
    n = L.shape[0]
    dinv = np.zeros(((n + 63) // 64) * 4096)
    mask = np.zeros(n, dtype=np.int32)
    fail = C.c_int(0)
    _chk(ulib().hipsdp_potrf_ex(device, n, _dp(L), int(psd), int(v1), _dp(dinv), _ip(mask), C.byref(fail)), "hipsdp_potrf_ex")
    return L, dinv, mask, fail.value


def potrs(A, rhs, device=0):
    A = _f64(A)
    r = _f64(rhs).copy()
    r2 = r.reshape(-1, A.shape[0])
    _chk(ulib().hipsdp_potrs(device, A.shape[0], _dp(A), r2.shape[0], _dp(r2)), "hipsdp_potrs")
    return r2.reshape(r.shape)


def potrs_seq(A, calls, psd=False, device=0):
    """one factorization, then the solves of `calls` = [(mode, rhs[k, n]), ...] one behind the other on ONE hs_trsv_sync workspace
    -> (list of solved rhs, zeroed-column mask, fail)"""
    A = _f64(A)
    n = A.shape[0]
    nc = len(calls)
    slab = np.zeros((max(nc, 1), 4, n))
    nrhs = np.zeros(max(nc, 1), dtype=np.int32)
    mode = np.zeros(max(nc, 1), dtype=np.int32)
    for c, (md, r) in enumerate(calls):
        r = _f64(r).reshape(-1, n)
        nrhs[c], mode[c] = r.shape[0], md
        slab[c, :min(r.shape[0], 4)] = r[:4]
    mask = np.zeros(n, dtype=np.int32)
    fail = C.c_int(0)
    _chk(ulib().hipsdp_potrs_seq(device, n, _dp(A), int(psd), nc, _ip(nrhs), _ip(mode), _dp(slab), _ip(mask), C.byref(fail)),
         "hipsdp_potrs_seq")
    return [slab[c, :nrhs[c]].copy() for c in range(nc)], mask, fail.value


def potrf_small_unit(base, dir=None, alpha=0.0, pair=False, set_flag=False, want_gram=False, device=0):
    """fused single-block factorization of base + alpha dir; pair: base (and dir) hold two problems [2, n, n]
    -> dict(L, dinv, Mout, Linv, Gram or None, flag) with a leading axis of 2 when pair"""
    base = _f64(base)
    n = base.shape[-1]
    npb = 2 if pair else 1
    assert base.size == npb * n * n
    d = None if dir is None else _f64(dir)
    assert d is None or d.size == base.size
    shp = (2, n, n) if pair else (n, n)
    out = {"L": np.zeros(shp), "dinv": np.zeros((2, 64, 64) if pair else (64, 64)), "Mout": np.zeros(shp), "Linv": np.zeros(shp),
           "Gram": np.zeros(shp) if want_gram else None}
    flag = np.zeros(2, dtype=np.int32)
    _chk(ulib().hipsdp_potrf_small_unit(device, n, int(pair), _dp(base), None if d is None else _dp(d), C.c_double(alpha), int(set_flag),
                                        int(want_gram), _dp(out["L"]), _dp(out["dinv"]), _dp(out["Mout"]), _dp(out["Linv"]),
                                        None if not want_gram else _dp(out["Gram"]), _ip(flag)), "hipsdp_potrf_small_unit")
    out["flag"] = flag.copy() if pair else int(flag[0])
    return out


def potrf_pair_unit(A2, pair=True, device=0):
    """strict-mode blocked Cholesky of two matrices A2[2, n, n], through hs_potrf_pair or (pair=False) two hs_potrf calls
    -> (L[2, n, n] with the upper part as stored, dinv[2, len] with the staging blocks, fail[2])"""
    L = _f64(A2).copy()
    n = L.shape[-1]
    assert L.shape == (2, n, n)
    ulib().hipsdp_potrf_dinv_len.restype = C.c_longlong
    nd = int(ulib().hipsdp_potrf_dinv_len(n))
    dinv = np.zeros((2, nd))
    fail = np.zeros(2, dtype=np.int32)
    _chk(ulib().hipsdp_potrf_pair_unit(device, n, int(pair), _dp(L), _dp(dinv), _ip(fail)), "hipsdp_potrf_pair_unit")
    return L, dinv, fail


def trial_pair_unit(arrays, alpha, fused=True, first=True, device=0):
    """arrays[8, n, n] = X, Z, dX, dZ, Xs, Zs, Lx, Lz -> the same eight after the trial iterates of a step were formed by hs_trial_pair
    (fused) or by the copy / scale_add / copy launches it replaces"""
    io = _f64(arrays).copy()
    n = io.shape[-1]
    assert io.shape == (8, n, n)
    _chk(ulib().hipsdp_trial_pair_unit(device, n, int(fused), int(first), C.c_double(alpha), _dp(io)), "hipsdp_trial_pair_unit")
    return io


def _packed_len(n):
    t = n * (n + 1) // 2
    return t + (t & 1)


def tail_after_solve2_unit(rhs2, u1, fused, device=0):
    """-> (u2, wt, e2, e1) of k_after_solve2 + hs_make_ext twice, or of the one launch that replaces them"""
    rhs2, u1 = _f64(rhs2), _f64(u1)
    m = u1.size
    assert rhs2.size == 2 * m
    u2, wt, e2, e1 = np.zeros(m), np.zeros(m + 1), np.zeros(m + 1), np.zeros(m + 1)
    _chk(ulib().hipsdp_tail_after_solve2_unit(device, m, int(fused), _dp(rhs2), _dp(u1), _dp(u2), _dp(wt), _dp(e2), _dp(e1)),
         "hipsdp_tail_after_solve2_unit")
    return u2, wt, e2, e1


def tail_unpack3_unit(pk, n, fused, device=0):
    pk = _f64(pk)
    assert pk.shape == (3, _packed_len(n))
    out = np.zeros((3, n, n))
    _chk(ulib().hipsdp_tail_unpack3_unit(device, n, int(fused), _dp(pk), _dp(out)), "hipsdp_tail_unpack3_unit")
    return out


def tail_dz_unit(pk, P2, Rd, dtau, eta, fused, device=0):
    pk, P2, Rd = _f64(pk), _f64(P2), _f64(Rd)
    n = P2.shape[0]
    assert pk.size == _packed_len(n) and P2.shape == Rd.shape == (n, n)
    dZ = np.zeros((n, n))
    _chk(ulib().hipsdp_tail_dz_unit(device, n, int(fused), _dp(pk), _dp(P2), _dp(Rd), C.c_double(dtau), C.c_double(eta), _dp(dZ)),
         "hipsdp_tail_dz_unit")
    return dZ


def tail_dirmat_unit(s1, Zinv, X, GZ, fused, device=0):
    Zinv, X, GZ = _f64(Zinv), _f64(X), _f64(GZ)
    n = X.shape[0]
    H, pk = np.zeros((n, n)), np.zeros(_packed_len(n))
    _chk(ulib().hipsdp_tail_dirmat_unit(device, n, int(fused), C.c_double(s1), _dp(Zinv), _dp(X), _dp(GZ), _dp(H), _dp(pk)),
         "hipsdp_tail_dirmat_unit")
    return H, pk


def tail_dir_unit(B, H, rhs2, rp, b, u1, u2, par, sc, fused, device=0):
    """the scalars of a direction and its closing kernel -> (scalar block, dy, dyt)"""
    B, H = _f64(B), _f64(H)
    vs = [_f64(v) for v in (rhs2, rp, b, u1, u2)]
    m, n = vs[0].size, B.shape[0]
    par = _f64(par)
    sc = _f64(sc).copy()
    assert par.size == 6 and sc.size == ulib().hipsdp_tail_sc_len() and all(v.size == m for v in vs) and B.shape == H.shape == (n, n)
    dy, dyt = np.zeros(m), np.zeros(m + 1)
    _chk(ulib().hipsdp_tail_dir_unit(device, m, n, int(fused), _dp(B), _dp(H), _dp(vs[0]), _dp(vs[1]), _dp(vs[2]), _dp(vs[3]), _dp(vs[4]),
                                     _dp(par), _dp(sc), _dp(dy), _dp(dyt)), "hipsdp_tail_dir_unit")
    return sc, dy, dyt


def tail_sc_len():
    return int(ulib().hipsdp_tail_sc_len())


def tail_dots_unit(a, v, fused, device=0):
    a, v = _f64(a), _f64(v)
    n = int(round(np.sqrt(a.shape[1])))
    assert a.shape == (3, n * n) and v.shape[0] == 2
    out = np.zeros(3)
    _chk(ulib().hipsdp_tail_dots_unit(device, v.shape[1], n, int(fused), _dp(a), _dp(v), _dp(out)), "hipsdp_tail_dots_unit")
    return out


def _opt(a):
    return None if a is None else _dp(a)


def small_dir_block_unit(c, s1, X, R, E, Zinv, recorded, device=0):
    """hs_dir_block_small launched (recorded=False) or as a record of the batch kernel -> (out[n, n], records pending)"""
    X, R, Zinv = _f64(X), _f64(R), _f64(Zinv)
    E = None if E is None else _f64(E)
    n = X.shape[0]
    assert X.shape == R.shape == Zinv.shape == (n, n) and (E is None or E.shape == (n, n))
    out, pend = np.zeros((n, n)), C.c_int(-1)
    _chk(ulib().hipsdp_small_dir_block_unit(device, n, C.c_double(c), C.c_double(s1), _dp(X), _dp(R), _opt(E), _dp(Zinv), int(recorded),
                                            _dp(out), C.byref(pend)), "hipsdp_small_dir_block_unit")
    return out, pend.value


def small_lp_rows_unit(Dext, v, mode, eta, sigmu, x, z, rd, elp, recorded, device=0):
    """hs_lp_rows_small -> (out1[q], out2[q], records pending)"""
    Dext, v, x, z, rd = _f64(Dext), _f64(v), _f64(x), _f64(z), _f64(rd)
    elp = None if elp is None else _f64(elp)
    q, m1 = Dext.shape
    assert v.size == m1 and x.size == z.size == rd.size == q and (elp is None or elp.size == q)
    o1, o2, pend = np.zeros(q), np.zeros(q), C.c_int(-1)
    _chk(ulib().hipsdp_small_lp_rows_unit(device, q, m1, _dp(Dext), _dp(v), int(mode), C.c_double(eta), C.c_double(sigmu), _dp(x), _dp(z),
                                          _dp(rd), _opt(elp), int(recorded), _dp(o1), _dp(o2), C.byref(pend)), "hipsdp_small_lp_rows_unit")
    return o1, o2, pend.value


def small_apply_A_unit(As, Vs, Dext, vlp, epi, scal, vin, recorded, device=0):
    """hs_apply_A_small over the blocks As[k] (m1 x n2_k) with Vs[k] (n2_k) and the LP rows Dext (q x m1, q may be 0) with vlp
    -> (out[m1], vout[m1 - 1], records pending)"""
    As = [_f64(a) for a in As]
    Vs = [_f64(v).ravel() for v in Vs]
    m1 = As[0].shape[0]
    n2 = np.array([a.shape[1] for a in As], dtype=np.int32)
    assert all(a.shape[0] == m1 for a in As) and all(v.size == k for v, k in zip(Vs, n2))
    A = np.concatenate([a.ravel() for a in As])
    V = np.concatenate(Vs)
    Dext, vlp, vin = _f64(Dext).reshape(-1, m1), _f64(vlp), _f64(vin)
    q = Dext.shape[0]
    assert vlp.size == q and vin.size == m1 - 1
    out, vout, pend = np.zeros(m1), np.zeros(m1 - 1), C.c_int(-1)
    _chk(ulib().hipsdp_small_apply_A_unit(device, m1, len(As), _ip(n2), _dp(A), _dp(V), q, _dp(Dext), _dp(vlp), int(epi), C.c_double(scal),
                                          _dp(vin), int(recorded), _dp(out), _dp(vout), C.byref(pend)), "hipsdp_small_apply_A_unit")
    return out, vout, pend.value


def small_elementwise_unit(vecs, par, xs, ys, nn, use_elp, recorded, device=0):
    """hs_lp_dir, hs_vec_mul, hs_make_ext and hs_axpy3 in one call: vecs[6, n] = x, z, r, elp, a, b; par = sigmu, eta, alpha, s0, s1;
    xs, ys: the three vectors of hs_axpy3 (nn[0], nn[1], nn[2] entries) one behind the other
    -> (o_lp[n], o_mul[n], o_ext[n + 1], ys after the update, records pending)"""
    vecs, par, xs, ys = _f64(vecs), _f64(par), _f64(xs), _f64(ys).copy()
    nn = np.ascontiguousarray(nn, dtype=np.int32)
    n = vecs.shape[1]
    assert vecs.shape == (6, n) and par.size == 5 and nn.size == 3 and xs.size == ys.size == int(nn.sum())
    o_lp, o_mul, o_ext, pend = np.zeros(n), np.zeros(n), np.zeros(n + 1), C.c_int(-1)
    _chk(ulib().hipsdp_small_elementwise_unit(device, n, _ip(nn), _dp(par), int(use_elp), _dp(vecs), _dp(xs), int(recorded), _dp(o_lp),
                                              _dp(o_mul), _dp(o_ext), _dp(ys), C.byref(pend)), "hipsdp_small_elementwise_unit")
    return o_lp, o_mul, o_ext, ys, pend.value


def small_gemv_t_unit(A, E, coef, sa, add, add_mode, recorded, device=0):
    """hs_gemv_t on the first E entries of the rows of A[R, lda]; add_mode 0: no additive term, 1: add an array of its own, 2: add is
    what the output holds before the call -> (out[E], records pending)"""
    A, coef = _f64(A), _f64(coef)
    R, lda = A.shape
    add = None if add is None else _f64(add)
    assert coef.size == R and 1 <= E <= lda and (add_mode == 0 or add.size == E)
    out, pend = np.zeros(E), C.c_int(-1)
    _chk(ulib().hipsdp_small_gemv_t_unit(device, R, C.c_longlong(E), C.c_longlong(lda), _dp(A), _dp(coef), C.c_double(sa), int(add_mode),
                                         _opt(add), int(recorded), _dp(out), C.byref(pend)), "hipsdp_small_gemv_t_unit")
    return out, pend.value


def reductions_unit(kind, lens, slots, accumulate, a, b, c, preset, recorded, device=0):
    """reductions of one kind (0 dot, 1 absmax, 2 ratio_min, 3 lp_s0), reduction j over lens[j] entries of a, b, c (one behind the
    other) into slot slots[j] of preset.size slots, every slot first set to preset -> (out[nslots], records pending)"""
    lens, slots, accumulate = (np.ascontiguousarray(v, dtype=np.int32) for v in (lens, slots, accumulate))
    a, b, c, preset = _f64(a), _f64(b), _f64(c), _f64(preset)
    assert lens.size == slots.size == accumulate.size and a.size == b.size == c.size == int(lens.sum())
    out, pend = np.zeros(preset.size), C.c_int(-1)
    _chk(ulib().hipsdp_reductions_unit(device, int(kind), lens.size, _ip(lens), _ip(slots), _ip(accumulate), _dp(a), _dp(b), _dp(c),
                                       preset.size, _dp(preset), int(recorded), _dp(out), C.byref(pend)), "hipsdp_reductions_unit")
    return out, pend.value


def small_solve_unit(M, rhs, form, ld=None, device=0):
    """the small solves with the factor of M (m <= 64).  form 0: hs_red_batch_solve on rhs[nrhs, ld] in place -> (rhs, records pending,
    factorization flag); form 1: k_solve2_small on rhs = [g ; b] -> (rhs2[2 m], u2[m], wt[m + 1], factorization flag)"""
    M = _f64(M)
    m = M.shape[0]
    rhs = _f64(rhs).copy()
    pend, fail = C.c_int(-1), C.c_int(-1)
    if form == 0:
        nrhs, ld = rhs.shape
        _chk(ulib().hipsdp_small_solve_unit(device, m, _dp(M), 0, nrhs, C.c_longlong(ld), _dp(rhs), None, None, C.byref(pend),
                                            C.byref(fail)), "hipsdp_small_solve_unit")
        return rhs, pend.value, fail.value
    assert rhs.size == 2 * m
    u2, wt = np.zeros(m), np.zeros(m + 1)
    _chk(ulib().hipsdp_small_solve_unit(device, m, _dp(M), 1, 0, C.c_longlong(0), _dp(rhs), _dp(u2), _dp(wt), C.byref(pend),
                                        C.byref(fail)), "hipsdp_small_solve_unit")
    return rhs, u2, wt, fail.value


def gemv_t3_unit(A, E, c, fused, device=0):
    """three linear combinations c[3, R] of the first E entries of the rows of A[R, lda] -> (out[3, E], fused kernel took the shape)"""
    A, c = _f64(A), _f64(c)
    R, lda = A.shape
    assert c.shape == (3, R) and 1 <= E <= lda
    out, took = np.zeros((3, E)), C.c_int(-1)
    _chk(ulib().hipsdp_gemv_t3_unit(device, R, C.c_longlong(E), C.c_longlong(lda), _dp(A), _dp(c), int(fused), _dp(out), C.byref(took)),
         "hipsdp_gemv_t3_unit")
    return out, took.value


def pass_a_unit(A, E, V, voff=0, wsdoubles=0, device=0):
    """hs_gemv_n on the first E entries of the rows of A[R, lda] with the vectors V[nv, E] (device copies voff doubles behind an aligned
    address) and a workspace of wsdoubles -> (out[nv, R], slices a row was cut into, two-at-a-time kernel taken)"""
    A, V = _f64(A), _f64(V)
    R, lda = A.shape
    nv = V.shape[0]
    assert V.shape == (nv, E) and 1 <= E <= lda
    out = np.zeros((nv, R))
    info = np.zeros(2, dtype=np.int32)
    _chk(ulib().hipsdp_pass_a_unit(device, R, C.c_longlong(E), C.c_longlong(lda), _dp(A), nv, _dp(V), int(voff), C.c_longlong(wsdoubles),
                                   _dp(out), _ip(info)), "hipsdp_pass_a_unit")
    return out, int(info[0]), bool(info[1])


def trtri(A, device=0):
    A = _f64(A)
    Li = np.zeros_like(A)
    _chk(ulib().hipsdp_trtri(device, A.shape[0], _dp(A), _dp(Li)), "hipsdp_trtri")
    return Li


def lambda_min(W, steps=0, device=0):
    W = _f64(W)
    th = C.c_double(0.0)
    rs = C.c_double(0.0)
    _chk(ulib().hipsdp_lambda_min(device, W.shape[0], _dp(W), steps, C.byref(th), C.byref(rs)), "hipsdp_lambda_min")
    return th.value, rs.value


def lambda_min2_unit(W0, W1=None, steps=0, device=0):
    """hs_lanczos_lmin2 without a solver's exchange vectors on one or two host matrices (hipsdp_lambda_min2_unit of the units library):
    exact up to 16 rows, the fused launch per step up to 8192 rows, a launch per step and matrix above; steps 0: min(n, 250).
    Returns (theta[2], resid[2], steps_done[2]); without W1 slot 1 keeps (nan, nan, -1)"""
    W0 = _f64(W0)
    n = W0.shape[0]
    if W1 is not None:
        W1 = _f64(W1)
        assert W1.shape == W0.shape
    th, rs = np.zeros(2), np.zeros(2)
    sd = np.zeros(2, dtype=np.int32)
    _chk(ulib().hipsdp_lambda_min2_unit(device, n, _dp(W0), _dp(W1) if W1 is not None else None, int(steps), _dp(th), _dp(rs), _ip(sd)),
         "hipsdp_lambda_min2_unit")
    return th, rs, sd


def syev(A, device=0):
    A = _f64(A)
    n = A.shape[0]
    lam = np.zeros(n)
    V = np.zeros((n, n))
    _chk(lib().hipsdp_syev(device, n, _dp(A), _dp(lam), _dp(V)), "hipsdp_syev")
    return lam, V


def syevx(A, il, iu, vectors=True, device=0):
    """eigenpairs il..iu (1-based, ascending) of the symmetric matrix A, n <= 512, at most 32 of them: lam, V (row k = k-th returned
    unit eigenvector; None with vectors=False: no vector work is done)"""
    A = _f64(A)
    n = A.shape[0]
    k = max(0, iu - il + 1)
    lam = np.zeros(k)
    V = np.zeros((k, n)) if vectors else None
    _chk(lib().hipsdp_syevx(device, n, _dp(A), int(il), int(iu), _dp(lam), _dp(V) if vectors else None), "hipsdp_syevx")
    return lam, V


def syevx_below(A, bound, maxk, vectors=True, device=0):
    """eigenpairs with eigenvalue <= bound, ascending, at most maxk <= 32 of them: lam, V (as syevx), nbelow = eigenvalues <= bound
    altogether"""
    A = _f64(A)
    n = A.shape[0]
    lam = np.zeros(max(1, maxk))
    V = np.zeros((max(1, maxk), n)) if vectors else None
    cnt, nbelow = C.c_int(-1), C.c_int(-1)
    _chk(lib().hipsdp_syevx_below(device, n, _dp(A), C.c_double(bound), int(maxk), C.byref(cnt), C.byref(nbelow), _dp(lam),
                                  _dp(V) if vectors else None), "hipsdp_syevx_below")
    return lam[:cnt.value].copy(), (V[:cnt.value].copy() if vectors else None), nbelow.value


def syevr(A, vectors=True, device=0):
    """all eigenpairs of the symmetric matrix A, n <= 512, through the tridiagonal form: lam (ascending), V (row k = k-th unit
    eigenvector; None with vectors=False: no vector work is done)"""
    A = _f64(A)
    n = A.shape[0]
    lam = np.zeros(n)
    V = np.zeros((n, n)) if vectors else None
    _chk(lib().hipsdp_syevr(device, n, _dp(A), _dp(lam), _dp(V) if vectors else None), "hipsdp_syevr")
    return lam, V


def tvec_unit(d, e, device=0):
    """stages 2 and 3 of syevr alone (libhipsdp_units.so) on the tridiagonal matrix (d, e): lam (ascending), Z (row k = k-th unit
    eigenvector of T)"""
    d = _f64(d)
    e = _f64(e)
    n = d.shape[0]
    assert e.shape[0] == n - 1
    lam, Z = np.zeros(n), np.zeros((n, n))
    rc = ulib().hipsdp_tvec_unit(device, n, _dp(d), _dp(e), _dp(lam), _dp(Z))
    if rc != 0:
        raise RuntimeError("hipsdp_tvec_unit failed: rc=%d (%s)" % (rc, ulib().hipsdp_last_error().decode()))
    return lam, Z


def tridiag_unit(A, device=0):
    """stage 1 of syevx alone (libhipsdp_units.so): d, e (n - 1), Vrefl (row j = reflector j), tau"""
    A = _f64(A)
    n = A.shape[0]
    d, e, tau, Vr = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((n, n))
    rc = ulib().hipsdp_tridiag_unit(device, n, _dp(A), _dp(d), _dp(e), _dp(Vr), _dp(tau))
    if rc != 0:
        raise RuntimeError("hipsdp_tridiag_unit failed: rc=%d (%s)" % (rc, ulib().hipsdp_last_error().decode()))
    return d, e[:n - 1].copy(), Vr, tau


def gemv_n(A, V, device=0):
    A = _f64(A)
    V = _f64(V).reshape(-1, A.shape[1])
    out = np.zeros((V.shape[0], A.shape[0]))
    _chk(lib().hipsdp_gemv_n(device, A.shape[0], C.c_longlong(A.shape[1]), _dp(A), V.shape[0], _dp(V), _dp(out)),
         "hipsdp_gemv_n")
    return out


def gemv_t(A, coef, device=0):
    A = _f64(A)
    coef = _f64(coef)
    out = np.zeros(A.shape[1])
    _chk(lib().hipsdp_gemv_t(device, A.shape[0], C.c_longlong(A.shape[1]), _dp(A), _dp(coef), _dp(out)), "hipsdp_gemv_t")
    return out


def psd_project(n, row, col, val, minev, epsilon=1e-9, mode=0, device=0):
    """fused PSD projection chain (hipsdp_psd_project): returns (row, col, val) of the upper triangle, row-major order"""
    row = np.ascontiguousarray(row, dtype=np.int32)
    col = np.ascontiguousarray(col, dtype=np.int32)
    val = _f64(val)
    cap = n * (n + 1) // 2
    ro = np.zeros(cap, dtype=np.int32)
    co = np.zeros(cap, dtype=np.int32)
    vo = np.zeros(cap)
    k = C.c_int(0)
    _chk(lib().hipsdp_psd_project(device, n, len(val), _ip(row), _ip(col), _dp(val), C.c_double(minev), C.c_double(epsilon), mode,
                                  cap, C.byref(k), _ip(ro), _ip(co), _dp(vo)), "hipsdp_psd_project")
    return ro[:k.value], co[:k.value], vo[:k.value]


class PsdJob(C.Structure):
    """hipsdp_psd_job of include/hipsdp.h, field for field"""
    _fields_ = [("n", C.c_int), ("nnz", C.c_int), ("row", C.POINTER(C.c_int)), ("col", C.POINTER(C.c_int)),
                ("val", C.POINTER(C.c_double)), ("minev", C.c_double), ("cap", C.c_int), ("nnz_out", C.c_int),
                ("rowout", C.POINTER(C.c_int)), ("colout", C.POINTER(C.c_int)), ("valout", C.POINTER(C.c_double))]


def psd_project_many(jobs, epsilon=1e-9, mode=0, device=0):
    """hipsdp_psd_project_many: jobs is a list of (n, row, col, val, minev); returns the list of (row, col, val) psd_project returns
    for each of them, from one call (cap = n (n + 1) / 2 per job)"""
    count = len(jobs)
    tab = (PsdJob * max(count, 1))()
    keep = []
    for j, (n, row, col, val, minev) in enumerate(jobs):
        row = np.ascontiguousarray(row, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = _f64(val)
        cap = n * (n + 1) // 2
        ro = np.zeros(cap, dtype=np.int32)
        co = np.zeros(cap, dtype=np.int32)
        vo = np.zeros(cap)
        keep.append((row, col, val, ro, co, vo))
        tab[j].n, tab[j].nnz, tab[j].minev, tab[j].cap = n, len(val), minev, cap
        tab[j].row, tab[j].col, tab[j].val = _ip(row), _ip(col), _dp(val)
        tab[j].rowout, tab[j].colout, tab[j].valout = _ip(ro), _ip(co), _dp(vo)
    _chk(lib().hipsdp_psd_project_many(device, count, tab, C.c_double(epsilon), mode), "hipsdp_psd_project_many")
    return [(k[3][:tab[j].nnz_out], k[4][:tab[j].nnz_out], k[5][:tab[j].nnz_out]) for j, k in enumerate(keep)]


def psd_project_many_stats():
    """process totals of hipsdp_psd_project_many: (calls, kernel launches issued for batched jobs, device->host synchronisations)"""
    return _stats3("hipsdp_psd_project_many_stats")


def psd_project_many_large(jobs, epsilon=1e-9, mode=0, device=0):
    """hipsdp_psd_project_many_large: jobs as for psd_project_many; per job the (row, col, val) of its projection, or None for a job
    the call does not serve (fewer than 129 or more than 512 rows)"""
    count = len(jobs)
    tab = (PsdJob * max(count, 1))()
    keep = []
    for j, (n, row, col, val, minev) in enumerate(jobs):
        row = np.ascontiguousarray(row, dtype=np.int32)
        col = np.ascontiguousarray(col, dtype=np.int32)
        val = _f64(val)
        cap = n * (n + 1) // 2
        ro = np.zeros(cap, dtype=np.int32)
        co = np.zeros(cap, dtype=np.int32)
        vo = np.zeros(cap)
        keep.append((row, col, val, ro, co, vo))
        tab[j].n, tab[j].nnz, tab[j].minev, tab[j].cap = n, len(val), minev, cap
        tab[j].row, tab[j].col, tab[j].val = _ip(row), _ip(col), _dp(val)
        tab[j].rowout, tab[j].colout, tab[j].valout = _ip(ro), _ip(co), _dp(vo)
    _chk(lib().hipsdp_psd_project_many_large(device, count, tab, C.c_double(epsilon), mode), "hipsdp_psd_project_many_large")
    return [None if tab[j].nnz_out < 0 else (k[3][:tab[j].nnz_out], k[4][:tab[j].nnz_out], k[5][:tab[j].nnz_out])
            for j, k in enumerate(keep)]


def psd_project_many_large_stats():
    """process totals of hipsdp_psd_project_many_large: (calls, kernel launches, device->host synchronisations - one per chunk)"""
    return _stats3("hipsdp_psd_project_many_large_stats")


def syevr_many_unit(mats, cap, device=0):
    """the batched decomposition behind hipsdp_psd_project_many_large on dense host matrices of mixed sizes, 129 .. 512 rows each
    (hipsdp_syevr_many_unit of the units library), column launches of at most cap workgroups per matrix: per matrix (lam, V)"""
    mats = [np.asarray(a, dtype=np.float64) for a in mats]
    ns = np.ascontiguousarray([a.shape[0] for a in mats], dtype=np.int32)
    assert all(a.shape == (n, n) for a, n in zip(mats, ns))
    cat = _f64(np.concatenate([a.reshape(-1) for a in mats]))
    lam = np.zeros(int(ns.sum()))
    V = np.zeros(int((ns.astype(np.int64) ** 2).sum()))
    rc = ulib().hipsdp_syevr_many_unit(device, len(mats), _ip(ns), _dp(cat), int(cap), _dp(lam), _dp(V))
    if rc != 0:
        raise RuntimeError("hipsdp_syevr_many_unit: %d (%s)" % (rc, ulib().hipsdp_last_error()))
    out, lo, vo = [], 0, 0
    for n in ns:
        n = int(n)
        out.append((lam[lo:lo + n].copy(), V[vo:vo + n * n].reshape(n, n).copy()))
        lo += n
        vo += n * n
    return out
