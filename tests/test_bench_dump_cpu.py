"""bench.py --dump-outputs without a GPU: what the last timed solve returned is written as float64 .npy files, whole below the size
cap and as the same seeded sample of entries above it, at most 64 MB in all."""
import importlib.util
import os
import types
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Solver:
    def __init__(self, n, m):
        rng = np.random.default_rng(n + m)
        self._y, self._X, self._Z = rng.standard_normal(m), rng.standard_normal((n, n)), rng.standard_normal((n, n))

    def y(self):
        return self._y

    def X(self, k):
        return self._X

    def Z(self, k):
        return self._Z


def _info():
    return types.SimpleNamespace(status=0, iterations=7, pobj=1.5, dobj=1.25, pinf=1e-9, dinf=0.0, dabs=2e-9, gap=3e-7, mu=1e-8,
                                 tau=1.0, kappa=1e-10)


def test_small_outputs_are_written_whole(tmp_path):
    b = _bench()
    s = _Solver(30, 40)
    b.dump_outputs(str(tmp_path), s, _info())
    assert sorted(os.listdir(str(tmp_path))) == ["X.npy", "Z.npy", "info.npy", "y.npy"]
    for name, ref in (("y", s.y()), ("X", s.X(0)), ("Z", s.Z(0))):
        a = np.load(str(tmp_path / (name + ".npy")))
        assert a.dtype == np.float64 and np.array_equal(a, ref)
    assert np.array_equal(np.load(str(tmp_path / "info.npy")), [0, 7, 1.5, 1.25, 1e-9, 0.0, 2e-9, 3e-7, 1e-8, 1.0, 1e-10])


def test_large_outputs_are_the_same_seeded_sample_within_64_mb(tmp_path):
    b = _bench()
    n = 1500                                            # n^2 above the per-array cap
    assert n * n > b.DUMP_MAX_ENTRIES
    s = _Solver(n, 3000)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), s, _info())
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["X_sample.npy", "Z_sample.npy", "info.npy", "y.npy"]
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= 64 * 2 ** 20
    for f in files:
        a, c = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype == np.float64 and np.array_equal(a, c)
    x = np.load(str(tmp_path / "a" / "X_sample.npy"))
    assert x.size == b.DUMP_MAX_ENTRIES and np.all(np.isin(x, s.X(0)))
