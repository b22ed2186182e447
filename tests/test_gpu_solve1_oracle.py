"""GPU: the one-launch node solve (csrc/solve1_body.h) at the edges of its admission rule, against the oracle.  The shapes are chosen
from the rule itself (hs_solve1_fits through the units library's hipsdp_solve1_fits): for every combination of block count, variables
and LP rows, the largest block that fits and one row more.  Among them: single blocks of 33 to 49 rows (step lengths through s1_lmin),
shapes whose lists spill to the global workspace, every size class (c10, c16, c64, c64m), light and heavy matrices, dense and diagonal
constant matrices, and heavy shapes on both sides of the kernel's work estimate.

The kernel's own verdict is compared (HIPSDP_SOLVE1_NO_FALLBACK=1): on admitted shapes it must be the oracle's status with the oracle's
iteration count and history, an objective to 1e-6, an optimality certificate of its own y, X and x, and the same bits on a second
solve; declined shapes are served by the general path, which must meet the same checks."""
import numpy as np
import pytest
from threadpoolctl import threadpool_limits

import checker
import ipm_ref
import solve1_shapes
from test_gpu_solve1 import assert_history_matches, solve_one_launch
import test_gpu_solve_many as tsm

pytestmark = pytest.mark.gpu
TOL = dict(gaptol=1e-6, feastol=1e-6, pabstol=1e-5)


# (id, blocks, m, q, what is pushed to the edge: "n" the block size, "q" the LP rows at a fixed block size; keywords of
# solve1_shapes.planted; HIPSDP_SOLVE1_MAXM).  Every entry gives two shapes: the largest admitted and one more row (or one more LP row).
EDGES = [
    ("k1_m1",        1,   1,   0, ("n", None), dict(kinds="light3", const="dense"), None),                 # 49 rows
    ("k1_m64_l24",   1,  64,   0, ("n", None), dict(kinds="light24", const="diag"), None),                 # 41
    ("k1_m64_q200",  1,  64, 200, ("n", None), dict(kinds="light3", const="dense", lp="dens"), None),      # 38
    ("k1_m65",       1,  65,   0, ("n", None), dict(kinds="light3", const="diag"), None),                  # 44 (packed M)
    ("k1_m108",      1, 108,   0, ("n", None), dict(kinds="light3", const="dense"), None),                 # 37
    ("k1_m108_q60",  1, 108,  60, ("n", None), dict(kinds="light3", heavy=2, const="dense"), None),        # heavy matrices
    ("k1_m128",      1, 128,   0, ("n", None), dict(kinds="light3", const="dense"), "128"),                # 32
    ("k2_m1",        2,   1,   0, ("n", None), dict(kinds="light3", const="diag"), None),                  # 34
    ("k2_m64_q60",   2,  64,  60, ("n", None), dict(kinds="light3", heavy=3, const="dense"), None),
    ("k2_m108",      2, 108,   0, ("n", None), dict(kinds="light3", const="dense"), None),                 # 25
    ("k8_m1",        8,   1,   0, ("n", None), dict(kinds="light3", const="dense"), None),                 # 16: class c16
    ("k8_m64",       8,  64,   0, ("n", None), dict(kinds="light3", const="diag"), None),                  # 13: class c16
    ("k8_m108_q40",  8, 108,  40, ("n", None), dict(kinds="light3", const="dense"), None),
    ("k1_m64_n16_q", 1,  64, None, ("q", 16), dict(kinds="light3", const="dense", lp="bounds"), None),     # LP rows to the LDS limit
    ("k1_m108_n8_q", 1, 108, None, ("q", 8), dict(kinds="light3", const="diag", lp="bounds"), None),
]


def edge_shape(hb, nblk, m, q, edge):
    """(sizes, q) of the largest admitted shape of the combination"""
    what, fixed = edge
    if what == "n":
        n = max([n for n in range(1, 65) if hb.solve1_fits(m, q, [n] * nblk)])
        return [n] * nblk, q
    qs = [t for t in range(0, 4097) if hb.solve1_fits(m, t, [fixed] * nblk)]
    return [fixed] * nblk, max(qs)


def edge_core(hb, nblk, m, q, edge, kw, side):
    """(sizes, q, problem) of the largest admitted shape of the combination (side 0) or of one row / LP row more (side 1)"""
    sizes, q = edge_shape(hb, nblk, m, q, edge)
    if side:
        if edge[0] == "n":
            sizes = [n + 1 for n in sizes]
        else:
            q += 1
    return sizes, q, solve1_shapes.planted(sizes, m, q, 7100 + 10 * nblk + m + side, **kw)


def inside_core(sizes, m, q, kw):
    return solve1_shapes.planted(sizes, m, q, 7300 + m + q, **kw)


def cases():
    out = []
    for name, nblk, m, q, edge, kw, maxm in EDGES:
        for side in (0, 1):
            out.append(pytest.param(nblk, m, q, edge, kw, maxm, side, id="%s_%s" % (name, "max" if side == 0 else "over")))
    return out


# inside the region, away from the LDS edge: the small classes, light24 matrices, heavy matrices at about half and twice the work the
# kernel takes (schur_work), and light24 matrices at m = 108 whose pair lists alone cost more than that
INSIDE = [
    ("c10_k8",        [10] * 8, 64, 100, dict(kinds="light3", const="diag")),
    ("c10_k1_m1",     [10], 1, 0, dict(kinds="light3", const="dense")),
    ("c16_k2_l24",    [16, 16], 40, 200, dict(kinds="light24", const="dense")),
    ("c64m_k3",       [20, 9, 24], 90, 80, dict(kinds="light3", const="diag")),
    ("c64m_k1_n33",   [33], 108, 200, dict(kinds="light3", const="dense")),          # the smallest block of s1_lmin
]
# heavy shapes at about 0.5x and 2x the work the kernel takes.  2x needs nearly n^3 m = 6e6: one block of 36 or 37 rows at m = 108
# (every matrix heavy: 1.9x and 2.0x); two blocks of 24 rows reach 1.4x at most, so that shape is only taken at 0.5x
WORK = [
    ("heavy_k1_n37",      [37], 108, 0, 0.5),
    ("heavy_k1_n37",      [37], 108, 0, 2.0),
    ("heavy_k1_n36_q60",  [36], 108, 60, 0.5),
    ("heavy_k1_n36_q60",  [36], 108, 60, 2.0),
    ("heavy_k2_n24",      [24, 24], 100, 0, 0.5),
]


def heavy_to_work(sizes, m, q, ratio, seed):
    """the planted problem whose number of heavy matrices puts the kernel's work estimate closest to ratio * maxwork"""
    best = None
    for h in range(0, m + 1):
        core = solve1_shapes.planted(sizes, m, q, seed, kinds="light3", heavy=h)
        w = solve1_shapes.schur_work(core)
        if best is None or abs(np.log(w / (ratio * solve1_shapes.MAXWORK))) < abs(np.log(best[1] / (ratio * solve1_shapes.MAXWORK))):
            best = (core, w, h)
        if w > ratio * solve1_shapes.MAXWORK:
            break
    return best


def predicted_path(hb, core, maxm):
    """what the admission rule, the work estimate and the LP cost say: 1 the kernel, 0 declined"""
    ns = [A.shape[1] for A in core.blocks]
    if core.m > maxm or max(ns) > 64 or not hb.solve1_fits(core.m, core.q, ns):
        return 0
    if solve1_shapes.schur_work(core) > solve1_shapes.MAXWORK:
        return 0
    lo, hi = solve1_shapes.lp_cost_bounds(core)
    assert not (lo <= solve1_shapes.LP_COST_MAX < hi), "a shape on the fence of the LP cost model: pick another"
    return 1 if hi <= solve1_shapes.LP_COST_MAX else 0


def oracle(core):
    """(on one BLAS thread, as test_gpu_solve1.oracle_solve: a verdict that does not follow the host's thread count)"""
    with threadpool_limits(limits=1):
        return ipm_ref.hsd_solve(core, ipm_ref.Params(**TOL))


def assert_certified(core, ref, res, tag):
    info = res["info"]
    assert info.status == ref.status == 0, tag
    assert info.iterations == ref.iterations, tag
    assert abs(info.dobj - ref.dobj) <= 1e-6 * (1 + abs(ref.dobj)), (tag, info.dobj, ref.dobj)
    x = res["lp"][0] if core.q else np.zeros(0)
    ok, det = checker.certificate(core, res["y"], res["X"], x, 1e-5 * (1 + abs(ref.dobj)), 1e-5)
    assert ok, (tag, det)


def general_full(hb, core, monkeypatch):
    monkeypatch.setenv("HIPSDP_SOLVE1", "0")
    s = hb.Solver(0)
    s.load_core(core)
    info = s.solve(**TOL)
    out = dict(info=info, path=s.solve_path(), y=s.y(), X=[s.X(k) for k in range(len(core.blocks))], lp=s.lp())
    s.close()
    return out


def check_shape(hb, core, maxm, tag, monkeypatch):
    """the kernel's own verdict on an admitted shape, the general path's on a declined one - both against the oracle"""
    want = predicted_path(hb, core, maxm)
    ref = oracle(core)
    monkeypatch.setenv("HIPSDP_SOLVE1_NO_FALLBACK", "1")
    g = solve_one_launch(hb, core, monkeypatch, **TOL)
    tag = "%s path %d (predicted %d) status %d oracle %d; gave up at solve1_body.h:%d" % (
        tag, g["path"], want, g["info"].status, ref.status, int(g["trace"][44]) if g["path"] else 0)
    assert g["path"] == want, tag
    if want:
        assert_certified(core, ref, g, tag)
        assert_history_matches(g, ref)
        g2 = solve_one_launch(hb, core, monkeypatch, **TOL)
        assert g2["path"] == 1 and g2["info"].iterations == g["info"].iterations and g2["info"].dobj == g["info"].dobj, tag
        assert np.array_equal(g2["y"], g["y"]), tag
        for a, b in zip(g2["X"], g["X"]):
            assert np.array_equal(a, b), tag
        if core.q:
            assert np.array_equal(g2["lp"][0], g["lp"][0]), tag
    else:
        assert_certified(core, ref, general_full(hb, core, monkeypatch), tag)
    return g


@pytest.mark.parametrize("nblk,m,q,edge,kw,maxm,side", cases())
def test_admission_edge_against_the_oracle(gpu, nblk, m, q, edge, kw, maxm, side, monkeypatch):
    if maxm is not None:
        monkeypatch.setenv("HIPSDP_SOLVE1_MAXM", maxm)
    sizes, q, core = edge_core(gpu, nblk, m, q, edge, kw, side)
    tag = "sizes %s m %d q %d %s" % (sizes, m, q, kw)
    fits = gpu.solve1_fits(m, q, sizes)
    assert fits == (side == 0), tag                       # the edge is the rule's edge
    g = check_shape(gpu, core, int(maxm or 108), tag, monkeypatch)
    if side == 0 and edge[0] == "n" and sizes[0] > 32:
        assert g["path"] == 1, tag                         # blocks of more than 32 rows: s1_lmin in the kernel


def test_the_edges_include_every_row_count_of_s1_lmin(gpu):
    """single blocks of 33, 36 or 37, 41 and 49 rows are among the admitted shapes (the edges and the shapes inside the region)"""
    got = set()
    for name, nblk, m, q, edge, kw, maxm in EDGES:
        if nblk == 1 and edge[0] == "n":
            got.add(edge_shape(gpu, nblk, m, q, edge)[0][0])
    got |= {c[1][0] for c in INSIDE if len(c[1]) == 1}
    assert {33, 41, 49} <= got and (36 in got or 37 in got), got
    assert max(got) == 49


@pytest.mark.parametrize("name,sizes,m,q,kw", INSIDE, ids=[c[0] for c in INSIDE])
def test_inside_the_region_against_the_oracle(gpu, name, sizes, m, q, kw, monkeypatch):
    core = inside_core(sizes, m, q, kw)
    g = check_shape(gpu, core, 108, "%s sizes %s m %d q %d" % (name, sizes, m, q), monkeypatch)
    assert g["path"] == 1


@pytest.mark.parametrize("name,sizes,m,q,ratio", WORK, ids=["%s_x%.1f" % (c[0], c[4]) for c in WORK])
def test_work_estimate_decides_both_ways(gpu, name, sizes, m, q, ratio, monkeypatch):
    """heavy matrices at about 0.5x and 2x the kernel's work limit: the first shape runs in the kernel, the second is declined"""
    core, w, h = heavy_to_work(sizes, m, q, ratio, 7400 + m)
    assert 0.8 < w / solve1_shapes.MAXWORK / ratio < 1.25, (w, h)            # (the shape is what its name says)
    assert gpu.solve1_fits(m, q, sizes)
    g = check_shape(gpu, core, 108, "%s sizes %s m %d q %d heavy %d work %.3g" % (name, sizes, m, q, h, w), monkeypatch)
    assert g["path"] == (1 if ratio < 1 else 0)


def test_light_lists_beyond_the_work_limit_are_declined(gpu, monkeypatch):
    """108 matrices of 24 entries each: no heavy variable, but the pair formula alone (0.75 (nz - nzh)^2) is above the limit"""
    core = solve1_shapes.planted([30], 108, 0, 7500, kinds="light24", const="dense")
    assert solve1_shapes.schur_work(core) > solve1_shapes.MAXWORK
    g = check_shape(gpu, core, 108, "light24 m 108", monkeypatch)
    assert g["path"] == 0


def test_lists_in_global_memory_are_exercised(gpu, monkeypatch):
    """out[45] of the kernel's trace is 1 when every list found room in LDS and 0 when some went to the global workspace.  The
    49-row edge shape (k1_m1) spills and the 10-row shape c10_k1_m1 does not: the same problems as in their tests above, and both
    certified against the oracle here as well"""
    name, nblk, m, q, edge, kw, maxm = EDGES[0]
    sizes, q, spill = edge_core(gpu, nblk, m, q, edge, kw, 0)
    assert name == "k1_m1" and sizes == [49]
    name, sizes, m, q, kw = INSIDE[1]
    assert name == "c10_k1_m1"
    small = inside_core(sizes, m, q, kw)
    gs = check_shape(gpu, spill, 108, "k1_m1 edge", monkeypatch)
    gm = check_shape(gpu, small, 108, "c10_k1_m1", monkeypatch)
    assert gs["path"] == 1 and gm["path"] == 1
    assert gs["trace"][45] == 0 and gm["trace"][45] == 1


INFEASIBLE = [
    ("dinf_k1_n41", [41], 64, 20, "dinf"),
    ("dinf_k8_n10", [10] * 8, 64, 50, "dinf"),
    ("dunb_k1_n37", [37], 108, 0, "dunb"),
    ("dunb_k2_n16", [16, 16], 40, 10, "dunb"),
]


@pytest.mark.parametrize("name,sizes,m,q,kind", INFEASIBLE, ids=[c[0] for c in INFEASIBLE])
def test_infeasible_shapes_against_the_oracle(gpu, name, sizes, m, q, kind, monkeypatch):
    """the kernel's infeasibility verdict is the oracle's, and its own X, x (X-ray) or y (y-ray) proves it"""
    core = solve1_shapes.planted(sizes, m, q, 7600 + m, kinds="light3", infeasible=kind)
    ref = oracle(core)
    want = ipm_ref.STATUS_DINF if kind == "dinf" else ipm_ref.STATUS_DUNB
    assert ref.status == want, (name, ref.status)
    monkeypatch.setenv("HIPSDP_SOLVE1_NO_FALLBACK", "1")
    g = solve_one_launch(gpu, core, monkeypatch, **TOL)
    tag = "%s path %d status %d oracle %d" % (name, g["path"], g["info"].status, ref.status)
    assert g["path"] == 1, tag
    assert g["info"].status == ref.status, tag
    if kind == "dinf":
        x = g["lp"][0] if core.q else np.zeros(0)
        ok, det = checker.farkas_dual_infeasible(core, g["X"], x, 1e-6)
    else:
        ok, det = checker.farkas_dual_unbounded(core, g["y"], 1e-6)
    assert ok, (tag, det)


def test_edge_shapes_in_one_solve_many_call(gpu, monkeypatch):
    """the admitted edge shapes (but the one that needs HIPSDP_SOLVE1_MAXM) in one hipsdp_solve_many call: every problem ends with
    the bits hipsdp_solve alone gives it, the classes served are the rule's, one launch per class"""
    for v in ("HIPSDP_SOLVE1", "HIPSDP_SOLVE1_NO_FALLBACK", "HIPSDP_SOLVE1_HIST", "HIPSDP_SOLVE1_MAXM"):
        monkeypatch.delenv(v, raising=False)
    specs, tags, classes = [], [], []
    for name, nblk, m, q, edge, kw, maxm in EDGES:
        if maxm is not None:
            continue
        sizes, qq, core = edge_core(gpu, nblk, m, q, edge, kw, 0)
        specs.append(dict(core=core))
        tags.append(name)
        classes.append(gpu.solve1_class(m, sizes))
    for name, sizes, m, q, kw in INSIDE:
        specs.append(dict(core=inside_core(sizes, m, q, kw)))
        tags.append(name)
        classes.append(gpu.solve1_class(m, sizes))
    params = [TOL] * len(specs)
    ref, dref = tsm.solo(gpu, specs, params)
    l0, p0 = gpu.solve_many_stats()
    got, dgot = tsm.many(gpu, specs, params)
    l1, p1 = gpu.solve_many_stats()
    tsm.assert_same(got, ref, tags)
    assert np.array_equal(dgot, dref)
    served = {c for c, r in zip(classes, ref) if r["path"] == 1}
    assert all(r["path"] == 1 for r in ref), [t for t, r in zip(tags, ref) if r["path"] != 1]
    assert served == {10, 16, 64, 1064}
    assert [tsm.size_class(sp["core"]) for sp in specs] == classes          # problem by problem
    assert l1 - l0 == len(served) and p1 - p0 == len(specs)
