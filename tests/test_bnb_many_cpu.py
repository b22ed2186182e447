"""CPU: the branch-and-bound driver with many nodes in flight (tests/harness/bnb_many.py) over the numpy oracle.  At width 1 it
visits the nodes of bnb.branch_and_bound in the same order; at widths 4 and 16 it reaches the same optima (check/testset/
short.solu).  And the C ABI and the binding carry hipsdp_solve_many / hipsdp_solve_many_stats."""
import os
import re
import pytest
import bnb
import bnb_many
import sdpa_io
from conftest import GOLDEN, ROOT

SOLU = {"example_small.dat-s": -8.0, "example_TT.dat-s.gz": 2.11803, "example_inf.dat-s": None}


def load(name):
    inst = sdpa_io.read_sdpa(os.path.join(GOLDEN, "instances", name))
    return bnb.instance_to_sdpi(inst), inst.intvars


def recording(solve_one, seq):
    def solve(P):
        seq.append((tuple(P.lb), tuple(P.ub)))
        return solve_one(P)
    return solve


@pytest.mark.parametrize("name", ["example_small.dat-s", "example_TT.dat-s.gz"])
def test_width_one_visits_the_nodes_of_bnb(name):
    prob, ints = load(name)
    seq1, seqm = [], []
    r1 = bnb.branch_and_bound(prob, ints, recording(bnb.oracle_node_solver(), seq1))
    one = recording(bnb.oracle_node_solver(), seqm)
    rm = bnb_many.branch_and_bound_many(prob, ints, lambda Ps: [one(P) for P in Ps], 1)
    assert seqm == seq1
    assert rm[0] == r1[0] and rm[2] == r1[2] and rm[3] == r1[3]
    assert abs(rm[0] - SOLU[name]) <= 1e-4 * max(1.0, abs(SOLU[name]))


@pytest.mark.parametrize("width", [4, 16])
@pytest.mark.parametrize("name", sorted(SOLU))
def test_wider_searches_reach_the_same_optima(name, width):
    prob, ints = load(name)
    calls = []

    def solve_nodes(Ps):
        calls.append(len(Ps))
        return bnb_many.oracle_node_solver()(Ps)
    best, y, nodes, failed = bnb_many.branch_and_bound_many(prob, ints, solve_nodes, width)
    assert failed == 0
    assert max(calls) <= width
    if SOLU[name] is None:
        assert best is None
    else:
        assert best is not None and abs(best - SOLU[name]) <= 1e-4 * max(1.0, abs(SOLU[name]))
        assert all(abs(y[v] - round(y[v])) <= 1e-9 for v in ints)
    if name == "example_TT.dat-s.gz":
        assert max(calls) == width          # a tree this size has that many open nodes at once


def test_solve_many_is_declared_and_bound():
    with open(os.path.join(ROOT, "include", "hipsdp.h")) as f:
        hdr = f.read()
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_solve_many\s*\(\s*int\s+count\s*,\s*hipsdp_solver\s*\*\s*const\s*\*\s*solvers\s*,"
                     r"\s*const\s+hipsdp_params\s*\*\s*params\s*,\s*hipsdp_info\s*\*\s*infos\s*,\s*int\s*\*\s*rcs\s*\)", hdr)
    assert re.search(r"HIPSDP_API\s+int\s+hipsdp_solve_many_stats\s*\(\s*long\s+long\s*\*\s*launches\s*,\s*long\s+long\s*\*\s*problems\s*\)", hdr)
    with open(os.path.join(ROOT, "include", "hipsdp_units.h")) as f:
        assert "hipsdp_solve_many" not in f.read()
    import importlib.util
    spec = importlib.util.spec_from_file_location("hipsdp_binding_many", os.path.join(ROOT, "scip-sdp_amd", "binding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert callable(mod.solve_many) and callable(mod.solve_many_stats)
