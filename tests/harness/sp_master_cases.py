"""Instances and nodes for the tests of the master copy kept as triplets (tests/test_gpu_sparse_master.py, tests/devtools/
sparse_master_rate.py).  A master block is a list of per-slot triplet arrays (rows, cols, vals) in ORIGINAL indices, as a caller
hands them over (any triangle, repeated positions allowed: the later one counts).  A node names the slot of each active variable
(-1: the variable does not appear in the block), the kept rows in increasing order and the number m of variables of the engine."""
import numpy as np


class Node:
    def __init__(self, name, act, kept, m=None):
        self.name, self.act, self.kept = name, [int(a) for a in act], [int(r) for r in kept]
        self.m = len(self.act) if m is None else m


def marshal(slots, N, node):
    """the triplets the direct load hands hipsdp_add_entries for this node: active variables a + 1 in the order of a, each slot's
    entries in the caller's order, rows renumbered through kept, entries touching a removed row dropped"""
    inv = -np.ones(N, dtype=np.int64)
    inv[node.kept] = np.arange(len(node.kept))
    var, row, col, val = [], [], [], []
    for a, k in enumerate(node.act):
        if k < 0:
            continue
        r, c, v = slots[k]
        r2, c2 = inv[np.asarray(r, dtype=np.int64)], inv[np.asarray(c, dtype=np.int64)]
        keep = (r2 >= 0) & (c2 >= 0)
        var.append(np.full(int(keep.sum()), a + 1)); row.append(r2[keep]); col.append(c2[keep]); val.append(np.asarray(v, dtype=float)[keep])
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dtype=dt)
    return cat(var, np.int32), cat(row, np.int32), cat(col, np.int32), cat(val, np.float64)


def once_per_position(slots):
    """the same matrices with every position named once, in the lower triangle (the later entry of a repeated position stays)"""
    out = []
    for r, c, v in slots:
        ent = {}
        for ri, ci, vi in zip(r, c, v):
            ent[(max(int(ri), int(ci)), min(int(ri), int(ci)))] = float(vi)
        out.append(([k[0] for k in ent], [k[1] for k in ent], list(ent.values())))
    return out


def shape_a():
    """N = 12, 6 slots: slot 1 dense (78 lower entries: the ballot compaction crosses a wavefront), slot 2 sits entirely on rows 0,
    5 and 11, slot 3 on the diagonal, slot 4 is given partly in the upper triangle with repeated positions, all share (7, 3)"""
    N = 12
    rng = np.random.default_rng(12)
    il = np.tril_indices(N)
    slots = [None] * 6
    slots[0] = ([7, 2, 9, 4, 10], [3, 2, 1, 0, 10], rng.standard_normal(5))
    perm = rng.permutation(78)
    slots[1] = (il[0][perm], il[1][perm], rng.standard_normal(78))
    slots[2] = ([11, 0, 11, 5, 5, 7], [0, 0, 11, 5, 2, 5], rng.standard_normal(6))
    slots[3] = ([1, 4, 6, 11, 0], [1, 4, 6, 11, 0], rng.standard_normal(5))
    slots[4] = ([3, 8, 3, 7, 2, 8, 6], [7, 1, 7, 3, 9, 1, 6], rng.standard_normal(7))          # (7, 3) three times, (8, 1) twice, (9, 2) upper
    slots[5] = ([7, 10, 6], [3, 9, 2], rng.standard_normal(3))
    slots[2] = (list(slots[2][0]) + [3], list(slots[2][1]) + [0], np.append(slots[2][2], 0.5))        # (3, 0): on column 0
    allrows = list(range(N))
    cut = [r for r in allrows if r not in (0, 5, 11)]
    nodes = [Node("all", range(6), allrows),
             Node("rows-0-5-11-removed", range(6), cut),
             Node("absent-variables", [0, -1, 1, 2, -1, 5], allrows),
             Node("inactive-slot-in-the-middle", [0, 1, 3, 4, 5], [r for r in allrows if r != 11]),
             Node("trailing-empty-variables", [1, 4], [r for r in allrows if r != 3], m=6),
             Node("nothing-kept", [-1, -1], allrows, m=3),
             Node("slot-order-not-monotone", [4, 1, 5, 0, 3], [r for r in allrows if r != 11]),
             Node("not-monotone-and-rows-removed", [5, 2, -1, 1, 0], cut, m=7)]
    return N, slots, nodes


def _random_slots(N, S, per, npool, seed):
    """S slots of `per` distinct lower positions each, drawn from a pool of npool positions (so that slots share positions)"""
    rng = np.random.default_rng(seed)
    il = np.tril_indices(N)
    pool = rng.choice(len(il[0]), size=min(npool, len(il[0])), replace=False)
    slots = []
    for _ in range(S):
        pick = rng.choice(pool, size=per, replace=False)
        slots.append((il[0][pick].astype(np.int32), il[1][pick].astype(np.int32), rng.standard_normal(per)))
    return slots


def shape_b():
    """N = 40, 64 slots of 40 entries (2560 > 2048) on a pool of 500 positions: about five variables per position"""
    N, S = 40, 64
    slots = _random_slots(N, S, 40, 500, 40)
    rng = np.random.default_rng(41)
    cut = sorted(rng.choice(N, size=31, replace=False).tolist())
    perm = rng.permutation(S)[:50].tolist()
    nodes = [Node("all", range(S), range(N)),
             Node("permuted-subset-rows-removed", perm + [-1, -1], cut, m=60)]
    return N, slots, nodes


def shape_wide():
    """N = 64, 1100 slots of 3 entries on all 2080 positions: more variables and more positions than one workgroup of a scan takes
    (1024), so the block sums and their offsets are used for every list"""
    N, S = 64, 1100
    slots = _random_slots(N, S, 3, 2080, 64)
    rng = np.random.default_rng(65)
    act = rng.permutation(S)[:1060].tolist()
    nodes = [Node("all", range(S), range(N)),
             Node("permuted-subset-rows-removed", act, [r for r in range(N) if r % 9 != 4], m=1070)]
    return N, slots, nodes


def shape_long():
    """N = 760, 20 slots that share out all 289 180 lower positions (position p to slot p mod 20): more than 256 workgroups of a scan
    over the positions (262 144 entries), so the scan of the block sums itself runs in a second round with a carry"""
    N, S = 760, 20
    rng = np.random.default_rng(76)
    il = np.tril_indices(N)
    slots = [(il[0][k::S].astype(np.int32), il[1][k::S].astype(np.int32), rng.standard_normal(len(il[0][k::S]))) for k in range(S)]
    nodes = [Node("one-row-removed", list(range(S - 1, -1, -1)), [r for r in range(N) if r != 400])]
    return N, slots, nodes
