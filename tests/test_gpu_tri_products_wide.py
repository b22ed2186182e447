"""The wide instance of the paired-band kernel (scip-sdp_amd/csrc/dgemm2.hip: hs_dgemm5_kernel<.., .., 1> - tiles of 256 in the
streamed dimension on eight wavefronts) for the two triangular n^3 products of the Schur assembly, through hipsdp_tri_product_unit
with the instance forced.

TRI = 1: T = A_stack R, A_stack (m1 n) x n, R lower triangular.   TRI = 2: W_j = G T_j, G lower triangular, a batch of T_j.
Every case three ways:
  exact   integer entries in {-2 .. 2}: every partial sum is an integer of at most 4 n <= 2000 in magnitude, far below 2^53, so both
          instances must EQUAL float64 numpy;
  random  entries in [-0.5, 0.5): the wide instance must equal the forced 128 x 128 instance bit for bit (every output element sees
          the same K positions in the same order);
  counter the hook's counters say which instance ran.
C is handed in larger than M x N and filled with a sentinel: what lies outside the result must come back untouched.

Shapes: n = 128 (one panel, whole tiles), 130 (a second panel of two columns), 257 (odd: the persistent kernels need an even K and
N - 16-byte requests -, so NO instance may take it and the forced call must still give numpy's bits through the tile kernels),
500 (the workload's n: ragged K tail inside the band); m1 = 1, 3, 5 gives rows m1 n that are no multiple of 256 (130 * 5 = 650,
257 * 3 = 771, 500 * 5 = 2500; 128 * 1 is half a wide tile, 128 * 3 one and a half) and lists far shorter than the 256 workgroups,
(2, 128) is exactly one wide tile, and (136, 130) has 70 row panels of 256, more than eight per XCD, so that several workgroups of
an XCD walk the sets and the re-ordered tail of its list."""
import numpy as np
import pytest

import schur_cases as sc

pytestmark = pytest.mark.gpu

A_LOWTRI, B_LOWTRI, REMAP = 2, 4, 16
SENTINEL = -7.25e300
NS = (128, 130, 257, 500)
TRI1 = [(m1, n) for n in NS for m1 in (1, 3, 5)] + [(136, 130), (2, 128)]
TRI2 = [(b, n) for n in NS for b in (1, 3, 9)]

_CASES = {}


def operands(tri, cnt, n):
    """(A, B, flags) of both families for one shape, and numpy's product of the exact one; made once per shape"""
    key = (tri, cnt, n)
    if key not in _CASES:
        out = {}
        for fam in ("exact", "random"):
            rng = np.random.default_rng([tri, cnt, n, fam == "exact"])
            draw = (lambda *s: rng.integers(-2, 3, s).astype(np.float64)) if fam == "exact" else (lambda *s: rng.random(s) - 0.5)
            L = np.tril(draw(n, n))
            if tri == 1:
                A, B, flags = draw(cnt * n, n), L[None], B_LOWTRI
            else:
                A, B, flags = L, draw(cnt, n, n), A_LOWTRI | REMAP
            out[fam] = (np.ascontiguousarray(A), np.ascontiguousarray(B), flags)
        A, B, _ = out["exact"]
        out["ref"] = np.stack([A @ B[j] for j in range(B.shape[0])])
        out["ref"].setflags(write=False)
        _CASES[key] = out
    return _CASES[key]


def run(gpu, ops, mode):
    """the product with the instance forced -> (results, counters); the frame of sentinels around the results is checked here"""
    A, B, flags = ops
    C, used = gpu.tri_product_unit(A, B, flags, mode, sentinel=SENTINEL, pad_rows=3, pad_cols=2)
    M, N = A.shape[0], B.shape[2]
    assert np.all(C[:, M:, :] == SENTINEL) and np.all(C[:, :, N:] == SENTINEL), "written outside M x N"
    return C[:, :M, :N], used


def check(gpu, tri, cnt, n):
    case = operands(tri, cnt, n)
    takes = n % 2 == 0                      # odd K / N: not a shape of the persistent kernels
    Cw, uw = run(gpu, case["exact"], 1)
    Cn, un = run(gpu, case["exact"], 0)
    Rw, urw = run(gpu, case["random"], 1)
    Rn, urn = run(gpu, case["random"], 0)
    print("TRI %d count %d n %d: counters wide %s narrow %s; exact: wide %s narrow %s; random: wide against narrow %s" % (
        tri, cnt, n, uw, un, np.array_equal(Cw, case["ref"]), np.array_equal(Cn, case["ref"]), np.array_equal(Rw, Rn)))
    assert uw == urw == ((1, 1) if takes else (0, 0))
    assert un == urn == ((1, 0) if takes else (0, 0))
    assert np.array_equal(Cw, case["ref"])
    assert np.array_equal(Cn, case["ref"])
    assert np.array_equal(Rw, Rn)
    assert not np.any(Rw == SENTINEL)


@pytest.mark.parametrize("m1,n", TRI1, ids=["%dx%d" % s for s in TRI1])
def test_stacked_rows_times_lower_factor(gpu, m1, n):
    check(gpu, 1, m1, n)


@pytest.mark.parametrize("batch,n", TRI2, ids=["%dx%d" % s for s in TRI2])
def test_lower_factor_times_batch(gpu, batch, n):
    check(gpu, 2, batch, n)


def test_default_dispatch_counts_its_instance(gpu):
    """unforced, the counters follow the launcher's rule: a product of 24 wide items stays on the 128 x 128 instance"""
    case = operands(1, 3, 500)
    C, used = run(gpu, case["exact"], -1)
    assert used == (0, 0)                   # 12 x 4 tiles of 128: below the size from which the persistent kernels are used at all
    assert np.array_equal(C, case["ref"])


def test_assembly_with_the_wide_instance_forced(gpu):
    """hs_schur_W at m1 = 5, n = 130 with both triangular products on the wide instance: Mx equals the 128 x 128 instance's bit for bit
    (and numpy's: the exact family of tests/harness/schur_cases.py)"""
    m1, n = 5, 130
    assert sc.exact_premise(m1, n) < 2.0 ** 53
    A, R, G, _, _ = sc.exact(m1, n)
    got = {}
    try:
        for mode in (1, 0):
            w0 = gpu.tri_instance_force(mode)
            M, used = gpu.schur_form_unit(0, A, R, G)
            got[mode] = (M, used, gpu.tri_instance_force(mode) - w0)
    finally:
        gpu.tri_instance_force(-1)
    print("used (persistent, paired band, Gram), wide products: wide", got[1][1:], "narrow", got[0][1:])
    assert got[1][1][1] == 2 and got[1][2] == 2
    assert got[0][1][1] == 2 and got[0][2] == 0
    assert np.array_equal(got[1][0], got[0][0])
    assert np.array_equal(got[1][0], sc.exact_ref(m1, n))
