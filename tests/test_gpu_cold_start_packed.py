"""The first assembly of a cold solve from the packed lower triangles (csrc/schur.hip: hs_schur_W_identity_packed).

At the cold start X = Z = xi I the Schur matrix is the Gram matrix M_ij = <A_i, A_j> of the constraint matrices.  Every A_i is
symmetric, so with P = the packed lower triangles (the copy the sweeps use) and D[i][r] = A_i[r][r]

    M = 2 P P^T - D D^T

with K = n (n + 1) / 2 instead of n^2 in the big product.  The unit entry hipsdp_schur_identity_unit runs hs_pack_rows and the new
function (or, on request, the full-storage hs_schur_W_identity) on host matrices and reports the matrix-core flops it executed.

Bound of the products against numpy: max |diff| <= 1e-11 max |ref| over the lower triangle, the project's bound for the Gram product at
the bench shape (test_gpu_units.py::test_schur_products_at_bench_shape_against_numpy)."""
import numpy as np
import pytest

import ipm_ref
import instances

pytestmark = pytest.mark.gpu

BOUND = 1e-11
# (m1, n, ws_gbytes, the Gram kernel takes the product, what the shape exercises)
SHAPES = [(1001, 500, 0.0, True, "Gram kernel"),
          (300, 100, 0.0, False, "K below the Gram kernel's floor: tile kernel, plain split-K in slabs"),
          (200, 65, 0.0, False, "odd n: the pad entry of Lp and of D (tile kernel, plain split-K in slabs)"),
          (1101, 128, 0.01, False, "the chunked workspace of the existing small-workspace test: tile kernel, the few slabs that fit"),
          (901, 200, 0.0, False, "m1 >= 900, K = 20100 and no Gram plan: tile kernel, XCD-walked K slices in slabs"),
          (1501, 192, 0.01, False, "XCD-walked slices wanted, chunked workspace below two slabs: straight into Mx")]


def gram_kernel_has_plan(gpu, m1, K):
    import ctypes as C
    no, nd, ni, sp = C.c_int(0), C.c_int(0), C.c_int(0), C.c_double(0.0)
    return gpu.ulib().hipsdp_gram_plan_info(0, m1, C.c_longlong(K), 64, C.byref(no), C.byref(nd), C.byref(ni), C.byref(sp)) == 0


def sym_stack(m1, n, seed):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((m1, n, n))
    A += A.transpose(0, 2, 1)
    return A


def gram_ref(A):
    F = A.reshape(A.shape[0], -1)
    return F @ F.T


@pytest.mark.parametrize("m1,n,ws,gram,what", SHAPES, ids=["%dx%d" % (s[0], s[1]) for s in SHAPES])
def test_packed_first_assembly_against_numpy(gpu, m1, n, ws, gram, what):
    """2 P P^T - D D^T on a zeroed Mx against numpy's F F^T over the full rows; a second call repeats the bits; the upper triangle is
    not touched.

    Upper triangle: where the Gram kernel takes the big product (the bench shape) the summation of its partial tiles and the
    subtraction of D D^T write the lower triangle entry by entry, so EVERY entry above the diagonal keeps the caller's bits.  Where the
    tile kernels take it (hs_dgemm with HS_GEMM_LOWER) they compute every TILE that touches the lower triangle - a diagonal tile is
    written whole, exactly as the full-storage form does, and the engine mirrors the lower triangle over it afterwards.  Tiles are 64 or
    128 wide, so an entry (r, c) with c // 128 > r // 128 lies in no such tile: those keep the caller's bits on every path, and what the
    caller put into the upper triangle never reaches the lower."""
    Lp = (n * (n + 1) // 2 + 1) & ~1
    assert gram == (m1 >= 256 and Lp >= 16384 and ws == 0.0 and gram_kernel_has_plan(gpu, m1, Lp))      # the label tells the truth
    A = sym_stack(m1, n, 100 + n)
    ref = gram_ref(A)
    il = np.tril_indices(m1)
    M1, f1 = gpu.schur_identity_unit(A, ws_gbytes=ws)
    err = np.max(np.abs(M1[il] - ref[il]))
    print("%s: (m1, n) = (%d, %d): max |diff| = %.3e = %.3e max |ref|, executed %.4e flops" % (what, m1, n, err, err / np.max(np.abs(ref)), f1))
    assert err <= BOUND * np.max(np.abs(ref))
    M2, f2 = gpu.schur_identity_unit(A, ws_gbytes=ws)
    assert np.array_equal(M1[il], M2[il]) and f1 == f2
    # a sentinel in the strict upper triangle
    r, c = np.triu_indices(m1, 1)
    M0 = np.zeros((m1, m1))
    M0[r, c] = 3.25
    M3, _ = gpu.schur_identity_unit(A, Mx=M0, ws_gbytes=ws)
    assert np.array_equal(M3[il], M1[il])
    kept = np.ones(len(r), dtype=bool) if gram else c // 128 > r // 128
    assert np.all(M3[r[kept], c[kept]] == 3.25)
    assert np.all(M1[r[kept], c[kept]] == 0.0)


def test_packed_first_assembly_executes_half_the_matrix_core_flops(gpu):
    """at the bench shape the packed call executes at most 0.52 of the full-storage call's matrix-core flops (0.5 for the halved K,
    0.004 for D D^T, the rest for the even pad and the tile edges), and the two results agree to the bound of the products"""
    m1, n = 1001, 500
    A = sym_stack(m1, n, 7)
    Mp, fp = gpu.schur_identity_unit(A)
    Mf, ff = gpu.schur_identity_unit(A, full_storage=True)
    il = np.tril_indices(m1)
    err = np.max(np.abs(Mp[il] - Mf[il]))
    print("executed flops: packed %.4e, full storage %.4e, ratio %.4f; max |packed - full| = %.3e max |full|"
          % (fp, ff, fp / ff, err / np.max(np.abs(Mf[il]))))
    assert ff > 0.0 and fp <= 0.52 * ff
    assert err <= BOUND * np.max(np.abs(Mf[il]))


def test_cold_solve_takes_the_packed_first_assembly(gpu, monkeypatch):
    """planted_dense(150, 320) cold, against the same solve with HIPSDP_NO_IDENTITY_START=1 (the general products in the first iteration
    too): same iteration count, objective to 1e-11 and y to 1e-9 relative - the tolerances of
    test_gpu_ipm.py::test_first_assembly_of_a_cold_solve_is_the_gram_matrix_of_the_constraint_matrices.  That the solve took the packed
    form is read from its executed flops: the products of a general assembly depend on the shape alone, so the first assembly's flops
    are the cold solve's total minus (assemblies - 1) general ones - and they must be what the unit entry executes for the packed form
    on these matrices, not what it executes for the full storage.

    Allowance: the engine counts what is queued between the start and the end of an assembly, and in some iterations that includes the
    inverse factor of X, which is launched from a hook behind the assembly's first product (an n x n triangular inversion: at most
    2 (128 ceil(n / 128))^3 executed flops, 3.4e7 here; 2.06e6 measured in this solve).  The derived figure may therefore be off by that
    much per assembly, 2.4e8 in all, where the packed and the full-storage form differ by 1.2e9 (2.27e9 against 3.46e9: at this size the
    packed product runs on the tile kernels, which compute the diagonal tiles whole): the test requires the difference between the two
    forms to be at least four times the allowance, so it cannot pass on the full-storage path."""
    b, A, ys, Xs, Zs = instances.planted_dense(150, 320)
    core = ipm_ref.CoreProblem(b, [A])

    def solve():
        s = gpu.Solver(0)
        s.load_core(core)
        info = s.solve(gaptol=1e-6, feastol=1e-6)
        y = s.y()
        s.close()
        return info, y

    monkeypatch.delenv("HIPSDP_NO_IDENTITY_START", raising=False)
    i1, y1 = solve()
    monkeypatch.setenv("HIPSDP_NO_IDENTITY_START", "1")
    i2, y2 = solve()
    monkeypatch.delenv("HIPSDP_NO_IDENTITY_START", raising=False)
    assert i1.status == 0 and i2.status == 0
    assert i1.iterations == i2.iterations and i1.schur_calls == i2.schur_calls
    assert abs(i1.dobj - i2.dobj) <= 1e-11 * (1 + abs(i2.dobj))
    assert np.max(np.abs(y1 - y2)) <= 1e-9 * (1 + np.max(np.abs(y2)))
    assert i1.schur_flops_executed < i2.schur_flops_executed
    general = i2.schur_flops_executed / i2.schur_calls
    first = i1.schur_flops_executed - (i1.schur_calls - 1) * general
    _, fp = gpu.schur_identity_unit(A)
    _, ff = gpu.schur_identity_unit(A, full_storage=True)
    print("first assembly %.6e flops; unit entry: packed %.6e, full storage %.6e; a general assembly %.6e" % (first, fp, ff, general))
    allowance = i1.schur_calls * 2.0 * (128.0 * ((150 + 127) // 128)) ** 3
    assert ff - fp >= 4.0 * allowance
    assert abs(first - fp) <= allowance
