/* hipsdp_units.h - TEST / BENCH entry points around single device kernels (csrc/units.hip), exported by lib/libhipsdp_units.so - a
 * library of its own that holds the engine's objects plus these entries.  The product library libhipsdp.so does not contain them
 * (include/hipsdp.h is the product's C ABI).  Used by tests/, tests/devtools/ and bench.py (measured matrix peak) only. */
#ifndef HIPSDP_UNITS_H
#define HIPSDP_UNITS_H

#include "hipsdp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* both GEMM kernels (one tile per workgroup; persistent with LDS-DMA staging) on the same device-generated operands:
 * used_v2 = 1 when the persistent kernel accepts the shape, ndiff = elements of C that differ in any bit (must be 0) */
HIPSDP_API int  hipsdp_dgemm_selfcheck(int device, int M, int N, int K, int layB, int batch, int splitk, int flags, double beta,
   int* used_v2, long long* ndiff);
/* the same with a free alpha and, for reps > 0 and beta = 0, the average milliseconds of one product through the tile kernel alone
 * (ms_tile) and through the default dispatch (ms_fast).  *used: bit 0 the persistent tile kernel took the product, bit 1 the strip
 * kernel of the two triangular Schur products (alpha = 1, beta = 0 only) */
/* unit entry: out[e] = sum_i coef[i] A[i][e] + sa add[e] over R rows of E entries (the pass A^T); split = 1: as the engine calls it
 * (row chunks side by side when the block has few entries; *chunks = how many, 0 = the plain kernel) */
HIPSDP_API int  hipsdp_pass_at_unit(int device, int R, long long E, const double* A, const double* coef, double sa, const double* add, int split,
   double* out, int* chunks);
HIPSDP_API int  hipsdp_dgemm_selfcheck2(int device, int M, int N, int K, int layB, int batch, int splitk, int flags, double alpha, double beta,
   int reps, int* used, long long* ndiff, double* ms_tile, double* ms_fast);
HIPSDP_API int  hipsdp_gram_plan_info(int device, int M, long long K, int nslab, int* no, int* nd, int* nitems, double* span);
/* Gram product W W^T (lower triangle) through the K-sliced tile kernels and through the Gram kernel of csrc/gram.hip */
HIPSDP_API int  hipsdp_gram_selfcheck(int device, int M, long long K, int reps, int* used, double* maxdiff, long long* nrepro, double* ms_tile,
   double* ms_gram);
/* the same, also returning the largest absolute difference of the two results and the number of elements that differ between
 * TWO runs of the default dispatch (must be 0) */
HIPSDP_API int  hipsdp_dgemm_selfcheck3(int device, int M, int N, int K, int layB, int batch, int splitk, int flags, double alpha, double beta,
   int reps, int* used, long long* ndiff, double* maxdiff, long long* nrepro, double* ms_tile, double* ms_fast);
/* one product with a triangular operand (flags: HS_GEMM_A_LOWTRI / HS_GEMM_B_LOWTRI) from the caller's operands with the instance of
 * the paired-band kernel forced (mode 0: 128 x 128, 1: 256 in the streamed dimension, -1: default dispatch).  A [M][K], B [batch][K][N]
 * (layB = 1) or [batch][N][K] (0), C [batch][crows][ldc] in and out (crows >= M, ldc >= N); used[2]: products taken by the paired-band
 * kernel, of these by its wide instance */
HIPSDP_API int  hipsdp_tri_product_unit(int device, int mode, int M, int N, int K, int layB, int batch, int flags, const double* A,
   const double* B, double* Cio, int crows, int ldc, int* used);
/* the same choice for products reached through other entries (hipsdp_schur_form_unit); returns the wide instance's products so far */
HIPSDP_API int  hipsdp_tri_instance_force(int mode);
/* one Gram product from the caller's operands with the instance of the Gram kernel (csrc/gram.hip) forced (mode 0: 128 x 128 tiles, 1:
 * 256 x 256 on eight wavefronts, -1: chosen per shape): W [M][ldw], ldw >= K; Cio [M][M] in and out, lower triangle = alpha W W^T +
 * beta Cio; nslab (1 .. 64) slabs of M x M doubles granted; used[2]: the Gram kernel took the product, and its wide instance did */
HIPSDP_API int  hipsdp_gram_product_unit(int device, int mode, int M, long long K, const double* W, long long ldw, double alpha, double beta,
   double* Cio, int nslab, int* used);
/* the same choice for products reached through other entries (hipsdp_schur_form_unit, hipsdp_schur_identity_unit,
 * hipsdp_gram_selfcheck); returns the wide instance's products so far */
HIPSDP_API int  hipsdp_gram_instance_force(int mode);
/* host only: the plan of one instance for a shape.  info[4] = items, lists (512 / 256), partial tiles per off-diagonal / diagonal tile;
 * off[lists + 1]; the first cap items as six ints each (ti, tj, k0, k1, slab, column half).  HIPSDP_ERR_ARG when the instance has no plan */
HIPSDP_API int  hipsdp_gram_plan_unit(int inst, int forced, int M, long long K, int nslab, int cap, int* items, int* off, int* info);
/* first assembly of a cold solve: Mx += <A_i, A_j> on the lower tiles, from the packed lower triangles (full_storage = 0) or from the
 * full rows (1); *flops: FP64 matrix-core flops executed by the call */
HIPSDP_API int  hipsdp_schur_identity_unit(int device, int m1, int n, const double* A, double ws_gbytes, int full_storage, double* Mx,
   double* flops);
/* Schur block Mx[(m1) x (m1)] = tr(A_i X A_j Zinv) for i, j = 0..m1-1 */
HIPSDP_API int  hipsdp_schur_dense(int device, int m1, int n, const double* A, const double* X, const double* Zinv, double* Mx,
   double ws_gbytes);
/* the same matrix through the W formulation (W_j = G A_j R, Mx = W W^T); takes X and Z, factors them on the device */
HIPSDP_API int  hipsdp_schur_w(int device, int m1, int n, const double* A, const double* X, const double* Z, double* Mx);
/* one dense block through ONE form of the assembly from the caller's operands, all parts of a sharded form added up on this device:
 * form 0 hs_schur_W            P = R, Q = G  (lower triangular, upper triangle zero: X = R R^T, Z^-1 = G^T G; nothing is factored here)
 *      1 hs_schur_Wcols        P = R, Q = G; the `parts` slices of hs_shard_cols one behind the other into the same Mx
 *      2 hs_schur_Urows        P = X, Q = Zinv; the 2 * parts chunks of hs_shard_rows, then hs_mirror_upper
 *      3 hs_schur_U            P = X, Q = Zinv; ws_gbytes > 0 chunks it as hipsdp_schur_dense does
 *      4 hs_schur_Wvar         P = R, Q = G; null communicator of ONE rank, column slices of `parts` columns
 * Mx: m1 x m1, both triangles.  used[3] (may be NULL): products of this call taken by the persistent kernels of dgemm2.hip, of these
 * by the paired-band kernel, and Gram products taken by gram.hip.  parts: 1 .. 64 (forms 1, 2), >= 1 (form 4), ignored otherwise;
 * anything else HIPSDP_ERR_ARG before the first launch */
HIPSDP_API int  hipsdp_schur_form_unit(int device, int form, int parts, int m1, int n, const double* A, const double* P, const double* Q,
   double ws_gbytes, double* Mx, int* used);
/* hs_schur_small alone: nblk <= 8 blocks of ns[k] <= 48 rows (A[k]: m1 matrices of ns[k] x ns[k]), q LP rows (Dext[q][m1], x[q], z[q];
 * q = 0: NULL).  *taken = its return value (0: shape not admitted, nothing written: Mx, Lm, diagM come back as they were passed in);
 * Mx m1 x m1, Lm (m1-1) x (m1-1), diagM[m1-1] */
HIPSDP_API int  hipsdp_schur_small_unit(int device, int m1, int nblk, const int* ns, const double* const* A, const double* const* X,
   const double* const* Zinv, int q, const double* Dext, const double* x, const double* z, double* Mx, double* Lm, double* diagM, int* taken);
/* milliseconds one rank of an nranks-way sharded assembly spends on its share of the Schur matrix (by_columns: column slices
 * of the W formulation, else row chunks of the U formulation); synthetic operands made in HBM */
HIPSDP_API int  hipsdp_schur_shard_time(int device, int m1, int n, int nranks, int rank, int by_columns, int reps, double ws_gbytes, double* ms);
/* the same for one rank of the variable-sharded assembly (hipsdp_shard_matrices): only that rank's rows of A are allocated, the
 * column slices are cw wide, the all-to-all keeps the rank's own piece; *a2a_bytes = bytes the rank would send per assembly */
HIPSDP_API int  hipsdp_schur_var_share_time(int device, int m1, int n, int nranks, int rank, int cw, int reps, double* ms, double* a2a_bytes);
/* sparse block mode: Schur entries of matrices given as triplets (var 1 .. m; either triangle, the last of several entries with the
 * same (var, row, col) counts) exactly as the engine assembles them (csrc/sparse.hip); Mx (m + 1) x (m + 1), lower triangle of
 * rows / columns 1 .. m */
HIPSDP_API int  hipsdp_schur_sparse_unit(int device, int n, int m, long long nnz, const int* var, const int* row, const int* col,
   const double* val, const double* X, const double* Zinv, double* Mx);
/* the same with the kernel chosen by the caller: kernel = -1 the engine's rule (fewer than 24 full entries per matrix on average: one
 * thread per pair), 0 forces k_sp_schur_t (one thread per pair), 1 forces k_sp_schur (one wavefront per pair); *took (may be NULL):
 * the kernel that ran, 0 or 1 */
HIPSDP_API int  hipsdp_schur_sparse_unit2(int device, int n, int m, long long nnz, const int* var, const int* row, const int* col,
   const double* val, const double* X, const double* Zinv, double* Mx, int kernel, int* took);
/* the two passes over a block kept as nonzeros, on the structure built from the caller's triplets: outA[m] = <A_v, V>, v = 1 .. m
 * (hs_sp_apply_A; V[n][n] need not be symmetric, both V[r][c] and V[c][r] are read); outAT[n][n] = base + sum_{v >= 1} coef[v] A_v
 * (hs_sp_apply_AT on a copy of base[n][n]; coef[m + 1], coef[0] is not used).  V / outA or coef / base / outAT may be NULL: that
 * half is skipped */
HIPSDP_API int  hipsdp_sparse_ops_unit(int device, int n, int m, long long nnz, const int* var, const int* row, const int* col,
   const double* val, const double* V, const double* coef, const double* base, double* outA, double* outAT);
/* measured FP64 matrix peak of the device: a chip-filling launch of register-only v_mfma_f64_16x16x4_f64 for about ms milliseconds;
 * *tflops by HIP events, *ghz = shader clocks per wall tick inside the kernel (bench.py prices its roofline against this as well) */
HIPSDP_API int  hipsdp_mfma_peak(int device, double ms, double* tflops, double* ghz);
HIPSDP_API int  hipsdp_potrf(int device, int n, double* A, int* fail);                       /* lower Cholesky in place, row-major */
/* both forms of the blocked factorization for the parity tests: v1 = 1 the four-launch form, 0 one launch per block column; psd = 1
 * semidefinite pivot rule with diag0 = diag(A), forced pivots in regmask[n]; dinv[ceil(n / 64) * 4096] (any output may be NULL) */
HIPSDP_API int  hipsdp_potrf_ex(int device, int n, double* A, int psd, int v1, double* dinv, int* regmask, int* fail);
HIPSDP_API int  hipsdp_potrs(int device, int n, const double* A, int nrhs, double* rhs);     /* factor + solve, rhs[k * n + i] */
/* one factorization of A (psd = 0: hs_potrf; 1: hs_potrf_psd with diag0 = diag(A) and a mask, as hipsdp_potrf_ex), then ncalls solves one
 * behind the other on ONE hs_trsv_sync workspace with one epoch counter, as the engine issues them: call c has nrhs[c] in 1..4 right-hand
 * sides and mode[c] in {3, 5, 6, 7} (1 forward + 2 backward + 4 corrected) and runs in place on slab c of rhs (row k of the slab at
 * rhs[(4 c + k) n]).  Anything else: HIPSDP_ERR_ARG before the first launch.  regmask[n] (may be NULL): the zeroed columns (psd = 1);
 * *fail: the factorization flag.  HIPSDP_ERR_NUMERIC when a solve set the error word of the workspace */
HIPSDP_API int  hipsdp_potrs_seq(int device, int n, const double* A, int psd, int ncalls, const int* nrhs, const int* mode, double* rhs,
   int* regmask, int* fail);
/* the fused single-block factorization of base + alpha dir (dir may be NULL), 1 <= n <= 64: pair = 0 one problem through
 * hs_potrf_small_ext, pair = 1 two problems of n rows, one behind the other in every array, through hs_potrf_small_ext_pair.  L (upper
 * triangle zeroed), Mout, Linv, Gram: n x n each, dinv: 4096 each, flag: one word each, cleared before the launch (set_flag as in
 * hs_potrf_psd); Mout, Linv may be NULL; Gram (the inverse of the matrix) only with want_gram = 1, which n > 32 answers with
 * HIPSDP_ERR_ARG as the engine function does */
HIPSDP_API int  hipsdp_potrf_small_unit(int device, int n, int pair, const double* base, const double* dir, double alpha, int set_flag,
   int want_gram, double* L, double* dinv, double* Mout, double* Linv, double* Gram, int* flag);
/* strict-mode factorization of two matrices of n rows, one behind the other in A: pair = 1 through hs_potrf_pair (n > 64: one launch per
 * block column for both), 0 through two calls of hs_potrf.  dinv: hipsdp_potrf_dinv_len(n) doubles per matrix (inverses of the diagonal
 * blocks, then the staging blocks of the block-column kernel; zero where nothing is written), fail[2]: the flag of each matrix */
HIPSDP_API long long hipsdp_potrf_dinv_len(int n);
HIPSDP_API int  hipsdp_potrf_pair_unit(int device, int n, int pair, double* A, double* dinv, int* fail);
/* the trial iterates X + alpha dX, Z + alpha dZ of a step with the saved iterate and the copies the Cholesky check factors: io = X, Z, dX,
 * dZ, Xs, Zs, Lx, Lz (n x n each, all read, all but dX and dZ come back); fused = 1: hs_trial_pair, 0: the hs_copy / hs_scale_add /
 * hs_copy launches it replaces; first = 1: first attempt (base X, Z, saved on the way), 0: halved step (base Xs, Zs) */
HIPSDP_API int  hipsdp_trial_pair_unit(int device, int n, int fused, int first, double alpha, double* io);
/* The merged launches between two Schur assemblies on the general path, each against the launches it replaces (fused = 1 / 0); outputs
 * that a form does not write come back as NaN.  Lp = n (n + 1) / 2 rounded up to even, the packed lower triangle.
 * after_solve2: rhs2[2 m], u1[m] -> u2[m], wt[m + 1], e2[m + 1] = [1; u2], e1[m + 1] = [0; u1] (k_after_solve2 + hs_make_ext twice).
 * unpack3: pk[3][Lp] -> out[3][n][n] (hs_unpack_sym three times).  dz: pk[Lp], P2, Rd, dtau, eta -> dZ = (unpack(pk) - dtau P2) + eta Rd
 * (hs_unpack_sym + k_dz_combine).  dirmat: H = s1 Zinv - X - sym(GZ) and its packed, weighted copy pk[Lp] (hs_dirmat + hs_pack_weighted).
 * dir: the scalars of a direction and its closing kernel through the engine's own function, one block of n rows, m variables: B, H [n][n];
 * rhs2, rp, b, u1, u2 [m]; par = eta, rg, sigmu, tau, kappa, etk; sc[hipsdp_tail_sc_len()] read and written; dy[m], dyt[m + 1].
 * dots: out[0] = <a0, a1> + <a0, a2>, out[1] = <a2, a2> over n^2 entries and out[2] = <v0, v1> over m inside one batch of deferred
 * reductions (hs_dot against hs_dot_deferred); a[3][n^2], v[2][m], out[3] */
HIPSDP_API int  hipsdp_tail_after_solve2_unit(int device, int m, int fused, const double* rhs2, const double* u1, double* u2, double* wt,
   double* e2, double* e1);
HIPSDP_API int  hipsdp_tail_unpack3_unit(int device, int n, int fused, const double* pk, double* out);
HIPSDP_API int  hipsdp_tail_dz_unit(int device, int n, int fused, const double* pk, const double* P2, const double* Rd, double dtau, double eta,
   double* dZ);
HIPSDP_API int  hipsdp_tail_dirmat_unit(int device, int n, int fused, double s1, const double* Zinv, const double* X, const double* GZ, double* H,
   double* pk);
HIPSDP_API int  hipsdp_tail_sc_len(void);
HIPSDP_API int  hipsdp_tail_dir_unit(int device, int m, int n, int fused, const double* B, const double* H, const double* rhs2, const double* rp,
   const double* b, const double* u1, const double* u2, const double* par, double* sc, double* dy, double* dyt);
HIPSDP_API int  hipsdp_tail_dots_unit(int device, int m, int n, int fused, const double* a, const double* v, double* out);
HIPSDP_API int  hipsdp_trtri(int device, int n, const double* A, double* Linv);              /* A spd -> inverse of its Cholesky factor */
HIPSDP_API int  hipsdp_lambda_min(int device, int n, const double* W, int steps, double* theta, double* resid);
/* the Lanczos entry of the engine without a solver's exchange vectors, one or two matrices per launch (W1 may be NULL): exact up to 16
 * rows, the fused launch per step up to 8192, a launch per step and matrix above; steps <= 0: min(n, 250).  theta[2], resid[2],
 * steps_done[2]: {theta, residual bound, size of the tridiagonal matrix} per matrix (NaN, NaN, -1 for a matrix that is not given) */
HIPSDP_API int  hipsdp_lambda_min2_unit(int device, int n, const double* W0, const double* W1, int steps, double* theta, double* resid,
   int* steps_done);
/* lambda_min(L D L^T), n <= 64, L lower triangular, D symmetric: the small-block step-length kernels; theta[2], resid[2] */
HIPSDP_API int  hipsdp_lambda_min_scaled(int device, int n, const double* L, const double* D, int steps, double* theta, double* resid);
/* host only: whether the one-launch kernel admits a shape (m variables, q LP rows, nblk blocks of ns[k] rows: its LDS layout fits),
 * and the size class that would serve it (10 / 16 / 64: largest block, 1064: m > 64; -1: no such shape) */
HIPSDP_API int  hipsdp_solve1_fits(int m, int q, int nblk, const int* ns);
HIPSDP_API int  hipsdp_solve1_class(int m, int nblk, const int* ns);
/* host only: the bookkeeping of the cold-start store (csrc/hs_gram_cache.h).  hipsdp_gram_gen_next: the next generation number of
 * *counter.  hipsdp_gram_key_match_unit: 1 when a Gram matrix stored under key a (m variables, nblk blocks of n[k] rows with form[k]
 * - 1 full rows, 2 packed - and generation gen[k], workspace ws = {kws_len, chunk_cols, full}) serves a cold solve with key b; 0 when
 * it does not, or when either key is none the store would take */
HIPSDP_API unsigned long long hipsdp_gram_gen_next(unsigned long long* counter);
HIPSDP_API int  hipsdp_gram_key_match_unit(int m_a, int nblk_a, const int* n_a, const int* form_a, const unsigned long long* gen_a,
   const long long* ws_a, int m_b, int nblk_b, const int* n_b, const int* form_b, const unsigned long long* gen_b, const long long* ws_b);
/* the batched full decomposition behind hipsdp_eigencuts_all on `count` host matrices, one behind the other in A: matrix j has
 * ns[j] <= 128 rows; lam: ns[j] eigenvalues each (ascending), V: ns[j] x ns[j] each (row k = k-th eigenvector) - for every matrix
 * the bits of hipsdp_syev_small; *launches: kernel launches issued (at most 3, whatever count is) */
HIPSDP_API int  hipsdp_syev_many_unit(int device, int count, const int* ns, const double* A, double* lam, double* V, int* launches);
/* k_sc_tpower (csrc/sparsecuts.hip) alone on `count` host matrices, one behind the other in Z: matrix j has ns[j] <= 128 rows, the
 * start vector v0 (ns[j] values each, one behind the other), the largest eigenvalue maxeig[j] and the target sparsity sizes[j].
 * Every matrix takes part (opts->tol is not used: there is no decomposition to take lmin from); feastol, convtol, maxcuts >= 1 and
 * maxit as in hipsdp_sparsecuts_all.  ncuts[count], eigvals[count * maxcuts], vecs (maxcuts x ns[j] each, one behind the other),
 * iters[count], flags[count] as that call returns them; slots c >= ncuts[j] are not written. */
HIPSDP_API int  hipsdp_sparsecuts_unit(int device, int count, const int* ns, const double* Z, const double* v0, const double* maxeig,
   const int* sizes, const hipsdp_sparsecut_opts* opts, int* ncuts, double* eigvals, double* vecs, int* iters, int* flags);
/* k_sc_tpower_large (csrc/sparsecuts_large.hip) alone on ONE host matrix Z of 129 <= n <= 512 rows with the start vector v0[n], the
 * largest eigenvalue maxeig and the target sparsity size >= 1; opts as above (tol is not used, maxcuts >= 1).  *ncuts, eigvals[maxcuts],
 * vecs[maxcuts x n], *iters, *flags as hipsdp_sparsecuts returns them; slots c >= *ncuts are not written. */
HIPSDP_API int  hipsdp_sparsecuts_large_unit(int device, int n, const double* Z, const double* v0, double maxeig, int size,
   const hipsdp_sparsecut_opts* opts, int* ncuts, double* eigvals, double* vecs, int* iters, int* flags);
/* the batched selection of SEVERAL eigenpairs behind hipsdp_eigencuts_all_large (hs_syevx_many_below, csrc/syevx.hip) on `count` host
 * matrices of mixed sizes, one behind the other in A (matrix j: n[j] x n[j], 2 <= n[j] <= 512, read as hipsdp_syevx_below reads it):
 * through the staging of that call, the column launches with at most cap (1 .. 128) workgroups per matrix and the selection of the
 * eigenvalues <= bound, at most maxk <= 32.  cnt[j]: pairs returned, lam + j maxk: their eigenvalues (ascending), V + maxk (n[0] + ... +
 * n[j - 1]): their unit vectors, row k of n[j] values (V may be NULL) - for every matrix the bits of hipsdp_syevx_below on it alone,
 * whatever cap is.  Entries behind cnt[j] are not written. */
HIPSDP_API int  hipsdp_syevx_many_below_unit(int device, int count, const int* n, const double* A, double bound, int maxk, int cap, int* cnt,
   double* lam, double* V);
/* the first stage of hipsdp_syevx alone, 2 <= n <= 512: the tridiagonal matrix Q^T A Q (d[n], e[n - 1] in e[0 .. n - 2], e[n - 1] = 0)
 * and Q = H_0 H_1 ... H_{n-2}, H_j = I - tau[j] v_j v_j^T, row j of Vrefl (n x n) = v_j (zeros up to entry j, entry j + 1 one) */
HIPSDP_API int  hipsdp_tridiag_unit(int device, int n, const double* A, double* d, double* e, double* Vrefl, double* tau);
/* stages 2 and 3 of the full decomposition above 128 rows (csrc/syevr.hip) alone on a caller's symmetric tridiagonal matrix, 2 <= n <= 512,
 * diagonal d[n], off-diagonal e[n - 1]: all eigenvalues (ascending) and the unit eigenvectors of T as the rows of Z (n x n) */
HIPSDP_API int  hipsdp_tvec_unit(int device, int n, const double* d, const double* e, double* lam, double* Z);
/* the batched full decomposition of the large PSD projections (csrc/psd_large.hip: hs_syevx_many_cols, hs_syevr_many_tvec, hs_syevr_many_back) on
 * `count` dense host matrices of mixed sizes, one behind the other in A (matrix j: n[j] x n[j], 129 <= n[j] <= 512, read as hipsdp_syevr
 * reads it): the column launches with at most cap (1 .. 128) workgroups per matrix, then all eigenpairs of every matrix.  lam: the
 * eigenvalues of matrix j (ascending) at n[0] + ... + n[j - 1]; V: its unit eigenvectors, row k of n[j] values, at n[0]^2 + ... +
 * n[j - 1]^2 - for every matrix the bits of hipsdp_syevr on it alone, whatever the table holds beside it and whatever cap is. */
HIPSDP_API int  hipsdp_syevr_many_unit(int device, int count, const int* n, const double* A, int cap, double* lam, double* V);
/* the device structure of engine block `block` of a solver CREATED FROM THIS LIBRARY (it contains the engine), a block kept as
 * nonzeros - built first if triplets are waiting: counts[6] = n, m, nnz, npos, nfull, nslots, then every array that is not NULL:
 * voff[m + 1], vrow / vcol / vval[nnz]; poff[npos + 1], prow / pcol[npos], pvar / pval[nnz]; foff[m + 1], frow / fcol / fval[nfull];
 * soff[m + 1], srow[nslots], sent[nslots + 1].  A first call with the arrays NULL gives the counts to size them by. */
HIPSDP_API int  hipsdp_sparse_dump_unit(hipsdp_solver* solver, int block, long long* counts, int* voff, int* vrow, int* vcol, double* vval,
   int* poff, int* prow, int* pcol, int* pvar, double* pval, int* foff, int* frow, int* fcol, double* fval, int* soff, int* srow, int* sent);
/* the first launch of hipsdp_check_y_many (csrc/check_many.hip: k_cm_form_z) alone on a loaded solver CREATED FROM THIS LIBRARY: Z_b(Y[j])
 * of every candidate j < count (Y: count x m, row-major, host) and every block b of at most 512 rows the call serves, as plain n_b x n_b
 * arrays: Z + j (n_0^2 + ... + n_{nb-1}^2) + (n_0^2 + ... + n_{b-1}^2).  served[b] (may be NULL) = 0, or -1 for a block that is not
 * served, whose parts of Z are not written.  *launches: the kernel launches issued (one, whatever count and the blocks are).
 * HIPSDP_ERR_ARG: solver NULL or without a shape, count < 1, Y, Z or launches NULL. */
HIPSDP_API int  hipsdp_form_z_many_unit(hipsdp_solver* solver, int count, const double* Y, double* Z, int* served, int* launches);
/* the candidates k_cm_form_z serves per pass over a block's storage (HS_CM_G, a compile-time constant of csrc/hs_kernels.h) */
HIPSDP_API int  hipsdp_check_many_group(void);
/* the minors launch of hipsdp_rank1_check_many (csrc/rank1.hip: k_r1_minors's scans) alone on `count` host matrices, matrix k of n[k]
 * rows (1 .. 512), one behind the other in Z (the lower triangle at [i n + k], k <= i, is read): minorev[k], minorind[2 k ..],
 * minordet[k], detind[2 k ..] as the call returns them for one (candidate, block).  HIPSDP_ERR_ARG: count < 1, a size outside 1 .. 512,
 * feastol negative or not a number, a NULL pointer. */
HIPSDP_API int  hipsdp_rank1_minors_unit(int device, int count, const int* n, const double* Z, double feastol, double* minorev, int* minorind,
   double* minordet, int* detind);
/* the three-index values kernels of hipsdp_rank1_check_many on `count` (at most 65535) host matrices laid out as above, every matrix by
 * the kernels of its size class (1 .. 64 rows, 65 .. 128 rows, 129 .. 512 rows: the column launches and the one values launch) and the
 * launch that stores the eigenvalues: lam[3 k ..] = eigenvalues 1, n - 1, n of matrix k (n = 1, 2: the call's conventions) */
HIPSDP_API int  hipsdp_lsel_many_unit(int device, int count, const int* n, const double* Z, double* lam);
/* the coefficient launches of hipsdp_rounding_frame (csrc/rounding.hip: k_rf_gather, k_rf_coefs_scalar, k_rf_coefs_mc, k_rf_store) alone
 * on host data of ONE block, through the routing rule of the call: V (n x n, row j = v_j) and the block's matrices in the form `form` -
 * 0: dense rows, A = (m + 1) x n^2; 1: packed lower triangles, A = (m + 1) x n (n + 1) / 2, entry (r, c), c <= r, at r (r + 1) / 2 + c;
 * 2: nonzeros, A = the dense constant matrix (n x n) and the variables' lower-triangular nonzeros as nnz triplets (var 1 .. m, row >= col,
 * val) sorted by var.  out[j (m + 1) + i] = v_j^T A_i v_j, i = 0: the constant matrix.  *route (may be NULL) = 1: the matrix-core kernel
 * served the block (more than 64 rows, forms 0 and 1), 0: the scalar one; *slices (may be NULL): the slices of the storage index.
 * HIPSDP_ERR_ARG: n outside 1 .. 512, m < 0, another form, V, A or out NULL, a triplet outside the lower triangle or out of order. */
HIPSDP_API int  hipsdp_rounding_coefs_unit(int device, int n, int m, int form, const double* V, const double* A, long long nnz, const int* var,
   const int* row, const int* col, const double* val, double* out, int* route, int* slices);
/* the Newton kernel of hipsdp_onevar_bounds (csrc/eigi.hip: k_onevar_small for n <= 64, k_onevar_mid for n <= 128) alone on host
 * matrices: Z (n x n) and, for job j < count, the dense A + j n^2 (n x n), the shift shift[j] (= u_i), kind[j] (NULL: all NEWTON),
 * lb[j], ub[j]: M_j(mu) = Z + (mu - shift[j]) A_j.  infinity is 1e20, maxevals <= 0 means 100.  status, optval, lmin, grad, evals as
 * hipsdp_onevar_bounds returns them (lmin, grad, evals may be NULL). */
HIPSDP_API int  hipsdp_onevar_unit(int device, int n, int count, const double* Z, const double* A, const double* shift, const int* kind,
   const double* lb, const double* ub, double feastol, int maxevals, int* status, double* optval, double* lmin, double* grad, int* evals);
/* the launches of hipsdp_onevar_bounds_all (csrc/eigi.hip: k_onevar_all_small, k_onevar_all_mid) alone on host matrices given PER JOB:
 * job j < count has n[j] rows (1 .. 128), Z + zoff[j] (n[j]^2 doubles) and the dense A + zoff[j] (the same offsets: zoff[j] = sum of
 * n[k]^2, k < j), shift[j], kind[j] (NULL: all NEWTON; EXTREMES allowed), lb[j], ub[j].  mid_cap >= 1: the cap on the grid of the
 * 65-128 launch (the product call passes the device's compute units), so that a handful of jobs stride.  infinity is 1e20. */
HIPSDP_API int  hipsdp_onevar_all_unit(int device, int count, const int* n, const double* Z, const double* A, const double* shift,
   const int* kind, const double* lb, const double* ub, double feastol, int maxevals, int mid_cap,
   int* status, double* optval, double* lmin, double* grad, int* evals);
/* the rounds of hipsdp_onevar_bounds_large (csrc/onevar_large.hip: hs_onevar_large_chunk) alone on host matrices given PER JOB, as
 * hipsdp_onevar_all_unit takes them, with n[j] = 2 .. 512 and mixed sizes in one call: the batched kernels at small sizes.  Every job
 * is a block of its own with dense rows and its Z given, so no Z(u) launch is issued.  wg_cap: the cap on the workgroups per job of
 * the column launches (<= 0: the product call's default for the number of jobs); chunk: jobs per chunk at most (<= 0: all in one).
 * rounds (may be NULL): the sum of the rounds of the chunks.  infinity is 1e20. */
HIPSDP_API int  hipsdp_onevar_large_unit(int device, int count, const int* n, const double* Z, const double* A, const double* shift,
   const int* kind, const double* lb, const double* ub, double feastol, int maxevals, int wg_cap, int chunk,
   int* status, double* optval, double* lmin, double* grad, int* evals, int* rounds);
/* the fan-out kernel of hipsdp_solve_objectives (hs_objs_fanout, csrc/kernels.hip) alone: count jobs of a problem with m variables, q LP
 * rows and nblk blocks of ns[k] rows.  B: count x m objectives, b_own[m]: the solver's own; have_start = 1: the start point y[m], x[q],
 * z[q] and XZ = X_0, Z_0, X_1, Z_1, ... one behind the other (have_start = 0: not read, only the objectives are fanned out).
 * lanes: (count + 1) lanes of *lane_len doubles, lane 0 the home lane (b_own and the start), lane 1 + j job j; every double of it is set
 * to `guard` before the launch, and every array of a lane (offs[4 + 2 nblk]: b, y, x, z, X_0, Z_0, ...) is followed by `gap` (even, >= 0)
 * doubles that nothing may write.  A call with lanes = NULL returns *lane_len and offs alone; *launches (may be NULL): kernel
 * launches issued (1 whatever count is) */
HIPSDP_API int  hipsdp_objs_fanout_unit(int device, int count, int m, int q, int nblk, const int* ns, const double* B, const double* b_own,
   int have_start, const double* y, const double* x, const double* z, const double* XZ, int gap, double guard, long long* lane_len,
   long long* offs, double* lanes, int* launches);
/* The small-problem passes and their recorded forms inside the single-workgroup batch kernel (csrc/kernels.hip: the RB_* records of
 * k_red_batch).  recorded = 0: the engine function with no batch open, so the kernel gets its own launch; 1: the same call between
 * hs_red_batch_hold and hs_red_batch_release.  *pending: the records waiting just before the release: 0 when the call declined (too much
 * work for one workgroup) or recorded = 0.  Outputs that an operation does not write come back as NaN.
 * dir_block: out = s1 Zinv - X - sym((c X R + E) Zinv), n x n each, E may be NULL; n > 48 gives the engine's HIPSDP_ERR_ARG.
 * lp_rows: t_r = Dext[r, :] . v (Dext q x m1); mode 0: out1 = t - z; mode 1: out1 = t + eta rd, out2 = sigmu / z - x - (x out1 + elp) / z
 *    (elp may be NULL); out1[q], out2[q].
 * apply_A: out[i] = sum_k <A_k[i], V_k> + sum_r Dext[r][i] vlp[r], i < m1: nblk in 1 .. 8 blocks of n2[k] entries, one behind the other
 *    in A (block k as m1 x n2[k]) and in V; q >= 0 LP rows (Dext q x m1); epi 1: vout[i - 1] = out[i] - scal vin[i - 1], epi 2:
 *    vout[i - 1] = vin[i - 1] scal - out[i] for i >= 1; out[m1], vin[m1 - 1], vout[m1 - 1].
 * elementwise: in[6][n] = x, z, r, elp, a, b; par = sigmu, eta, alpha, s0, s1.  hs_lp_dir: o_lp = sigmu / z - x - (eta x r + elp) / z
 *    (use_elp = 0: no elp); hs_vec_mul: o_mul = a .* b; hs_make_ext: o_ext[n + 1] = [s0; s1 a]; hs_axpy3: ys += alpha xs on three vectors
 *    of nn[0], nn[1], nn[2] >= 0 entries, one behind the other in xs and ys.
 * gemv_t: out[e] = sum_i coef[i] A[i lda + e] + sa add[e], R rows of lda >= E doubles; add_mode 0: no additive term, 1: add[E] an array
 *    of its own, 2: the output itself, which starts as add[E]. */
HIPSDP_API int  hipsdp_small_dir_block_unit(int device, int n, double c, double s1, const double* X, const double* R, const double* E,
   const double* Zinv, int recorded, double* out, int* pending);
HIPSDP_API int  hipsdp_small_lp_rows_unit(int device, int q, int m1, const double* Dext, const double* v, int mode, double eta, double sigmu,
   const double* x, const double* z, const double* rd, const double* elp, int recorded, double* out1, double* out2, int* pending);
HIPSDP_API int  hipsdp_small_apply_A_unit(int device, int m1, int nblk, const int* n2, const double* A, const double* V, int q,
   const double* Dext, const double* vlp, int epi, double scal, const double* vin, int recorded, double* out, double* vout, int* pending);
HIPSDP_API int  hipsdp_small_elementwise_unit(int device, int n, const int* nn, const double* par, int use_elp, const double* in,
   const double* xs, int recorded, double* o_lp, double* o_mul, double* o_ext, double* ys, int* pending);
HIPSDP_API int  hipsdp_small_gemv_t_unit(int device, int R, long long E, long long lda, const double* A, const double* coef, double sa,
   int add_mode, const double* add, int recorded, double* out, int* pending);
/* `count` <= 8 reductions of one kind (0 hs_dot <a, b>, 1 hs_absmax max |a|, 2 hs_ratio_min min over b < 0 of -a / b, 3 hs_lp_s0
 * sum (a / b) c^2), reduction j over len[j] entries (operands one behind the other in a, b, c) into out[slot[j]], slot[j] < nslots <= 32,
 * accumulate[j] = 1: combined with what the slot holds.  Every slot is first set to preset[.] by hs_fill_scalar.  recorded = 1: fills and
 * reductions inside one hs_red_batch_begin / hs_red_batch_end (the fills are records too: *pending counts them, and more records than a
 * batch holds are launched on the way); 0: every call a launch of its own */
HIPSDP_API int  hipsdp_reductions_unit(int device, int kind, int count, const int* len, const int* slot, const int* accumulate,
   const double* a, const double* b, const double* c, int nslots, const double* preset, int recorded, double* out, int* pending);
/* the two small solves with the factor of M (m <= 64, M symmetric positive definite, factored on the device as the engine does it;
 * *fail its flag).  form 0: hs_red_batch_solve inside a batch, nrhs <= 8 right-hand sides ld >= m apart, rhs[nrhs x ld] in place.
 * form 1: k_solve2_small: rhs[2 m] comes in as [g ; b] and goes out as the two solutions, u2[m], wt[m + 1].  The environment switch
 * HIPSDP_SMALL_SOLVE=subst is read by the call */
HIPSDP_API int  hipsdp_small_solve_unit(int device, int m, const double* M, int form, int nrhs, long long ld, double* rhs, double* u2,
   double* wt, int* pending, int* fail);
/* out[v][e] = sum_i c[v][i] A[i lda + e], v < 3 (c[3][R], out[3][E]): fused = 1 hs_gemv_t3 (and, when it does not take the shape, the
 * three hs_gemv_t calls the engine then makes), 0: three hs_gemv_t calls; *took = 1 when the fused kernel ran */
HIPSDP_API int  hipsdp_gemv_t3_unit(int device, int R, long long E, long long lda, const double* A, const double* c, int fused, double* out,
   int* took);
/* hs_gemv_n: out[v][i] = sum_e A[i lda + e] V[v][e], nv <= 4 (V[nv][E], out[nv][R]); the device copies of the vectors start voff doubles
 * behind a 16-byte aligned address; wsdoubles: the workspace given for the split form.  info[0] = slices a row is cut into, info[1] = 1
 * when the two-at-a-time kernel is taken (the launcher's rule recomputed from the same inputs) */
HIPSDP_API int  hipsdp_pass_a_unit(int device, int R, long long E, long long lda, const double* A, int nv, const double* V, int voff,
   long long wsdoubles, double* out, int* info);

#ifdef __cplusplus
}
#endif

#endif
