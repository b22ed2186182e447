/* hs_kernels.h - launch wrappers of the bandwidth-bound kernels (kernels.hip), the dense factorizations (chol.hip) and the
 * eigen kernels (eig.hip).  All pointers are device pointers unless a name ends in _h.  Every wrapper only enqueues work
 * on the given stream; nothing here synchronizes. */
#ifndef HS_KERNELS_H
#define HS_KERNELS_H

#include "hs_common.h"
#include "hs_cut_plan.h"
#include <vector>

/* ---- kernels.hip ---------------------------------------------------------------------------------------------- */
int hs_fill(hipStream_t s, double* p, long long n, double v);
int hs_set_identity(hipStream_t s, double* A, int n, double v);
int hs_copy(hipStream_t s, double* dst, const double* src, long long n);
int hs_axpy(hipStream_t s, long long n, double a, const double* x, double* y);              /* y += a x */
int hs_scale_add(hipStream_t s, long long n, double a, const double* x, double b, const double* y, double* out); /* out = a x + b y (y may be NULL) */
/* the trial iterates of a step for X and Z in one launch: V <- alpha dV + 1.0 base, the value also into L (the matrix the Cholesky check
 * factors in place); first = 1: base is V itself, saved to Vs on the way; 0 (halved step): base is the saved Vs.  Element for element
 * what hs_copy(Vs, V), hs_scale_add(alpha, dV, 1.0, Vs, V), hs_copy(L, V) leave behind */
struct hs_trial_job { double* V; const double* dV; double* Vs; double* L; };
int hs_trial_pair(hipStream_t s, long long n, double alpha, int first, const hs_trial_job* jobs);
int hs_mirror_lower(hipStream_t s, double* A, int n, long long lda);                        /* A[i][j] = A[j][i] for i < j */
int hs_symmetrize(hipStream_t s, double* A, int n);
int hs_transpose(hipStream_t s, int n, const double* src, double* dst);                     /* dst[i][j] = src[j][i], n x n, dst != src */                                         /* A = (A + A^T) / 2 */

/* out[v * ldo + i] = sum_e A[i * lda + e] * V_v[e],  i < R, e < E, v < nv <= 4 (one pass over A for all nv vectors) */
int hs_gemv_n(hipStream_t s, int R, long long E, const double* A, long long lda, int nv, const double* const* V,
   double* out, long long ldo, double* ws, long long wsdoubles);
/* out[e] = sum_i coef[i] * A[i * lda + e] + sa * add[e]   (add may be NULL) */
int hs_gemv_t(hipStream_t s, int R, long long E, const double* A, long long lda, const double* coef, double sa,
   const double* add, double* out);

/* three linear combinations of the rows in one sweep over A (o_v[e] = sum_i c_v[i] A[i * lda + e]); 1: done, 0: shapes do not
 * qualify (E, lda even, 16-byte aligned), < 0: error code negated */
/* the same with a workspace: few entries and many rows are summed in row chunks side by side (kernels.hip); hs_gemv_t_chunks(R, E)
 * * E doubles are needed for that (0: never split) */
int hs_gemv_t_chunks(int R, long long E);
int hs_gemv_t_ws(hipStream_t s, int R, long long E, const double* A, long long lda, const double* coef, double sa,
   const double* add, double* out, double* ws, long long wsdoubles);
int hs_gemv_t3(hipStream_t s, int R, long long E, const double* A, long long lda, const double* c0, const double* c1, const double* c2,
   double* o0, double* o1, double* o2);

/* out[slot] = sum_e a[e] * b[e]  (deterministic two-stage; partials in ws, >= 512 doubles) ; accumulate: out[slot] += */
/* deferred scalar reductions (kernels.hip): between begin and end, reductions over short vectors, scalar fills and scalar
 * copies on that stream are recorded and then executed in order by one launch */
void hs_red_batch_begin(hipStream_t s);
int hs_red_batch_end(void);
int hs_red_batch_end_publish(hipStream_t s, int n, const double* src, double* dst, unsigned long long seq, unsigned long long* flag);
void hs_red_batch_reset(void);
int hs_fill_scalar(hipStream_t s, double* p, double v);
/* single-block solves (m <= 64) and the direction's closing kernel can be part of a batch: see kernels.hip */
int hs_red_batch_solve(hipStream_t s, int m, const double* dinv, const double* L, int nrhs, double* vec, long long ld);
struct hs_rb_finish { int m; double eta, rg, sigmu, tau, kappa, etk; const double* u1; const double* u2; double* dy; double* dyt; double* sc;
   int s0, bub, bh, wrp, bu1, dtau, dkappa, den; };
int hs_red_batch_finish(hipStream_t s, const void* fin, size_t bytes);
int hs_copy_scalar(hipStream_t s, double* dst, const double* src);
/* regions in which everything recordable on the stream is recorded (the small single-workgroup kernels of the B&B-sized regime too:
 * kernels.hip) and everything else launches the records first; regions nest, a read-back (hs_red_batch_end_publish) ends them */
void hs_red_batch_hold(hipStream_t s);
int hs_red_batch_release(void);
int hs_red_batch_flush(void);
int hs_red_batch_pending(void);            /* records waiting for the launch */
int hs_red_batch_end_all(void);
int hs_make_ext(hipStream_t s, int m, double s0, double s1, const double* v, double* ext);
int hs_lp_rows_small(hipStream_t s, int q, int m1, const double* Dext, const double* v, int mode, double eta, double sigmu, const double* x,
   const double* z, const double* rd, const double* elp, double* out1, double* out2);
#define HS_AS_MAXBLK 8
struct hs_as_args { int nblk; int n2[HS_AS_MAXBLK]; const double* A[HS_AS_MAXBLK]; const double* V[HS_AS_MAXBLK]; };
int hs_apply_A_small(hipStream_t s, int m1, const hs_as_args* B, int q, const double* Dext, const double* vlp, double* out, int epi,
   double scal, const double* vin, double* vout);
int hs_axpy3(hipStream_t s, double a, long long n1, const double* x1, double* y1, long long n2, const double* x2, double* y2,
   long long n3, const double* x3, double* y3);
int hs_dot(hipStream_t s, long long n, const double* a, const double* b, double* out, int accumulate, double* ws);
/* hs_dot of a long vector inside a batch (begin without a held region): first stage launched at once, second stage a record of the batch;
 * slot 0 .. 3 selects 256 doubles of ws (>= 1024) for the partial sums; anything else falls back to hs_dot.  See kernels.hip */
#define HS_DOT_SLOT_DOUBLES 256        /* partial sums of one dot: the first stage never has more workgroups */
#define HS_DOT_SLOTS 4                /* deferred dots of one batch */
#define HS_RED_WS_DOUBLES (HS_DOT_SLOTS * HS_DOT_SLOT_DOUBLES)      /* what the engine allocates for ws */
int hs_dot_deferred(hipStream_t s, long long n, const double* a, const double* b, double* out, int accumulate, double* ws, int slot);
/* out[slot] = max(out[slot] if accumulate, max_e |a[e]|) */
int hs_absmax(hipStream_t s, long long n, const double* a, double* out, int accumulate, double* ws);
/* out[slot] = min(out[slot] if accumulate, min over e with d[e] < 0 of -x[e] / d[e]); +1e300 when no such e */
int hs_ratio_min(hipStream_t s, long long n, const double* x, const double* d, double* out, int accumulate, double* ws);

/* H = s1 * Zinv - X - (GZ + GZ^T) / 2,  all n x n */
/* largest block size of the single-workgroup ("small") variants that keep whole matrices in LDS */
#define HS_SMALL_N 48
/* n <= HS_SMALL_N: out = s1 Zinv - X - sym((c X R + E) Zinv) in one launch (E may be NULL) */
int hs_dir_block_small(hipStream_t s, int n, double c, const double* X, const double* R, const double* E, const double* Zinv,
   double s1, double* out);
int hs_dirmat(hipStream_t s, int n, double s1, const double* Zinv, const double* X, const double* GZ, double* H);
/* hs_dirmat that also stores hs_pack_weighted(H) to pk (same values, one launch) */
int hs_dirmat_pack(hipStream_t s, int n, double s1, const double* Zinv, const double* X, const double* GZ, double* H, double* pk);

/* LP block element-wise pieces (length q) */
int hs_lp_dir(hipStream_t s, int q, double sigmu, double eta, const double* x, const double* z, const double* rd_or_dz,
   const double* elp, double* out);      /* out = sigmu / z - x - (eta * x * r + elp) / z ; elp may be NULL */
int hs_lp_scale_rows(hipStream_t s, int q, int cols, const double* x, const double* z, const double* D, double* S); /* S[r] = (x_r / z_r) D[r] */
int hs_vec_mul(hipStream_t s, long long n, const double* a, const double* b, double* out);   /* out = a .* b */
int hs_lp_s0(hipStream_t s, int q, const double* x, const double* z, const double* beta, double* out, int accumulate, double* ws); /* sum (x/z) beta^2 */

/* packed lower copies for the bandwidth-bound passes (half the bytes of the full storage) */
int hs_pack_rows(hipStream_t s, int m1, int n, long long Lp, const double* A, double* Apk);
/* D[i][r] = A_i[r][r] (r < n; 0 for n <= r < ldd) gathered from the packed rows */
int hs_packed_diag(hipStream_t s, int m1, int n, int ldd, long long Lp, const double* Apk, double* D);
/* C[r][c] -= S[r][c] for c <= r (both n x n, leading dimension n) */
int hs_sub_lower(hipStream_t s, int n, const double* S, double* C);
int hs_pack_weighted(hipStream_t s, int n, const double* V, double* pk);
int hs_unpack_sym(hipStream_t s, int n, const double* pk, double sa, const double* add, double* out);
/* cnt <= 3 calls hs_unpack_sym(n, pk[k], 0.0, NULL, out[k]) in one launch */
int hs_unpack_sym3(hipStream_t s, int n, int cnt, const double* const* pk, double* const* out);
/* hs_unpack_sym(n, pk, 0.0, NULL, dZ) and dZ = (dZ - sc[idtau] P2) + eta Rd (the engine's k_dz_combine) in one launch */
int hs_unpack_dz_combine(hipStream_t s, int n, const double* pk, const double* P2, const double* sc, int idtau, double eta, const double* Rd,
   double* dZ);
int hs_zero_upper(hipStream_t s, double* A, int n);                                         /* A[i][j] = 0 for i < j */

/* ---- schur.hip ------------------------------------------------------------------------------------------------ */
struct hs_schur_ws
{
   double*   T;            /* chunk_cols x n^2 */
   double*   U;            /* chunk_cols x n^2 */
   double*   K;            /* split-K slabs */
   double*   V;            /* variable-sharded form only: the received pieces, m1 x (rows of this rank) x (slice width) */
   long long capT, capV;   /* variable-sharded form: doubles in T (= U) and in V */
   long long chunk_cols;
   long long n2;           /* doubles per matrix the allocation was sized for */
   long long kws_len;
   int       full;         /* 1: T and U hold all m1 matrices (hs_schur_W usable) */
   /* variable-sharded form, overlapped exchange: second send / receive buffers and the events of the two-slice pipeline */
   double*   U2;
   double*   V2;
   void*     evP[2];       /* hipEvent_t: the products of a slice are in its send buffer */
   void*     evX[2];       /* hipEvent_t: the exchange of a slice has arrived */
   void*     ev_g2;        /* hipEvent_t or NULL: hs_schur_W waits for it between its first and its second product (the inverse factor of Z
                            * is formed on another queue while A_stack R runs; set and cleared by the caller around the call) */
   int       (*after_g1)(void*);   /* or NULL: called by hs_schur_W when its first product is in the queue (the caller puts work of its
                                    * own into other queues there - it may set ev_g2); once, then cleared */
   void*     after_g1_arg;
};
int  hs_schur_ws_alloc(hs_schur_ws* w, int m1, long long n2max, double budget_gb);
void hs_schur_ws_free(hs_schur_ws* w);
/* accumulate the lower triangle of Mx (ld m1) for the columns [j_begin, j_end) with U_j = X A_j Zinv */
int  hs_schur_U(hipStream_t s, int m1, int n, const double* A, const double* X, const double* Zinv, double* Mx,
   hs_schur_ws* w, int j_begin, int j_end);
/* accumulate the lower triangle of Mx with W_j = G A_j R (R: lower Cholesky factor of X with a ZERO upper triangle,
 * G: inverse of the lower Cholesky factor of Z) */
int  hs_schur_W(hipStream_t s, int m1, int n, const double* A, const double* R, const double* G, double* Mx, hs_schur_ws* w);
int  hs_schur_W_identity(hipStream_t s, int m1, int n, const double* A, double* Mx, hs_schur_ws* w);
int  hs_schur_W_identity_range(hipStream_t s, int m1, int n, const double* A, long long k0, long long k1, double* Mx, hs_schur_ws* w);
/* the same Gram matrix from the packed lower triangles Apk[m1][Lp] (hs_pack_rows): Mx += 2 P P^T - D D^T, D[i][r] = A_i[r][r] gathered
 * into w->T; hs_schur_identity_packed_fits: 1 when w->T holds D.  Both identity forms write the lower triangle of Mx exactly when the
 * Gram kernel takes the product, and the lower TILES (every 64- or 128-wide tile that touches the lower triangle: a diagonal tile whole)
 * when the tile kernels do; nothing above the diagonal tiles is ever written, and the caller mirrors the lower triangle afterwards */
int  hs_schur_W_identity_packed(hipStream_t s, int m1, int n, const double* Apk, long long Lp, double* Mx, hs_schur_ws* w);
int  hs_schur_identity_packed_fits(const hs_schur_ws* w, int m1, int n);

int  hs_schur_Urows(hipStream_t s, int m1, int n, const double* A, const double* X, const double* Zinv, double* Mx,
   hs_schur_ws* w, int r_begin, int r_end);
void hs_shard_rows(int m1, int nranks, int rank, int* chunk_rows, int* first_begin, int* second_begin);
/* column-slice sharding of the W formulation: this rank's share [c0, c0 + cw) of the columns of the W_j, accumulated into the
 * lower tiles of Mx; the ranks' partial matrices add up to the Schur matrix (all-reduce) */
int  hs_schur_Wcols(hipStream_t s, int m1, int n, const double* A, const double* R, const double* G, double* Mx, hs_schur_ws* w,
   int c0, int cw);
void hs_shard_cols(int m1, int n, int nranks, int rank, int* c_begin, int* c_width);
/* variable-sharded form (A_j lives on the rank that owns variable j; A is the pointer row 0 WOULD have): the column slice
 * [c0, c0 + cw) of W_j = G A_j R is formed for the rank's own rows [r0, r1) of A, cut into row ranges, exchanged all-to-all so
 * that every rank holds its row range of ALL W_j, and that rank's part of W W^T is accumulated into the lower tiles of Mx.
 * All ranks call it with the same (c0, cw); the partial matrices add up to the Schur matrix (all-reduce afterwards). */
int  hs_schur_Wvar(hipStream_t s, void* comm, int rank, int nranks, int m1, int n, const double* A, const double* R, const double* G,
   double* Mx, hs_schur_ws* w, int c0, int cw);
int  hs_schur_ws_alloc_var(hs_schur_ws* w, int m1, int nranks, int n, int cwmax);
/* the second pair of buffers + events for hs_schur_Wvar_all(overlap); HS_ERR_NOMEM leaves the in-order form usable */
int  hs_schur_ws_alloc_var_overlap(hs_schur_ws* w);
/* all column slices of one block: slice after slice as hs_schur_Wvar does (overlap = 0), or - overlap = 1, second buffers present -
 * as a two-slice pipeline: the all-to-all of slice s runs on the communication queue `sc` behind an event while the compute queue
 * forms the products of slice s + 1; the Gram update of slice s waits for its exchange.  Same kernels, same arguments, same order
 * of the updates of Mx: bit-identical to the in-order form. */
int  hs_schur_Wvar_all(hipStream_t s, hipStream_t sc, void* comm, int rank, int nranks, int m1, int n, const double* A, const double* R,
   const double* G, double* Mx, hs_schur_ws* w, int cwmax, int overlap);
void hs_var_rows(int m1, int nranks, int rank, int* r0, int* r1);            /* rows of A (variables) a rank owns */
void hs_var_wrows(int n, int nranks, int rank, int* q0, int* q1);            /* rows of the W_j a rank receives */
int  hs_alltoall(void* comm, const double* send, double* recv, const long long* cnt, hipStream_t stream);
int  hs_allreduce_sum(void* comm, double* buf, long long count, hipStream_t stream);
int  hs_mirror_upper(hipStream_t s, double* A, int n, long long lda);                       /* A[i][j] = A[j][i] for i > j */
/* multi.hip: in-place all-gather of equal pieces, piece of rank r at buf + r * count */
int  hs_allgather_inplace(void* comm, double* buf, long long count_per_rank, int rank, hipStream_t stream);
int  hs_allgather(void* comm, const double* send, double* recv, long long count_per_rank, hipStream_t stream);

/* ---- sparse.hip: constraint matrices kept as nonzeros (see there) ----------------------------------------------------- */
struct hs_sparse
{
   int        n, m;
   long long  nnz;
   /* by variable: entries of variable v (1 .. m) are [voff[v - 1], voff[v]) */
   int*       voff;
   int*       vrow;
   int*       vcol;
   double*    vval;
   /* by position: position k (a lower-triangular (row, col) that occurs) has the entries [poff[k], poff[k + 1]) */
   long long  npos;
   int*       poff;
   int*       prow;
   int*       pcol;
   int*       pvar;        /* variable (1-based) of an entry */
   double*    pval;
   /* FULL symmetric entries by variable, row-major (the two-stage Schur assembly): entries of variable v are [foff[v - 1], foff[v]),
    * entry e = (frow[e], fcol[e], fval[e]); the non-empty rows of variable v are the slots [soff[v - 1], soff[v]): slot s is row
    * srow[s] with the entries [sent[s], sent[s + 1]); Tc: nslots x n doubles of workspace, Tc[s][c] = (A_v Zinv)[srow[s]][c] */
   long long  nfull, nslots;
   int*       foff;
   int*       frow;
   int*       fcol;
   double*    fval;
   int*       soff;
   int*       srow;
   int*       sent;
   double*    Tc;
   int        borrowed;    /* 1: every array above belongs to the gather workspace of a triplet master block (sp_master.hip): not freed here */
};
int  hs_sp_prefers_sparse(int n, int m, long long nnz);
int  hs_sp_build(hs_sparse** out, int n, int m, long long nnz, const int* var, const int* row, const int* col, const double* val);
void hs_sp_free(hs_sparse* sp);
long long hs_sp_nnz(const hs_sparse* sp);
int  hs_sp_apply_A(hipStream_t s, const hs_sparse* sp, const double* V, double* out_var1);       /* out[v - 1] = <A_v, V>, v = 1 .. m */
int  hs_sp_apply_AT(hipStream_t s, const hs_sparse* sp, const double* coef, double* out);        /* out += sum_{v >= 1} coef[v] A_v */
int  hs_sp_schur(hipStream_t s, const hs_sparse* sp, const double* X, const double* Zinv, double* Mx);   /* lower triangle, i, j >= 1 */
/* hs_sp_schur with the choice of kernel in the caller's hand (kernel: -1 the engine's rule, 0 one thread per pair, 1 one wavefront
 * per pair) and the kernel that ran in *took (may be NULL) - the unit entries */
int  hs_sp_schur_ex(hipStream_t s, const hs_sparse* sp, const double* X, const double* Zinv, double* Mx, int kernel, int* took);
int  hs_sp_expand(hipStream_t s, const hs_sparse* sp, double* A);

/* ---- sp_master.hip: master copy of a block kept as triplets in ORIGINAL indices, and the gather of a node from it ------- */
struct hs_spm;
int  hs_spm_create(hs_spm** out, int N, int S);
void hs_spm_free(hs_spm* M);
int  hs_spm_size(const hs_spm* M);
int  hs_spm_slots(const hs_spm* M);
/* collects entries on the host (indices checked: HS_ERR_ARG and nothing taken); slot == NULL: all entries belong to `oneslot` */
int  hs_spm_add(hs_spm* M, long long nnz, const int* slot, int oneslot, const int* row, const int* col, const double* val);
/* the complete structure of the node (n kept rows, m variables of which the first nactive are act[a] = slot or -1) in the block's
 * workspace: *out is a borrowed hs_sparse (hs_sp_free releases only the handle).  launches / readbacks are added to. */
int  hs_spm_gather_sparse(hipStream_t s, hs_spm* M, int n, int m, int nactive, const int* act, const int* kept, hs_sparse** out,
   long long* launches, long long* readbacks);
/* A[(a + 1) n^2 ..] = the matrix of slot dact[a] restricted to the kept rows (dinv[N]: new index of an original row, -1 removed),
 * zeros elsewhere; dact, dinv are device-visible: one launch */
int  hs_spm_gather_dense(hipStream_t s, hs_spm* M, int n, int nactive, const int* dact, const int* dinv, double* A, long long* launches);
/* ipm.hip: the device structure of a sparse block of a solver, built if need be (csrc/units.hip: hipsdp_sparse_dump_unit) */
struct hipsdp_solver;
int  hs_solver_sparse_block(struct hipsdp_solver* s, int block, const hs_sparse** sp);

/* ---- ipm.hip: pieces of an iteration's tail that have a unit entry (tests/test_gpu_tail_fusions.py) ------------------ */
struct hs_dir_tail_args { int m, q, K; const int* n; const double* const* B; const double* const* H; const double* beta; const double* hl;
   const double* rhs2; const double* rp; const double* b; double* u1; const double* u2; double* dy; double* dyt; double* sc; double* red_ws;
   const double* dinvm; const double* Lm; double eta, rg, sigmu, tau, kappa, etk; };
int hs_ipm_dir_tail(hipStream_t st, const hs_dir_tail_args* a, int tail, int fuse_solve);
int hs_ipm_after_solve2(hipStream_t st, int m, const double* rhs2, double* u2, double* wt, const double* u1, double* e2, double* e1, int fused);
int hs_ipm_dz_combine(hipStream_t st, long long n2, double* dZ, const double* P2, const double* sc, double eta, const double* Rd);
int hs_ipm_sc_dtau(void);             /* index of dtau in the scalar block */
int hs_ipm_sc_len(int nblocks);       /* doubles of the scalar block */

/* ---- chol.hip ------------------------------------------------------------------------------------------------- */
/* In-place blocked Cholesky of the lower triangle of the row-major n x n matrix A (lda = n): A = L L^T, L stored in the
 * lower triangle (upper triangle is left untouched).  dinv receives the inverses of the 64 x 64 diagonal blocks of L
 * (ceil(n/64) * 64 * 64 doubles; the buffer must hold hs_potrf_dinv_len(n) doubles).  *flag (device int) is set to 1 + index of the first non-positive pivot.
 * diag0 == NULL: strict (definite) mode.  diag0 != NULL (the n original diagonal entries): semidefinite mode, pivots
 * below 1e-13 * diag0[k] are replaced by 1e-13 * diag0[k] and no failure is flagged. */
int hs_potrf(hipStream_t s, int n, double* A, double* dinv, int* flag, const double* diag0);
long long hs_potrf_dinv_len(int n);         /* doubles dinv must hold (inverses + staging blocks of the fused block-column kernel) */
/* set_flag: the (single-launch, n <= 64) factorization stores its result into *flag instead of recording a failure into a
 * cleared flag - for callers where it is the only writer of that flag between two reads */
int hs_potrf_psd(hipStream_t s, int n, double* A, double* dinv, int* flag, const double* diag0, int* regmask, int set_flag);
/* hs_potrf in strict mode for two matrices of the same order (n > 64: one launch per block column serves both; the bits of either are
 * those of hs_potrf alone).  A job: the matrix, its dinv (hs_potrf_dinv_len(n) doubles) and its own failure flag */
struct hs_potrf_job { double* A; double* dinv; int* flag; };
int hs_potrf_pair(hipStream_t s, int n, const hs_potrf_job* jobs);
/* Linv = L^-1 (lower triangular, full n x n storage, upper triangle zero); needs dinv from hs_potrf */
int hs_trtri(hipStream_t s, int n, const double* L, const double* dinv, double* Linv, double* tmp);
/* solves L y = r (nrhs <= 4 right-hand sides, rhs[k * ldr + i]) then optionally L^T x = y, in place.  mode 1: forward only,
 * 2: backward only, 3: both */
/* n <= 64: Cholesky of base + alpha * dir in one launch; optionally stores the matrix (Mout), inv(L) as n x n (Linv) and,
 * for n <= 32, the inverse of the matrix (Gram); L gets a zero upper triangle */
/* the same for two matrices of the same order in one launch (arrays of two) */
int hs_potrf_small_ext_pair(hipStream_t s, int n, double* const* L, double* const* dinv, int* const* flag, const double* const* base,
   const double* const* dir, double alpha, double* const* Mout, double* const* Linv, double* const* Gram, int set_flag);
int hs_potrf_small_ext(hipStream_t s, int n, double* L, double* dinv, int* flag, const double* base, const double* dir, double alpha,
   double* Mout, double* Linv, double* Gram, int set_flag);
/* all blocks n <= 32: the extended Schur matrix (SDP blocks + LP part, symmetric), Lm = Mx[1:, 1:] and its diagonal in one
 * launch; returns 1 if done, 0 if the sizes do not qualify, < 0 on error */
int hs_schur_small(hipStream_t s, int m1, int nblk, const int* n, const double* const* A, const double* const* X,
   const double* const* Zinv, int q, const double* Dext, const double* x, const double* z, double* Mx, double* Lm, double* diagM);
/* mode: 1 forward, 2 backward, 3 both; + 4: every 64-wide diagonal solve x = inv(L_bb) r is corrected once with the factor itself
 * (x += inv(L_bb) (r - L_bb x)), which brings its residual from cond(L_bb) eps |r| down to that of a substitution */
int hs_trsv(hipStream_t s, int n, const double* L, const double* dinv, int nrhs, double* rhs, long long ldr, int mode);
/* the same solve with one workgroup per 64-row block (the blocks hand their parts of the solution over through exchange
 * vectors in sync_ws); sync_ws: hs_trsv_sync_ws(n) ints, put into their initial state by hs_trsv_sync_init once after
 * allocation; *epoch: call counter owned by the caller (hs_trsv_sync_init zeroes it) */
long long hs_trsv_sync_ws(int n);
int hs_trsv_sync_init(hipStream_t s, int n, int* sync_ws, int* epoch);
int hs_trsv_sync(hipStream_t s, int n, const double* L, const double* dinv, int nrhs, double* rhs, long long ldr, int mode,
   int* sync_ws, int* epoch);

/* ---- eig.hip -------------------------------------------------------------------------------------------------- */
/* Lanczos estimate of the smallest eigenvalue of the symmetric n x n matrix W.  res[0] = Ritz value theta,
 * res[1] = residual bound (an eigenvalue lies within res[1] of theta), res[2] = steps used.
 * ws: (maxsteps + 2) * n + 4 * maxsteps + 64 doubles. */
int hs_lanczos_lmin(hipStream_t s, int n, const double* W, int maxsteps, double* res, double* ws);
long long hs_lanczos_ws(int n, int maxsteps);
/* 16 < n <= 64: lambda_min(L0 D0 L0^T), lambda_min(L1 D1 L1^T) by Lanczos with the products, all steps and the tridiagonal
 * problem in one launch */
/* step-length estimates of several small blocks in one launch (eig.hip): all n[j] <= 16 or all in 17 .. 64 */
#define HS_STEP_MAXJOBS 32
struct hs_step_jobs { int nblk; int n[HS_STEP_MAXJOBS]; const double* L0[HS_STEP_MAXJOBS]; const double* D0[HS_STEP_MAXJOBS];
   const double* L1[HS_STEP_MAXJOBS]; const double* D1[HS_STEP_MAXJOBS]; double* res0[HS_STEP_MAXJOBS]; double* res1[HS_STEP_MAXJOBS]; };
int hs_steplen_small_multi(hipStream_t s, const hs_step_jobs* P, int maxsteps);
/* 17 .. 64 rows: the eigenvalue itself (Householder reduction + multisection, eigi.hip) instead of the Lanczos estimate */
int hs_lmin_exact_multi(hipStream_t st, const hs_step_jobs* P);
int hs_lanczos_scaled_small(hipStream_t s, int n, int maxsteps, const double* L0, const double* D0, const double* L1, const double* D1,
   double* res0, double* res1);
int hs_lmin_scaled_tiny(hipStream_t s, int n, const double* L0, const double* D0, const double* L1, const double* D1, double* res0,
   double* res1);
/* rot, dsync (may be NULL: one launch per Lanczos step): two host integers and hs_lanczos_sync_words() device words owned by
 * the caller, put into their initial state by hs_lanczos_sync_reset (after allocation, and again after a run that reported
 * NaN); with them the whole run is one launch whose workgroups hand the product vector over through those words; nwipe: the
 * largest n of all runs that share these words */
int hs_lanczos_lmin2(hipStream_t s, int n, const double* W0, const double* W1, int maxsteps, double* res0, double* res1,
   double* ws0, double* ws1, int* rot, unsigned long long* dsync, int nwipe);
long long hs_lanczos_sync_words(void);
int hs_lanczos_sync_reset(hipStream_t s, unsigned long long* dsync, int* rot);

/* eigi.hip: n <= 128, all eigenpairs in one launch on device buffers (same results as hipsdp_syev_small) */
long long hs_syev_small_scratch(int n);
int hs_syev_small_dev(hipStream_t st, int n, const double* A, double* lam, double* V, double* scratch);
/* the same decompositions for many matrices in at most three launches (see eigi.hip); ws: hs_syev_small_scratch(n) doubles per job */
struct hs_eig_job { int n; int pad; const double* in; double* ws; };
long long hs_syev_many_vecpos(int n);
int hs_syev_many_class(int n);
int hs_syev_small_many(hipStream_t st, int count, const hs_eig_job* hjobs, const hs_eig_job* jobs, int* launches);

/* psd.hip: the PSD projection chain of one matrix on host buffers (arguments and results of hipsdp_psd_project, which is this) */
int hs_psd_project_one(int device, int n, int nnz, const int* row, const int* col, const double* val, double minev,
   double epsilon, int mode, int cap, int* nnz_out, int* rowout, int* colout, double* valout);

/* ---- eigcuts.hip: the separation round of all blocks (hipsdp_eigencuts_all) ------------------------------------------------- */
#define HS_EC_DENSE  0     /* A: (m + 1) rows of n^2 */
#define HS_EC_PACKED 1     /* A: (m + 1) rows of Lp, entry (r, c), c <= r, at r (r + 1) / 2 + c */
#define HS_EC_SPARSE 2     /* A0 dense n x n; the variables' lower-triangular nonzeros by variable and by position (hs_sp_view) */
struct hs_sp_view { long long nnz, npos; const int *voff, *vrow, *vcol; const double* vval; const int *poff, *prow, *pcol, *pvar; const double* pval; };
void hs_sp_get_view(const hs_sparse* sp, hs_sp_view* v);
struct hs_ec_job
{
   int n, form, blk, pad;        /* blk: the block's index in the result arrays */
   long long ld;                 /* n^2 or Lp */
   const double* A;              /* dense / packed rows (row 0 = constant matrix); sparse: the dense constant matrix */
   hs_sp_view sp;
   double* Z;                    /* n x n: Z(y) */
   double* ws;                   /* the slab of the block's decomposition (hs_eig_job.ws) */
   long long vpos;               /* eigenvectors of the decomposition: row k at ws + vpos + k n (hs_syev_many_vecpos) */
   long long vecoff;             /* where the block's vectors start in the result: maxcuts * (rows of the blocks before it) */
};
/* the result block of a call for nb blocks, doubles: ncuts[nb] | lmin[nb] | eigvals[nb maxcuts] | lhs[nb maxcuts] |
 * coefs[nb maxcuts m] | vecs[maxcuts sum n] (written down once for the host side: hs_ec_layout in hs_cut_plan.h) */
int hs_ec_form_z(hipStream_t st, int count, int nmax, int m, const hs_ec_job* jobs, const double* y);
int hs_ec_cuts(hipStream_t st, int count, int nmax, int m, int nb, int maxcuts, double tol, const hs_ec_job* jobs, double* res);

/* ---- eigi.hip: the one-variable SDPs of a block, one workgroup per job (hipsdp_onevar_bounds; host side: onevar.hip) ----------- */
#define HS_OV_MAXN 128
#define HS_OV_TAB 5        /* doubles of a job in the table: variable (0-based engine index), kind, lb, ub, shift u_i */
#define HS_OV_RES 6        /* doubles of a job in the result: status, optval, lmin, grad, evals, 0 */
/* blk != NULL: an entry of a job table in device memory - Z(u) at blk->Z, A_i from the block's storage form; blk == NULL: Z and the
 * dense A + j n^2 of job j are given.  slab: 2 n^2 doubles per job when n > 64 (the dense A_i and M(mu)), else not used. */
struct hs_ov_par
{
   int n, count, maxevals, pad;
   double feastol, infinity;
   const hs_ec_job* blk;
   const double* Z; const double* A;
   const double* tab;            /* [count][HS_OV_TAB] */
   double* slab;
   double* res;                  /* [count][HS_OV_RES] */
};
long long hs_onevar_slab(int n, int count);
int hs_onevar_newton(hipStream_t st, const hs_ov_par* P);
/* ... and of ALL blocks of a solver in one call (hipsdp_onevar_bounds_all): a row of the table carries the job's block and its slot */
#define HS_OVA_TAB 8       /* doubles of a row: the five of HS_OV_TAB, the index of the block's entry in `jobs`, the job's slot in the result, 0 */
#define HS_OV_KIND_EXTREMES 2    /* = HIPSDP_ONEVAR_EXTREMES, in these launches alone: lambda_min and lambda_max of A_i, no Z */
/* one launch of one size class (hs_onevar_all): count rows in workgroup order; jobs: the hs_ec_job table of the blocks (Z(u) at Z, no
 * decomposition slab); nmax: the largest block among the rows; res: job of slot k at res + k HS_OV_RES.  Class 1 (65 to 128 rows): grid
 * workgroups, workgroup w runs the rows w, w + grid, ... in its own slab + w 2 nmax^2. */
struct hs_ova_par
{
   int count, grid, maxevals, nmax;
   double feastol, infinity;
   const hs_ec_job* jobs;
   const double* tab;            /* [count][HS_OVA_TAB] */
   double* slab;
   double* res;
};
int hs_onevar_all(hipStream_t st, int cls, const hs_ova_par* P);
/* ... and of blocks of up to 512 rows as ROUNDS over all jobs (hipsdp_onevar_bounds_large; host side: onevar_large.hip): the eigenpairs
 * come from the batched tridiagonal path of syevx.hip (hs_sxm_job, declared below), and the two launches here stand around it.
 *   hs_onevar_large_form:   M = Z_b(u) + (mu - u_i) A_i (EXTREMES: A_i) of every active job into its hs_sxm_job.A, zeros into .R; the
 *                           point mu is that of ov_begin in round 0, afterwards that of the job's state.
 *   hs_onevar_large_decide: g = v^T A_i v from the block's storage form in a fixed order, the branch of the job (ov_decide /
 *                           ov_extreme), its next point or its row of the result and act = 0; a second launch of one workgroup
 *                           writes to *nactive how many jobs go on (TWO launches).
 * tab: rows of HS_OVA_TAB; state: HS_OVL_STATE doubles per row; act: the flags of hs_sxm_job's launches (the host sets those of round 0:
 * HS_SXM_ACTIVE, | HS_SXM_VEC for NEWTON, | HS_SXM_BOTH for EXTREMES); grid: workgroups per job of the form launch. */
#define HS_OVL_STATE 10
struct hs_sxm_job;
struct hs_ovl_par
{
   int count, maxevals, round, grid;
   double feastol, infinity;
   const hs_ec_job* blocks;
   const double* tab;            /* [count][HS_OVA_TAB] */
   const hs_sxm_job* jobs;       /* [count] */
   int* act;                     /* [count] */
   int* nactive;
   double* state;                /* [count][HS_OVL_STATE] */
   double* res;
};
int hs_onevar_large_form(hipStream_t st, const hs_ovl_par* P);
int hs_onevar_large_decide(hipStream_t st, const hs_ovl_par* P);
/* onevar_large.hip: ONE CHUNK of the call, as hipsdp_onevar_bounds_large and the unit entry (units.hip) run it.  rows: the chunk's jobs
 * by descending n, none of them declined (hs_onevar_large_declined: those never reach the device); entry: the index of the job's
 * block in dblocks, a table in device memory whose first nz entries get their Z(u) formed here (nz = 0: every Z lies there already).
 * hs_onevar_large_plan lays the chunk out (z_len: doubles of all Z of the chunk); the caller then provides dev / pin of L.len.dev_len /
 * L.len.pin_len doubles and the table of blocks with their Z from dev + L.Z on; hs_onevar_large_chunk uploads, runs the rounds and
 * leaves row k's result at pin + L.res + k HS_OV_RES.  cap <= 0: the default number of workgroups per job for this many jobs.
 * launches / readbacks are added to; *rounds: the rounds the chunk took. */
struct hs_ovl_row { int n, var, kind, entry; double lb, ub, shift; };
struct hs_ovl_chunk
{
   int m, count, nz, nzmax, cap, maxevals;
   double feastol, infinity;
   const double* u;
   const hs_ovl_row* rows;
   const hs_ec_job* dblocks;
   double* dev; double* pin;
};
static inline bool hs_onevar_large_declined(int kind, double lb, double ub, double infinity)
{
   return kind != HS_OV_KIND_EXTREMES && (lb <= -infinity || ub >= infinity);
}
long long hs_onevar_large_job_len(int n);
void hs_onevar_large_plan(int m, int count, const hs_ovl_row* rows, long long z_len, hs_ovl_layout* L, std::vector<long long>* ws,
   std::vector<long long>* out);
int hs_onevar_large_chunk(hipStream_t st, const hs_ovl_chunk* c, const hs_ovl_layout& L, const std::vector<long long>& ws,
   const std::vector<long long>& out, long long* launches, long long* readbacks, int* rounds);

/* ---- sparsecuts.hip: sparse eigenvector cuts of all blocks (hipsdp_sparsecuts_all) -------------------------------------------- */
#define HS_SC_MAXN 128
struct hs_sc_par { double tol, feastol, convtol; int maxcuts, maxit; };      /* convtol > 0, maxit >= 1: the defaults are the caller's */
/* hs_sc_out, where the kernels put their results: hs_cut_plan.h, with the layouts of the workspace it points into */
/* one workgroup per job: Z from job.Z, eigenvalues ascending at job.ws (lmin first, maxeig last), v0 at job.ws + job.vpos;
 * sizes[job.blk]: the target sparsity */
int hs_sc_tpower(hipStream_t st, int count, int nmax, const hs_ec_job* jobs, const int* sizes, const hs_sc_par* par, const hs_sc_out* out);
int hs_sc_coefs(hipStream_t st, int count, int m, int maxcuts, const hs_ec_job* jobs, const int* sizes, const hs_sc_out* out);

/* ---- sparsecuts_rounds.hip: the same loop as a sequence of rounds, for the switches recomputesparseev, recomputeinitial, exacttrans --- */
#define HS_SCR_SPARSEEV   1u     /* = HIPSDP_SC_RECOMPUTE_SPARSEEV */
#define HS_SCR_INITIAL    2u     /* = HIPSDP_SC_RECOMPUTE_INITIAL */
#define HS_SCR_EXACTTRANS 4u     /* = HIPSDP_SC_EXACTTRANS */
/* what a block has besides its hs_ec_job (same index in the table): its state between the launches (hs_scr_state, hs_cut_plan.h), the
 * start vector of round 0 (n doubles), and the job of its principal submatrix - Z_S (sizes[blk]^2 doubles, row-major), the slab of
 * that decomposition and where its eigenvectors start in it */
struct hs_scr_job { hs_scr_state* st; double* v0; double* ZS; double* wsS; long long vposS; };
/* round `round` (0: the state is set up from the decomposition in job.ws) of every job: one TPower run and its decision; without
 * HS_SCR_SPARSEEV also the cut, with it the support and Z_S for hs_scr_cut behind the decomposition of the Z_S */
int hs_scr_tpower(hipStream_t st, int count, int nmax, const hs_ec_job* jobs, const hs_scr_job* xjobs, const int* sizes, const hs_sc_par* par,
   unsigned variant, int round, const hs_sc_out* out);
int hs_scr_cut(hipStream_t st, int count, const hs_ec_job* jobs, const hs_scr_job* xjobs, const int* sizes, const hs_sc_par* par,
   const hs_sc_out* out);
/* `launches` empty launches: in place of the classes of a decomposition that have no job, the sequence of a call being a function of
 * (variant, maxcuts) alone */
int hs_scr_pad(hipStream_t st, int launches);

/* ---- sparsecuts_large.hip: the same for ONE block of 129 .. 512 rows (hipsdp_sparsecuts) ---------------------------------------- */
#define HS_SCL_MAXN 512
/* one workgroup: Z (n x n), lmin[0], maxeig[0] and the start vector v0[n] in device memory, MT: n^2 doubles that only this launch
 * touches; the results go to index 0 of out (slots 0 .. maxcuts - 1, vectors from out.vec, supports with pitch out.smax) */
int hs_scl_tpower(hipStream_t st, int n, int size, const double* Z, const double* lmin, const double* maxeig, const double* v0, double* MT,
   const hs_sc_par* par, const hs_sc_out* out);
/* grid (m + 1): x_c^T A_i x_c of every cut of job[0] (its blk and vecoff are 0) in any of the three storage forms */
int hs_scl_coefs(hipStream_t st, int m, int maxcuts, int size, const hs_ec_job* job, const hs_sc_out* out);

/* ---- sparsecuts_large_rounds.hip: the same for ALL blocks of 129 .. 512 rows per launch, switches included (hipsdp_sparsecuts_all_large) --
 * Entry j of the three tables belongs to served block j: jobs[j] its hs_ec_job (Z(y), later the deflated Z, at .Z; .blk its index in the
 * result), sx[j] its job of the batched tridiagonal path (hs_sxm_job: lmin at out[HS_SYEVX_OUT_LAM], the first vector at out +
 * HS_SYEVX_OUT_VEC, maxeig at out2[HS_SYEVX_OUT_LAM]), xjobs[j] what it has besides; act[j]: the flags of hs_syevx_many_* for block j. */
struct hs_sxm_job;
struct hs_sclr_job
{
   hs_scr_state* st; double* v0; double* MT;         /* state between the launches, the start vector of round 0, n^2 doubles for M^T */
   double* ZS; double* wsS; long long vposS;         /* with HS_SCR_SPARSEEV: Z_S, the slab of its decomposition, its eigenvectors in it */
   long long vecoff;                                 /* where the block's vectors start in the result */
};
/* Z of every block with act != 0 into its sx.A in the form the column launches consume (they destroy it), zeros into sx.R; init_zs: the
 * Z_S of every block becomes the identity (in front of round 0 with HS_SCR_SPARSEEV) */
int hs_sclr_stage(hipStream_t st, int count, const hs_ec_job* jobs, const hs_sxm_job* sx, const hs_sclr_job* xjobs, const int* sizes,
   const int* act, int init_zs);
/* variant 0: the whole loop over cuts and iterations of every block in ONE launch, a workgroup of 512 threads per block (the loop of
 * k_sc_tpower_large) */
int hs_sclr_tpower_all(hipStream_t st, int count, int m, const hs_ec_job* jobs, const hs_sxm_job* sx, const hs_sclr_job* xjobs, const int* sizes,
   const hs_sc_par* par, const hs_sc_out* out);
/* variant != 0, round `round` of every block: M^T from the current Z, ONE TPower run, its decision; without HS_SCR_SPARSEEV the cut, with
 * it the support and Z_S for hs_sclr_cut behind the decomposition of the Z_S.  act_on: what act[j] of a block that goes on becomes (a
 * finished block gets 0) */
int hs_sclr_tpower(hipStream_t st, int count, int m, const hs_ec_job* jobs, const hs_sxm_job* sx, const hs_sclr_job* xjobs, const int* sizes,
   const hs_sc_par* par, unsigned variant, int round, int act_on, int* act, const hs_sc_out* out);
int hs_sclr_cut(hipStream_t st, int count, int m, const hs_ec_job* jobs, const hs_sclr_job* xjobs, const int* sizes, const hs_sc_par* par,
   int* act, const hs_sc_out* out);
/* grid (m + 1, count): the coefficients of every cut of every block */
int hs_sclr_coefs(hipStream_t st, int count, int m, int maxcuts, const hs_ec_job* jobs, const hs_sclr_job* xjobs, const int* sizes,
   const hs_sc_out* out);

/* ---- ipm.hip: what the cut calls (cut_calls.hip) and hipsdp_onevar_bounds (onevar.hip) need of a solver, whose definition they do not see --
 * hs_solver_dims: 0 when s is NULL or has no shape, else 1 with the number of variables and blocks; hs_solver_block_n: rows of a block.
 * hs_solver_cut_enter: the device is set, staged entries are flushed, the packed triangles and the device form of blocks kept as
 *    nonzeros are up to date; ids: the blocks whose round runs in the shared launches (the whole matrices on this device, at most 128
 *    rows), ordered by decomposition class - none for a solver with a communicator or sharded matrices.  only >= 0: that block alone,
 *    if it is one of them, and such a solver is not touched at all.
 * hs_solver_cut_prepare: the workspace of the cut calls holds len.dev_len / len.pin_len doubles, and the job tables of a round over ids
 *    (vecoff[block]: where a block's vectors start in the result; Z and decomposition slab of every job from dev + slabs on) are on
 *    the device, uploaded only when they differ from what it holds; nmax: the largest block of the round.
 * hs_solver_cut_rounds: the same for the two further tables of sparsecuts_rounds.hip (fills dxjobs, dsjobs, sjobs of w alone).
 * hs_solver_cut_job: *served = 0 (nothing else done) for a solver with a communicator or sharded matrices or a block without matrices
 *    on this device; else as hs_solver_cut_enter, the workspace holds dev_len / pin_len doubles, and its job table is the block's
 *    hs_ec_job with Z at dev + zoff and ws at dev + wsoff (wsoff < 0: none).
 * hs_solver_cut_blocks: behind hs_solver_cut_enter(s, -1, ..), for a subset `ids` of the blocks it gave, in any order: the workspace
 *    holds dev_len / pin_len doubles, and its job table is their hs_ec_job in that order, Z of ids[j] at dev + zoff[j], no
 *    decomposition slab (hipsdp_onevar_bounds_all); uploaded only when it differs from what the device holds, as every table.
 * hs_solver_eigencuts_block: hipsdp_eigencuts behind its argument checks (maxcuts may be 0), lam0: the block's first eigenvalue. */
struct hipsdp_solver;
struct hs_solver_cut_ws
{
   hipStream_t stream; double* dev; double* pin;
   const hs_ec_job* djobs; const hs_eig_job* dejobs;        /* the tables on the device */
   const hs_eig_job* ejobs;                                 /* the host copy hs_syev_small_many wants, valid until the next prepare */
   const hs_scr_job* dxjobs; const hs_eig_job* dsjobs; const hs_eig_job* sjobs;      /* the same of the rounds */
};
int hs_solver_dims(const hipsdp_solver* s, int* m, int* nblocks);
int hs_solver_block_n(const hipsdp_solver* s, int block);
int hs_solver_cut_enter(hipsdp_solver* s, int only, std::vector<int>* ids);
/* its sibling without the 128-row filter: every block with whole matrices on this device and at most maxn rows, in index order (none
 * for a solver with a communicator or sharded matrices, which is not touched); hs_solver_cut_blocks serves any subset of them too */
int hs_solver_cut_enter_large(hipsdp_solver* s, int maxn, std::vector<int>* ids);
int hs_solver_cut_prepare(hipsdp_solver* s, const std::vector<int>& ids, const std::vector<long long>& vecoff, long long slabs,
   const hs_cut_lens& len, int* nmax, hs_solver_cut_ws* w);
int hs_solver_cut_rounds(hipsdp_solver* s, const std::vector<hs_scr_job>& xjobs, const std::vector<hs_eig_job>& sjobs, hs_solver_cut_ws* w);
int hs_solver_cut_job(hipsdp_solver* s, int block, long long dev_len, long long pin_len, long long zoff, long long wsoff, hs_solver_cut_ws* w,
   int* served);
int hs_solver_cut_blocks(hipsdp_solver* s, const std::vector<int>& ids, const std::vector<long long>& zoff, long long dev_len,
   long long pin_len, hs_solver_cut_ws* w);
int hs_solver_eigencuts_block(hipsdp_solver* s, int block, const double* y, double tol, int maxcuts, int* ncuts, double* eigvals,
   double* coefs, double* lhs, double* vecs, double* lam0);

/* Cyclic Jacobi eigen-decomposition of the symmetric n x n matrix A (destroyed): eigenvalues ascending in lam[n],
 * eigenvectors as rows of V (row k = k-th eigenvector).  info (device int) = sweeps used or -1. */
int hs_syev_jacobi(hipStream_t s, int n, double* A, double* lam, double* V, int* info, double* ws);
long long hs_syev_ws(int n);

/* ---- syevx.hip: selected eigenpairs of a matrix of 2 .. 512 rows without a full decomposition ------------------------------
 * dA: n x n in device memory, the triangle at memory positions [j n + i], i >= j, is read and nothing of it is changed.
 * mode: HS_SYEVX_INDEX (eigenpairs il .. iu, 1-based, at most HS_SYEVX_MAXK of them) or HS_SYEVX_BELOW (those with eigenvalue
 * <= bound, at most maxk <= HS_SYEVX_MAXK), | HS_SYEVX_NOVEC: eigenvalues only, the two vector kernels are not launched.
 * dOut, HS_SYEVX_OUT(n) doubles: [0] pairs returned, [1] eigenvalues <= bound altogether (-1 for an index range),
 * [HS_SYEVX_OUT_LAM + k] k-th returned eigenvalue (ascending), [HS_SYEVX_OUT_VEC + k n + i] component i of its unit vector.
 * ws: hs_syevx_ws(n) doubles.  Everything in stream order on st: n + 1 launches for the values, two more for the vectors. */
#define HS_SYEVX_MAXN 512
#define HS_SYEVX_MAXK 32
#define HS_SYEVX_INDEX 0
#define HS_SYEVX_BELOW 1
#define HS_SYEVX_NOVEC 2
#define HS_SYEVX_OUT_LAM 8
#define HS_SYEVX_OUT_VEC 40
#define HS_SYEVX_OUT(n) (HS_SYEVX_OUT_VEC + (long long) HS_SYEVX_MAXK * (n))
int hs_syevx_dev(hipStream_t st, int n, const double* dA, int mode, int il, int iu, double bound, int maxk, double* dOut, double* ws);
size_t hs_syevx_ws(int n);
/* its first stage alone (the unit entry): d, e, tau (n each) and the reflectors (row j = v_j, entry j + 1 one, zeros before) in ws */
int hs_syevx_tridiag_dev(hipStream_t st, int n, const double* dA, double* ws);
void hs_syevx_tridiag_view(int n, double* ws, double** d, double** e, double** R, double** tau);
/* its stages 2 to 4 alone on the form hs_syevx_tridiag_dev left in ws: the arguments of hs_syevx_dev without the matrix, one launch
 * for the values and two more for the vectors.  Several requests may follow one tridiagonalisation, each with a dOut of its own. */
int hs_syevx_select_dev(hipStream_t st, int n, int mode, int il, int iu, double bound, int maxk, double* dOut, double* ws);
/* the same four stages for MANY matrices per launch (mixed n, 2 .. 512 each): a table of hs_sxm_job in device memory and one int per
 * matrix, act[k] = 0: matrix k takes no part in the launches; else HS_SXM_ACTIVE | HS_SXM_VEC (the unit vector of eigenvalue 1 to
 * out + HS_SYEVX_OUT_VEC) | HS_SXM_BOTH (eigenvalue n as well, to out2[HS_SYEVX_OUT_LAM]); eigenvalue 1 lies at out[HS_SYEVX_OUT_LAM].
 * The caller's own kernel writes the symmetric matrix to A (n x n, no pitch) and zeros to R (n x n) before hs_syevx_many_cols.
 * hs_syevx_many_job fills an entry from the matrix's workspace (hs_syevx_ws(n) doubles) and output (HS_SXM_OUT(n) doubles).
 * hs_syevx_many_cols: nmax - 1 launches (nmax: the largest n of the table; cap: workgroups per matrix at most - the bits do not depend
 * on it; hs_syevx_many_cap(count): the cap the calls use that name none, 4 x compute units / count within 8 .. 128);
 * hs_syevx_many_select: 3 launches (both != 0: some matrix may carry HS_SXM_BOTH).  No launch depends on act. */
#define HS_SXM_ACTIVE 1
#define HS_SXM_VEC    2
#define HS_SXM_BOTH   4
#define HS_SXM_OUT(n) (2 * HS_SYEVX_OUT_VEC + (((long long) (n) + 1) & ~1LL))
struct hs_sxm_job { int n, pad; double* ws; double* A; double* R; double* out; double* out2; };
int hs_syevx_many_job(int n, double* ws, double* out, hs_sxm_job* J);
int hs_syevx_many_cols(hipStream_t st, int count, int nmax, int cap, const hs_sxm_job* djobs, const int* dact);
int hs_syevx_many_cap(int count);
int hs_syevx_many_select(hipStream_t st, int count, int nmax, int both, const hs_sxm_job* djobs, const int* dact);
/* SEVERAL pairs per matrix on the forms hs_syevx_many_cols leaves: the eigenvalues <= bound of every matrix with act != 0, at most maxk
 * <= HS_SYEVX_MAXK of them, ascending, with their unit vectors - to out in the layout of hs_syevx_dev (HS_SYEVX_OUT(n): pairs returned
 * at [0], values from HS_SYEVX_OUT_LAM, vectors from HS_SYEVX_OUT_VEC) - and eigenvalue 1 by index to out2[HS_SYEVX_OUT_LAM].  The bits
 * of a matrix are those of hs_syevx_dev(HS_SYEVX_BELOW) on it alone.  hs_syevx_many_below_job: the entry of hs_syevx_many_job with out
 * of HS_SXB_OUT(n) doubles, out2 behind the selection.  1 launch with maxk == 0 (eigenvalue 1 alone), 3 with maxk > 0. */
#define HS_SXB_OUT(n) (HS_SYEVX_OUT(n) + HS_SYEVX_OUT_VEC)
int hs_syevx_many_below_job(int n, double* ws, double* out, hs_sxm_job* J);
int hs_syevx_many_below(hipStream_t st, int count, int nmax, double bound, int maxk, const hs_sxm_job* djobs, const int* dact);

/* ---- eigcuts_large.hip: the dense eigenvector cuts of ALL blocks of 129 .. 512 rows per launch (hipsdp_eigencuts_all_large) ----------------
 * Entry j of the tables belongs to served block j: jobs[j] its hs_ec_job (.Z is sx[j].A: hs_ec_form_z writes Z(y) where the column
 * launches consume it; .blk its index in the result), sx[j] its job of hs_syevx_many_below, vecoff[j] where its vectors start in the
 * result.  hs_ecl_clear: zeros into the reflector array sx[j].R of every block.  hs_ecl_cuts, grid (m + 1, count) - (1, count) with
 * maxcuts == 0 -: workgroup (i, j) takes the count and the vectors of block j from the selection, sweeps A_i once for all cuts
 * (hs_ec_sweep.h); workgroup (0, j) also stores ncuts, lmin (eigenvalue slot 0 when there is a cut, else out2), eigenvalues, vectors. */
int hs_ecl_clear(hipStream_t st, int count, const hs_sxm_job* sx);
int hs_ecl_cuts(hipStream_t st, int count, int nmax, int m, int maxcuts, const hs_ec_job* jobs, const hs_sxm_job* sx, const long long* vecoff,
   const hs_sc_out* out);

/* ---- check_many.hip: feasibility of MANY candidate points per call (hipsdp_check_y_many; host side: cut_calls.hip) ------------------------
 * A chunk of cc candidates runs in groups of HS_CM_G: Yg[g][i][k] = y_i of candidate g HS_CM_G + k of the chunk (zeros behind the last
 * candidate), so that a group's values of one variable lie side by side.  Entry b of the two device tables belongs to served block b:
 * jobs[b] its hs_ec_job (n and the storage form; .Z and .ws are not used), blks[b] where its matrices and eigenvalues go - Z of candidate
 * c at Z + c zstride (n x n, no pitch), its eigenvalue 1 at lam[c lstride].
 *   hs_cm_form_z: grid (entry tiles, blocks, groups), ONE launch: Z_b(Y[c]) of every block and candidate, one pass over the block's
 *                 storage per group; candidate c's Z has the bits hs_ec_form_z gives for Y[c] alone.
 *   hs_cm_result: grid (cc), ONE launch, the last of a chunk: res[c nblk + b] = eigenvalue 1 of (c, b), and behind those cc nblk values
 *                 res[cc nblk + c] = max(0, max_r (c_r - (D Y[c])_r)) over the q rows of Dext (q x (m + 1), column 0 = c), 0 with q = 0.
 * (eigi.hip) hs_lmin_many_small / hs_lmin_many_mid: eigenvalue 1 of the matrices of the blocks of at most 64 / of 65 .. 128 rows. */
#define HS_CM_G 8
struct hs_cm_blk { double* Z; long long zstride; double* lam; long long lstride; };
int hs_cm_form_z(hipStream_t st, int nblk, int nmax, int m, int cc, const hs_ec_job* jobs, const hs_cm_blk* blks, const double* Yg);
int hs_cm_result(hipStream_t st, int nblk, int cc, int m, int q, const double* Dext, const hs_cm_blk* blks, const double* Yg, double* res);
int hs_lmin_many_small(hipStream_t st, int nblk, int cc, int nmax, const hs_ec_job* jobs, const hs_cm_blk* blks);
int hs_lmin_many_mid(hipStream_t st, int nblk, int cc, int nmax, int grid, const hs_ec_job* jobs, const hs_cm_blk* blks);
/* cut_calls.hip, for the unit entry: hs_cm_form_z alone on a loaded solver - Z of candidate j and block b to Zout + j (n_0^2 + ... +
 * n_{nb-1}^2) + (n_0^2 + ... + n_{b-1}^2) for every block of at most 512 rows the call serves (served[b] = 0, else -1 and its part is not
 * written), *launches: the kernel launches issued */
int hs_check_many_form_z(hipsdp_solver* s, int count, const double* Y, double* Zout, int* served, int* launches);
/* ---- rank1.hip: the rank-1 constraints for MANY candidate points per call (hipsdp_rank1_check_many; host side: cut_calls.hip) ------------
 * The tables of check_many.hip, with blks[b].lam + c lstride the FOUR doubles of hs_lsel_many_small / hs_lsel_many_mid (eigi.hip:
 * eigenvalue 1 with the bits of hs_lmin_many_*, the half width of its interval, eigenvalue max(n - 1, 1), eigenvalue n) for a block of at
 * most 128 rows, and for a larger one out[HS_SYEVX_OUT_LAM] of its hs_sxm_job, which hs_syevx_many_index (syevx.hip) fills.  The result
 * block: HS_R1_RESW doubles per (candidate c, block b) at res + (c nblk + b) HS_R1_RESW - eigenvalues 1, n - 1, n | minorev | minordet |
 * minorind, detind (four ints).
 *   hs_r1_minors: grid (cc, nblk), ONE launch: both scans over the 2 x 2 principal minors of every Z - which must still be intact, so in
 *                 front of hs_syevx_many_cols; writes [3 .. 6] of a row.
 *   hs_r1_result: grid (cc), ONE launch, the last of a chunk: [0 .. 2] of every row (n = 1: value, 0.0, value; n = 2: eigenvalue 1 twice).
 *   hs_r1_minors_unit: the scans on `count` matrices, matrix k of n[k] rows at Z + off[k] (device arrays), o[2 k]: minorev, minordet,
 *                 ind[4 k]: minorind, detind. */
#define HS_R1_RESW 7
int hs_lsel_many_small(hipStream_t st, int nblk, int cc, int nmax, const hs_ec_job* jobs, const hs_cm_blk* blks);
int hs_lsel_many_mid(hipStream_t st, int nblk, int cc, int nmax, int grid, const hs_ec_job* jobs, const hs_cm_blk* blks);
int hs_syevx_many_index(hipStream_t st, int count, int nmax, const hs_sxm_job* djobs, const int* dact);
int hs_r1_minors(hipStream_t st, int nblk, int cc, int nmax, double feastol, const hs_ec_job* jobs, const hs_cm_blk* blks, double* res);
int hs_r1_result(hipStream_t st, int nblk, int cc, const hs_ec_job* jobs, const hs_cm_blk* blks, double* res);
int hs_r1_minors_unit(hipStream_t st, int count, int nmax, const int* n, const long long* off, const double* Z, double feastol, double* o, int* ind);
/* hipsdp_rank1_approx: row j of the table belongs to jobs[j] (hs_ec_job: n, the storage form, A_0) - lam[0]: the eigenvalue, taken times
 * sign (-1: it is eigenvalue 1 of -Z); vec: its unit vector; lmax, vec and rhs of the block go to res_lmax[j], res_vec + voff, res_rhs + roff.
 *   hs_r1_negate: grid (tiles, count), ONE launch: A = -A and R = 0 of every job of the batched tridiagonal path (Z was formed into A).
 *   hs_r1_rhs:    grid (tiles, count), ONE launch: rhs[i (i + 1) / 2 + k] = A_0[i][k] + (lam v_i) v_k, k <= i, every operation rounded on
 *                 its own; A_0 from row 0 of dense rows or packed triangles, or the dense constant matrix of a block kept as nonzeros. */
struct hs_r1a_job { const double* lam; const double* vec; double sign; long long voff, roff; };
int hs_r1_negate(hipStream_t st, int count, int nmax, const hs_sxm_job* sx);
int hs_r1_rhs(hipStream_t st, int count, int nmax, const hs_ec_job* jobs, const hs_r1a_job* tab, double* res_lmax, double* res_vec, double* res_rhs);
/* ipm.hip: the LP rows of a solver - 0 (nothing set) for a solver with a communicator or sharded matrices, else 1, the number of rows and
 * the device array q x (m + 1) whose column 0 is c */
int hs_solver_lp_rows(const hipsdp_solver* s, int* q, const double** Dext);

/* ---- syevr.hip: ALL eigenpairs of a matrix of 2 .. 512 rows through the tridiagonal form (stage 1 is hs_syevx_tridiag_dev) --------
 * dA as for hs_syevx_dev.  dOut, HS_SYEVR_OUT(n) doubles: [k] k-th eigenvalue (ascending), [HS_SYEVR_OUT_VEC(n) + k n + i] component
 * i of its unit vector (vectors != 0; otherwise no vector kernel is launched).  ws: hs_syevr_ws(n) doubles, its head is the
 * workspace of syevx.hip.  Everything in stream order on st: n + 2 launches for the values, 4 + 6 ceil(n / 32) more for the vectors. */
#define HS_SYEVR_OUT_VEC(n) (((long long) (n) + 1) & ~1LL)
#define HS_SYEVR_OUT(n) (HS_SYEVR_OUT_VEC(n) + (long long) (n) * (n))
int hs_syevr_dev(hipStream_t st, int n, const double* dA, int vectors, double* dOut, double* ws);
size_t hs_syevr_ws(int n);
/* its stages 2 and 3 alone (the unit entry) on the d, e that lie in ws (hs_syevx_tridiag_view; e[n - 1] = 0): eigenvalues to
 * dOut[0 .. n - 1], the eigenvectors of the tridiagonal matrix as the rows of the n x n array hs_syevr_tvec_view returns */
int hs_syevr_tvec_dev(hipStream_t st, int n, int vectors, double* dOut, double* ws);
double* hs_syevr_tvec_view(int n, double* ws);
/* its stages 2 to 4 for MANY matrices per launch (mixed n, 2 .. 512 each) on the forms hs_syevx_many_cols leaves: a table of hs_srm_job
 * in device memory, entry k filled by hs_syevr_many_job from the matrix's workspace (hs_syevr_ws(n) doubles; its head is the workspace
 * of the matrix's hs_sxm_job) and its output (HS_SYEVR_OUT(n) doubles, the layout of hs_syevr_dev).  hs_syevr_many_tvec:
 * 5 + 6 ceil(nmax / 32) launches (nmax: the largest n of the table); hs_syevr_many_back: one.  The bits of a matrix are those of
 * hs_syevr_dev on it alone, whatever the table holds beside it. */
struct hs_srm_job { int n, pad; double* d; double* e; double* R; double* tau; double* sr; double* out; };
int hs_syevr_many_job(int n, double* ws, double* out, hs_srm_job* J);
int hs_syevr_many_tvec(hipStream_t st, int count, int nmax, const hs_srm_job* djobs);
int hs_syevr_many_back(hipStream_t st, int count, int nmax, const hs_srm_job* djobs);
/* psd_large.hip, for the unit entry: the three calls above (with hs_syevx_many_cols, `cap` workgroups per matrix) on `count` dense host
 * matrices of 129 .. 512 rows through the calling thread's context of hipsdp_psd_project_many_large; lam and V one matrix behind the other */
int hs_ppl_syevr_many_host(int device, int count, const int* n, const double* A, int cap, double* lam, double* V);

/* ---- psd_many.hip / psd_large.hip: the expand, recombine and packed-write launches of hipsdp_psd_project_many[_large] over a job table in
 * device memory - shared with hipsdp_rounding_frame (the expand launches) and hipsdp_rounding_recombine (the other two, on jobs that
 * point at a solver's rounding frame and at the caller's lambda; minev = -infinity raises no eigenvalue).  nmax: the largest n of the
 * table.  hs_pp_*: jobs of at most 128 rows, one workgroup per job; hs_ppl_*: jobs of 129 .. 512 rows. */
struct hs_pp_job
{
   int n, nnz, cap, pad;
   long long trip;             /* first triplet of the job in the packed arrays */
   double* A;                  /* n x n slab: the matrix, later the upper triangle of the result */
   const double* lam;          /* the decomposition: eigenvalues ascending, row k of V = k-th eigenvector */
   const double* V;
   double minev;
   int* rowoff;                /* n + 1: where the rows start inside the job's result */
};
int hs_pp_expand(hipStream_t st, int count, const hs_pp_job* djobs, const int* row, const int* col, const double* val);
int hs_pp_recombine(hipStream_t st, int count, int nmax, const hs_pp_job* djobs, double eps, int mode, int* dtot);
int hs_pp_write(hipStream_t st, int count, int nmax, const hs_pp_job* djobs, const int* dtot, double eps, long long outlen, int* htot,
   int* orow, int* ocol, double* oval);
struct hs_ppl_job
{
   int n, nnz, cap, ntc;
   long long trip;             /* first triplet of the job in the packed arrays */
   double* A;                  /* n x n, no pitch: the matrix (head of the decomposition's workspace), later the upper triangle of the result */
   double* R;                  /* n x n: the reflector array of the tridiagonalisation */
   const double* lam;          /* the decomposition: eigenvalues ascending, row k of V = k-th eigenvector */
   const double* V;
   double minev;
   int* cnt;                   /* [i ntc + q]: kept entries of row i inside tile column q >= i / 64; from n ntc on [ti ntc + tj]: tile totals */
};
int hs_ppl_expand(hipStream_t st, int count, const hs_ppl_job* djobs, const int* row, const int* col, const double* val);
int hs_ppl_recombine(hipStream_t st, int count, int nmax, const hs_ppl_job* djobs, double eps, int mode);
int hs_ppl_write(hipStream_t st, int count, int nmax, const hs_ppl_job* djobs, double eps, long long outlen, int* tot, int* orow, int* ocol,
   double* oval);

/* ---- rounding.hip: the coefficient table of ALL eigenvectors of every served block (hipsdp_rounding_frame; host side: cut_calls.hip) --------
 * Entry k of the two device tables belongs to served block k of a chunk: ejobs[k] its hs_ec_job (n, storage form, matrices; .Z and .ws
 * are not used), jobs[k] where its pairs come from and go to:
 *   hs_rf_gather        grid (32, count), ONE launch: eigenvalues and vectors from where the decomposition left them into the solver's
 *                       frame (lam, V: row j = v_j), and for a block of the scalar route the transposed copy VT[r n + j] = v_j[r]
 *   hs_rf_coefs_scalar  ONE launch: blocks with route 0 (at most 64 rows, or kept as nonzeros) - thread j owns v_j for matrix i and sums
 *                       over the entries of A_i in storage order, weights hs_rf_weight; no reduction across threads
 *   hs_rf_coefs_mc      ONE launch: blocks with route 1 on v_mfma_f64_16x16x4_f64 - tiles of 64 vectors x 64 matrices over the storage
 *                       index in ascending order, `slices` slices of pps panels each (hs_round_plan.h)
 *                       both write part[(s n + j) (m + 1) + i], i = 0: the constant matrix
 *   hs_rf_store         grid (32, count), ONE launch: eig, obj, coef (the slices added in slice order) and, with vec != NULL, the vectors
 *                       into the chunk's result arrays, rows row0 .. row0 + n - 1 of the block, its vectors from vec0 on
 * nmax, the largest block of the table, and tiles, the most workgroups a block of the matrix-core route has (hs_rf_tiles of
 * hs_round_plan.h; 1 without such a block), size the grids; a block of the other route leaves at once. */
struct hs_rf_job
{
   int n, route, slices, pad;
   long long pps, klen;                /* panels per slice; entries of a stored matrix (matrix-core route) */
   const double* lam_src; const double* V_src;
   double* lam; double* V;             /* the frame */
   double* VT;                         /* scalar route: n x n */
   double* part;                       /* slices x n x (m + 1) */
   long long row0, vec0;
};
int hs_rf_gather(hipStream_t st, int count, const hs_rf_job* jobs);
int hs_rf_coefs_scalar(hipStream_t st, int count, int nmax, int m, const hs_ec_job* ejobs, const hs_rf_job* jobs);
int hs_rf_coefs_mc(hipStream_t st, int count, long long tiles, int m, const hs_ec_job* ejobs, const hs_rf_job* jobs);
int hs_rf_store(hipStream_t st, int count, int m, const hs_rf_job* jobs, double* eig, double* obj, double* coef, double* vec);
/* the three coefficient launches alone (gather, scalar, matrix cores) and a copy of the summed table, for the unit entry
 * hipsdp_rounding_coefs_unit (units.hip): host V (n x n, row j = v_j) and host matrices of ONE block in the form `form` (HS_EC_DENSE:
 * (m + 1) x n^2; HS_EC_PACKED: (m + 1) x n (n + 1) / 2; HS_EC_SPARSE: A = the dense constant matrix, the variables' lower-triangular
 * nonzeros as nnz triplets (var 1 .. m, row >= col, val) sorted by variable), through the routing rule of the call; out: n x (m + 1),
 * out[j (m + 1) + i] = v_j^T A_i v_j; *route, *slices: what the rule chose */
int hs_rf_coefs_host(int device, int n, int m, int form, const double* V, const double* A, long long nnz, const int* var, const int* row,
   const int* col, const double* val, double* out, int* route, int* slices);

/* ipm.hip: the rounding frame of a solver - a grow-only device allocation of N + sum n_b^2 doubles (eigenvalues of block b at off[b],
 * its vectors at N + voff[b]), valid from a hipsdp_rounding_frame that returned HIPSDP_OK until the next one, hipsdp_set_shape* or
 * hipsdp_free; served[b] = 0: the frame holds block b.  hs_solver_round_frame: the solver's frame, grown to `need` doubles when
 * need > 0 (the device is set by the caller: hs_solver_cut_enter_large / hs_solver_cut_plain).  hs_solver_cut_plain: the device is set
 * and the cut workspace holds dev_len / pin_len doubles - no table, no matrix is looked at. */
struct hs_round_frame { double* dev = NULL; long long len = 0; int valid = 0; std::vector<int> served; };
int hs_solver_round_frame(hipsdp_solver* s, long long need, hs_round_frame** frame);
int hs_solver_cut_plain(hipsdp_solver* s, long long dev_len, long long pin_len, hs_solver_cut_ws* w);
/* the storage form (HS_EC_*) the job tables of hs_solver_cut_blocks name for the block, behind hs_solver_cut_enter[_large] */
int hs_solver_block_form(const hipsdp_solver* s, int block);

/* ---- solve1.hip: a whole node solve of a B&B-sized problem in one launch of one workgroup ------------------------------- */
#define HS_S1_MAXBLK 8
/* termination status written to out[0]: the HIPSDP_STATUS_* values of include/hipsdp.h, or -2: declined (too much work for one
 * compute unit, or the workspace is too small) - nothing was solved, the caller takes the general path */
#define HS_S1_OPTIMAL 0
#define HS_S1_DINF 1
#define HS_S1_DUNB 2
#define HS_S1_PDINF 3
#define HS_S1_ITERLIM 4
#define HS_S1_NUMERIC 5
#define HS_S1_TIMELIM 6
#define HS_S1_OBJLIM 7
#define HS_S1_OUT_DOUBLES 64
/* ---- the deferred setters of a node (csrc/ipm.hip: stage_*, flush_cmds): commands in pinned memory, run in order by one workgroup -
 * the first thing the one-launch solve does, or a launch of their own before anything else touches the device data */
enum { NC_ZERO = 1, NC_COPY = 2, NC_GATHER = 3, NC_SCATTER = 4 };
struct NodeCmd
{
   int op, i0, i1, i2, i3, i4, pad0, pad1;
   long long n;
   double* dst;                 /* ZERO, COPY: destination; GATHER, SCATTER: the block's matrices */
   double* dst2;                /* SCATTER: the constant matrix */
   const double* src;           /* COPY: data; GATHER: master copy; SCATTER: values */
   const int* idx;              /* GATHER: active slots then kept indices; SCATTER: var, row, col */
   long long pad2;
};
#define NC_MAX 48
#define NC_BYTES (NC_MAX * sizeof(NodeCmd))
#define NC_LIMIT 65536           /* elements a deferred command may touch */
#ifdef __HIPCC__
/* all threads of ONE workgroup; sc: NC_MAX commands of LDS.  stage != NULL: `staged` bytes (a multiple of 16) of LDS that take the
 * first `staged` bytes of the arena - the command list and everything the commands read from pinned memory - in ONE pipelined pass
 * over PCIe; the commands then read their data and index arrays out of LDS.  (Read where the commands use them, every element is a
 * PCIe round trip of its own in a chain per thread - the gather reads three indices per entry -: 12 us for the six commands of a
 * node of example_TT, 4 us this way.)  sc is not used then. */
__device__ __forceinline__ void hs_run_node_cmds(const NodeCmd* __restrict__ cmds, int ncmd, NodeCmd* sc, double* stage = NULL, long long staged = 0)
{
   const char* const arena = reinterpret_cast<const char*>(cmds);
   if ( stage != NULL )
   {
      typedef double nc_v2 __attribute__((ext_vector_type(2)));
      const nc_v2* src = reinterpret_cast<const nc_v2*>(cmds);
      nc_v2* dst = reinterpret_cast<nc_v2*>(stage);
      const int n16 = (int) (staged >> 4);
      for (int b = threadIdx.x; b < n16; b += 4 * blockDim.x)
      {
         nc_v2 v[4];
#pragma unroll
         for (int u = 0; u < 4; ++u)
         {
            const int i = b + u * (int) blockDim.x;
            v[u] = src[i < n16 ? i : n16 - 1];
         }
#pragma unroll
         for (int u = 0; u < 4; ++u)
         {
            const int i = b + u * (int) blockDim.x;
            if ( i < n16 )
               dst[i] = v[u];
         }
      }
      sc = reinterpret_cast<NodeCmd*>(stage);
   }
   else
   {
      const long long* src = reinterpret_cast<const long long*>(cmds);
      long long* dst = reinterpret_cast<long long*>(sc);
      const int words = ncmd * (int) (sizeof(NodeCmd) / sizeof(long long));
      for (int i = threadIdx.x; i < words; i += blockDim.x)
         dst[i] = src[i];
   }
   __syncthreads();
   /* an address inside the staged part of the arena -> its copy in LDS */
   auto loc = [&](const void* p) -> const void*
   {
      const char* c = reinterpret_cast<const char*>(p);
      if ( stage != NULL && c >= arena && c < arena + staged )
         return reinterpret_cast<const char*>(stage) + (c - arena);
      return p;
   };
   for (int c = 0; c < ncmd; ++c)
   {
      const NodeCmd& q = sc[c];
      if ( q.op == NC_ZERO )
      {
         for (long long e = threadIdx.x; e < q.n; e += blockDim.x)
            q.dst[e] = 0.0;
      }
      else if ( q.op == NC_COPY )
      {
         const double* src = reinterpret_cast<const double*>(loc(q.src));
         for (long long e = threadIdx.x; e < q.n; e += blockDim.x)
            q.dst[e] = src[e];
      }
      else if ( q.op == NC_GATHER )
      {
         /* (k_master_gather) i0 = active variables, i1 = kept rows, i2 = order of the master matrices */
         const int nactive = q.i0, nk = q.i1, N = q.i2;
         const int* act = reinterpret_cast<const int*>(loc(q.idx)); const int* kept = act + nactive;
         const long long nk2 = (long long) nk * nk, total = (long long) nactive * nk2;
         for (long long e = threadIdx.x; e < total; e += blockDim.x)
         {
            const long long a = e / nk2;
            const long long rc = e - a * nk2;
            const int r = (int) (rc / nk), cc = (int) (rc - (long long) r * nk);
            q.dst[(a + 1) * nk2 + rc] = act[a] >= 0 ? q.src[((long long) act[a] * N + kept[r]) * N + kept[cc]] : 0.0;
         }
      }
      else if ( q.op == NC_SCATTER )
      {
         /* (k_scatter_coo, indices checked by the host) i0 = order of the block, i1, i2 = the rows of A this rank holds */
         const int n = q.i0, r0 = q.i1, r1 = q.i2;
         const long long n2 = (long long) n * n;
         const int* var = reinterpret_cast<const int*>(loc(q.idx)); const int* row = var + q.n; const int* col = var + 2 * q.n;
         const double* val = reinterpret_cast<const double*>(loc(q.src));
         for (long long e = threadIdx.x; e < q.n; e += blockDim.x)
         {
            const int v = var[e], r = row[e], cc = col[e];
            if ( v != 0 && (v < r0 || v >= r1) )
               continue;
            double* a = (v == 0) ? q.dst2 : q.dst + (long long) v * n2;
            a[(long long) r * n + cc] = val[e];
            a[(long long) cc * n + r] = val[e];
         }
      }
      __syncthreads();
   }
}
#endif

#ifdef __HIPCC__
#include "hs_wave.h"

/* ---- one wavefront: x = (L L^T)^-1 r for a single-block factor (m <= 64) in the ORACLE's order (oracle/ipm_ref.py: msolve) - forward
 * substitution, one correction with the factor itself, backward substitution, one correction - where the default multiplies by an
 * explicitly inverted factor (with the same corrections).  An option (HIPSDP_SMALL_SOLVE=subst, kernels.hip:
 * hs_small_solve_by_substitution), built in round 6 to test whether the inverted blocks are why the general path parts from the oracle
 * on singular Schur complements; they are not.
 * sL: LDS image of L, row i at sL + 65 i (entries j <= i valid, the diagonal included); lane = row; r, result: this lane's entry. */
__device__ __forceinline__ double hs_wl_fwd(const double* sL, int m, int lane, double di, double x)
{
   const bool live = lane < m;
   const double* row = sL + (live ? lane : 0) * 65;
   double a = live ? x : 0.0;
   for (int k = 0; k < m; ++k)
   {
      const double y = hs_lane(a * di, k);
      const double c = row[k];
      if ( live && lane > k )
         a = fma(-c, y, a);
   }
   return a * di;
}
__device__ __forceinline__ double hs_wl_bwd(const double* sL, int m, int lane, double di, double x)
{
   const bool live = lane < m;
   const int col = live ? lane : 0;
   double a = live ? x : 0.0;
   for (int k = m - 1; k >= 0; --k)
   {
      const double y = hs_lane(a * di, k);
      const double c = sL[k * 65 + col];
      if ( live && lane < k )
         a = fma(-c, y, a);
   }
   return a * di;
}
/* (L w)_lane and (L^T v)_lane */
__device__ __forceinline__ double hs_wl_mulL(const double* sL, int m, int lane, double w)
{
   const bool live = lane < m;
   const double* row = sL + (live ? lane : 0) * 65;
   double acc = 0.0;
   for (int j = 0; j < m; ++j)
   {
      const double wj = hs_lane(w, j);
      const double c = row[j];
      if ( live && j <= lane )
         acc = fma(c, wj, acc);
   }
   return acc;
}
__device__ __forceinline__ double hs_wl_mulLt(const double* sL, int m, int lane, double v)
{
   const bool live = lane < m;
   const int col = live ? lane : 0;
   double acc = 0.0;
   for (int j = 0; j < m; ++j)
   {
      const double vj = hs_lane(v, j);
      const double c = sL[j * 65 + col];
      if ( live && j >= lane )
         acc = fma(c, vj, acc);
   }
   return acc;
}
/* the same for 64 < m <= 128: two rows per lane (lane and lane + 64), L at pitch P (odd) in LDS; x[0], x[1]: this lane's two entries */
template<int P>
__device__ __forceinline__ void hs_wl2_fwd(const double* sL, int m, int lane, const double (&di)[2], double (&a)[2])
{
   const int r0 = lane, r1 = lane + 64;
   const bool l1 = r1 < m;
   const double* row0 = sL + r0 * P;
   const double* row1 = sL + (l1 ? r1 : 0) * P;
   for (int k = 0; k < m; ++k)
   {
      const double y = (k < 64) ? hs_lane(a[0] * di[0], k) : hs_lane(a[1] * di[1], k - 64);
      const double c0 = row0[k], c1 = row1[k];
      if ( r0 > k ) a[0] = fma(-c0, y, a[0]);
      if ( l1 && r1 > k ) a[1] = fma(-c1, y, a[1]);
   }
   a[0] *= di[0]; a[1] *= di[1];
}
template<int P>
__device__ __forceinline__ void hs_wl2_bwd(const double* sL, int m, int lane, const double (&di)[2], double (&a)[2])
{
   const int r0 = lane, r1 = lane + 64;
   const bool l1 = r1 < m;
   const int c1col = l1 ? r1 : 0;
   for (int k = m - 1; k >= 0; --k)
   {
      const double y = (k < 64) ? hs_lane(a[0] * di[0], k) : hs_lane(a[1] * di[1], k - 64);
      const double c0 = sL[k * P + r0], c1 = sL[k * P + c1col];
      if ( r0 < k ) a[0] = fma(-c0, y, a[0]);
      if ( l1 && r1 < k ) a[1] = fma(-c1, y, a[1]);
   }
   a[0] *= di[0]; a[1] *= di[1];
}
template<int P, bool TRANS>
__device__ __forceinline__ void hs_wl2_mul(const double* sL, int m, int lane, const double (&w)[2], double (&out)[2])
{
   const int r0 = lane, r1 = lane + 64;
   const bool l1 = r1 < m;
   const int q1 = l1 ? r1 : 0;
   double s0 = 0.0, s1 = 0.0;
   for (int j = 0; j < m; ++j)
   {
      const double wj = (j < 64) ? hs_lane(w[0], j) : hs_lane(w[1], j - 64);
      const double c0 = TRANS ? sL[j * P + r0] : sL[r0 * P + j];
      const double c1 = TRANS ? sL[j * P + q1] : sL[q1 * P + j];
      if ( TRANS ? j >= r0 : j <= r0 ) s0 = fma(c0, wj, s0);
      if ( l1 && (TRANS ? j >= r1 : j <= r1) ) s1 = fma(c1, wj, s1);
   }
   out[0] = s0; out[1] = s1;
}
/* sL must hold zeros above the diagonal (the transposed accesses of rows past a lane's own are masked, the others read them) */
template<int P>
__device__ __forceinline__ void hs_wl2_msolve(const double* sL, int m, int lane, double (&x)[2])
{
   const int r1 = lane + 64;
   double di[2] = {1.0 / sL[lane * P + lane], r1 < m ? 1.0 / sL[r1 * P + r1] : 0.0};
   double r[2] = {x[0], r1 < m ? x[1] : 0.0}, w[2] = {r[0], r[1]}, t[2], c[2];
   hs_wl2_fwd<P>(sL, m, lane, di, w);
   hs_wl2_mul<P, false>(sL, m, lane, w, t);
   c[0] = r[0] - t[0]; c[1] = r[1] - t[1];
   hs_wl2_fwd<P>(sL, m, lane, di, c);
   w[0] += c[0]; w[1] += c[1];
   double v[2] = {w[0], w[1]};
   hs_wl2_bwd<P>(sL, m, lane, di, v);
   hs_wl2_mul<P, true>(sL, m, lane, v, t);
   c[0] = w[0] - t[0]; c[1] = w[1] - t[1];
   hs_wl2_bwd<P>(sL, m, lane, di, c);
   x[0] = v[0] + c[0]; x[1] = v[1] + c[1];
}
__device__ __forceinline__ double hs_wl_msolve(const double* sL, int m, int lane, double r)
{
   const double di = lane < m ? 1.0 / sL[lane * 65 + lane] : 0.0;
   double w = hs_wl_fwd(sL, m, lane, di, r);
   w += hs_wl_fwd(sL, m, lane, di, r - hs_wl_mulL(sL, m, lane, w));
   double v = hs_wl_bwd(sL, m, lane, di, w);
   v += hs_wl_bwd(sL, m, lane, di, w - hs_wl_mulLt(sL, m, lane, v));
   return v;
}
#endif

struct hs_solve1_args
{
   int m, q, nblk;
   int n[HS_S1_MAXBLK];
   const double* A[HS_S1_MAXBLK];          /* dense (m + 1) x n^2 rows */
   double* X[HS_S1_MAXBLK];                /* n x n: start point in (have_start), final iterate out (unscaled) */
   double* Z[HS_S1_MAXBLK];
   double* Xpre[HS_S1_MAXBLK];             /* preoptimal iterate (preoptgap > 0) */
   const double* b; const double* Dext;
   double *y, *x, *z, *pre_y, *pre_x;
   const void* cmds; int ncmd;         /* deferred setters of the node (NodeCmd list in pinned memory), run before anything else */
   long long cmd_bytes;                /* bytes of the arena behind cmds that hold the list and the data of its commands (multiple of 16) */
   double *hy, *hx, *hz;               /* optional: y, x, z once more into pinned host memory (the caller's read-backs of a node need no copy) */
   double gaptol, feastol, infeastol, objlimit, timelimit, gamma, pabstol, preoptgap;
   double elapsed0;                        /* seconds of the time limit already used when the kernel starts */
   double maxwork;                         /* decline above this many multiply-adds per Schur assembly */
   int maxiter, settings, have_start, pivot_rule, prof_on, hist_len;
   int keep_on_fail;                       /* 1: on a numerical failure leave y, x, z, X, Z as they were handed in (the general path retries from them) */
   double* gws; long long gws_len;         /* workspace in device memory (hs_solve1_ws_doubles) */
   double* out;                            /* HS_S1_OUT_DOUBLES result scalars (device-visible; pinned host memory works) */
   double* hist;                           /* optional: 16 doubles per iteration (tests, tools) */
   unsigned long long seq; unsigned long long* flag;   /* when flag != NULL: *flag = seq once out[] is complete */
};
/* the parameter of the one-launch kernel (csrc/solve1_body.h): the arguments by value, or in the instances of hipsdp_solve_many
 * (S1_MANY, csrc/solve1_*_many.hip) an array of them in device memory, one per workgroup, bound by reference - read where they are
 * used, like kernel arguments, with no copy of the struct into registers.  (Defined here rather than in solve1_body.h: the kernel
 * reports the line of a numerical failure in its results, so the lines of that file stay where they are.) */
#ifdef S1_MANY
#define S1_PARAMS const hs_solve1_args* __restrict__ PA
#define S1_BIND_P const hs_solve1_args& P = PA[blockIdx.x];
#else
#define S1_PARAMS const hs_solve1_args P
#define S1_BIND_P
#endif
int hs_small_solve_by_substitution(void);
/* k_solve2_small (ipm.hip), m <= 64: rhs2 = [g ; b] with g = Mx[0, 1:], both solved with the single-block factor (dinv = inv(L) as 64 x 64,
 * L as m x m), then u2 = rhs2[m:] - rhs2[:m] and wt = [1, -rhs2[:m]]; subst: hs_small_solve_by_substitution() */
int hs_solve2_small(hipStream_t st, int m, const double* Mx, const double* b, const double* dinv, const double* L, double* rhs2, double* u2,
   double* wt, int subst);
int hs_solve1_fits(int m, int q, int nblk, const int* n);
long long hs_solve1_ws_doubles(int m, int q, int nblk, const int* n);
int hs_solve1_launch(hipStream_t st, const hs_solve1_args* a);
int hs_solve1_class(const hs_solve1_args* a);
int hs_solve1_launch_many(hipStream_t st, int cls, const hs_solve1_args* dev_args, int count);
int hs_solve1_debug_counts(unsigned int* out2);

/* ---- the lanes of hipsdp_solve_objectives (csrc/ipm.hip): one loaded problem, one lane per objective.  A lane holds, in device memory
 * and in this order, b[m], y[m], x[q], z[q] and X_k, Z_k (n_k x n_k) of every block; every array starts at an even offset (16 bytes)
 * and is followed by `gap` doubles (even; 0 in the engine, guard words in the unit test).  hs_objs_lane_layout writes the 4 + 2 nblk
 * offsets and returns the length of a lane (even). */
#define HS_FAN_MAXSEG (4 + 2 * HS_S1_MAXBLK)
long long hs_objs_lane_layout(int m, int q, int nblk, const int* n, int gap, long long* off);
/* the fan-out (csrc/kernels.hip): segment i of lane j is len doubles at lanes + j lane_stride + dst, copied from src0 for lane 0 (the
 * home lane: the solver's own objective and start point, kept for the jobs the general path solves later) and from src + (j - 1) stride
 * for the lanes of the jobs (stride 0: the same start point for all).  Every address is a multiple of 16 bytes.  ONE launch over
 * (lane, segment), 16-byte loads and stores, one 8-byte copy more where len is odd; it copies and does nothing else. */
struct hs_fan_seg { const double* src0; const double* src; long long stride, dst, len; };
struct hs_fan_plan { int nseg; hs_fan_seg seg[HS_FAN_MAXSEG]; };
int hs_objs_fanout(hipStream_t st, const hs_fan_plan* plan, double* lanes, long long lane_stride, int nlanes);

#endif
