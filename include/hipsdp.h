/* hipsdp.h - C ABI of the MI355X interior-point engine (libhipsdp.so).
 *
 * This is the layer UNDER the SCIP-SDP solver interface: src/sdpi/sdpisolver_hip.c (the drop-in for the reference's
 * src/sdpi/sdpisolver_{dsdp,sdpa,mosek}.c, see include/sdpisolver_hip.h) marshals the arguments of
 * SCIPsdpiSolverLoadAndSolveWithPenalty (reference: src/sdpi/sdpisolver.h:258-322) into the calls below, exactly where
 * the reference backends call DSDPCreate/SDPConeSetASparseVecMat/LPConeSetData2/DSDPSolve/DSDPComputeX
 * (src/sdpi/sdpisolver_dsdp.c:983-1520) or SDPA::inputElement/initializeSolve/solve
 * (src/sdpi/sdpisolver_sdpa.cpp:1179-1670).  Plain C types only; no torch, no C++ in the signatures.
 *
 * Problem handed to the engine (all fixings / index compaction already applied by the caller):
 *
 *    min  b^T y   s.t.  sum_i A_i^k y_i - A_0^k  psd  (k = 0..nblocks-1),    D y - c >= 0  (q rows)
 *
 * All functions return 0 (HIPSDP_OK) or an HIPSDP_ERR_* code; hipsdp_last_error() gives a message.
 * There is NO CPU fallback: without a usable gfx950 device every computing call returns HIPSDP_ERR_NODEVICE.
 */
#ifndef HIPSDP_H
#define HIPSDP_H

#ifdef __cplusplus
extern "C" {
#endif

/* libhipsdp.so is built with hidden visibility: only what this header declares is exported */
#define HIPSDP_API __attribute__((visibility("default")))

#define HIPSDP_OK             0
#define HIPSDP_ERR_NODEVICE   1
#define HIPSDP_ERR_HIP        2
#define HIPSDP_ERR_ARG        3
#define HIPSDP_ERR_NOMEM      4
#define HIPSDP_ERR_NUMERIC    5

/* termination status of hipsdp_solve (hipsdp_info.status) */
#define HIPSDP_STATUS_OPTIMAL   0    /* both problems feasible, tolerances met */
#define HIPSDP_STATUS_DINF      1    /* the y-problem ("dual" in SCIP-SDP terms) is infeasible: X-ray found */
#define HIPSDP_STATUS_DUNB      2    /* the y-problem is unbounded / the X-problem infeasible: y-ray found */
#define HIPSDP_STATUS_PDINF     3    /* both certificates */
#define HIPSDP_STATUS_ITERLIM   4
#define HIPSDP_STATUS_NUMERIC   5    /* stalled / factorization failure */
#define HIPSDP_STATUS_TIMELIM   6
#define HIPSDP_STATUS_OBJLIM    7    /* the X-problem objective (a lower bound) exceeded the objective limit */
#define HIPSDP_STATUS_UNSOLVED -1

typedef struct hipsdp_solver hipsdp_solver;

typedef struct hipsdp_params
{
   double gaptol;        /* absolute duality gap tolerance            (SCIP_SDPPAR_GAPTOL, type_sdpi.h:50) */
   double feastol;       /* absolute feasibility tolerance of y        (SCIP_SDPPAR_SDPSOLVERFEASTOL, type_sdpi.h:52) */
   double infeastol;     /* relative tolerance of Farkas certificates */
   double objlimit;      /* stop when the lower bound exceeds this; >= 1e20: off (SCIP_SDPPAR_OBJLIMIT, type_sdpi.h:53) */
   double timelimit;     /* seconds for this call; <= 0: off */
   double gamma;         /* fraction of the step to the boundary */
   double ws_gbytes;     /* workspace budget of the Schur assembly in GB; <= 0: default */
   int    maxiter;
   int    verbose;       /* 1: one line per iteration on stdout (SCIP_SDPPAR_SDPINFO) */
   int    lanczos_steps; /* Lanczos steps per step-length estimate; 0 (default): 24, or 16 when every block has > 64 rows */
   int    settings;      /* conservativeness of the iteration, the backend's retry ladder (SCIP_SDPSOLVERSETTING, type_sdpi.h:69-77;
                          * sdpisolver_sdpa.cpp:1415-1449, 1698-1795): 0 fast (default), 1 medium (step fraction <= 0.9, twice the
                          * Lanczos steps, more patient stall tests, centrality floor 1e-4), 2 stable (step fraction <= 0.75, four
                          * times the Lanczos steps, even more patient, centrality floor 1e-2) */
   double pabstol;       /* > 0: optimal termination also needs ||b - A(X)||_2 <= pabstol, ABSOLUTE: the caller's own check of
                          * the X-side is absolute (sdpsolchecker.c:775-931 with SCIP_SDPPAR_FEASTOL) while pinf is relative */
   double preoptgap;     /* > 0: the first iterate that is feasible to feastol with relative gap
                          * gap / (1 + |pobj| / 2 + |dobj| / 2) < preoptgap is kept as "preoptimal solution"
                          * (SCIP_SDPPAR_WARMSTARTPOGAP, type_sdpi.h:61; capture rule of sdpisolver_dsdp.c:323-358) */
} hipsdp_params;

typedef struct hipsdp_info
{
   int    status;
   int    iterations;
   double pobj;          /* sum_k <A_0^k, X_k> + c^T x   (X-problem, lower bound when feasible) */
   double dobj;          /* b^T y */
   double pinf;          /* ||b - A(X)|| / (1 + ||b||) */
   double dinf;          /* ||A^T y - A_0 - Z|| / (1 + ||A_0||) */
   double dabs;          /* max_k ||A^T y - A_0 - Z||_F : absolute violation bound of y */
   double gap;           /* |pobj - dobj| */
   double mu;
   double tau, kappa;
   double solve_seconds;    /* wall time of hipsdp_solve */
   double schur_seconds;    /* device time spent in the Schur assembly (sum of HIP event intervals) */
   double schur_flops;      /* algorithmic flops of the assemblies: (4 m1 n^3 + m1^2 n^2) per block and iteration */
   int    schur_calls;      /* assemblies, one per iteration.  A first assembly taken from the cold-start store (hipsdp_gram_cache_stats)
                             * counts as a call - its copy's time is in schur_seconds - and adds nothing to schur_flops or
                             * schur_flops_executed: no matrix-core flops ran for it */
   int    chol_fail;        /* number of step halvings forced by a failed Cholesky */
   int    warm_started;     /* 1: the point given with hipsdp_set_start was interior and has been used */
   int    settings_used;    /* the hipsdp_params.settings this solve ran with */
   double schur_flops_executed; /* FP64 matrix-core flops the assemblies' GEMM launches were ISSUED (whole tiles over the K ranges
                                 * actually walked: triangular factors, lower tiles, skipped zero slabs) - what MFMA utilisation is
                                 * measured against; schur_flops is the algorithmic count */
} hipsdp_info;

HIPSDP_API const char* hipsdp_last_error(void);
HIPSDP_API const char* hipsdp_version(void);
HIPSDP_API int  hipsdp_device_count(void);
HIPSDP_API void hipsdp_default_params(hipsdp_params* p);

HIPSDP_API int  hipsdp_create(hipsdp_solver** solver, int device);
HIPSDP_API void hipsdp_free(hipsdp_solver** solver);

/* Declares the shape: m variables, nblocks dense SDP blocks of the given sizes, q LP rows.  Allocates the device storage
 * A_k[(m+1) x n_k^2] (row i = vec(A_i), row 0 = constant matrix), zero filled. */
HIPSDP_API int  hipsdp_set_shape(hipsdp_solver* solver, int m, int nblocks, const int* blocksizes, int q);
/* The same with the number of lower-triangular triplets the caller is going to add per block (nnz[k] >= 0; NULL or a negative
 * entry: unknown).  A block whose count makes the pair formula over nonzeros the cheaper Schur assembly (4 (sum nnz)^2 multiply-adds
 * against 4 (m + 1) n^3 + (m + 1)^2 n^2; never for n <= 64) is kept SPARSE: no (m + 1) x n^2 array is allocated, the matrices of the
 * variables stay the triplets of hipsdp_add_entries (what the reference backends hand DSDP / SDPA:
 * sdpisolver_dsdp.c:1126-1195, sdpisolver_sdpa.cpp:1223-1267), the constant matrix a dense n x n array.  Such a block takes
 * hipsdp_add_entries, or hipsdp_master_gather from a master block kept as triplets (hipsdp_master_define2), not
 * hipsdp_set_block_dense / hipsdp_master_gather from a dense master block / hipsdp_gen_planted. */
HIPSDP_API int  hipsdp_set_shape2(hipsdp_solver* solver, int m, int nblocks, const int* blocksizes, int q, const long long* nnz);
HIPSDP_API int  hipsdp_block_is_sparse(hipsdp_solver* solver, int block);
/* 0: never keep a block as nonzeros, 1 (default; environment HIPSDP_SPARSE): by the cost rule above, 2: whenever a count is given */
HIPSDP_API int  hipsdp_sparse_policy(hipsdp_solver* solver, int mode);
/* how many (kernel, device) pairs have had their dynamic-LDS limit raised on that device so far: the attribute
 * (hipFuncAttributeMaxDynamicSharedMemorySize) belongs to the pair, the engine keeps one bit per device and kernel (tests) */
HIPSDP_API int  hipsdp_func_attr_sets(int device);
/* free and total bytes of the device's memory (tests: what a problem allocates) */
HIPSDP_API int  hipsdp_mem_info(int device, double* free_bytes, double* total_bytes);
/* objective b[m] (host) */
HIPSDP_API int  hipsdp_set_obj(hipsdp_solver* solver, const double* b);
/* Scatter lower-triangular COO entries (row >= col) into block k: entry e belongs to matrix var[e] (0 = constant matrix,
 * i = variable i, 1-based) at (row[e], col[e]); both triangles of the dense storage are written.  Host arrays.  An entry with
 * row < col stands for its mirror position.  A position named more than once in one call keeps its LAST entry, in a block kept as
 * nonzeros and - for calls of at most 16384 entries, which are checked on the host - in dense storage alike; a larger call into
 * dense storage is scattered by the device in no order and must name every position once. */
HIPSDP_API int  hipsdp_add_entries(hipsdp_solver* solver, int block, long long nnz, const int* var, const int* row, const int* col,
   const double* val);
/* Master copy (optional, for callers that solve many nodes of one problem): the matrices of the variables in ORIGINAL block
 * sizes are uploaded once (COO, lower triangle) and stay in HBM across hipsdp_set_shape calls.  Block b has nblockvars[b] slots,
 * one per variable that appears in it (nblockvars == NULL: nvars slots per block); entries name their slot.  A node's compact
 * block is then filled on the device:  A_engine[a + 1][r][c] = master[slots[a]][kept[r]][kept[c]]  (slots[a] = -1: the
 * a-th active variable does not appear in the block, zeros).  HIPSDP_ERR_NOMEM from define leaves no master copy behind. */
HIPSDP_API int  hipsdp_master_define(hipsdp_solver* solver, int nvars, int nblocks, const int* blocksizes, const int* nblockvars);
HIPSDP_API int  hipsdp_master_add_entries(hipsdp_solver* solver, int block, long long nnz, const int* slot, const int* row, const int* col,
   const double* val);
/* the same upload straight from per-slot arrays (slot k: nnz[k] entries row[k][.], col[k][.], val[k][.] - the caller's
 * sdprow[b][k] / sdpcol[b][k] / sdpval[b][k] of sdpisolver.h:176-233), streamed through pinned staging chunks */
HIPSDP_API int  hipsdp_master_add_vars(hipsdp_solver* solver, int block, int nslots, const int* nnz, const int* const* row,
   const int* const* col, const double* const* val);
HIPSDP_API int  hipsdp_master_gather(hipsdp_solver* solver, int engine_block, int master_block, int nactive, const int* slots,
   int nkept, const int* kept);
/* hipsdp_master_define with a storage per block: nnz == NULL or nnz[b] < 0 gives the dense slots x N x N array above, nnz[b] >= 0
 * (the number of triplets to come; a hint) a master block KEPT AS TRIPLETS - nothing of size N^2 per slot is allocated.  Its entries
 * (hipsdp_master_add_entries / _add_vars) are collected and checked on the host; the larger index is the row and a later entry at
 * the same (slot, row, col) replaces an earlier one.  The first hipsdp_master_gather after the entries changed sorts and uploads
 * them once (HIPSDP_ERR_ARG when the mirrored entries do not fit int offsets).  From such a block hipsdp_master_gather
 *  - into an engine block kept as nonzeros builds the node's whole device structure on the device, in a number of launches that
 *    does not depend on the sizes, with one read-back of the four counts, bit for bit what hipsdp_add_entries of the node's triplets
 *    (active variables a + 1, rows renumbered through kept, entries on removed rows dropped) builds on the host.  The slots of
 *    the active variables must be distinct.  Until the next hipsdp_set_shape* such a block takes hipsdp_add_entries for the constant
 *    matrix only (var >= 1: HIPSDP_ERR_ARG), and it is valid until the master copy is defined again or the same master block is
 *    gathered into another engine block;
 *  - into a dense engine block zeroes and scatters the rows of the active variables in one launch: the bits of the dense master.
 * A DENSE master block into an engine block kept as nonzeros stays an error. */
HIPSDP_API int  hipsdp_master_define2(hipsdp_solver* solver, int nvars, int nblocks, const int* blocksizes, const int* nblockvars,
   const long long* nnz);
HIPSDP_API int  hipsdp_master_block_is_sparse(hipsdp_solver* solver, int master_block);
/* totals of this solver (any pointer may be NULL): structures of blocks kept as nonzeros built on the device by hipsdp_master_gather /
 * built on the host from the triplets of hipsdp_add_entries; kernel launches and device -> host synchronisations the gathers from
 * triplet master blocks issued */
HIPSDP_API int  hipsdp_master_gather_stats(hipsdp_solver* solver, long long* device_builds, long long* host_builds, long long* launches,
   long long* readbacks);
/* dense upload of a whole block: A[(m+1) * n * n] host, row-major */
HIPSDP_API int  hipsdp_set_block_dense(hipsdp_solver* solver, int block, const double* A);
/* LP rows: Dext[q x (m+1)] host, row-major, column 0 = c (constant), columns 1..m = D */
HIPSDP_API int  hipsdp_set_lp(hipsdp_solver* solver, const double* Dext);
/* device-resident access for generators / benchmarks: pointer to A_k on the device.  The engine cannot see what is written through
 * it: the first assembly of such a block is computed in every cold solve (no cold-start store) for as long as the allocation lives */
HIPSDP_API int  hipsdp_block_device_ptr(hipsdp_solver* solver, int block, double** dptr);

/* optional warm start (host arrays; X, Z: nblocks dense n_k x n_k matrices; x, z: q) */
HIPSDP_API int  hipsdp_set_start(hipsdp_solver* solver, const double* y, const double* const* X, const double* const* Z,
   const double* x, const double* z);

HIPSDP_API int  hipsdp_solve(hipsdp_solver* solver, const hipsdp_params* params, hipsdp_info* info);
/* Cold-start store.  A cold solve starts from X = Z = xi I, where the first Schur matrix is the Gram matrix <A_i, A_j> of the
 * constraint matrices: a function of the matrices alone, whatever b, the LP rows, the tolerances and the settings are.  On one
 * device, on the general path, with every block dense, the solver keeps that matrix (8 (m + 33) (m + 1) bytes) and a later cold solve
 * of the SAME matrices copies it instead of computing it - bit for bit what it would have computed.  Every call that writes, gathers,
 * generates, clears or re-shapes the matrices of a block makes the next cold solve compute (and store) it again.  Not used: warm
 * starts, the one-launch path, blocks kept as nonzeros, several ranks, sharded matrices.  hits / misses (either may be NULL): cold
 * solves of this solver so far that took the matrix from the store / that computed and stored it. */
HIPSDP_API int  hipsdp_gram_cache_stats(hipsdp_solver* solver, long long* hits, long long* misses);

/* B&B-sized problems (no communicator, every block <= 64 rows, m <= 108 (HIPSDP_SOLVE1_MAXM; 128 fit), q <= 4096, the fixed part of the state fits the 160 KiB of
 * LDS of one compute unit - hs_solve1_fits: with no LP rows one block of 49 rows at m = 1, 37 at m = 108, two of 34 / 25, eight of 16 / 12 -, and one Schur assembly
 * stays below 3e6 multiply-adds: few nonzeros per matrix) are solved by ONE launch of one workgroup (csrc/solve1_body.h, one kernel
 * instance per size class; HIPSDP_SOLVE1=0 switches it off).  hipsdp_solve_path: 1 when the last solve ran there, 0 the general path.
 * hipsdp_solve1_trace: scalars of the last one-launch solve - out[0..63] (status, iterations, ..., device cycles per phase; see
 * csrc/solve1_body.h) and, with HIPSDP_SOLVE1_HIST=1 in the environment, up to maxrows rows of 16 doubles per iteration
 * (it, mu, pinf, dinf, gap, tau, kappa, pobj, dobj, predictor step, step, dtau, residual of the linearised primal equation, forced pivots, |dy|, |h|) - what the parity tests compare with the oracle's
 * history.  Either pointer may be NULL. */
HIPSDP_API int  hipsdp_solve_path(hipsdp_solver* solver);
HIPSDP_API long long hipsdp_solve1_solves(void);      /* solves of this process served by the one launch so far */
HIPSDP_API long long hipsdp_solve1_fallbacks(void);   /* cold solves the one-launch kernel gave up on numerically and the general path solved again */
HIPSDP_API long long hipsdp_solve1_fallbacks_warm(void);   /* ... of these: warm-started solves, retried on the general path from the caller's start point */
/* library built with -DS1_DEBUG (developer build of the one-launch kernel: NaN-poisoned LDS and workspace, full fences, wave-uniformity
 * checks; csrc/solve1_body.h): counts[0] = values declared wave-uniform that were not, counts[1] = solves the kernel ran.  Returns 1
 * in such a build, 0 in a release build (counts zero) */
HIPSDP_API int hipsdp_solve1_debug_counts(unsigned int* counts2);
HIPSDP_API int  hipsdp_solve1_trace(hipsdp_solver* solver, double* out64, int maxrows, double* hist);

/* Solve count independent problems, each already shaped and loaded on its own solver (same device, no communicator).
 * Every eligible problem runs in the one-launch kernel, all of them together: ONE launch of one workgroup per problem for each
 * size class present.  Problems the kernel declines or gives up on, and problems the one-launch path is not offered, are solved
 * afterwards by the general path exactly as hipsdp_solve would solve them.  params: count entries, or NULL for defaults.
 * For every i, solvers[i] and infos[i] end as hipsdp_solve(solvers[i], &params[i], &infos[i]) leaves them (solve_seconds aside).
 * HIPSDP_ERR_ARG, and nothing launched: count < 0, a NULL or unshaped solver, the same solver twice, solvers on different devices,
 * a solver with a communicator.  count == 0 does nothing.
 * rcs (optional): per-solver return code.  Returns HIPSDP_OK when every rcs[i] is HIPSDP_OK, else the first failing code.
 * Two host threads may call it at the same time on disjoint sets of solvers. */
HIPSDP_API int hipsdp_solve_many(int count, hipsdp_solver* const* solvers, const hipsdp_params* params,
                                 hipsdp_info* infos, int* rcs);
HIPSDP_API int hipsdp_solve_many_stats(long long* launches, long long* problems);  /* process totals of the one-launch part */

/* Solve ONE loaded problem under count objectives: job j is the solver's problem with b = row j of B (count x m, host, row-major),
 * everything else shared - what optimisation-based bound tightening asks for (min / max y_v over one node relaxation).  Every job
 * starts from the solver's start point when one is set (hipsdp_set_start), cold otherwise.  An eligible problem runs in the one-launch
 * kernel, one workgroup per job on the solver's matrices: the node's pending setters in at most one launch, one fan-out launch per
 * chunk that writes every job's objective (and start point) into a lane of its own, one solve launch per chunk of at most 512 jobs
 * (fewer when 512 lanes would take more than 256 MiB of device memory; HIPSDP_OBJECTIVES_CHUNK in the environment sets another
 * number).  The lanes belong to the solver and only grow.  Jobs the kernel declines or gives up on are solved afterwards by the
 * general path, in job order, from the same start; a problem the one-launch path is not offered is solved count times on the general path.
 * infos[j] (solve_seconds and schur_seconds aside) and row j of Y (count x m, may be NULL) are bit for bit what hipsdp_set_obj(B + j m),
 * hipsdp_solve, hipsdp_get_y give on a solver loaded the same way (and given the same start point before every solve).
 * params: ONE set for all jobs, or NULL for defaults.  params->preoptgap > 0 is refused: the preoptimal iterate is kept per solver,
 * not per job.  Afterwards the solver has its own objective back, its start point is consumed and it holds no solution.
 * HIPSDP_ERR_ARG, with nothing launched and nothing changed: a NULL or unshaped solver, count < 0, B or infos NULL with count > 0, a
 * solver with a communicator or sharded matrices, preoptgap > 0.  count == 0 does nothing.
 * rcs (optional): per-job return code.  Returns HIPSDP_OK when every rcs[j] is HIPSDP_OK, else the first failing code.
 * Two host threads may call it at the same time on different solvers. */
HIPSDP_API int hipsdp_solve_objectives(hipsdp_solver* solver, int count, const double* B, const hipsdp_params* params,
                                       hipsdp_info* infos, double* Y, int* rcs);
/* process totals: calls that passed the argument checks with count > 0, launches of the fan-out and of the one-launch kernel, jobs
 * whose result that kernel delivered; any pointer may be NULL */
HIPSDP_API int hipsdp_solve_objectives_stats(long long* calls, long long* launches, long long* problems);

/* solution readback (host arrays).  For STATUS_OPTIMAL the iterate scaled by 1 / tau; for the infeasibility statuses
 * the normalised ray. */
HIPSDP_API int  hipsdp_get_y(hipsdp_solver* solver, double* y);
HIPSDP_API int  hipsdp_get_X(hipsdp_solver* solver, int block, double* X);
HIPSDP_API int  hipsdp_get_Z(hipsdp_solver* solver, int block, double* Z);
HIPSDP_API int  hipsdp_get_lp(hipsdp_solver* solver, double* x, double* z);
/* the preoptimal iterate of the last solve (params.preoptgap > 0): *available = 0 when none was captured; y (m), x (q) and
 * X of a block as hipsdp_get_y / get_lp / get_X return the final ones; any output pointer may be NULL */
HIPSDP_API int  hipsdp_get_preoptimal(hipsdp_solver* solver, int* available, double* y, double* x);
HIPSDP_API int  hipsdp_get_preoptimal_X(hipsdp_solver* solver, int block, double* X);

/* smallest eigenvalue of  sum_i A_i^k y_i - A_0^k  for every block, on the device (backs the feasibility check of
 * sdpsolchecker.c:201-257 inside the backend); y: m host values; lmin: nblocks host values.  Per block: up to 200 rows the
 * Lanczos value minus its residual norm of a run of n steps (up to 16 rows: the exact kernel), no decomposition - a run that stopped
 * before n steps (the start vector lies in an invariant subspace: repeated eigenvalues) has not seen the whole space, and the block
 * is served like the next class; 201 .. HIPSDP_SYEVX_MAXN (512) rows the first eigenvalue
 * as hipsdp_syevx computes it, relative to the norm of Z(y) in the scale range stated there; above that a lower bound
 * estimate - 1e-9 (1 + |estimate|) certified by a Cholesky factorization, whose margin is absolute, or the computed eigenvalue
 * where the factorization fails */
HIPSDP_API int  hipsdp_check_y(hipsdp_solver* solver, const double* y, double* lmin, double* lpviol);
/* the same against a known tolerance: blocks above 64 rows are certified by one Cholesky factorization of Z(y) + 0.999 tol I
 * (lmin = -0.999 tol on success: a rigorous lower bound that passes "lmin >= -tol"); the exact eigenvalue is computed only when
 * that fails */
HIPSDP_API int  hipsdp_check_y_tol(hipsdp_solver* solver, const double* y, double tol, double* lmin, double* lpviol);

/* Several ranks making the same calls (SPMD): *flag becomes rank 0's value on every rank, so that decisions taken from a host
 * clock (time limits) are the same everywhere and no rank is left alone in a collective.  One rank / no communicator: no-op. */
HIPSDP_API int  hipsdp_sync_flag(hipsdp_solver* solver, int* flag);

/* Phase anatomy of the last hipsdp_solve (profiling on): device milliseconds between HIP events recorded at the phase
 * boundaries of the engine's main stream, summed over the iterations.  phases: 0 residuals + termination read-back,
 * 1 factorizations of X and Z, 2 Schur assembly, 3 Cholesky of M + the two solves + the tau-elimination pass, 4 predictor,
 * 5 corrector, 6 update with its Cholesky check.  The same boundaries are roctx ranges (rocprofv3 --marker-trace), always. */
#define HIPSDP_NPHASES 7
HIPSDP_API int  hipsdp_set_profiling(hipsdp_solver* solver, int on);
HIPSDP_API int  hipsdp_get_phase_times(hipsdp_solver* solver, double* ms /* [HIPSDP_NPHASES] */);
HIPSDP_API const char* hipsdp_phase_name(int phase);

/* Eigenvector cuts for the LP-based mode (replaces the host loop of cons_sdp.c:896-1010 / :1612-1803 for one block): for every
 * eigenvector v of Z(y) = sum_i A_i y_i - A_0 of block `block` with eigenvalue <= -tol (most negative first, at most maxcuts)
 *     sum_i coefs[c][i] y_i >= lhs[c],   coefs[c][i] = v^T A_i v,  lhs[c] = v^T A_0 v
 * is violated at y by -eigvals[c].  y: m host values (engine variables); coefs: maxcuts x m; vecs: maxcuts x n or NULL. */
HIPSDP_API int  hipsdp_eigencuts(hipsdp_solver* solver, int block, const double* y, double tol, int maxcuts, int* ncuts, double* eigvals,
                      double* coefs, double* lhs, double* vecs);
/* The separation round of cons_sdp.c (separateSol over all constraints) and the eigenvalue part of CONSCHECK in one call:
 * for EVERY block b, lmin[b] = smallest eigenvalue of Z_b(y), and the cuts hipsdp_eigencuts(solver, b, y, tol, maxcuts, ...)
 * would return.  Slot (b, c) of eigvals / lhs is entry b * maxcuts + c, of coefs row b * maxcuts + c (m values); the vectors
 * of block b start at vecs + maxcuts * (n_0 + ... + n_{b-1}), row c has n_b values.  Slots c >= ncuts[b] are not written.
 * maxcuts == 0: only ncuts (all 0) and lmin - a pure feasibility check; then eigvals, coefs, lhs may be NULL.
 * lmin and vecs may be NULL.
 * Blocks of at most 128 rows of a solver without communicator and without sharded matrices are BATCHED: whatever their number
 * and the number of cuts, the call issues one upload of y, one launch that forms all Z_b(y), at most three launches for the
 * decompositions, one for the selection and all coefficients, and one read-back (csrc/eigcuts.hip).  Every other block is served
 * inside the same call the way hipsdp_eigencuts serves it (hipsdp_eigencuts_all_large, below, batches the blocks of 129 .. 512 rows of
 * a solver that is asked for them there).  Two host threads may call it at the same time on different solvers. */
HIPSDP_API int hipsdp_eigencuts_all(hipsdp_solver* solver, const double* y, double tol, int maxcuts, int* ncuts, double* lmin,
                                    double* eigvals, double* coefs, double* lhs, double* vecs);
/* process totals: calls, kernel launches those calls issued for batched blocks, device->host synchronisations they waited on */
HIPSDP_API int hipsdp_eigencuts_all_stats(long long* calls, long long* launches, long long* readbacks);

/* Sparse eigenvector cuts of all blocks in one call: the separation mode `multiplesparsecuts` of cons_sdp.c (:1340-1607,
 * addMultipleSparseCuts, after Algorithm 1 of Dey et al., "Cutting plane generation through sparse principal component analysis")
 * in its default configuration (recomputesparseev, recomputeinitial and exacttrans FALSE; with one of them set:
 * hipsdp_sparsecuts_all_ex below).  Per block b with lmin[b] < -tol:
 *     Z = Z_b(y), (lam, V) its decomposition, v0 = V[0], maxeig = lam[n - 1]
 *     (x, theta) = TPower(maxeig I - Z, v0), scalar = maxeig - theta
 *     while scalar < -feastol and ncuts < maxcuts:  cut (scalar, x);  Z -= scalar x x^T;  maxeig -= scalar;  TPower again from v0
 * TPower (the truncated power method, cons_sdp.c:1140-1234) keeps the sizes[b] entries of largest absolute value of every iterate -
 * of two equal absolute values the one with the smaller index - and stops when its Rayleigh quotient grew by <= convtol.
 * The cut of slot (b, c), laid out as in hipsdp_eigencuts_all: sum_i coefs[i] y_i >= lhs with coefs[i] = x^T A_i x, lhs = x^T A_0 x,
 * violated at y by -eigvals; row c of the block's vectors is x, dense, with exact zeros outside its support of sizes[b] entries.
 * Slots c >= ncuts[b] are not written.  iters[b]: TPower iterations of the block, summed; flags[b] bit 0: a TPower run stopped at
 * maxit (its iterate was used as it stood), bit 1: a truncated iterate had norm 0 (the block's loop ended there).  lmin, vecs,
 * iters and flags may be NULL.
 * ncuts[b] = 0: lmin[b] >= -tol, or sizes[b] > n_b (as :1403-1407), or maxcuts == 0 (a pure feasibility check; then eigvals, coefs
 * and lhs may be NULL).  ncuts[b] = -1: the block is NOT served - more than 128 rows, or a solver with a communicator or with
 * sharded matrices; nothing else is written for it.  hipsdp_sparsecuts (below) gives the sparse cuts of such a block of up to 512
 * rows, hipsdp_eigencuts dense eigenvector cuts of any block.  The call still serves the other blocks.
 * Whatever the number of blocks, cuts and iterations: one upload of y and sizes, 4 to 6 launches (Z_b(y), at most three for the
 * decompositions, TPower, coefficients; 3 to 5 with maxcuts == 0) and one read-back (csrc/sparsecuts.hip).  Same input, same bits,
 * whatever other blocks the solver has.  Two host threads may call it at the same time on different solvers. */
#define HIPSDP_SPARSECUTS_MAXIT 10000
typedef struct hipsdp_sparsecut_opts {
   double tol;      /* a block takes part when lambda_min(Z_b(y)) < -tol            (cons_sdp.c:1690) */
   double feastol;  /* cuts are produced while the sparse eigenvalue is < -feastol   (SCIPisFeasNegative, :1450/:1458) */
   double convtol;  /* TPower stops when its Rayleigh quotient grew by <= convtol; <= 0: 1e-6 (:1441) */
   int    maxcuts;  /* per block, >= 0 (maxnsparsecuts; the output arrays are sized by it) */
   int    maxit;    /* cap on the iterations of ONE TPower run; <= 0: HIPSDP_SPARSECUTS_MAXIT */
} hipsdp_sparsecut_opts;
HIPSDP_API int hipsdp_sparsecuts_all(hipsdp_solver* solver, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts,
   int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags);
/* process totals: calls, kernel launches those calls issued, device->host synchronisations they waited on */
HIPSDP_API int hipsdp_sparsecuts_all_stats(long long* calls, long long* launches, long long* readbacks);

/* The same for ONE block of up to HIPSDP_SPARSECUTS_MAXN rows: the per-block partner of hipsdp_sparsecuts_all, as hipsdp_eigencuts is
 * of hipsdp_eigencuts_all.  Algorithm, options, tie rule, flags and the meaning of every output are those of hipsdp_sparsecuts_all
 * restricted to block `block` with target sparsity `size`: eigvals[maxcuts], lhs[maxcuts], coefs[maxcuts x m], vecs[maxcuts x n]
 * (dense rows, exact zeros off the support), *ncuts, *lmin, *iters, *flags; slots c >= *ncuts are not written; lmin, vecs, iters and
 * flags may be NULL, with maxcuts == 0 also eigvals, coefs and lhs.
 * A block of at most 128 rows runs through the launches of hipsdp_sparsecuts_all with that block as the only job and returns the
 * bits that call returns for it.  A block of 129 .. 512 rows (csrc/sparsecuts_large.hip): Z(y) in one launch, ONE
 * tridiagonalisation (n launches), from it (lmin, v0) in three launches and maxeig in one, the whole TPower loop in one launch of a
 * single workgroup, the coefficients in one - n + 7 launches, one upload of y, one read-back and one synchronisation whatever the
 * number of cuts and iterations; with maxcuts == 0 only lmin is computed: n + 2 launches.  lmin and maxeig have the accuracy of
 * hipsdp_syevx.  Same input, same bits.
 * *ncuts = -1 with HIPSDP_OK and nothing else written: a block of more than 512 rows, or a solver with a communicator or with
 * sharded matrices.  HIPSDP_ERR_ARG, nothing launched: solver NULL or without a shape, block out of range, y, opts or ncuts NULL,
 * size < 1, maxcuts < 0, maxcuts > 0 with eigvals, coefs or lhs NULL.  Two host threads may call it at the same time on different
 * solvers. */
#define HIPSDP_SPARSECUTS_MAXN 512      /* = the largest matrix of hipsdp_syevx */
HIPSDP_API int hipsdp_sparsecuts(hipsdp_solver* solver, int block, const double* y, int size, const hipsdp_sparsecut_opts* opts,
   int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags);
/* process totals of hipsdp_sparsecuts alone: calls that served their block, kernel launches they issued, device->host
 * synchronisations they waited on (the totals of hipsdp_sparsecuts_all_stats do not move) */
HIPSDP_API int hipsdp_sparsecuts_stats(long long* calls, long long* launches, long long* readbacks);

/* The two calls above with the reference's three switches on the loop of addMultipleSparseCuts (cons_sdp.c:156-158), as a bit mask.
 * With x, S and theta the vector, support and value of a TPower run on maxeig I - Z and scalar = maxeig - theta, a cut is produced
 * while scalar < -feastol and ncuts < maxcuts, and
 *   HIPSDP_SC_RECOMPUTE_SPARSEEV (recomputesparseev, :1460-1514): (lambda, w) is the smallest eigenpair of the principal submatrix
 *       Z_S of the current (deflated) Z, w normalised.  lambda >= -tol ENDS the block's loop with no cut from this run (:1487) and
 *       sets flags bit 2; otherwise the cut vector is w lifted with zeros outside S, and the cut and the deflation use lambda.
 *   (always) Z -= value x x^T, with value = lambda or scalar and x the cut vector.
 *   HIPSDP_SC_RECOMPUTE_INITIAL (recomputeinitial, :1532-1550): the next TPower run starts from the eigenvector of the smallest
 *       eigenvalue of the DEFLATED Z instead of v0.
 *   HIPSDP_SC_EXACTTRANS (exacttrans, :1552-1568): maxeig becomes the largest eigenvalue of the deflated Z instead of maxeig - value.
 * As in the default loop one more TPower run follows the last cut, and its iterations are counted.
 * Arguments, layouts, NULL rules, flags and the meaning of ncuts = 0 / -1 are those of hipsdp_sparsecuts_all and hipsdp_sparsecuts.
 * eigvals[c] is the value the cut and the deflation used (lambda with HIPSDP_SC_RECOMPUTE_SPARSEEV, else scalar), the vector row is the
 * cut vector with exact zeros off its support.  The per-block call returns the bits the all-blocks call returns for that block; a
 * block's bits do not depend on the other blocks of the solver; same input, same bits.  Two host threads may call them at the same
 * time on different solvers.
 * variant == 0: the call IS hipsdp_sparsecuts_all / hipsdp_sparsecuts - the same launches, the same bits, booked under their stats;
 * the totals of hipsdp_sparsecuts_ex_stats do not move.  A bit above HIPSDP_SC_EXACTTRANS set: HIPSDP_ERR_ARG, nothing launched.
 * variant != 0 serves blocks of AT MOST 128 ROWS of a solver without communicator and without sharded matrices, in all three storage
 * forms of a block.  A block of more than 128 rows gets ncuts = -1 and nothing else written, from BOTH calls: the blocks of
 * 129 .. 512 rows are served by hipsdp_sparsecuts_all_large (below) - call it for the blocks that came back with -1.
 * The loop runs as maxcuts + 1 rounds on the device (csrc/sparsecuts_rounds.hip): the state of a block stays in the workspace, the
 * decompositions stand between the TPower launches, and nothing is read back in between.  With s = 1 for
 * HIPSDP_SC_RECOMPUTE_SPARSEEV (else 0) and d = 1 for HIPSDP_SC_RECOMPUTE_INITIAL or HIPSDP_SC_EXACTTRANS (else 0) a call issues
 * 5 + maxcuts (1 + 4 s + 3 d) launches and one more for the coefficients when maxcuts > 0 - at most 5 + (maxcuts + 1) (2 + 3 s + 3 d),
 * a function of (variant, maxcuts) alone: a class of the batched decompositions that has no job gets an empty launch -, one upload
 * of y and sizes, and one read-back, whatever the number of blocks, cuts and iterations. */
#define HIPSDP_SC_RECOMPUTE_SPARSEEV 1
#define HIPSDP_SC_RECOMPUTE_INITIAL  2
#define HIPSDP_SC_EXACTTRANS         4
HIPSDP_API int hipsdp_sparsecuts_all_ex(hipsdp_solver* solver, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts,
   unsigned variant, int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags);
HIPSDP_API int hipsdp_sparsecuts_ex(hipsdp_solver* solver, int block, const double* y, int size, const hipsdp_sparsecut_opts* opts,
   unsigned variant, int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags);
/* process totals of the two calls with variant != 0: calls, kernel launches they issued, device->host synchronisations they waited on */
HIPSDP_API int hipsdp_sparsecuts_ex_stats(long long* calls, long long* launches, long long* readbacks);

/* The partner of hipsdp_sparsecuts_all_ex for the blocks it turns away: the sparse cuts of ALL blocks of 129 .. HIPSDP_SPARSECUTS_MAXN
 * rows of a solver in one call, with every combination of the three switches (variant 0 .. 7, zero included).  Call
 * hipsdp_sparsecuts_all_ex first, then this for the blocks that came back with ncuts = -1.  Arguments, output layout (slot (b, c), the
 * vectors of block b at vecs + maxcuts (n_0 + ... + n_{b-1})), NULL rules, the meaning of ncuts = 0, of flags bits 0 - 2 and of
 * eigvals[c], "slots c >= ncuts[b] are not written" and the argument errors (HIPSDP_ERR_ARG before the device is looked at; a variant
 * bit above HIPSDP_SC_EXACTTRANS is one) are those of hipsdp_sparsecuts_all_ex.
 * Served: blocks of 129 .. 512 rows of a solver without communicator and without sharded matrices, in all three storage forms.
 * ncuts[b] = -1 and nothing else written: a block of at most 128 rows, a block of more than 512 rows, and - LIMIT - a block whose
 * sizes[b] exceeds 128 while HIPSDP_SC_RECOMPUTE_SPARSEEV is set (its Z_S goes through the one-launch decompositions, which end at 128
 * rows).  The other blocks are still served.  A solver with a communicator or sharded matrices: every ncuts = -1, nothing launched; a
 * call with no served block launches nothing.
 * The device side (csrc/sparsecuts_large_rounds.hip): Z_b(y) of the served blocks in one launch; (lmin, v0) and maxeig of every block
 * from the batched tridiagonal path of hipsdp_onevar_bounds_large (one staging launch, nmax - 1 column launches that hold the matrices
 * of all blocks, 3 selection launches; nmax: rows of the largest served block); then with variant == 0 ONE launch with a workgroup per
 * block that runs the block's whole loop (the loop of hipsdp_sparsecuts), and with variant != 0 maxcuts + 1 rounds as in
 * hipsdp_sparsecuts_all_ex - a TPower launch over all blocks, with HIPSDP_SC_RECOMPUTE_SPARSEEV (s = 1, else 0) three decomposition
 * launches and the cut, with HIPSDP_SC_RECOMPUTE_INITIAL or HIPSDP_SC_EXACTTRANS (d = 1, else 0) the nmax + 3 launches of the
 * tridiagonal path on the deflated matrices of the blocks that go on; the coefficients in one launch.  Kernel launches of a call:
 *     1 + (nmax + 3) + r (1 + 4 s + d (nmax + 3)) + 1 + [maxcuts > 0],    r = maxcuts with variant != 0, r = 0 with variant == 0
 * - a function of (variant, maxcuts, nmax) alone, whatever the number of blocks, cuts and iterations -, one upload and ONE read-back.
 * A block takes about 4.3 n^2 doubles of the solver's cut workspace (9 MB at 512 rows): the blocks are ordered by descending n and run
 * in chunks of at most 512 MiB (HIPSDP_SPARSECUTS_LARGE_CHUNK in the environment, read at every call: blocks per chunk instead), and
 * every chunk is a call of its own in launches and read-backs (nmax: the chunk's largest block).
 * The bits of a block depend on the block, y, its size, the options and the mask alone - not on the other blocks, their order or the
 * chunks; same input, same bits.  With variant == 0 counts, supports and flags are those of hipsdp_sparsecuts.  lmin and maxeig have
 * the accuracy of hipsdp_syevx.  Two host threads may call it at the same time on different solvers. */
HIPSDP_API int hipsdp_sparsecuts_all_large(hipsdp_solver* solver, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts,
   unsigned variant, int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags);
/* process totals of hipsdp_sparsecuts_all_large alone: calls that served a block, kernel launches they issued, device->host
 * synchronisations they waited on (one per chunk); the totals of the other three sparse-cut stats calls do not move, and the reverse */
HIPSDP_API int hipsdp_sparsecuts_all_large_stats(long long* calls, long long* launches, long long* readbacks);

/* The partner of hipsdp_eigencuts_all for the blocks of 129 .. 512 rows, which that call serves one after the other with a full
 * decomposition each: the DENSE eigenvector cuts (the default separation mode of cons_sdp.c) and the feasibility eigenvalue of ALL such
 * blocks of a solver per launch, from the wanted eigenpairs alone.  Arguments, output layout, the NULL rules (lmin and vecs may be NULL;
 * with maxcuts == 0 also eigvals, coefs, lhs), "slots c >= ncuts[b] are not written" and maxcuts == 0 as a pure feasibility check
 * (ncuts = 0 and lmin of every served block) are those of hipsdp_eigencuts_all; the selection is the rule of hipsdp_eigencuts:
 * eigenvalue <= -tol, most negative first, at most maxcuts.
 * Served: blocks of 129 .. 512 rows of a solver without communicator and without sharded matrices, in all three storage forms.
 * ncuts[b] = -1 and nothing else written, lmin[b] included: a block of at most 128 rows (hipsdp_eigencuts_all batches it) and a block of
 * more than 512 rows.  The other blocks are still served.  A solver with a communicator or sharded matrices: every ncuts = -1, nothing
 * launched; a call with no served block launches nothing and leaves the totals unchanged.
 * HIPSDP_ERR_ARG, before the device is looked at: solver NULL or without a shape, y or ncuts NULL, maxcuts < 0 or maxcuts >
 * HIPSDP_EIGENCUTS_LARGE_MAXCUTS, maxcuts > 0 with eigvals, coefs or lhs NULL.
 * lmin[b] is eigenvalue 1 of Z_b(y) with the accuracy of hipsdp_syevx; when ncuts[b] > 0 it is eigvals slot (b, 0) bit for bit.
 * The device side (csrc/eigcuts_large.hip, csrc/syevx.hip): Z_b(y) of the served blocks formed straight into the matrices of the
 * batched tridiagonalisation and their reflector arrays cleared (2 launches), nmax - 1 column launches that hold the matrices of all
 * blocks (nmax: rows of the largest served block), one launch for eigenvalue 1 and the eigenvalues <= -tol of every block, with
 * maxcuts > 0 one for their eigenvectors of the tridiagonal matrices and one for the back-transformation, and one launch that stores
 * counts and lmin and sweeps every A_i once for all cuts of its block.  Kernel launches of a call:
 *     2 + (nmax - 1) + 1 + 2 [maxcuts > 0] + 1   =   nmax + 3 + 2 [maxcuts > 0]
 * - a function of nmax and of maxcuts > 0 alone, whatever the number of blocks and cuts -, one upload and ONE read-back.
 * A block takes about 2 n^2 + 165 n doubles of the solver's cut workspace (4.9 MB at 512 rows): the blocks are ordered by descending n
 * and run in chunks of at most 512 MiB (HIPSDP_EIGENCUTS_LARGE_CHUNK in the environment, read at every call: blocks per chunk instead),
 * and every chunk is a call of its own in launches and read-backs (nmax: the chunk's largest block).
 * The bits of a block depend on the block, y, tol and maxcuts alone - not on the other blocks, their order or the chunks; same input,
 * same bits.  Two host threads may call it at the same time on different solvers. */
#define HIPSDP_EIGENCUTS_LARGE_MAXN    512     /* = HIPSDP_SPARSECUTS_MAXN */
#define HIPSDP_EIGENCUTS_LARGE_MAXCUTS 32      /* = the most pairs hipsdp_syevx returns */
HIPSDP_API int hipsdp_eigencuts_all_large(hipsdp_solver* solver, const double* y, double tol, int maxcuts, int* ncuts, double* lmin,
                                          double* eigvals, double* coefs, double* lhs, double* vecs);
/* process totals of hipsdp_eigencuts_all_large alone: calls that served a block, kernel launches they issued, device->host
 * synchronisations they waited on (one per chunk); the totals of hipsdp_eigencuts_all and of the sparse-cut calls do not move, and the
 * reverse */
HIPSDP_API int hipsdp_eigencuts_all_large_stats(long long* calls, long long* launches, long long* readbacks);

/* The feasibility check of MANY candidate points in one call: what SCIPsdpSolcheckerCheck / CONSCHECK (sdpsolchecker.c:201-257) computes
 * for every solution a heuristic proposes - per block the smallest eigenvalue of Z_b(y) = sum_i A_i^b y_i - A_0^b, and the LP rows - for
 * count points at once (the roundings of heur_sdprand.c:353-420, the fully fixed nodes of a branch and bound).  Y: count x m, row-major,
 * host values (engine variables).
 *     lmin[j nblocks + b] = eigenvalue 1 of Z_b(Y[j]), a COMPUTED eigenvalue at every served size (not the Lanczos lower estimate
 *                           hipsdp_check_y returns up to 200 rows), with the accuracy of the SCALE RANGE paragraph below: within 1e-12 of
 *                           the largest eigenvalue in absolute value;
 *     lpviol[j]           = max(0, max_r (c_r - (D Y[j])_r)), the convention of hipsdp_check_y; 0 without LP rows; lpviol may be NULL;
 *     served[b]           = 0: block b is served; -1: it is not, and column b of lmin is not written.  served may be NULL.
 * Served: blocks of 1 .. 512 rows of a solver without communicator and without sharded matrices, in all three storage forms (dense rows,
 * packed lower triangles, nonzeros).  Not served: a block of more than 512 rows or without matrices on this device; the other blocks
 * are still served.  A solver with a communicator or sharded matrices: every served = -1, nothing launched, lmin and lpviol not written,
 * HIPSDP_OK.  hipsdp_check_y remains the call for one point, with its own semantics.
 * HIPSDP_ERR_ARG, before the device is looked at and with nothing launched: solver NULL or without a shape, count < 0, Y or lmin NULL
 * with count > 0.  count == 0: HIPSDP_OK, nothing launched, nothing written (served included), the totals unchanged.
 * The device side (csrc/check_many.hip, csrc/eigi.hip, csrc/syevx.hip): ONE launch forms Z_b(Y[j]) of all served blocks and candidates,
 * a group of 8 candidates per pass over a block's storage - the pass a loop over hipsdp_check_y or hipsdp_eigencuts_all makes once per
 * candidate; eigenvalue 1 alone, no vector, by the tridiagonalisation and Sturm multisection of hipsdp_syevi_small up to 128 rows (a
 * matrix per workgroup up to 64 rows, one launch; at most a workgroup per compute unit that runs its matrices one after the other for
 * 65 .. 128 rows, one launch) and by the batched tridiagonal path of hipsdp_syevx for 129 .. 512 rows (the reflector arrays cleared,
 * nmax - 1 column launches that hold the matrices of all candidates and blocks, 3 selection launches; nmax: rows of the largest served
 * block above 128 rows); ONE launch stores lmin and evaluates the LP rows.  Kernel launches of a call, with [..] = 1 when a served block
 * of that class exists:
 *     [any block] + [1 .. 64 rows] + [65 .. 128 rows] + [129 .. 512 rows] (nmax + 3) + 1
 * - a function of the classes present and of nmax alone, never of count or of the number of blocks -, one upload and ONE read-back.
 * A candidate takes n_b^2 doubles of the solver's grow-only cut workspace per block up to 128 rows and about 2 n_b^2 + 165 n_b above: the
 * candidates run in chunks of at most 512 MiB (HIPSDP_CHECK_MANY_CHUNK in the environment, read at every call: candidates per chunk
 * instead), and every chunk is a call of its own in launches and read-backs.
 * The bits of (j, b) depend on the block and on row j of Y alone - not on count, the other candidates, j's position, the other blocks or
 * the chunks; same input, same bits; no floating-point atomics.  Two host threads may call it at the same time on different solvers. */
HIPSDP_API int hipsdp_check_y_many(hipsdp_solver* solver, int count, const double* Y /* count x m, row-major, host */,
                                   double* lmin   /* count x nblocks */,
                                   double* lpviol /* count; may be NULL */,
                                   int* served    /* nblocks; may be NULL */);
/* process totals of hipsdp_check_y_many alone: calls that launched something, kernel launches they issued, device->host synchronisations
 * they waited on (one per chunk); any pointer may be NULL.  The totals of the other calls do not move, and the reverse */
HIPSDP_API int hipsdp_check_y_many_stats(long long* calls, long long* launches, long long* readbacks);

/* The rank-1 constraints of MANY candidate points in one call: what the rank-1 part of CONSCHECK (consCheckSdp, cons_sdp.c:7735-7865)
 * computes per solution and rank-1 constraint - isMatrixRankOne (:733-823): eigenvalue n - 1 of Z_b(y) = sum_i A_i^b y_i - A_0^b and, when
 * that is not zero, the scan of all n (n - 1) / 2 principal 2 x 2 minors for the largest smaller eigenvalue; with quadconsrank1
 * checkRank1QuadConss (:3712-3785): the scan of the minors' determinants against feastol - for count points at once, the points
 * hipsdp_check_y_many checks for eigenvalue 1.  Y: count x m, row-major, host values (engine variables).  With Z = Z_b(Y[j]), o = j nblocks + b:
 *     lam[3 o ..]         = COMPUTED eigenvalues 1, n - 1 and n of Z, each with the accuracy of the SCALE RANGE paragraph below: within
 *                           1e-12 of the largest eigenvalue in absolute value.  n = 2: slot 1 is eigenvalue 1.  n = 1: slots 0 and 2 are the
 *                           scalar, slot 1 is 0.0.  Slot 0 is what hipsdp_check_y_many returns for the same row, bit for bit.
 *     minorev[o],         = the scan of :788-806: over the pairs (i, k), k < i, i ascending and then k ascending, the smaller eigenvalue
 *     minorind[2 o ..]      of [[Z_ii, Z_ik], [Z_ik, Z_kk]]; the largest value that is > 0 and its pair (i, k); of equal values the FIRST
 *                           pair in that order (the reference's strict >).  No minor with a positive smaller eigenvalue, or n = 1: 0.0
 *                           and (-1, -1) - the reference asserts that case away (it scans only when eigenvalue n - 1 is not zero).  The
 *                           value is the closed form  h - sqrt(g g + b b),  h = (a + c) / 2, g = (a - c) / 2, a = Z_ii, b = Z_ik,
 *                           c = Z_kk, in plain FP64, every operation rounded on its own: absolute error a few ulp of |a| + |b| + |c|.
 *     minordet[o],        = the scan of :3756-3780: minor = Z_ii Z_kk - Z_ik^2, both products rounded and then subtracted, no
 *     detind[2 o ..]        contraction; minordet = the largest |minor| (0.0 for n = 1), detind = the FIRST pair in the same order with
 *                           minor < -feastol || minor > feastol (the reference's early exit), else (-1, -1).
 *     served[b]           = 0: block b is served; -1: it is not, and nothing of column b is written.  served may be NULL.
 * Of the four output groups only lam is required: a NULL pair (minorev with minorind, minordet with detind) skips nothing on the device
 * but is not copied out.
 * Served: as hipsdp_check_y_many - blocks of 1 .. 512 rows of a solver without communicator and without sharded matrices, in all three
 * storage forms; a block of more than 512 rows or without matrices on this device is not served and the other blocks still are; a solver
 * with a communicator or sharded matrices: every served = -1, nothing launched, nothing written, HIPSDP_OK.
 * HIPSDP_ERR_ARG, before the device is looked at and with nothing launched: solver NULL or without a shape, count < 0, feastol negative or
 * not a number, Y or lam NULL with count > 0, one pointer of a pair NULL and the other not.  count == 0: HIPSDP_OK, nothing launched,
 * nothing written (served included), the totals unchanged.
 * The device side (csrc/rank1.hip, csrc/check_many.hip, csrc/eigi.hip, csrc/syevx.hip): the ONE launch of hipsdp_check_y_many forms
 * Z_b(Y[j]) of all served blocks and candidates; ONE launch (k_r1_minors) runs both scans over the lower triangle of every Z, a workgroup
 * per matrix, a fixed reduction order - while Z is still intact: the column launches below consume it; the eigenvalues {1, n - 1, n} come
 * from ONE reduction per matrix, values only - up to 128 rows the tridiagonalisation of hipsdp_syevi_small once and its Sturm
 * multisection once per index (one launch per class: 1 .. 64 rows, 65 .. 128 rows), for 129 .. 512 rows the batched tridiagonal path of
 * hipsdp_syevx (the reflector arrays cleared, nmax - 1 column launches, ONE values launch for the ranges [1, 1] and [n - 1, n]; no vector
 * launches; nmax: rows of the largest served block above 128 rows); ONE launch stores the eigenvalues.  Kernel launches of a call, with
 * [..] = 1 when a served block of that class exists:
 *     3 [any block] + [1 .. 64 rows] + [65 .. 128 rows] + [129 .. 512 rows] (nmax + 1)
 * - a function of the classes present and of nmax alone, never of count or of the number of blocks -, one upload and ONE read-back.
 * The workspace and the chunks are those of hipsdp_check_y_many (at most 512 MiB per chunk; HIPSDP_RANK1_CHUNK in the environment, read at
 * every call: candidates per chunk instead), and every chunk is a call of its own in launches and read-backs.
 * The bits of (j, b) depend on the block and on row j of Y alone - not on count, the other candidates, j's position, the other blocks or
 * the chunks; same input, same bits; no atomics.  Two host threads may call it at the same time on different solvers. */
HIPSDP_API int hipsdp_rank1_check_many(hipsdp_solver* solver, int count, const double* Y /* count x m, row-major, host */,
                                       double feastol,
                                       double* lam      /* count x nblocks x 3: eigenvalues 1, n-1, n of Z_b(Y[j]) */,
                                       double* minorev  /* count x nblocks */, int* minorind /* count x nblocks x 2 */,
                                       double* minordet /* count x nblocks */, int* detind   /* count x nblocks x 2 */,
                                       int* served      /* nblocks; may be NULL */);
/* process totals of hipsdp_rank1_check_many alone: calls that launched something, kernel launches they issued, device->host
 * synchronisations they waited on (one per chunk); any pointer may be NULL.  The totals of the other calls do not move, and the reverse */
HIPSDP_API int hipsdp_rank1_check_many_stats(long long* calls, long long* launches, long long* readbacks);

/* The device part of the best rank-1 approximation heuristic (constraints/SDP/rank1approxheur, cons_sdp.c:7869-8185): per violated rank-1
 * constraint the reference decomposes Z_b(y) FULLY, forms lambda_max v v^T by a matrix product and from it the right-hand side
 * A_0 + lambda_max v v^T of a least-squares system - ONE eigenpair is used.  Here, for every asked-for block b (want[b] != 0; want NULL:
 * all), with off_b = n_0 + ... + n_{b-1} and pos_b = sum_{b' < b} n_b' (n_b' + 1) / 2 over ALL blocks:
 *     lmax[b]                           = eigenvalue n of Z_b(y), used as it is (the reference only asserts that the others are >= 0);
 *     vec[off_b + i]                    = component i of its unit vector v;
 *                                         the eigen entries' bounds: |lmax - ev| <= 1e-12 scale, | ||v|| - 1 | <= 1e-12, residual
 *                                         |Z v - lmax v| <= 1e-9 scale (SCALE RANGE paragraph below);
 *     rhs[pos_b + i (i + 1) / 2 + k]    = A_0[i][k] + (lmax v_i) v_k for k <= i - rhsmatrix of :8058-8092 in the reference's row order,
 *                                         every operation rounded on its own, no contraction;
 *     served[b]                         = 0: served; 1: not asked for; -1: asked for and not served.  served may be NULL.
 * The slices of a block that is not served or not asked for are not written.  The coefficient matrix of the least-squares system is the
 * caller's own constant data, and SCIPlapackLinearSolve (DGELSD) stays on the host ("Rank-1 constraints").
 * Served: blocks of 1 .. 512 rows of a solver without communicator and without sharded matrices, in all three storage forms; such a solver
 * otherwise: nothing launched, every asked-for block -1, HIPSDP_OK.
 * HIPSDP_ERR_ARG, before the device is looked at: solver NULL or without a shape, y, lmax, vec or rhs NULL.
 * The device side (csrc/rank1.hip, csrc/eigcuts.hip, csrc/eigi.hip, csrc/syevx.hip): ONE launch writes Z_b(y) of the asked-for blocks; up to
 * 128 rows the batched full decomposition of hipsdp_eigencuts_all (3 launches) gives pair n; for 129 .. 512 rows ONE launch negates Z in the
 * matrices of the batched tridiagonal path and clears the reflector arrays, nmax - 1 column launches and the 3 selection launches give
 * eigenvalue 1 of -Z with its vector, which is pair n of Z (nmax: rows of the largest asked-for block above 128 rows); ONE launch stores
 * lmax (the sign put back), vec and rhs, A_0 read from the block's storage form.  Kernel launches, with [..] = 1 when an asked-for served
 * block of that class exists:
 *     2 + 3 [1 .. 128 rows] + [129 .. 512 rows] (nmax + 3)
 * one upload and ONE read-back.  The blocks are taken by descending size in chunks of at most 512 MiB of the cut workspace
 * (HIPSDP_RANK1_APPROX_CHUNK in the environment, read at every call: blocks per chunk instead); every chunk is a call of its own in
 * launches and read-backs.  The bits of a block do not depend on the other blocks, on want or on the chunks. */
HIPSDP_API int hipsdp_rank1_approx(hipsdp_solver* solver, const double* y /* m */, const int* want /* nblocks, or NULL: all */,
                                   double* lmax /* nblocks */, double* vec /* sum n_b, block b at off_b */,
                                   double* rhs  /* sum n_b (n_b + 1) / 2 */,
                                   int* served  /* nblocks; may be NULL: 0 served, 1 not asked for, -1 not served */);
/* process totals of hipsdp_rank1_approx alone (calls that launched something, kernel launches, read-backs: one per chunk); any pointer may
 * be NULL */
HIPSDP_API int hipsdp_rank1_approx_stats(long long* calls, long long* launches, long long* readbacks);

/* All one-variable SDPs of a block in one call: the bound-tightening loops of cons_sdp.c - tightenBounds (:1968-2201) and
 * tightenMatrices (:1856-1961) solve one SDP PER VARIABLE of a block, each the semismooth Newton method of
 * SCIPsolveOneVarSDPDense (solveonevarsdp.c:370-533) on  mu A_i - C_i,  C_i = A_0 - sum_{k != i} ub_k A_k.  With
 * Z(u) = sum_k u_k A_k - A_0 that matrix is
 *     M_i(mu) = Z_block(u) + (mu - u_i) A_i        (tightenBounds: u = ub; tightenMatrices: u = 0),
 * and the loop over i never changes u: the jobs of a block are independent.  Job j, i = vars[j], with f(mu) the smallest
 * eigenvalue of M_i(mu) and g(mu) = v^T A_i v at its unit eigenvector v (a supergradient of the concave f):
 *   HIPSDP_ONEVAR_NEWTON, the order of evaluations and the comparisons of solveonevarsdp.c:434-525 with obj = 1:
 *     at ub:  f < -feastol and g > 0   -> INFEASIBLE, optval = ub
 *     at lb:  f >= -feastol            -> LB, optval = lb, grad = 0;      g <= 0 -> INFEASIBLE, optval = lb
 *     loop:   mu <- mu - (feastol / 2 + f) / g;  mu > ub -> INFEASIBLE, optval = mu;  evaluate at mu;  while f < -feastol and g > 0
 *     then:   f < -feastol -> INFEASIBLE, else INNER, optval = mu
 *   HIPSDP_ONEVAR_TWOPOINT, the binary-variable branch of tightenBounds (:2102-2153), eigenvalues only:
 *     f(lb) >= -feastol -> LB;  else f(ub) < -feastol -> INFEASIBLE, optval = ub;  else UBONLY, optval = ub
 * u: m host values (engine variables, as y of hipsdp_eigencuts); vars: count engine variable indices (0-based), NULL: all m
 * variables in index order (count must be m); kind: one HIPSDP_ONEVAR_* kind per job, NULL: all NEWTON; lb, ub: per job.
 * Per job: status, optval, lmin (the last eigenvalue computed), grad (the last supergradient; 0 for LB and for TWOPOINT), evals
 * (eigenvalue evaluations); lmin, grad and evals may be NULL.  DECLINED (an infinite bound, solveonevarsdp.c:407-411) computes
 * nothing: optval = lmin = grad = 0, evals = 0.  GAVEUP (opts->maxevals evaluations done and one more needed, or a non-finite
 * eigenvalue or supergradient): optval is the last point evaluated.
 * Whatever the number of jobs and evaluations: ONE upload (u, the job table, bounds and kinds in one buffer), TWO launches (Z(u),
 * then one workgroup per job that runs the whole loop of its job: csrc/eigi.hip, k_onevar_small up to 64 rows, k_onevar_mid up to
 * 128) and ONE read-back.  Same input, same bits; the bits of a job do not depend on the other jobs of the call.  Two host
 * threads may call it at the same time on different solvers.
 * Every status[j] = -1 with HIPSDP_OK and nothing else written: a block of more than HIPSDP_ONEVAR_MAXN rows, or a solver with a
 * communicator or with sharded matrices.  HIPSDP_ERR_ARG, checked before the device is looked at, nothing launched: solver NULL or
 * without a shape, block out of range, u, lb, ub, opts, status or optval NULL, count < 0, a variable index outside [0, m), a kind
 * other than the two, feastol < 0, vars == NULL with count != m.  count == 0: HIPSDP_OK, nothing launched. */
#define HIPSDP_ONEVAR_MAXN      128
/* kind of a job */
#define HIPSDP_ONEVAR_NEWTON    0   /* SCIPsolveOneVarSDPDense with obj = 1 (solveonevarsdp.c:370-533) */
#define HIPSDP_ONEVAR_TWOPOINT  1   /* the binary-variable branch of tightenBounds (cons_sdp.c:2102-2153): two eigenvalues, no vectors */
/* status of a job */
#define HIPSDP_ONEVAR_LB          0   /* M(lb) is psd to feastol: optval = lb, nothing to tighten */
#define HIPSDP_ONEVAR_INNER       1   /* NEWTON: optval = the last iterate mu in (lb, ub] */
#define HIPSDP_ONEVAR_INFEASIBLE  2   /* optval = the point where it was detected (ub, lb or the last mu, as the reference) */
#define HIPSDP_ONEVAR_UBONLY      3   /* TWOPOINT: M(lb) is not psd, M(ub) is: optval = ub */
#define HIPSDP_ONEVAR_DECLINED    4   /* lb <= -infinity or ub >= infinity (solveonevarsdp.c:407-411): nothing computed */
#define HIPSDP_ONEVAR_GAVEUP      5   /* maxevals reached, or a non-finite eigenvalue / supergradient: optval = last mu */
typedef struct hipsdp_onevar_opts { double feastol; double infinity; int maxevals; /* <= 0: 100 */ } hipsdp_onevar_opts;

HIPSDP_API int hipsdp_onevar_bounds(hipsdp_solver* solver, int block, const double* u, int count, const int* vars, const int* kind,
   const double* lb, const double* ub, const hipsdp_onevar_opts* opts,
   int* status, double* optval, double* lmin, double* grad, int* evals);
/* process totals: calls that served their block, kernel launches they issued, device->host synchronisations they waited on (NULL
 * pointers are accepted; works without a device) */
HIPSDP_API int hipsdp_onevar_bounds_stats(long long* calls, long long* launches, long long* readbacks);

/* The same one-variable SDPs for ALL blocks of the solver in one call: a round of tightenBounds / tightenMatrices runs over all
 * constraints (for (c = 0; c < nconss; ++c)), and a call per block leaves most of the device idle and waits for the host once per
 * block.  Job j is the pair (blocks[j], vars[j]) with kind[j] and the bounds lb[j], ub[j]; u: the m engine variables, ONE vector for
 * the call (u = ub: tightenBounds, u = 0: tightenMatrices).  blocks == NULL AND vars == NULL: every (block, variable) pair in
 * block-major order (job b m + i is variable i of block b), count must be nblocks * m; exactly one of the two NULL is an error.
 * kind == NULL: all NEWTON.
 *   HIPSDP_ONEVAR_NEWTON, HIPSDP_ONEVAR_TWOPOINT: as hipsdp_onevar_bounds documents them, DECLINED and GAVEUP included, on
 *     M(mu) = Z_b(u) + (mu - u_i) A_i^b, and with the BITS hipsdp_onevar_bounds(solver, block, u, 1, &var, &kind, &lb, &ub, opts, ..)
 *     returns for the job on the same solver.
 *   HIPSDP_ONEVAR_EXTREMES (this call alone): lmin = lambda_min(A_i^b), optval = lambda_max(A_i^b), grad = 0, evals = 2, status
 *     HIPSDP_ONEVAR_DONE - what the lock computation asks of every A_i (cons_sdp.c:4007/:4020, :4096/:4104, :6787/:6809).  It reads
 *     neither u nor the job's bounds, so it is never DECLINED; GAVEUP if an eigenvalue is not finite.  With opts->maxevals == 1
 *     lambda_min ALONE is computed: evals = 1, optval = lmin, status DONE - the precondition allmatricespsd of both loops
 *     (computeAllmatricespsd, cons_sdp.c:1832-1842), one job per (block, variable).  A block of one row is a scalar.
 * A job gets status[j] = -1 and nothing else written when its block has more than HIPSDP_ONEVAR_MAXN rows or no matrices on this
 * device; the OTHER jobs of the call are still served.  A solver with a communicator or with sharded matrices: every status -1,
 * nothing launched.
 * Whatever the number of blocks, jobs and evaluations: ONE upload (u, the job table, bounds and kinds in one buffer), ONE launch of
 * the Z(u) kernel over the blocks with a served NEWTON or TWOPOINT job (none: left out), ONE launch per size class with a served job
 * (up to 64 rows: a workgroup per job; 65 to 128 rows: at most a workgroup per compute unit, each running its jobs one after the
 * other in its own slab, so the workspace is bounded by the grid - 64 MB on 256 compute units - not by the job count), ONE
 * read-back.  The bits of a job depend neither on the other jobs of the call nor on their order; same input, same bits.  Two host
 * threads may call it at the same time on different solvers.
 * HIPSDP_ERR_ARG, checked before the device is looked at, nothing launched: solver NULL or without a shape, u, lb, ub, opts, status or
 * optval NULL, count < 0, a block index outside [0, nblocks), a variable index outside [0, m), a kind outside {0, 1, 2}, feastol < 0,
 * one of blocks / vars NULL without the other, both NULL with count != nblocks * m.  count == 0: HIPSDP_OK, nothing launched.
 * lmin, grad and evals may be NULL. */
#define HIPSDP_ONEVAR_EXTREMES  2   /* kind, accepted by hipsdp_onevar_bounds_all ONLY: lambda_min and lambda_max of A_i alone */
#define HIPSDP_ONEVAR_DONE      6   /* status of an EXTREMES job */
HIPSDP_API int hipsdp_onevar_bounds_all(hipsdp_solver* solver, const double* u, int count,
   const int* blocks, const int* vars, const int* kind, const double* lb, const double* ub,
   const hipsdp_onevar_opts* opts,
   int* status, double* optval, double* lmin, double* grad, int* evals);
/* process totals: calls that served at least one job, kernel launches they issued, device->host synchronisations they waited on
 * (NULL pointers are accepted; works without a device).  The totals of hipsdp_onevar_bounds_stats do not move, and the reverse. */
HIPSDP_API int hipsdp_onevar_bounds_all_stats(long long* calls, long long* launches, long long* readbacks);

/* The same one-variable SDPs for the blocks of 129 .. HIPSDP_ONEVAR_LARGE_MAXN rows, the ones hipsdp_onevar_bounds_all turns away: call
 * hipsdp_onevar_bounds_all first, then this with the jobs that came back -1.  Arguments, job list (the implicit block-major list
 * included), NULL rules, kinds (NEWTON, TWOPOINT, EXTREMES; EXTREMES with opts->maxevals == 1: lambda_min alone), argument errors
 * (checked before the device is looked at, nothing launched) and the meaning of every output are those of hipsdp_onevar_bounds_all;
 * every comparison and the order of evaluations are those hipsdp_onevar_bounds documents.  DECLINED is decided before anything is read.
 * A job on a block of at most HIPSDP_ONEVAR_MAXN rows (they belong to hipsdp_onevar_bounds_all), of more than
 * HIPSDP_ONEVAR_LARGE_MAXN rows or without matrices on this device gets status[j] = -1 and nothing else written; the other jobs are
 * still served.  A solver with a communicator or sharded matrices: every status -1, nothing launched.  count == 0 or no served job:
 * HIPSDP_OK, nothing launched.
 * Above 128 rows an eigenpair is the tridiagonal path of hipsdp_syevx - one launch per column -, so the loop of a job cannot stay in one
 * launch; the JOBS go into the launches instead.  The call runs as rounds: round r is evaluation r of every job still active, all its
 * launches batched over the jobs (form M_j straight into the job's workspace, nmax - 1 column launches, values, vector, back-
 * transformation, decide, count), then ONE int is read back, the number of jobs that go on.  Eigenvalues and vectors have the accuracy stated
 * for hipsdp_syevx in its scale range, relative to ||M(mu)||: the eigenvalue to 1e-12 of the largest one in absolute value, the residual
 * of the unit vector to 1e-9 of it (EXTREMES: relative to ||A_i||).
 * Launches and read-backs of a call whose jobs fit one chunk, with nmax the largest served block, R the most tridiagonalisations a
 * served job needed (its evals for NEWTON and TWOPOINT, 1 for EXTREMES) and z = 1 if a served job that is not declined is NEWTON or
 * TWOPOINT (Z(u) is formed), else 0:
 *     launches = z + R (nmax + 5)   (<= 1 + R (nmax + 6)),      read-backs = R + 1   (R when R = maxevals)
 * - functions of (nmax, R, z) alone, whatever the number of jobs and blocks; a call whose jobs are all declined launches nothing.  A job
 * needs about 4.7 MB of the solver's grow-only cut workspace at 512 rows, so the jobs, ordered by descending n, run in chunks of at
 * most 512 MiB of it (HIPSDP_ONEVAR_LARGE_CHUNK in the environment: jobs per chunk instead), one after the other on the solver's
 * stream; each chunk has the launches and read-backs above for ITS nmax, R and z.
 * Same input, same bits; the bits of a job depend neither on the other jobs, nor on their order, nor on the number of workgroups a job
 * gets, nor on the chunking; no floating-point atomics.  Two host threads may call it at the same time on different solvers. */
#define HIPSDP_ONEVAR_LARGE_MAXN 512     /* = HIPSDP_SYEVX_MAXN */
HIPSDP_API int hipsdp_onevar_bounds_large(hipsdp_solver* solver, const double* u, int count,
   const int* blocks, const int* vars, const int* kind, const double* lb, const double* ub,
   const hipsdp_onevar_opts* opts,
   int* status, double* optval, double* lmin, double* grad, int* evals);
/* process totals: calls that served at least one job, kernel launches they issued, device->host synchronisations they waited on
 * (NULL pointers are accepted; works without a device).  The totals of the two other one-variable calls do not move, and the reverse. */
HIPSDP_API int hipsdp_onevar_bounds_large_stats(long long* calls, long long* launches, long long* readbacks);

/* multi-GPU: Schur rows are sharded over the ranks of an RCCL communicator (one process per GPU); comm comes from hipsdp_comm_create[_host] */
/* Small problems (one assembly below HIPSDP_SHARD_MIN_FLOPS, default 2e10 algorithmic flops) are not sharded: every rank solves
 * them alone with the single-rank kernels and rank 0's outcome (status, iterate, preoptimal iterate) is broadcast once per solve. */
HIPSDP_API int  hipsdp_set_comm(hipsdp_solver* solver, void* comm, int rank, int nranks);
/* Constraint matrices sharded by variable ("A is sharded by variable when it cannot be replicated",
 * n = 4000 / m = 8000 is 1 TB of A): rank g of the communicator holds the matrices of the variables [g c, (g + 1) c),
 * c = ceil((m + 1) / ranks) (index 0 = the constant matrix, which every rank keeps as well); hipsdp_add_entries,
 * hipsdp_set_block_dense and hipsdp_gen_planted store only what the rank holds, the passes over A are completed by an
 * all-gather / all-reduce, and the Schur assembly forms W_j = G A_j R where A_j lives, re-distributes the ENTRIES of the W_j
 * with one all-to-all per column slice (rank h receives its n / ranks rows of all W_j) and sums the partial Gram matrices.
 * mode 1: shard; -1: shard only when the replicated matrices would take more than 75 % of the device memory; 0: replicate
 * (default).  Call after hipsdp_set_comm and before hipsdp_set_shape; the mode applies to every later hipsdp_set_shape. */
HIPSDP_API int  hipsdp_shard_matrices(hipsdp_solver* solver, int mode);
HIPSDP_API int  hipsdp_matrices_sharded(hipsdp_solver* solver);       /* what the last hipsdp_set_shape decided: 1 sharded, 0 replicated */
/* measurement transport: a communicator of nranks ranks of which only `rank` exists - collectives move nothing, results are
 * meaningless; it times one rank's share of a sharded solve at sizes that need several GPUs (tests/devtools/shard_time.py) */
HIPSDP_API int  hipsdp_comm_create_null(int rank, int nranks, void** comm);
/* host-only helper: column ranges of the sharded assembly, bounds[0 .. nranks]; rank g owns [bounds[g], bounds[g + 1]) */
HIPSDP_API int  hipsdp_shard_columns(int m1, int n, int nranks, int* bounds);
HIPSDP_API int  hipsdp_comm_create(const void* unique_id_128bytes, int rank, int nranks, void** comm);
HIPSDP_API int  hipsdp_comm_unique_id(void* unique_id_128bytes);
HIPSDP_API void hipsdp_comm_destroy(void* comm);
/* what the transport says about itself: *count = ncclCommCount for RCCL; *kind (may be NULL) 0 RCCL, 1 host-staged, 2 measurement */
HIPSDP_API int  hipsdp_comm_count(void* comm, int* count, int* kind);
/* optional statistics: a HIP event pair around every collective, booked under the phase the engine is in - 0 Schur exchange
 * (all-reduce / all-gather / all-to-all), 1 passes over A, 2 decision scalars and flags, 3 other.  hipsdp_comm_stats waits for
 * the recorded events and returns seconds[4], calls[4], bytes[4] since the last reset (any pointer may be NULL). */
HIPSDP_API int  hipsdp_comm_stats_enable(void* comm, int on);
HIPSDP_API int  hipsdp_comm_stats(void* comm, double* seconds, long long* calls, double* bytes, int reset);
/* SPMD hosts (N identical processes, one per GPU, making the same calls): the process-wide communicator the environment
 * describes - HIPSDP_WORLD / WORLD_SIZE, HIPSDP_RANK / RANK, and HIPSDP_COMM_FILE=path (RCCL: rank 0 writes the unique id there,
 * the others read it) or HIPSDP_COMM_SHM=/name (host-staged, ranks sharing one device).  *comm = NULL with one rank.  Created at
 * the first call, shared by all solvers of the process, never destroyed.  sdpisolver_hip.c calls it when it creates its engine. */
HIPSDP_API int  hipsdp_comm_from_env(int device, void** comm, int* rank, int* nranks);
/* host-staged communicator for several ranks on ONE device (RCCL refuses that): payloads travel through the POSIX
 * shared-memory segment `name` ("/something", unique per job; every rank passes the same name and staging size).  Same
 * collectives, same results; meant for validating the sharded path on a one-GPU machine, not for speed. */
HIPSDP_API int  hipsdp_comm_create_host(const char* name, int rank, int nranks, long long staging_bytes, double timeout_seconds, void** comm);

/* Synthetic instance of BASELINE.md section 3 generated in HBM.  The solver must have the shape (m, one block of size n,
 * q = 0).  Fills A_1..A_m from the counter stream of oracle/instances.py (seed + i), then plants the optimum the caller
 * supplies: A_0 = sum_i ystar_i A_i - Zstar,  b_i = <A_i, Xstar> (both computed on the device); b is set as objective and
 * returned in b_out[m].  Xstar, Zstar: n x n host arrays; ystar: m host values. */
HIPSDP_API int  hipsdp_gen_planted(hipsdp_solver* solver, int n, int m, long long seed, const double* Xstar, const double* Zstar,
   const double* ystar, double* b_out);
/* the same with matrices of the given density (0 < density <= 1: an off-diagonal entry is nonzero with that probability; SURVEY.md
 * 8(d) names rho = 0.1).  The storage and the assembly stay the dense ones: below the density where the pair formula over nonzeros
 * wins (hipsdp_set_shape2) the three GEMMs are the cheaper formulation whatever the zeros */
HIPSDP_API int  hipsdp_gen_planted_density(hipsdp_solver* solver, int n, int m, long long seed, double density, const double* Xstar,
   const double* Zstar, const double* ystar, double* b_out);
/* copies block k's dense storage A[(m+1) * n * n] back to the host (used to hand identical bits to the CPU baseline) */
HIPSDP_API int  hipsdp_get_block_dense(hipsdp_solver* solver, int block, double* A);

/* ---- host-buffer entry points behind the SCIPlapack* surface (src/sdpi/lapack_interface_hip.c; csrc/host_entries.hip, eigi.hip,
 * psd.hip): every calling thread owns a context per device (own stream, pinned mapped staging, grow-only device pool) - no
 * hipMalloc / hipFree / device-wide synchronisation per call ---- */
/* C[M x N] = alpha * op(A) * op(B) + beta * C, row-major; layA/layB: 0 = K contiguous, 1 = M (resp. N) contiguous */
HIPSDP_API int  hipsdp_dgemm(int device, int layA, int layB, int M, int N, int K, double alpha, const double* A, long long lda,
   const double* B, long long ldb, double beta, double* C, long long ldc, int lower_only, int splitk);
/* shader frequency DURING the Schur assemblies of a solve: with sampling on, ONE thread on a queue of its own (k_clock_window) starts
 * with every assembly and counts its shader-clock cycles and the 100 MHz wall ticks until the assembly's last kernel has set a word
 * (a pair of samples from launches before and after the assembly lands on different XCDs, whose cycle counters are not aligned);
 * *ghz = sum of cycles / sum of wall time over the assemblies of the last solve (0 when none was sampled) */
HIPSDP_API int  hipsdp_set_clock_sampling(hipsdp_solver* solver, int on);
HIPSDP_API int  hipsdp_get_assembly_clock(hipsdp_solver* solver, double* ghz);
HIPSDP_API int  hipsdp_syev(int device, int n, const double* A, double* lam, double* V);     /* ascending, eigenvectors as rows */
/* i-th smallest eigenvalue (1-based) and optionally its unit eigenvector of a symmetric matrix with n <= 128 in one launch through
 * pinned, device-mapped staging memory of the calling thread (no allocation, no copy engine, no stream synchronisation):
 * Householder tridiagonalisation in LDS, Sturm multisection, inverse iteration, back-transformation - one eigenpair as DSYEVR
 * RANGE = 'I' computes it (lapack_interface.c:178-288); n <= 64 with the matrix in registers, 64 < n <= 128 in LDS (round 3).
 * HIPSDP_ERR_ARG for n > 128. */
HIPSDP_API int  hipsdp_syevi_small(int device, int n, const double* A, int i, double* eigval, double* eigvec);
/* all eigenpairs, n <= 128, the same way (what DSYEVR RANGE = 'A' computes, lapack_interface.c:507-603): eigenvalues by multisection,
 * eigenvectors by inverse iteration with re-orthogonalisation inside clusters, one launch; hipsdp_syev takes this path for n <= 128 */
HIPSDP_API int  hipsdp_syev_small(int device, int n, const double* A, double* lam, double* V);
/* Selected eigenpairs of a symmetric matrix of up to 512 rows without a full decomposition (above 128 rows: Householder
 * tridiagonalisation over several workgroups, Sturm multisection for the wanted eigenvalues, inverse iteration and back-transformation
 * of the wanted vectors only - csrc/syevx.hip; up to 128 rows the one-launch kernels above serve the call).  The triangle of A that
 * hipsdp_syevi_small reads is read.  Sign of a vector and basis inside a multiple eigenvalue are free; the returned vectors are
 * orthonormal among themselves.  HIPSDP_ERR_ARG, nothing launched: n < 1, n > HIPSDP_SYEVX_MAXN, il < 1, iu > n, il > iu, more than
 * HIPSDP_SYEVX_MAXK pairs, maxk outside 0 .. HIPSDP_SYEVX_MAXK, A, lam or count NULL.  Same input, same bits.
 * An eigenvalue is the midpoint of its own bisection interval, and the copies of a multiple eigenvalue are made ascending by a running
 * maximum over the returned range: the last bit of lam for one index may differ between calls with another il, and from hipsdp_syevr
 * and hipsdp_syev_small on the same matrix.
 * SCALE RANGE of all eigen entries (hipsdp_syev, hipsdp_syev_small, hipsdp_syevi_small, hipsdp_syevx, hipsdp_syevx_below, hipsdp_syevr,
 * the decompositions behind hipsdp_eigencuts_all): a finite symmetric matrix that is 2^-100 .. 2^100 times a matrix with entries of
 * order 1 .. n - squares of entries and sums of n of them stay far from overflow and underflow there.  Inside the range the accuracy
 * is relative to the norm of the matrix (eigenvalues to 1e-12 of the largest one in absolute value, residuals to 1e-9 of it, vectors
 * orthonormal to 1e-11, whatever the scale), and the zero matrix returns eigenvalues below 1e-200 in absolute value with
 * orthonormal vectors.  Larger or smaller scales, NaN, Inf and non-symmetric input are outside the contract.  hipsdp_check_y: see there. */
#define HIPSDP_SYEVX_MAXN 512
#define HIPSDP_SYEVX_MAXK 32
/* eigenpairs il..iu (1-based, ascending) of the symmetric n x n host matrix A: DSYEVR RANGE='I'.  lam: iu-il+1 values;
 * V: (iu-il+1) x n, one unit eigenvector per row, or NULL (values only, no vector work is done). */
HIPSDP_API int hipsdp_syevx(int device, int n, const double* A, int il, int iu, double* lam, double* V);
/* eigenpairs with eigenvalue <= bound, ascending, at most maxk of them: *count = how many were returned,
 * *nbelow (may be NULL) = how many eigenvalues are <= bound altogether (DSYEVR RANGE='V' with a cap). V may be NULL. */
HIPSDP_API int hipsdp_syevx_below(int device, int n, const double* A, double bound, int maxk, int* count, int* nbelow,
                                  double* lam, double* V);
/* all eigenpairs, ascending, eigenvectors as rows of V (what DSYEVR RANGE = 'A' computes); n <= HIPSDP_SYEVX_MAXN.  Above 128 rows:
 * the tridiagonalisation of hipsdp_syevx, all eigenvalues by multisection over several workgroups, the eigenvectors of the
 * tridiagonal matrix by inverse iteration with re-orthogonalisation inside clusters (per block where the matrix splits), the
 * back-transformation of all n vectors - csrc/syevr.hip; up to 128 rows hipsdp_syev_small.  Conventions of hipsdp_syevx: the same
 * triangle is read, signs and the basis of a multiple eigenvalue are free, the n vectors are orthonormal, same input, same bits.
 * V may be NULL: values only, no vector work is launched.  HIPSDP_ERR_ARG, nothing launched: n < 1, n > HIPSDP_SYEVX_MAXN, A or
 * lam NULL.  hipsdp_syev is not routed here. */
HIPSDP_API int hipsdp_syevr(int device, int n, const double* A, double* lam, double* V);
/* PSD projection chain of the warm-start producer (relax_sdp.c:2715-2766 for Z, :3405-3445 for X), fused on the device: sparse
 * lower/upper triangle (row, col, val; both triangles are filled) -> eigen-decomposition -> eigenvalues below minev (by more
 * than epsilon, SCIPisLT) raised to minev -> recombination -> entries with row <= col and |value| > epsilon in row-major order.
 * mode 0: the reference's literal chain R[i][j] = sum_c V[i][c] lambda_c V[j][c] (V[k][:] = k-th eigenvector; this is what
 * scaleTransposedMatrix + SCIPlapackMatrixMatrixMult(V, TRUE, S, FALSE) evaluate); mode 1: spectral R = sum_k lambda_k v_k v_k^T.
 * cap = length of the output arrays; *nnz_out = entries produced (when it exceeds cap: HIPSDP_ERR_ARG, nothing is written). */
HIPSDP_API int  hipsdp_psd_project(int device, int n, int nnz, const int* row, const int* col, const double* val, double minev, double epsilon,
   int mode, int cap, int* nnz_out, int* rowout, int* colout, double* valout);
/* The projections of ALL blocks of a node - or of many nodes - in one call: the warm-start producer projects Z and X of every block
 * (relax_sdp.c:2680-2774 and :3405-3445 loop over the blocks), 2 B projections for B blocks.  Job j is exactly
 * hipsdp_psd_project(device, n, nnz, row, col, val, minev, epsilon, mode, cap, &nnz_out, rowout, colout, valout): mode 0 the literal
 * chain, mode 1 the spectral form, entries with row <= col and |value| > epsilon in row-major order, an eigenvalue lam is raised
 * when lam - minev < -epsilon.  A job that does not fit its cap gets the needed length in nnz_out and nothing written; the other jobs
 * are written normally and the call returns HIPSDP_ERR_ARG.
 * Jobs of at most 128 rows are BATCHED: whatever their number, the call issues one upload (job table and all triplets through the
 * calling thread's pinned staging), one launch that expands all matrices, at most three for the decompositions, one that recombines
 * and counts, one that writes the packed result, and one device->host synchronisation (csrc/psd_many.hip).  A job above 128 rows
 * takes, inside the same call, the chain of hipsdp_psd_project and returns its bits.  A batched job returns the same bits whatever
 * count is, whatever the other jobs are and wherever it stands in the array (its values agree with hipsdp_psd_project's to rounding:
 * the recombination sums in index order by fma instead of through the GEMM).
 * HIPSDP_ERR_ARG, checked on the host before anything is launched: count < 0 or count > HIPSDP_PSD_MANY_MAXJOBS, jobs NULL with
 * count > 0, device < 0, a mode other than 0 / 1, and per job n < 1, nnz < 0, cap < 0, a triplet index outside the matrix, a NULL
 * array where the length (nnz, cap) is positive.  count == 0: HIPSDP_OK, nothing launched.
 * Outside the contract, as for hipsdp_psd_project: a position that appears twice in a job's triplets.
 * Two host threads may call it at the same time (contexts are thread-local). */
#define HIPSDP_PSD_MANY_MAXJOBS 1024
typedef struct hipsdp_psd_job {
   int n, nnz;                       /* in: order of the matrix; triplets (both triangles are filled, as hipsdp_psd_project) */
   const int *row, *col; const double* val;
   double minev;                     /* in: per job (the reference uses warmstartmevdual for Z, warmstartmevprimal for X) */
   int cap;                          /* in: length of rowout / colout / valout */
   int nnz_out;                      /* out: entries the projection has (the needed length when it exceeds cap) */
   int *rowout, *colout; double* valout;
} hipsdp_psd_job;
HIPSDP_API int hipsdp_psd_project_many(int device, int count, hipsdp_psd_job* jobs, double epsilon, int mode);
/* process totals: calls with count > 0 that passed the argument checks, kernel launches they issued for batched jobs, device->host
 * synchronisations they waited on (one for all batched jobs of a call, one more per job above 128 rows); any pointer may be NULL */
HIPSDP_API int hipsdp_psd_project_many_stats(long long* calls, long long* launches, long long* readbacks);
/* The partner of hipsdp_psd_project_many for jobs of HIPSDP_PSD_LARGE_MINN .. HIPSDP_PSD_LARGE_MAXN rows: all of them go through the
 * same launches instead of the single-call chain one after the other (csrc/psd_large.hip).  Job structure, modes, epsilon rule, output
 * order, cap rule, HIPSDP_PSD_MANY_MAXJOBS and the argument-error list are those of hipsdp_psd_project_many: a kept entry has
 * row <= col and |value| > epsilon, row-major order; an eigenvalue lam is raised when lam - minev < -epsilon; a job that does not fit
 * its cap gets the needed length in nnz_out and nothing written, the others are written and the call returns HIPSDP_ERR_ARG.
 * A job with n < HIPSDP_PSD_LARGE_MINN or n > HIPSDP_PSD_LARGE_MAXN is NOT SERVED: nnz_out = -1, nothing written, the call still
 * returns HIPSDP_OK and serves the others (the convention of hipsdp_eigencuts_all_large); hand such jobs to hipsdp_psd_project_many.
 * DECOMPOSITION: through the tridiagonal form - eigenvalues and eigenvectors of a served job are, bit for bit, what hipsdp_syevr
 * returns for its expanded matrix alone (NOT the block Jacobi of hipsdp_psd_project / hipsdp_syev).
 * mode 0 depends on the basis and the signs of the eigenvectors: its result is the literal chain of hipsdp_psd_project evaluated on
 * hipsdp_syevr's vectors, so it agrees with hipsdp_psd_project(mode 0) only as far as the two bases agree.  mode 1 does not depend on
 * the basis and agrees with hipsdp_psd_project(mode 1) to rounding.
 * LAUNCHES: the served jobs are taken in chunks of at most 512 MiB of device workspace (HIPSDP_PSD_LARGE_CHUNK = MiB overrides the
 * limit; a chunk holds at least one job).  A chunk whose largest job has nmax rows issues one upload, then
 *      nmax + 8 + 6 ceil(nmax / 32)
 * kernel launches whatever the number of its jobs (1 expand, nmax - 1 columns of the tridiagonalisation, 2 for the eigenvalues,
 * 3 + 6 ceil(nmax / 32) for the eigenvectors of the tridiagonal matrices, 1 back-transformation, 1 recombination, 1 write), one
 * device->host copy and one synchronisation.  The bits of a job do not depend on count, on the other jobs, on the job's position,
 * on the chunking or on the calling thread.  Two host threads may call it at the same time (contexts are thread-local).
 * HIPSDP_ERR_ARG is checked on the host before the device is looked at; count == 0: HIPSDP_OK, nothing launched. */
#define HIPSDP_PSD_LARGE_MINN 129
#define HIPSDP_PSD_LARGE_MAXN 512
HIPSDP_API int hipsdp_psd_project_many_large(int device, int count, hipsdp_psd_job* jobs, double epsilon, int mode);
/* process totals: calls with count > 0 that passed the argument checks, kernel launches they issued, device->host synchronisations
 * they waited on (one per chunk); any pointer may be NULL */
HIPSDP_API int hipsdp_psd_project_many_large_stats(long long* calls, long long* launches, long long* readbacks);
/* The device work of the PRIMAL ROUNDING PROBLEM of a warm-started node (relax/warmstartproject = 4: solvePrimalRoundingProblem,
 * relax_sdp.c:1551-2640) in two calls.  The reference decomposes the start matrix X* of every block (:1875-1877), computes for EVERY
 * eigenvector v_j of a block - all n_b of them - the coefficients of the rounding LP, obj[j] = v_j^T A_0 v_j (:1906-1923) and
 * val[j][i] = v_j^T A_i v_j (:1926-1947), and recombines V^T diag(lambda) V once for X from the primal rounding LP (:2164-2207) and once
 * for Z from the dual one (:2550-2591), both on the same eigenvectors.  off_b = n_0 + .. + n_{b-1}, N = sum n_b.
 * STAGE 1, hipsdp_rounding_frame: X_b as the triplets of expandSparseMatrix (relax_sdp.c:243-277; the convention of hipsdp_psd_project:
 * both triangles are filled, a position named twice is outside the contract, xnnz[b] = 0 is the zero matrix).  For a served block:
 *     eigvals[off_b + j]            the eigenvalues of X_b, ascending;
 *     obj[off_b + j]              = v_j^T A_0^b v_j;
 *     coefs[(off_b + j) m + i]    = v_j^T A_{i+1}^b v_j - the reference's val[evind * nvars + varind], dense: dropping the SCIPisZero
 *                                   entries stays with the caller; variables are the engine's, as in hipsdp_eigencuts;
 *     vecs[sum_{k<b} n_k^2 + j n_b + r] = component r of v_j (vecs may be NULL): the caller builds the -V_iv V_jv rows of the dual
 *                                   rounding LP (:2353-2375) from it on the host;
 *     served[b]                   = 0: block b is served; -1: it is not, and none of its slots is written.  served may be NULL.
 * The eigenvectors stay on the device: the solver's ROUNDING FRAME, a grow-only allocation of N + sum n_b^2 doubles.
 * Served: blocks of 1 .. 512 rows of a solver without communicator and without sharded matrices, in all three storage forms, all size
 * classes in one call.  Not served: a block of more than 512 rows or without matrices on this device; the others are still served.  A
 * solver with a communicator or sharded matrices: every served = -1, nothing launched, HIPSDP_OK.
 * HIPSDP_ERR_ARG, before the device is looked at and with nothing launched: solver NULL or without a shape; xnnz, eigvals, obj or coefs
 * NULL; xnnz[b] < 0; a NULL triplet array with xnnz[b] > 0; an index outside the block.
 * EIGENPAIRS of a served block are, bit for bit, those of hipsdp_syev_small (up to 128 rows) or hipsdp_syevr (129 .. 512 rows) on the
 * expanded matrix alone; the SCALE RANGE paragraph above applies.  A block of one row is a scalar.
 * COEFFICIENTS: blocks of more than 64 rows held as packed triangles or dense rows go through a GEMM over the storage index p on
 * v_mfma_f64_16x16x4_f64 - C[j][i] = sum_p P[j][p] A_i[p], P[j][p] = w_p V[j][r_p] V[j][c_p], w = 1 on the diagonal of a packed triangle
 * and 2 off it, formed from V while it is staged; tiles of 64 vectors x 64 matrices, p ascending, and for a block with few tiles p in
 * slices whose number depends on (n_b, m) alone and whose partial tables are added in slice order.  Blocks of at most 64 rows and blocks
 * kept as nonzeros: one thread per (vector, matrix) sums over the stored entries in storage order (csrc/rounding.hip).
 * STAGE 2, hipsdp_rounding_recombine, any number of times per frame: R_b = the recombination of the frame's vectors of block b with
 * lambda[off_b .. off_b + n_b), used as given (nothing is clamped):
 *     mode 0  R[i][j] = sum_c V[i][c] lambda_c V[j][c], the reference's literal chain (scaleTransposedMatrix +
 *             SCIPlapackMatrixMatrixMult(V, TRUE, S, FALSE), :2172-2183), mode 0 of hipsdp_psd_project;
 *     mode 1  R = sum_k lambda_k v_k v_k^T.
 * Output per block as hipsdp_psd_project_many writes it: the entries with row <= col and |value| > epsilon in row-major order, their
 * number in nnz_out; a block over its cap gets the needed length in nnz_out and nothing written, the others are written and the call
 * returns HIPSDP_ERR_ARG; a block the frame does not hold gets nnz_out = -1.  The launches are those of hipsdp_psd_project_many (up to
 * 128 rows) and hipsdp_psd_project_many_large (above), on jobs that point at the frame.
 * It needs a frame: HIPSDP_ERR_ARG without one, and for solver, lambda or out NULL, a mode other than 0 / 1, cap < 0, a NULL output
 * array with cap > 0.  The frame lives from a hipsdp_rounding_frame that returned HIPSDP_OK until the next hipsdp_rounding_frame,
 * hipsdp_set_shape* or hipsdp_free; it does not depend on the constraint matrices, so writing them does not invalidate it.
 * LAUNCHES.  The served blocks are taken by descending size in chunks of at most 512 MiB of the solver's cut workspace
 * (HIPSDP_ROUNDING_CHUNK in the environment, read at every call: blocks per chunk instead); the frame itself is not chunked.  Every chunk
 * issues one upload and ONE read-back, and with [..] = 1 when the chunk has a block of that class and nmax the rows of its largest block
 * above 128 rows:
 *     stage 1:  [1 .. 128 rows] 4 + [129 .. 512 rows] (nmax + 6 + 6 ceil(nmax / 32)) + 4
 *     stage 2:  [1 .. 128 rows] 2 + [129 .. 512 rows] 2
 * (stage 1: per class the expand launch and the decomposition - 3 launches up to 128 rows, nmax - 1 columns, 5 + 6 ceil(nmax / 32) for
 * the values and vectors of the tridiagonal matrices and the back-transformation above; then the move into the frame, the two
 * coefficient launches and the store) - a function of the classes present and of nmax alone, never of the number of blocks.
 * The bits of a block depend on its X and its matrices (stage 1), or on its V and lambda (stage 2), alone - not on the other blocks,
 * their order or the chunks; same input, same bits; no floating-point atomics.  Two host threads may call either function at the same
 * time on different solvers. */
HIPSDP_API int hipsdp_rounding_frame(hipsdp_solver* solver,
   const int* xnnz, const int* const* xrow, const int* const* xcol, const double* const* xval,   /* per block: triplets of X_b */
   double* eigvals /* N */, double* obj /* N */, double* coefs /* N x m */, double* vecs /* sum n_b^2, may be NULL */,
   int* served /* nblocks, may be NULL */);
typedef struct hipsdp_rounding_out { int cap; int nnz_out; int *rowout, *colout; double* valout; } hipsdp_rounding_out;
HIPSDP_API int hipsdp_rounding_recombine(hipsdp_solver* solver, const double* lambda /* N */, double epsilon, int mode,
   hipsdp_rounding_out* out /* nblocks */);
/* process totals of both stages: calls that launched something, kernel launches they issued, device->host synchronisations they
 * waited on (one per chunk); any pointer may be NULL.  The totals of the other calls do not move, and the reverse */
HIPSDP_API int hipsdp_rounding_stats(long long* calls, long long* launches, long long* readbacks);
HIPSDP_API int  hipsdp_gemv_n(int device, int R, long long E, const double* A, int nv, const double* V, double* out);
HIPSDP_API int  hipsdp_gemv_t(int device, int R, long long E, const double* A, const double* coef, double* out);

#ifdef __cplusplus
}
#endif

#endif
