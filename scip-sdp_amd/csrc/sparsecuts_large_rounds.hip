/* sparsecuts_large_rounds.hip - sparse eigenvector cuts of ALL blocks of 129 .. 512 rows of a solver per launch, the reference's three
 * refinement switches included (hipsdp_sparsecuts_all_large; host side: cut_calls.hip).
 *
 * A block of this size does not fit into LDS: its M = maxeig I - Z lives transposed in global memory and ONE workgroup of 512 threads
 * runs the truncated power method on it (hs_scl_tpower.h, the body of k_sc_tpower_large), and (lmin, v0), maxeig come from the batched
 * tridiagonal path of syevx.hip (hs_syevx_many_cols / hs_syevx_many_select), whose column launches hold the matrices of all blocks.
 *
 *    k_sclr_stage       grid (G, blocks), 256 threads    the current Z of every block with act != 0 into the workspace of its
 *                                                        tridiagonalisation (which consumes it), zeros into the reflector array
 *    k_sclr_tpower_all  grid (blocks), 512 threads       variant 0: the whole loop over cuts and iterations, a block per workgroup
 *    k_sclr_tpower      grid (blocks), 512 threads       variant != 0, one ROUND (sparsecuts_rounds.hip): M^T rebuilt from the
 *                                                        deflated Z and the block's maxeig, ONE TPower run from its current start vector,
 *                                                        the decision; without recomputesparseev the cut (Z -= value x x^T on the size^2
 *                                                        pairs, in place in global memory), with it the support and the gather of Z_S
 *    k_sclr_cut         grid (blocks), 512 threads       with recomputesparseev, behind hs_syev_small_many on the Z_S: the lambda >= -tol
 *                                                        rule, w normalised and lifted, the cut
 *    k_sclr_coefs       grid (m + 1, blocks), 256 thr.   x_c^T A_i x_c of every cut of every block
 *
 * The state of a block (hs_scr_state: maxeig, cuts, iterations, flags, done) lives in the workspace between the launches.  A block
 * whose loop has ended has done = 1 and act = 0: the kernels here return at once for it - the test is uniform over the workgroup and
 * stands before the first barrier - and its matrix takes no part in the tridiagonalisations that follow.
 * HAZARD RULE: no grid barrier, no flag, no waiting on another workgroup, no atomic operation.  Workgroup j of a launch reads and writes
 * the memory of block j alone (its Z, MT, state, Z_S, act[j], its slots of the result); the tables and y are read-only; stream order
 * is the only synchronisation between launches.  Inside the TPower kernels SCL_STORES_DONE and a workgroup barrier stand between the
 * workgroup's stores to MT and its later loads; Z is read (the fill, at the start) and written (the cut, behind the run's barriers) by
 * the same workgroup.  Every loop is bounded by maxit, maxcuts or the block's rows, and every loop condition is false for a NaN.
 * The bits of a block depend on the block alone: no sum crosses workgroups, and the column launches give a matrix the same bits for
 * every number of workgroups (syevx.hip). */
#include "hs_kernels.h"
#include "hs_scl_tpower.h"

#define SCLR_ST 256        /* k_sclr_stage */

/* The current Z of block blockIdx.y into the workspace of its tridiagonalisation, in the form hs_syevx_tridiag_dev gives it: the
 * triangle at the memory positions [c n + i], i >= c, mirrored - symmetric to the bit.  init_zs (the stage launch in front of round 0,
 * with recomputesparseev): every Z_S becomes the identity, a matrix the decompositions of every round can take whether its block ever
 * gathers one or not. */
__global__ void __launch_bounds__(SCLR_ST) k_sclr_stage(const hs_ec_job* __restrict__ jobs, const hs_sxm_job* __restrict__ sx,
   const hs_sclr_job* __restrict__ xjobs, const int* __restrict__ sizes, const int* __restrict__ act, int init_zs)
{
   const int j = blockIdx.y;
   if ( init_zs && blockIdx.x == 0 )
   {
      const int ns = sizes[jobs[j].blk];
      double* __restrict__ ZS = xjobs[j].ZS;
      if ( ZS != NULL && ns >= 1 && ns <= HS_SC_MAXN )
         for (int e = threadIdx.x; e < ns * ns; e += SCLR_ST)
            ZS[e] = e / ns == e % ns ? 1.0 : 0.0;
   }
   if ( act[j] == 0 )
      return;
   const int n = jobs[j].n;
   const double* __restrict__ Z = jobs[j].Z;
   double* __restrict__ A = sx[j].A;
   double* __restrict__ R = sx[j].R;
   for (int idx = blockIdx.x * SCLR_ST + threadIdx.x; idx < n * n; idx += gridDim.x * SCLR_ST)
   {
      const int i = idx / n, c = idx - i * n;
      A[idx] = (c <= i) ? Z[(size_t) c * n + i] : Z[(size_t) i * n + c];
      R[idx] = 0.0;
   }
}

__global__ void __launch_bounds__(SCL_NT) k_sclr_tpower_all(int m, const hs_ec_job* __restrict__ jobs, const hs_sxm_job* __restrict__ sx,
   const hs_sclr_job* __restrict__ xjobs, const int* __restrict__ sizes, hs_sc_par par, hs_sc_out out)
{
   SCL_LDS_DECL(L);
   const hs_ec_job job = jobs[blockIdx.x];
   const hs_sxm_job X = sx[blockIdx.x];
   const hs_sclr_job xj = xjobs[blockIdx.x];
   scl_tpower_loop(job.n, sizes[job.blk], job.Z, X.out[HS_SYEVX_OUT_LAM], X.out2[HS_SYEVX_OUT_LAM], X.out + HS_SYEVX_OUT_VEC, xj.MT, par,
      scl_block_view(out, job.blk, par.maxcuts, m, xj.vecoff), L);
}

/* the block's loop has ended: its counts go to the result, done = 1 and act = 0 keep every later launch away from it */
__device__ __forceinline__ void sclr_finish(hs_scr_state* S, const hs_sc_out& o, int* act, int nc, int iters, int flags)
{
   if ( threadIdx.x == 0 )
   {
      o.ncuts[0] = nc; o.iters[0] = iters; o.flags[0] = flags;
      S->nc = nc; S->iters = iters; S->flags = flags; S->done = 1;
      *act = 0;
   }
}

/* Cut nc of a block, by all threads of its workgroup (o: the view of the block): value, the dense vector (xi: this thread's entry, an
 * exact zero off the support) and the ascending support go to the result; Z -= value x x^T on the size^2 pairs of the support, in
 * place; maxeig -= value (with exacttrans the tridiagonalisation that follows replaces it).  xs, sup: values and indices on the support,
 * in LDS, complete before the call. */
__device__ __forceinline__ void sclr_apply_cut(int n, double* Z, hs_scr_state* S, const hs_sc_out& o, int* act, int act_on, int size, int nc,
   int iters, int flags, double maxeig, double value, double xi, const double* xs, const int* sup)
{
   const int tid = threadIdx.x;
   if ( tid == 0 )
      o.eig[nc] = value;
   if ( tid < n )
      o.vec[(long long) nc * n + tid] = xi;
   if ( tid < size )
      o.sup[(long long) nc * o.smax + tid] = sup[tid];
   for (int e = tid; e < size * size; e += SCL_NT)
   {
      const int p = e / size, q = e - p * size;
      const double t = value * xs[p] * xs[q];
      Z[(size_t) sup[p] * n + sup[q]] -= t;
   }
   if ( tid == 0 )
   {
      S->maxeig = maxeig - value;
      S->nc = nc + 1; S->iters = iters; S->flags = flags; S->done = 0;
      *act = act_on;
   }
}

__global__ void __launch_bounds__(SCL_NT) k_sclr_tpower(int m, const hs_ec_job* __restrict__ jobs, const hs_sxm_job* __restrict__ sx,
   const hs_sclr_job* __restrict__ xjobs, const int* __restrict__ sizes, hs_sc_par par, unsigned variant, int round, int act_on, int* act,
   hs_sc_out out)
{
   SCL_LDS_DECL(L);
   const int j = blockIdx.x, tid = threadIdx.x;
   const hs_ec_job job = jobs[j];
   const hs_sxm_job X = sx[j];
   const hs_sclr_job xj = xjobs[j];
   hs_scr_state* S = xj.st;
   const int n = job.n, size = sizes[job.blk];
   const bool sparseev = (variant & HS_SCR_SPARSEEV) != 0, initial = (variant & HS_SCR_INITIAL) != 0;
   const hs_sc_out o = scl_block_view(out, job.blk, par.maxcuts, m, xj.vecoff);
   double maxeig;
   int nc = 0, iters = 0, flags = 0;
   if ( round == 0 )
   {
      const double lmin = X.out[HS_SYEVX_OUT_LAM];
      if ( tid == 0 )
         o.lmin[0] = lmin;
      if ( n < 1 || n > SCL_NT || !(lmin < -par.tol) || size > n || size < 1 || par.maxcuts <= 0 || (sparseev && size > HS_SC_MAXN) )
      {
         sclr_finish(S, o, act + j, 0, 0, 0);
         return;
      }
      maxeig = X.out2[HS_SYEVX_OUT_LAM];
   }
   else
   {
      if ( S->done )
         return;
      maxeig = (variant & HS_SCR_EXACTTRANS) ? X.out2[HS_SYEVX_OUT_LAM] : S->maxeig;
      nc = S->nc; iters = S->iters; flags = S->flags;
   }
   const bool row = tid < n;
   scl_fill_mt(n, job.Z, maxeig, xj.MT, L.zd);
   {
      /* the start vector: the first eigenvector of the tridiagonal path - of Z(y) in round 0, of the deflated Z with recomputeinitial -
       * or the one of round 0, kept with the block's state */
      double v = 0.0;
      if ( row )
      {
         v = (round == 0 || initial) ? X.out[HS_SYEVX_OUT_VEC + tid] : xj.v0[tid];
         if ( round == 0 && !initial )
            xj.v0[tid] = v;
      }
      L.v0s[tid] = v;
   }
   L.keys[tid] = -1;
   L.sup[tid] = 0;
   const double* mcol = xj.MT + (row ? tid : 0);
   /* ---- one TPower run from v0 on M ---- */
   const scl_run run = scl_tpower_run(n, size, row, mcol, L, par.convtol, par.maxit);
   const double newv = run.newv, oldv = run.oldv;
   const int it = run.it;
   iters += it;
   /* ---- the decision (all of it uniform over the workgroup) ---- */
   bool cut = false;
   double scalar = 0.0;
   if ( run.dead )
      flags |= 2;
   else if ( it > 0 )            /* (it == 0 - convtol >= 1: no iterate, no support) */
   {
      if ( it >= par.maxit && newv - oldv > par.convtol )
         flags |= 1;
      scalar = maxeig - newv;
      cut = scalar < -par.feastol && nc < par.maxcuts;
   }
   if ( !cut )
   {
      sclr_finish(S, o, act + j, nc, iters, flags);
      return;
   }
   if ( !sparseev )
   {
      sclr_apply_cut(n, job.Z, S, o, act + j, act_on, size, nc, iters, flags, maxeig, scalar, run.x, L.xc, L.sup);
      return;
   }
   /* recomputesparseev: the support and the principal submatrix Z_S of the current Z (ascending support) for the decomposition that
    * follows; k_sclr_cut takes the cut from its smallest eigenpair */
   if ( tid < size )
      o.sup[(long long) nc * o.smax + tid] = L.sup[tid];
   for (int e = tid; e < size * size; e += SCL_NT)
   {
      const int p = e / size, q = e - p * size;
      xj.ZS[e] = job.Z[(size_t) L.sup[p] * n + L.sup[q]];
   }
   if ( tid == 0 )
   {
      S->maxeig = maxeig;
      S->nc = nc; S->iters = iters; S->flags = flags; S->done = 0;
      act[j] = act_on;
   }
}

__global__ void __launch_bounds__(SCL_NT) k_sclr_cut(int m, const hs_ec_job* __restrict__ jobs, const hs_sclr_job* __restrict__ xjobs,
   const int* __restrict__ sizes, hs_sc_par par, int* act, hs_sc_out out)
{
   __shared__ double xs[HS_SC_MAXN];         /* w on the support */
   __shared__ double xd[HS_SCL_MAXN];        /* w lifted */
   __shared__ int sup[HS_SC_MAXN];
   const int j = blockIdx.x, tid = threadIdx.x;
   const hs_ec_job job = jobs[j];
   const hs_sclr_job xj = xjobs[j];
   hs_scr_state* S = xj.st;
   if ( S->done )
      return;
   const int n = job.n, size = sizes[job.blk];
   if ( n > HS_SCL_MAXN || size < 1 || size > HS_SC_MAXN || size > n )      /* (never: such a block is finished in round 0) */
      return;
   const hs_sc_out o = scl_block_view(out, job.blk, par.maxcuts, m, xj.vecoff);
   const int nc = S->nc, iters = S->iters, flags = S->flags;
   const double maxeig = S->maxeig;
   const double lambda = xj.wsS[0];          /* the smallest eigenvalue of Z_S; its vector is row 0 behind vposS */
   if ( !(lambda < -par.tol) )               /* cons_sdp.c:1487: the loop ends, no cut from this run */
   {
      sclr_finish(S, o, act + j, nc, iters, flags | 4);
      return;
   }
   if ( tid < size )
   {
      sup[tid] = o.sup[(long long) nc * o.smax + tid];
      xs[tid] = xj.wsS[xj.vposS + tid];
   }
   if ( tid < n )
      xd[tid] = 0.0;
   __syncthreads();
   double s = 0.0;                           /* (:1493-1499; every thread forms the same sum in the same order) */
   for (int p = 0; p < size; ++p)
      s += xs[p] * xs[p];
   const double nrm = sqrt(s);
   __syncthreads();
   if ( tid < size )
   {
      const double v = xs[tid] / nrm;
      xs[tid] = v;
      xd[sup[tid]] = v;
   }
   __syncthreads();
   sclr_apply_cut(n, job.Z, S, o, act + j, act[j], size, nc, iters, flags, maxeig, lambda, tid < n ? xd[tid] : 0.0, xs, sup);
}

__global__ void __launch_bounds__(SCL_CT) k_sclr_coefs(int m, int maxcuts, const hs_ec_job* __restrict__ jobs,
   const hs_sclr_job* __restrict__ xjobs, const int* __restrict__ sizes, hs_sc_out out)
{
   __shared__ double xs[HS_SCL_MAXN];
   __shared__ int sup[HS_SCL_MAXN];
   __shared__ double part[SCL_CT / 64];
   const hs_ec_job job = jobs[blockIdx.y];
   scl_coefs_block(m, maxcuts, sizes[job.blk], (int) blockIdx.x, job, scl_block_view(out, job.blk, maxcuts, m, xjobs[blockIdx.y].vecoff), xs,
      sup, part);
}

/* workgroups per block of the stage launch: 64 rows of 256 entries cover a matrix of 128 rows in one pass, 512 rows in sixteen */
#define SCLR_STAGE_G 64

int hs_sclr_stage(hipStream_t st, int count, const hs_ec_job* jobs, const hs_sxm_job* sx, const hs_sclr_job* xjobs, const int* sizes,
   const int* act, int init_zs)
{
   if ( count < 1 || jobs == NULL || sx == NULL || xjobs == NULL || sizes == NULL || act == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_sclr_stage, dim3(SCLR_STAGE_G, count), dim3(SCLR_ST), 0, st, jobs, sx, xjobs, sizes, act, init_zs);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_sclr_tpower_all(hipStream_t st, int count, int m, const hs_ec_job* jobs, const hs_sxm_job* sx, const hs_sclr_job* xjobs, const int* sizes,
   const hs_sc_par* par, const hs_sc_out* out)
{
   if ( count < 1 || m < 0 || jobs == NULL || sx == NULL || xjobs == NULL || sizes == NULL || out->smax < 1 || out->smax > HS_SCL_MAXN )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_sclr_tpower_all, dim3(count), dim3(SCL_NT), 0, st, m, jobs, sx, xjobs, sizes, *par, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_sclr_tpower(hipStream_t st, int count, int m, const hs_ec_job* jobs, const hs_sxm_job* sx, const hs_sclr_job* xjobs, const int* sizes,
   const hs_sc_par* par, unsigned variant, int round, int act_on, int* act, const hs_sc_out* out)
{
   if ( count < 1 || m < 0 || jobs == NULL || sx == NULL || xjobs == NULL || sizes == NULL || act == NULL || round < 0 || out->smax < 1
      || out->smax > HS_SCL_MAXN )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_sclr_tpower, dim3(count), dim3(SCL_NT), 0, st, m, jobs, sx, xjobs, sizes, *par, variant, round, act_on, act, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_sclr_cut(hipStream_t st, int count, int m, const hs_ec_job* jobs, const hs_sclr_job* xjobs, const int* sizes, const hs_sc_par* par,
   int* act, const hs_sc_out* out)
{
   if ( count < 1 || jobs == NULL || xjobs == NULL || sizes == NULL || act == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_sclr_cut, dim3(count), dim3(SCL_NT), 0, st, m, jobs, xjobs, sizes, *par, act, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_sclr_coefs(hipStream_t st, int count, int m, int maxcuts, const hs_ec_job* jobs, const hs_sclr_job* xjobs, const int* sizes,
   const hs_sc_out* out)
{
   if ( maxcuts <= 0 || count < 1 )
      return HS_OK;
   hipLaunchKernelGGL(k_sclr_coefs, dim3(m + 1, count), dim3(SCL_CT), 0, st, m, maxcuts, jobs, xjobs, sizes, out[0]);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
