/* sparsecuts_rounds.hip - the loop of sparsecuts.hip as a fixed sequence of rounds, for the reference's three refinement switches
 * recomputesparseev, recomputeinitial and exacttrans (cons_sdp.c:1460-1514, :1532-1550, :1552-1568; hipsdp_sparsecuts_all_ex,
 * hipsdp_sparsecuts_ex with variant != 0).  Each of the switches puts an eigen-decomposition between two TPower runs, so the loop over
 * the cuts of k_sc_tpower cannot stay inside one launch: here a round is one TPower run of every block and what its cut needs, and the
 * state of a block lives in the workspace between the launches - the deflated Z in place in job.Z, the rest in its hs_scr_state.
 *
 *    k_scr_tpower     grid (blocks), 128 threads      a block per workgroup, thread i = row i: M = maxeig I - Z built in LDS from the
 *                                                     current Z, ONE TPower run from the block's current start vector, the decision
 *                                                     (dead iterate, no iterate, scalar, cut limit); then, without recomputesparseev,
 *                                                     the cut itself, and with it the gather of Z_S for the decomposition that follows
 *    k_scr_cut        grid (blocks), 128 threads      with recomputesparseev: the lambda >= -tol rule, w normalised and lifted, the cut
 *
 * The decompositions between them are hs_syev_small_many (csrc/eigi.hip) on two static job tables: the Z_S (n = sizes[b]) and the
 * blocks' own jobs (the deflated Z; it refreshes lam[0], the first vector and lam[n - 1] in job.ws).  A block whose loop has ended has
 * done = 1: both kernels return at once for it - the test is uniform over the workgroup and stands before the first barrier - and
 * what the decompositions compute for it is never read.  Nothing waits on another workgroup: no flag, no grid barrier, no atomic
 * operation; the order of the stream is the only synchronisation.  A TPower run is sc_tpower_run of hs_sc_tpower.h, the one
 * k_sc_tpower calls: the row product, the ranking with the smaller-index tie rule, the block sum and the stop rule give the same
 * summands in the same order.  Every loop condition is false for a NaN, and every loop is bounded by maxit, maxcuts or the block's
 * rows. */
#include "hs_kernels.h"
#include "hs_sc_tpower.h"

#define SCR_NT SC_NT       /* 128: one thread per row, HS_SC_MAXN rows at most */

/* dynamic LDS of k_scr_tpower for a block of n rows: M | x on its support | |w| | v0 | red[2] | support (int) | kept per wavefront
 * (int[2]); at 128 rows 135.7 KB of the 160 KB of a compute unit - a second n x n array does not fit, Z stays in its slab */
static size_t scr_lds(int n)
{
   return ((size_t) n * (n | 1) + 3 * (size_t) n + 2) * sizeof(double) + ((size_t) n + 2) * sizeof(int);
}

/* the block's loop has ended: its counts go to the result block, and done = 1 keeps every later launch away from it */
__device__ __forceinline__ void scr_finish(hs_scr_state* S, const hs_sc_out& out, int blk, int nc, int iters, int flags)
{
   if ( threadIdx.x == 0 )
   {
      out.ncuts[blk] = nc; out.iters[blk] = iters; out.flags[blk] = flags;
      S->nc = nc; S->iters = iters; S->flags = flags; S->done = 1;
   }
}

/* Cut nc of a block, by all threads of its workgroup: value, the dense vector (xi: this thread's entry, an exact zero off the support)
 * and the ascending support go to the result block; Z -= value x x^T on the size^2 pairs of the support, in place in the block's slab;
 * maxeig -= value (with exacttrans the decomposition that follows replaces it).  xs, sup: values and indices on the support, in LDS,
 * complete before the call. */
__device__ __forceinline__ void scr_apply_cut(const hs_ec_job& job, hs_scr_state* S, const hs_sc_out& out, int maxcuts, int size, int nc,
   int iters, int flags, double maxeig, double value, double xi, const double* xs, const int* sup)
{
   const int n = job.n, tid = threadIdx.x;
   const long long slot = (long long) job.blk * maxcuts + nc;
   if ( tid == 0 )
      out.eig[slot] = value;
   if ( tid < n )
      out.vec[job.vecoff + (long long) nc * n + tid] = xi;
   if ( tid < size )
      out.sup[slot * out.smax + tid] = sup[tid];
   for (int e = tid; e < size * size; e += SCR_NT)
   {
      const int p = e / size, q = e - p * size;
      const double t = value * xs[p] * xs[q];
      job.Z[sup[p] * n + sup[q]] -= t;
   }
   if ( tid == 0 )
   {
      S->maxeig = maxeig - value;
      S->nc = nc + 1; S->iters = iters; S->flags = flags; S->done = 0;
   }
}

__global__ void __launch_bounds__(SCR_NT) k_scr_tpower(const hs_ec_job* __restrict__ jobs, const hs_scr_job* __restrict__ xjobs,
   const int* __restrict__ sizes, hs_sc_par par, unsigned variant, int round, hs_sc_out out)
{
   extern __shared__ __attribute__((aligned(16))) double scr_mem[];
   const hs_ec_job job = jobs[blockIdx.x];
   const hs_scr_job xj = xjobs[blockIdx.x];
   hs_scr_state* S = xj.st;
   const int n = job.n, pitch = n | 1, tid = threadIdx.x;
   const int size = sizes[job.blk];
   const double* __restrict__ lam = job.ws;
   const bool sparseev = (variant & HS_SCR_SPARSEEV) != 0, initial = (variant & HS_SCR_INITIAL) != 0;
   double maxeig;
   int nc = 0, iters = 0, flags = 0;
   if ( round == 0 )
   {
      const double lmin = lam[0];
      if ( tid == 0 )
         out.lmin[job.blk] = lmin;
      if ( !(lmin < -par.tol) || size > n || par.maxcuts <= 0 )
      {
         /* (its Z_S job, of one row when size > n, is decomposed in every round all the same: a matrix it can take) */
         const int ns = size <= n ? size : 1;
         if ( sparseev )
            for (int e = tid; e < ns * ns; e += SCR_NT)
               xj.ZS[e] = e / ns == e % ns ? 1.0 : 0.0;
         scr_finish(S, out, job.blk, 0, 0, 0);
         return;
      }
      maxeig = lam[n - 1];
   }
   else
   {
      if ( S->done )
         return;
      maxeig = (variant & HS_SCR_EXACTTRANS) ? lam[n - 1] : S->maxeig;
      nc = S->nc; iters = S->iters; flags = S->flags;
   }
   double* Ms = scr_mem;                     /* M = maxeig I - Z, row i at Ms + i pitch */
   double* xc = Ms + (size_t) n * pitch;     /* x on its support: xc[p] = x[sup[p]] */
   double* aw = xc + n;
   double* v0s = aw + n;
   double* red = v0s + n;
   int* sup = reinterpret_cast<int*>(red + 2);
   int* wkept = sup + n;
   const bool row = tid < n;
   for (int e = tid; e < n * n; e += SCR_NT)
   {
      const int r = e / n, c = e - r * n;
      const double z = job.Z[e];
      Ms[r * pitch + c] = r == c ? maxeig - z : -z;
   }
   if ( row )
   {
      /* the start vector: the first eigenvector of the decomposition in job.ws - of Z(y) in round 0, of the deflated Z with
       * recomputeinitial - or the one of round 0, kept in the block's state because exacttrans overwrites job.ws */
      const double v = (round == 0 || initial) ? job.ws[job.vpos + tid] : xj.v0[tid];
      v0s[tid] = v;
      if ( round == 0 && !initial )
         xj.v0[tid] = v;
   }
   const double* mrow = Ms + (row ? tid : 0) * pitch;
   /* ---- one TPower run from v0 on M ---- */
   const sc_run run = sc_tpower_run(n, size, row, mrow, v0s, aw, xc, sup, wkept, red, par.convtol, par.maxit);
   const double x = run.x, newv = run.newv, oldv = run.oldv;
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
      if ( sparseev && round == 0 )          /* no Z_S was ever gathered: a matrix the decompositions of the later rounds can take */
         for (int e = tid; e < size * size; e += SCR_NT)
            xj.ZS[e] = e / size == e % size ? 1.0 : 0.0;
      scr_finish(S, out, job.blk, nc, iters, flags);
      return;
   }
   if ( !sparseev )
   {
      scr_apply_cut(job, S, out, par.maxcuts, size, nc, iters, flags, maxeig, scalar, x, xc, sup);
      return;
   }
   /* recomputesparseev: the support and the principal submatrix Z_S of the current Z (ascending support) for the decomposition that
    * follows; k_scr_cut takes the cut from its smallest eigenpair */
   const long long slot = (long long) job.blk * par.maxcuts + nc;
   if ( tid < size )
      out.sup[slot * out.smax + tid] = sup[tid];
   for (int e = tid; e < size * size; e += SCR_NT)
   {
      const int p = e / size, q = e - p * size;
      xj.ZS[e] = job.Z[sup[p] * n + sup[q]];
   }
   if ( tid == 0 )
   {
      S->maxeig = maxeig;
      S->nc = nc; S->iters = iters; S->flags = flags; S->done = 0;
   }
}

__global__ void __launch_bounds__(SCR_NT) k_scr_cut(const hs_ec_job* __restrict__ jobs, const hs_scr_job* __restrict__ xjobs,
   const int* __restrict__ sizes, hs_sc_par par, hs_sc_out out)
{
   __shared__ double xs[HS_SC_MAXN];         /* w on the support */
   __shared__ double xd[HS_SC_MAXN];         /* w lifted */
   __shared__ int sup[HS_SC_MAXN];
   const hs_ec_job job = jobs[blockIdx.x];
   const hs_scr_job xj = xjobs[blockIdx.x];
   hs_scr_state* S = xj.st;
   if ( S->done )
      return;
   const int n = job.n, tid = threadIdx.x, size = sizes[job.blk];
   const int nc = S->nc, iters = S->iters, flags = S->flags;
   const double maxeig = S->maxeig;
   const double lambda = xj.wsS[0];          /* the smallest eigenvalue of Z_S; its vector is row 0 behind vposS */
   if ( !(lambda < -par.tol) )               /* cons_sdp.c:1487: the loop ends, no cut from this run */
   {
      scr_finish(S, out, job.blk, nc, iters, flags | 4);
      return;
   }
   const long long slot = (long long) job.blk * par.maxcuts + nc;
   if ( tid < size )
   {
      sup[tid] = out.sup[slot * out.smax + tid];
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
   scr_apply_cut(job, S, out, par.maxcuts, size, nc, iters, flags, maxeig, lambda, tid < n ? xd[tid] : 0.0, xs, sup);
}

/* stands in for a launch of hs_syev_small_many whose class has no job, so that the sequence of a call is the same for every solver */
__global__ void k_scr_none(void)
{
}

int hs_scr_tpower(hipStream_t st, int count, int nmax, const hs_ec_job* jobs, const hs_scr_job* xjobs, const int* sizes, const hs_sc_par* par,
   unsigned variant, int round, const hs_sc_out* out)
{
   if ( count <= 0 )
      return HS_OK;
   if ( nmax < 1 || nmax > HS_SC_MAXN || out->smax < 1 || out->smax > HS_SC_MAXN || round < 0 )
      return HS_ERR_ARG;
   static hs_attr_mask attr_done;
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_scr_tpower), (int) scr_lds(HS_SC_MAXN), &attr_done) );
   hipLaunchKernelGGL(k_scr_tpower, dim3(count), dim3(SCR_NT), scr_lds(nmax), st, jobs, xjobs, sizes, *par, variant, round, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_scr_cut(hipStream_t st, int count, const hs_ec_job* jobs, const hs_scr_job* xjobs, const int* sizes, const hs_sc_par* par,
   const hs_sc_out* out)
{
   if ( count <= 0 )
      return HS_OK;
   hipLaunchKernelGGL(k_scr_cut, dim3(count), dim3(SCR_NT), 0, st, jobs, xjobs, sizes, *par, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_scr_pad(hipStream_t st, int launches)
{
   for (int k = 0; k < launches; ++k)
   {
      hipLaunchKernelGGL(k_scr_none, dim3(1), dim3(64), 0, st);
      HS_HIP( hipGetLastError() );
   }
   return HS_OK;
}
