/* sparsecuts.hip - sparse eigenvector cuts of ALL SDP blocks in a constant number of launches (hipsdp_sparsecuts_all).
 *
 * The reference's separation mode `multiplesparsecuts` (cons_sdp.c:1340-1607, addMultipleSparseCuts; Algorithm 1 of Dey et al.,
 * "Cutting plane generation through sparse principal component analysis") in its default configuration: per block one truncated
 * power method (TPower, cons_sdp.c:1140-1234) per cut on maxeig I - Z, started from the eigenvector of the smallest eigenvalue, the
 * matrix deflated by scalar x x^T after every cut.  Z_b(y) and its full decomposition come from the launches of
 * hipsdp_eigencuts_all (k_ec_form_z, hs_syev_small_many); behind them
 *
 *    k_sc_tpower      grid (blocks), 128 threads      a block per workgroup, thread i = row i: M in LDS (pitch n | 1), the whole loop
 *                                                     over cuts and TPower iterations; nothing leaves the device in between
 *    k_sc_coefs       grid (m + 1, blocks), 256       workgroup (i, b): x_c^T A_i^b x_c of every cut c over the size (size + 1) / 2
 *                                                     pairs of its support (a block kept as nonzeros: over the variable's nonzeros)
 *
 * M = maxeig I - Z is EXPLICIT in LDS, as in the reference (m_ii = maxeig - z_ii, m_ij = -z_ij), so that a product has the summands
 * of the reference's; the diagonal of Z is kept beside it, and a cut (Z -= scalar x x^T, maxeig -= scalar) adds scalar x_r x_c to the
 * size^2 entries of M on the support and forms M's diagonal again.  A single TPower run is sc_tpower_run of hs_sc_tpower.h, shared
 * with the rounds of sparsecuts_rounds.hip.  One product per iteration: the M x behind the Rayleigh quotient
 * of an iteration is the w of the next one (the reference forms it twice).  A product walks the support of x in ascending index
 * order - the skipped summands are exact zeros.  The truncation keeps entry i when fewer than `size` entries j have |w_j| > |w_i|, or
 * |w_j| == |w_i| and j < i: of two equal absolute values the smaller index stays.  All sums over the threads run in a fixed order
 * (hs_wave_sum_dpp: the butterfly inside the rows of 16 lanes, the four rows in order; then the wavefronts in index order), there
 * are no atomics and no waiting on another workgroup: same input, same bits, whatever other blocks the launch holds.  Every loop
 * condition is false for a NaN, and every loop is bounded by maxit or maxcuts. */
#include "hs_kernels.h"
#include "hs_wave.h"
#include "hs_sc_tpower.h"

#define SC_CT 256          /* k_sc_coefs */

/* dynamic LDS of k_sc_tpower for a block of n rows: M | diagonal of Z | x on its support | |w| | v0 | red[2] | support (int) | kept
 * per wavefront (int[2]) */
static size_t sc_lds(int n)
{
   return ((size_t) n * (n | 1) + 4 * (size_t) n + 2) * sizeof(double) + ((size_t) n + 2) * sizeof(int);
}

__global__ void __launch_bounds__(SC_NT) k_sc_tpower(const hs_ec_job* __restrict__ jobs, const int* __restrict__ sizes, hs_sc_par par,
   hs_sc_out out)
{
   extern __shared__ __attribute__((aligned(16))) double sc_mem[];
   const hs_ec_job job = jobs[blockIdx.x];
   const int n = job.n, pitch = n | 1, tid = threadIdx.x;
   const int size = sizes[job.blk];
   const double* __restrict__ lam = job.ws;
   const double lmin = lam[0];
   if ( !(lmin < -par.tol) || size > n || par.maxcuts <= 0 )
   {
      if ( tid == 0 )
      {
         out.ncuts[job.blk] = 0; out.iters[job.blk] = 0; out.flags[job.blk] = 0;
         out.lmin[job.blk] = lmin;
      }
      return;
   }
   double* Ms = sc_mem;                      /* M = maxeig I - Z, row i at Ms + i pitch */
   double* zd = Ms + (size_t) n * pitch;     /* the diagonal of Z: M's is formed from it again after every cut */
   double* xc = zd + n;                      /* x on its support: xc[p] = x[sup[p]] */
   double* aw = xc + n;
   double* v0s = aw + n;
   double* red = v0s + n;
   int* sup = reinterpret_cast<int*>(red + 2);
   int* wkept = sup + n;
   const bool row = tid < n;
   double maxeig = lam[n - 1];
   for (int e = tid; e < n * n; e += SC_NT)
   {
      const int r = e / n, c = e - r * n;
      const double z = job.Z[e];
      Ms[r * pitch + c] = r == c ? maxeig - z : -z;
      if ( r == c )
         zd[r] = z;
   }
   if ( row )
      v0s[tid] = job.ws[job.vpos + tid];
   const double* mrow = Ms + (row ? tid : 0) * pitch;
   const long long slot0 = (long long) job.blk * par.maxcuts;
   int nc = 0, iters = 0, flags = 0;
   for (;;)
   {
      /* ---- one TPower run from v0 on M (as in the reference, one more follows the last cut) ---- */
      const sc_run run = sc_tpower_run(n, size, row, mrow, v0s, aw, xc, sup, wkept, red, par.convtol, par.maxit);
      const double x = run.x, newv = run.newv, oldv = run.oldv;
      const int it = run.it;
      iters += it;
      if ( run.dead )
      {
         flags |= 2;
         break;
      }
      if ( it == 0 )             /* (convtol >= 1: no iterate, no support) */
         break;
      if ( it >= par.maxit && newv - oldv > par.convtol )
         flags |= 1;
      const double scalar = maxeig - newv;
      if ( !(scalar < -par.feastol) || nc >= par.maxcuts )
         break;
      /* ---- cut nc: its value, the dense vector, the ascending support; then Z -= scalar x x^T (its support only) and
       *      maxeig -= scalar: M's entries off the diagonal gain scalar x_r x_c, its diagonal is formed again ---- */
      if ( tid == 0 )
         out.eig[slot0 + nc] = scalar;
      if ( row )
         out.vec[job.vecoff + (long long) nc * n + tid] = x;
      if ( tid < size )
         out.sup[(slot0 + nc) * out.smax + tid] = sup[tid];
      for (int e = tid; e < size * size; e += SC_NT)
      {
         const int p = e / size, q = e - p * size;
         const double t = scalar * xc[p] * xc[q];
         if ( p == q )
            zd[sup[p]] -= t;
         else
            Ms[sup[p] * pitch + sup[q]] += t;
      }
      maxeig -= scalar;
      __syncthreads();
      if ( row )
         Ms[tid * pitch + tid] = maxeig - zd[tid];
      ++nc;
   }
   if ( tid == 0 )
   {
      out.ncuts[job.blk] = nc; out.iters[job.blk] = iters; out.flags[job.blk] = flags;
      out.lmin[job.blk] = lmin;
   }
}

__global__ void __launch_bounds__(SC_CT) k_sc_coefs(int m, int maxcuts, const hs_ec_job* __restrict__ jobs, const int* __restrict__ sizes,
   hs_sc_out out)
{
   __shared__ double xs[HS_SC_MAXN];         /* values on the support; a block kept as nonzeros: the dense vector */
   __shared__ int sup[HS_SC_MAXN];
   __shared__ double part[SC_CT / 64];
   const hs_ec_job job = jobs[blockIdx.y];
   const int n = job.n, i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int nc = out.ncuts[job.blk], size = sizes[job.blk];
   if ( nc <= 0 || nc > maxcuts || size > n )
      return;
   const long long slot0 = (long long) job.blk * maxcuts;
   const bool walk = job.form == HS_EC_SPARSE && i > 0;       /* (the constant matrix of a sparse block is its dense row 0) */
   const double* __restrict__ a = job.A + (walk ? 0LL : (long long) i * job.ld);
   const int np = size * (size + 1) / 2;
   for (int c = 0; c < nc; ++c)
   {
      const double* __restrict__ v = out.vec + job.vecoff + (long long) c * n;
      if ( walk )
      {
         if ( tid < n )
            xs[tid] = v[tid];
      }
      else if ( tid < size )
      {
         const int s = out.sup[(slot0 + c) * out.smax + tid];
         sup[tid] = s;
         xs[tid] = v[s];
      }
      __syncthreads();
      double acc = 0.0;
      if ( walk )
      {
         for (int e = job.sp.voff[i - 1] + tid; e < job.sp.voff[i]; e += SC_CT)
         {
            const int r = job.sp.vrow[e], q = job.sp.vcol[e];
            acc += (r == q ? 1.0 : 2.0) * job.sp.vval[e] * xs[r] * xs[q];
         }
      }
      else
      {
         for (int t = tid; t < np; t += SC_CT)
         {
            int p = (int) ((sqrt(8.0 * (double) t + 1.0) - 1.0) * 0.5);
            while ( p * (p + 1) / 2 > t ) --p;
            while ( (p + 1) * (p + 2) / 2 <= t ) ++p;
            const int q = t - p * (p + 1) / 2;
            const int r = sup[p], s = sup[q];                    /* s <= r: the list ascends */
            const long long at = job.form == HS_EC_PACKED ? (long long) r * (r + 1) / 2 + s : (long long) r * n + s;
            acc += (p == q ? 1.0 : 2.0) * a[at] * xs[p] * xs[q];
         }
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1)
         acc += __shfl_xor(acc, off, 64);
      if ( lane == 0 )
         part[wave] = acc;
      __syncthreads();
      if ( tid == 0 )
      {
         double t = 0.0;
         for (int w = 0; w < SC_CT / 64; ++w)
            t += part[w];
         if ( i == 0 )
            out.lhs[slot0 + c] = t;
         else
            out.coef[(slot0 + c) * m + (i - 1)] = t;
      }
      __syncthreads();
   }
}

int hs_sc_tpower(hipStream_t st, int count, int nmax, const hs_ec_job* jobs, const int* sizes, const hs_sc_par* par, const hs_sc_out* out)
{
   if ( count <= 0 )
      return HS_OK;
   if ( nmax < 1 || nmax > HS_SC_MAXN || out->smax < 1 || out->smax > HS_SC_MAXN )
      return HS_ERR_ARG;
   static hs_attr_mask attr_done;
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_sc_tpower), (int) sc_lds(HS_SC_MAXN), &attr_done) );
   hipLaunchKernelGGL(k_sc_tpower, dim3(count), dim3(SC_NT), sc_lds(nmax), st, jobs, sizes, *par, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_sc_coefs(hipStream_t st, int count, int m, int maxcuts, const hs_ec_job* jobs, const int* sizes, const hs_sc_out* out)
{
   if ( count <= 0 || maxcuts <= 0 )
      return HS_OK;
   hipLaunchKernelGGL(k_sc_coefs, dim3(m + 1, count), dim3(SC_CT), 0, st, m, maxcuts, jobs, sizes, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
