/* eigcuts.hip - the separation round of ALL SDP blocks in a constant number of launches (hipsdp_eigencuts_all).
 *
 * The reference separates one constraint at a time (cons_sdp.c:8255, :8446, :8473, :8500 call separateSol in a loop over the SDP
 * constraints): Z_k(y) = sum_i A_i^k y_i - A_0^k, its negative eigenpairs (:1683-1700), the coefficients v^T A_i^k v (:826-952).
 * At the sizes of that loop (blocks of 10 .. 128 rows) one block is work for ONE compute unit, so here a block is a workgroup
 * (or a column of workgroups) of a launch that serves all of them, bound through a job table in device memory:
 *
 *    k_ec_form_z      grid (entries / 256, blocks)   Z_b(y) of every block; the sum over the variables runs in index order
 *    (eigi.hip)       k_syevi_small_many / k_syev_mid_many: the full decompositions, a block per workgroup
 *    k_ec_cuts        grid (m + 1, blocks)           workgroup (i, b): number of cuts of block b from its eigenvalues (no read-back),
 *                                                    the selected vectors into LDS, then ONE sweep over A_i^b gives v_c^T A_i^b v_c
 *                                                    for all selected c; workgroup (0, b) also stores ncuts, lmin, eigenvalues, vectors
 *
 * The sweep of k_ec_cuts is bound by the bytes of A: per stored entry (8 bytes) it does about 2 flop per cut, i.e. at 16 cuts
 * at most 4 flop / byte, below the FP64 balance of the part (78 Tflop/s vector
 * against 8 TB/s: about 10 flop / byte) - plain vector FMA, no matrix cores.  All reductions run in a fixed order (wavefront
 * butterfly, then the wavefronts' partial sums in index order) and there are no floating-point atomics: two calls give the same
 * bits.  The three storage forms of a block (dense rows, packed lower triangles, nonzeros) are the three branches below; the
 * packed and the sparse form count an off-diagonal entry twice, as hs_pack_weighted and cons_sdp.c:826-865 do. */
#include "hs_kernels.h"

#define EC_NT 256
#define EC_CH 8            /* cuts swept together (accumulators in registers); more cuts of a block: further sweeps out of L2 */

/* index of the position (r, c), c <= r, in the list sorted by (row, column), or -1 */
__device__ __forceinline__ long long ec_find_pos(const hs_sp_view& sp, int r, int c)
{
   long long lo = 0, hi = sp.npos - 1;
   while ( lo <= hi )
   {
      const long long mid = (lo + hi) >> 1;
      const int pr = sp.prow[mid], pc = sp.pcol[mid];
      if ( pr == r && pc == c )
         return mid;
      if ( pr < r || (pr == r && pc < c) )
         lo = mid + 1;
      else
         hi = mid - 1;
   }
   return -1;
}

__global__ void __launch_bounds__(EC_NT) k_ec_form_z(int m, const hs_ec_job* __restrict__ jobs, const double* __restrict__ y)
{
   const hs_ec_job job = jobs[blockIdx.y];
   const int n = job.n;
   const long long e = (long long) blockIdx.x * EC_NT + threadIdx.x;
   if ( e >= (long long) n * n )
      return;
   const int r0 = (int) (e / n), c0 = (int) (e - (long long) r0 * n);
   const int r = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
   double acc;
   if ( job.form == HS_EC_SPARSE )
   {
      acc = -job.A[e];
      const long long k = ec_find_pos(job.sp, r, c);
      if ( k >= 0 )
         for (int t = job.sp.poff[k]; t < job.sp.poff[k + 1]; ++t)
            acc += y[job.sp.pvar[t] - 1] * job.sp.pval[t];
   }
   else
   {
      const long long at = job.form == HS_EC_PACKED ? (long long) r * (r + 1) / 2 + c : e;
      const double* __restrict__ a = job.A + at;
      acc = -a[0];
      for (int i = 1; i <= m; ++i)
         acc += y[i - 1] * a[(long long) i * job.ld];
   }
   job.Z[e] = acc;
}

/* partial sums of one sweep: v_c^T A v_c for the cuts c0 .. c0 + EC_CH - 1 (those below k) over the entries this thread visits */
template<int FORM>
__device__ __forceinline__ void ec_sweep(const hs_ec_job& job, int i, int n, int k, int c0, const double* vs, double* acc)
{
   const int tid = threadIdx.x;
   if ( FORM == HS_EC_DENSE )
   {
      const double* __restrict__ a = job.A + (long long) i * job.ld;
      for (int e = tid; e < n * n; e += EC_NT)
      {
         const int r = e / n, c = e - r * n;
         const double av = a[e];
#pragma unroll
         for (int u = 0; u < EC_CH; ++u)
            if ( c0 + u < k )
               acc[u] += av * vs[(c0 + u) * n + r] * vs[(c0 + u) * n + c];
      }
   }
   else if ( FORM == HS_EC_PACKED )
   {
      const double* __restrict__ a = job.A + (long long) i * job.ld;
      const int np = n * (n + 1) / 2;
      for (int p = tid; p < np; p += EC_NT)
      {
         int r = (int) ((sqrt(8.0 * (double) p + 1.0) - 1.0) * 0.5);
         while ( r * (r + 1) / 2 > p ) --r;
         while ( (r + 1) * (r + 2) / 2 <= p ) ++r;
         const int c = p - r * (r + 1) / 2;
         const double av = (r == c ? 1.0 : 2.0) * a[p];
#pragma unroll
         for (int u = 0; u < EC_CH; ++u)
            if ( c0 + u < k )
               acc[u] += av * vs[(c0 + u) * n + r] * vs[(c0 + u) * n + c];
      }
   }
   else
   {
      /* variable i >= 1: its lower-triangular nonzeros */
      for (int e = job.sp.voff[i - 1] + tid; e < job.sp.voff[i]; e += EC_NT)
      {
         const int r = job.sp.vrow[e], c = job.sp.vcol[e];
         const double av = (r == c ? 1.0 : 2.0) * job.sp.vval[e];
#pragma unroll
         for (int u = 0; u < EC_CH; ++u)
            if ( c0 + u < k )
               acc[u] += av * vs[(c0 + u) * n + r] * vs[(c0 + u) * n + c];
      }
   }
}

__global__ void __launch_bounds__(EC_NT) k_ec_cuts(int m, int nb, int maxcuts, double tol, const hs_ec_job* __restrict__ jobs,
   double* __restrict__ res)
{
   extern __shared__ __attribute__((aligned(16))) double ec_vs[];
   __shared__ double part[EC_NT / 64][EC_CH];
   const hs_ec_job job = jobs[blockIdx.y];
   const int n = job.n, i = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const double* __restrict__ lam = job.ws;
   const double* __restrict__ V = job.ws + job.vpos;
   /* the selection rule of hipsdp_eigencuts: eigenvalue <= -tol, most negative first, at most maxcuts (every thread, same answer) */
   int k = 0;
   while ( k < n && k < maxcuts && lam[k] <= -tol )
      ++k;
   double* __restrict__ r_ncuts = res;
   double* __restrict__ r_lmin = res + nb;
   double* __restrict__ r_eig = res + 2LL * nb;
   double* __restrict__ r_lhs = r_eig + (long long) nb * maxcuts;
   double* __restrict__ r_coef = r_lhs + (long long) nb * maxcuts;
   double* __restrict__ r_vec = r_coef + (long long) nb * maxcuts * m;
   const long long slot0 = (long long) job.blk * maxcuts;
   if ( i == 0 )
   {
      if ( tid == 0 )
      {
         r_ncuts[job.blk] = (double) k;
         r_lmin[job.blk] = lam[0];
      }
      if ( tid < k )
         r_eig[slot0 + tid] = lam[tid];
      for (int e = tid; e < k * n; e += EC_NT)
         r_vec[job.vecoff + e] = V[e];
   }
   if ( k == 0 )
      return;
   for (int e = tid; e < k * n; e += EC_NT)
      ec_vs[e] = V[e];
   __syncthreads();
   for (int c0 = 0; c0 < k; c0 += EC_CH)
   {
      double acc[EC_CH];
#pragma unroll
      for (int u = 0; u < EC_CH; ++u)
         acc[u] = 0.0;
      if ( job.form == HS_EC_PACKED )
         ec_sweep<HS_EC_PACKED>(job, i, n, k, c0, ec_vs, acc);
      else if ( job.form == HS_EC_SPARSE && i > 0 )
         ec_sweep<HS_EC_SPARSE>(job, i, n, k, c0, ec_vs, acc);
      else
         ec_sweep<HS_EC_DENSE>(job, i, n, k, c0, ec_vs, acc);      /* (the constant matrix of a sparse block is its dense row 0) */
#pragma unroll
      for (int u = 0; u < EC_CH; ++u)
      {
         double a = acc[u];
#pragma unroll
         for (int off = 32; off > 0; off >>= 1)
            a += __shfl_xor(a, off, 64);
         if ( lane == 0 )
            part[wave][u] = a;
      }
      __syncthreads();
      if ( tid < EC_CH && c0 + tid < k )
      {
         double t = 0.0;
         for (int w = 0; w < EC_NT / 64; ++w)
            t += part[w][tid];
         if ( i == 0 )
            r_lhs[slot0 + c0 + tid] = t;
         else
            r_coef[(slot0 + c0 + tid) * m + (i - 1)] = t;
      }
      __syncthreads();
   }
}

int hs_ec_form_z(hipStream_t st, int count, int nmax, int m, const hs_ec_job* jobs, const double* y)
{
   if ( count <= 0 )
      return HS_OK;
   hipLaunchKernelGGL(k_ec_form_z, dim3((nmax * nmax + EC_NT - 1) / EC_NT, count), dim3(EC_NT), 0, st, m, jobs, y);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_ec_cuts(hipStream_t st, int count, int nmax, int m, int nb, int maxcuts, double tol, const hs_ec_job* jobs, double* res)
{
   if ( count <= 0 )
      return HS_OK;
   const int kmax = maxcuts < nmax ? maxcuts : nmax;
   const size_t lds = (size_t) (kmax > 0 ? kmax : 1) * nmax * sizeof(double);
   static hs_attr_mask attr_done;
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_ec_cuts), 128 * 128 * (int) sizeof(double), &attr_done) );
   if ( nmax > 128 )
      return HS_ERR_ARG;
   /* without cuts to form only the workgroups (0, b) have work: ncuts = 0 and lmin */
   hipLaunchKernelGGL(k_ec_cuts, dim3(maxcuts > 0 ? m + 1 : 1, count), dim3(EC_NT), lds, st, m, nb, maxcuts, tol, jobs, res);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
