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
#include "hs_ec_sweep.h"         /* EC_NT, EC_CH, ec_sweep, ec_sweep_store: shared with eigcuts_large.hip */

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

__global__ void __launch_bounds__(EC_NT) k_ec_cuts(int m, int nb, int maxcuts, double tol, const hs_ec_job* __restrict__ jobs,
   double* __restrict__ res)
{
   extern __shared__ __attribute__((aligned(16))) double ec_vs[];
   __shared__ double part[EC_NT / 64][EC_CH];
   const hs_ec_job job = jobs[blockIdx.y];
   const int n = job.n, i = blockIdx.x, tid = threadIdx.x;
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
   ec_sweep_store(job, i, n, k, m, slot0, ec_vs, part, r_lhs, r_coef);
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
