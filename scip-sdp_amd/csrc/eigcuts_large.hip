/* eigcuts_large.hip - the dense eigenvector cuts of ALL blocks of 129 .. 512 rows of a solver per launch (hipsdp_eigencuts_all_large; host
 * side: cut_calls.hip).  The partner of eigcuts.hip for the blocks it hands to the per-block path: there a block is decomposed in full
 * to use five pairs; here the wanted pairs come from the batched tridiagonal path of syevx.hip (hs_syevx_many_cols,
 * hs_syevx_many_below), whose column launches hold the matrices of all blocks, and two kernels stand around it:
 *
 *    (eigcuts.hip)    k_ec_form_z, grid (entries / 256, blocks): Z_b(y) straight into the matrix the column launches consume
 *    k_ecl_clear      grid (64, blocks), 256 threads   zeros into the reflector array of every block
 *    (syevx.hip)      nmax - 1 column launches, the values, the vectors of T, the back-transformation
 *    k_ecl_cuts       grid (m + 1, blocks), 256 thr.   workgroup (i, b): the count and the selected vectors of block b from the
 *                                                      selection output into LDS, then ONE sweep over A_i^b gives v_c^T A_i^b v_c for
 *                                                      all cuts (hs_ec_sweep.h, the sweep of k_ec_cuts); workgroup (0, b) also stores
 *                                                      ncuts, lmin, eigenvalues, vectors
 *
 * The sweep is bound by the bytes of A (about 2 flop per cut and stored entry): plain vector FMA, one workgroup per
 * (i, b).  LDS: at most maxcuts x n doubles of vectors - 128 KB at 32 cuts of 512 rows, of the 160 KB of a compute unit.
 * HAZARD RULE: no grid barrier, no flag, no atomic operation; workgroup (i, b) writes its own slots of the result alone and reads what
 * earlier launches left; stream order is the only synchronisation.  Every reduction runs in a fixed order: same input, same bits, and
 * the bits of a block do not depend on the other blocks of the launch. */
#include "hs_kernels.h"
#include "hs_ec_sweep.h"

#define ECL_CLEAR_G 64     /* workgroups per block of the clear launch: 64 x 256 entries cover 128 rows in one pass, 512 rows in sixteen */

__global__ void __launch_bounds__(EC_NT) k_ecl_clear(const hs_sxm_job* __restrict__ sx)
{
   const int n = sx[blockIdx.y].n;
   double* __restrict__ R = sx[blockIdx.y].R;
   for (int idx = blockIdx.x * EC_NT + threadIdx.x; idx < n * n; idx += gridDim.x * EC_NT)
      R[idx] = 0.0;
}

/* dynamic LDS: maxcuts x nmax doubles */
__global__ void __launch_bounds__(EC_NT) k_ecl_cuts(int m, int maxcuts, const hs_ec_job* __restrict__ jobs, const hs_sxm_job* __restrict__ sx,
   const long long* __restrict__ vecoff, hs_sc_out out)
{
   extern __shared__ __attribute__((aligned(16))) double ecl_vs[];
   __shared__ double part[EC_NT / 64][EC_CH];
   const hs_ec_job job = jobs[blockIdx.y];
   const int n = job.n, i = blockIdx.x, tid = threadIdx.x;
   const double* __restrict__ sel = sx[blockIdx.y].out;
   const double* __restrict__ lam = sel + HS_SYEVX_OUT_LAM;
   const double* __restrict__ V = sel + HS_SYEVX_OUT_VEC;
   /* the selection rule of hipsdp_eigencuts - eigenvalue <= -tol, most negative first, at most maxcuts - is the count of the BELOW
    * selection; a count that is none (NaN input) is reported as -1 and nothing else is done (every thread, same answer) */
   int k = 0;
   if ( maxcuts > 0 )
   {
      const double cnt = sel[0];
      k = (cnt >= 0.0 && cnt <= (double) maxcuts && cnt <= (double) n) ? (int) cnt : -1;
   }
   const long long slot0 = (long long) job.blk * maxcuts;
   if ( i == 0 )
   {
      if ( tid == 0 )
      {
         out.ncuts[job.blk] = k;
         /* with a cut: eigenvalue slot 0 itself, bit for bit; without: eigenvalue 1 by index */
         out.lmin[job.blk] = k > 0 ? lam[0] : sx[blockIdx.y].out2[HS_SYEVX_OUT_LAM];
      }
      if ( tid < k )
         out.eig[slot0 + tid] = lam[tid];
      const long long voff = vecoff[blockIdx.y];
      for (int e = tid; e < k * n; e += EC_NT)
         out.vec[voff + e] = V[e];
   }
   if ( k <= 0 )
      return;
   for (int e = tid; e < k * n; e += EC_NT)
      ecl_vs[e] = V[e];
   __syncthreads();
   ec_sweep_store(job, i, n, k, m, slot0, ecl_vs, part, out.lhs, out.coef);
}

int hs_ecl_clear(hipStream_t st, int count, const hs_sxm_job* sx)
{
   if ( count < 1 || sx == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_ecl_clear, dim3(ECL_CLEAR_G, count), dim3(EC_NT), 0, st, sx);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_ecl_cuts(hipStream_t st, int count, int nmax, int m, int maxcuts, const hs_ec_job* jobs, const hs_sxm_job* sx, const long long* vecoff,
   const hs_sc_out* out)
{
   if ( count < 1 || nmax < 2 || nmax > HS_SYEVX_MAXN || m < 0 || maxcuts < 0 || maxcuts > HS_SYEVX_MAXK || jobs == NULL || sx == NULL
      || vecoff == NULL || out == NULL )
      return HS_ERR_ARG;
   static hs_attr_mask attr_done;
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_ecl_cuts), HS_SYEVX_MAXK * HS_SYEVX_MAXN * (int) sizeof(double), &attr_done) );
   const size_t lds = (size_t) (maxcuts > 0 ? maxcuts : 1) * nmax * sizeof(double);
   /* without cuts to form only the workgroups (0, b) have work: ncuts = 0 and lmin */
   hipLaunchKernelGGL(k_ecl_cuts, dim3(maxcuts > 0 ? m + 1 : 1, count), dim3(EC_NT), lds, st, m, maxcuts, jobs, sx, vecoff, out[0]);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
