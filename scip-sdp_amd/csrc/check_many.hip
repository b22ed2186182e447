/* check_many.hip - the feasibility check of MANY candidate points in a fixed number of launches (hipsdp_check_y_many; host side:
 * cut_calls.hip).
 *
 * The reference checks every solution a heuristic proposes (SCIPsdpSolcheckerCheck / CONSCHECK, sdpsolchecker.c:201-257): per block
 * Z_b(y) = sum_i A_i^b y_i - A_0^b and its smallest eigenvalue, and the LP rows.  A rounding heuristic proposes many points at once
 * (heur_sdprand.c:395-420 tries one per call because a check costs a decomposition on the host).  What the loop over the candidates costs
 * on the device is traffic: k_ec_form_z (eigcuts.hip) reads all (m + 1) n^2 doubles of a block to form ONE Z.  Here one pass feeds a
 * GROUP of HS_CM_G candidates:
 *
 *    k_cm_form_z      grid (entry tiles, blocks, groups)   a thread owns one stored entry, loads a_i of it ONCE per variable and updates
 *                                                          HS_CM_G accumulators - the expression and the order of k_ec_form_z (acc = -a_0,
 *                                                          acc += y_i a_i for i = 1 .. m), so candidate c's Z has the bits that kernel
 *                                                          gives for Y[c] alone, whatever the group holds beside it
 *    (eigi.hip)       k_lmin_many_small / k_lmin_many_mid: eigenvalue 1 of the matrices of at most 128 rows, no vector
 *    (syevx.hip)      blocks of 129 .. 512 rows: the batched tridiagonal path, values only; Z goes straight into its matrices and
 *                     k_ecl_clear (eigcuts_large.hip) clears the reflector arrays
 *    k_cm_result      grid (candidates)                    the last launch: every eigenvalue 1 into the result block, and the LP rows -
 *                                                          D Y[c] - c row by row in index order, its worst row by a maximum in a fixed tree
 *
 * k_cm_form_z is bound by the bytes of A: per loaded entry (8 bytes) 2 HS_CM_G flop, at HS_CM_G = 8 that is 2 flop / byte against a
 * balance of about 10 (78 Tflop/s FP64 vector, 8 TB/s) - plain vector FMA.  The y values of a group are the same for every lane: the
 * host lays them out as Yg[group][variable][HS_CM_G], a tile of CM_TI variables is staged in LDS (2 KB, one value per thread) and read
 * back as broadcasts, four 16-byte reads per variable.  Registers: 16 for the accumulators, 16 for the tile's values in flight, the
 * loads of eight variables ahead - far below the 128 at which a SIMD still holds four wavefronts.  The nonzero form has no uniform
 * variable index (a lane's position names its own variables): it reads the 64 contiguous bytes of Yg[group][variable] from the cache.
 * The packed form owns a stored entry (r, c), c <= r, and writes both halves of Z: half the bytes of the dense form, the same bits.
 * HAZARD RULE: no atomic operation, no flag; every word of the workspace is written by one thread of one launch, and stream order is the
 * only synchronisation.  Same input, same bits; the bits of (candidate, block) do not depend on the other candidates or blocks. */
#include "hs_kernels.h"
#include "hs_ec_sweep.h"         /* EC_NT */

#define CM_TI 32                 /* variables per staged tile */
static_assert(CM_TI * HS_CM_G == EC_NT, "a tile of y is one value per thread");

namespace {

/* index of the position (r, c), c <= r, in the list sorted by (row, column), or -1 (ec_find_pos of eigcuts.hip) */
__device__ __forceinline__ long long cm_find_pos(const hs_sp_view& sp, int r, int c)
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

/* dense rows (entry e of the n x n matrix) or packed lower triangles (entry e = r (r + 1) / 2 + c): the whole workgroup, barriers inside */
template<bool PACKED>
__device__ __forceinline__ void cm_form_rows(const hs_ec_job& job, const hs_cm_blk& B, int m, int cnt, long long c0, const double* __restrict__ yg,
   double (*ys)[HS_CM_G])
{
   const int n = job.n, tid = threadIdx.x;
   const long long nent = PACKED ? (long long) n * (n + 1) / 2 : (long long) n * n;
   const long long e = (long long) blockIdx.x * EC_NT + tid;
   const bool active = e < nent;
   const double* __restrict__ a = job.A + (active ? e : 0);
   double acc[HS_CM_G];
   {
      const double a0 = a[0];
#pragma unroll
      for (int k = 0; k < HS_CM_G; ++k)
         acc[k] = -a0;
   }
   for (int i0 = 0; i0 < m; i0 += CM_TI)
   {
      const int tl = m - i0 < CM_TI ? m - i0 : CM_TI;
      __syncthreads();
      if ( tid < tl * HS_CM_G )
         ys[0][tid] = yg[(long long) i0 * HS_CM_G + tid];
      __syncthreads();
      if ( active )
      {
         const double* __restrict__ ai = a + (long long) (i0 + 1) * job.ld;
#pragma unroll 8
         for (int t = 0; t < tl; ++t)
         {
            const double av = ai[(long long) t * job.ld];
#pragma unroll
            for (int k = 0; k < HS_CM_G; ++k)
               acc[k] += ys[t][k] * av;
         }
      }
   }
   if ( !active )
      return;                                                /* (behind the last barrier of the group) */
   if ( PACKED )
   {
      int r = (int) ((sqrt(8.0 * (double) e + 1.0) - 1.0) * 0.5);
      while ( (long long) r * (r + 1) / 2 > e ) --r;
      while ( (long long) (r + 1) * (r + 2) / 2 <= e ) ++r;
      const int c = (int) (e - (long long) r * (r + 1) / 2);
#pragma unroll
      for (int k = 0; k < HS_CM_G; ++k)
         if ( k < cnt )
         {
            double* __restrict__ Z = B.Z + (c0 + k) * B.zstride;
            Z[(long long) r * n + c] = acc[k];
            if ( r != c )
               Z[(long long) c * n + r] = acc[k];
         }
   }
   else
   {
#pragma unroll
      for (int k = 0; k < HS_CM_G; ++k)
         if ( k < cnt )
            B.Z[(c0 + k) * B.zstride + e] = acc[k];
   }
}

/* the nonzero form: a thread owns entry e of the n x n matrix, its constant from the dense A_0, its variables from the position lists */
__device__ __forceinline__ void cm_form_nonzeros(const hs_ec_job& job, const hs_cm_blk& B, int cnt, long long c0, const double* __restrict__ yg)
{
   const int n = job.n;
   const long long e = (long long) blockIdx.x * EC_NT + threadIdx.x;
   if ( e >= (long long) n * n )
      return;
   const int r0 = (int) (e / n), q0 = (int) (e - (long long) r0 * n);
   const int r = r0 > q0 ? r0 : q0, c = r0 > q0 ? q0 : r0;
   double acc[HS_CM_G];
   {
      const double a0 = job.A[e];
#pragma unroll
      for (int k = 0; k < HS_CM_G; ++k)
         acc[k] = -a0;
   }
   const long long p = cm_find_pos(job.sp, r, c);
   if ( p >= 0 )
      for (int t = job.sp.poff[p]; t < job.sp.poff[p + 1]; ++t)
      {
         const double* __restrict__ yv = yg + (long long) (job.sp.pvar[t] - 1) * HS_CM_G;
         const double av = job.sp.pval[t];
#pragma unroll
         for (int k = 0; k < HS_CM_G; ++k)
            acc[k] += yv[k] * av;
      }
#pragma unroll
   for (int k = 0; k < HS_CM_G; ++k)
      if ( k < cnt )
         B.Z[(c0 + k) * B.zstride + e] = acc[k];
}

__global__ void __launch_bounds__(EC_NT) k_cm_form_z(int m, int cc, const hs_ec_job* __restrict__ jobs, const hs_cm_blk* __restrict__ blks,
   const double* __restrict__ Yg)
{
   __shared__ __attribute__((aligned(16))) double ys[CM_TI][HS_CM_G];
   const hs_ec_job job = jobs[blockIdx.y];
   const hs_cm_blk B = blks[blockIdx.y];
   const int n = job.n;
   const long long nent = job.form == HS_EC_PACKED ? (long long) n * (n + 1) / 2 : (long long) n * n;
   if ( (long long) blockIdx.x * EC_NT >= nent )            /* (the whole workgroup) */
      return;
   const int groups = (cc + HS_CM_G - 1) / HS_CM_G;
   /* (the grid has a workgroup per group up to 65535 groups; the loop is there for more) */
   for (int g = blockIdx.z; g < groups; g += (int) gridDim.z)
   {
      const long long c0 = (long long) g * HS_CM_G;
      const int cnt = cc - c0 < HS_CM_G ? (int) (cc - c0) : HS_CM_G;
      const double* __restrict__ yg = Yg + (long long) g * m * HS_CM_G;
      if ( job.form == HS_EC_PACKED )
         cm_form_rows<true>(job, B, m, cnt, c0, yg, ys);
      else if ( job.form == HS_EC_DENSE )
         cm_form_rows<false>(job, B, m, cnt, c0, yg, ys);
      else
         cm_form_nonzeros(job, B, cnt, c0, yg);
   }
}

__global__ void __launch_bounds__(EC_NT) k_cm_result(int nblk, int cc, int m, int q, const double* __restrict__ Dext, const hs_cm_blk* __restrict__ blks,
   const double* __restrict__ Yg, double* __restrict__ res)
{
   __shared__ double red[EC_NT];
   const long long c = blockIdx.x;
   const int tid = threadIdx.x;
   for (int b = tid; b < nblk; b += EC_NT)
      res[c * nblk + b] = blks[b].lam[c * blks[b].lstride];
   /* candidate c of the chunk: entry c mod HS_CM_G of its group */
   const double* __restrict__ y = Yg + (c / HS_CM_G) * m * HS_CM_G + (c % HS_CM_G);
   double worst = 0.0;
   for (int r = tid; r < q; r += EC_NT)
   {
      const double* __restrict__ d = Dext + (long long) r * (m + 1);
      double acc = -d[0];
      for (int i = 0; i < m; ++i)
         acc += y[(long long) i * HS_CM_G] * d[1 + i];
      worst = fmax(worst, -acc);
   }
   red[tid] = worst;
   __syncthreads();
   for (int half = EC_NT / 2; half > 0; half >>= 1)
   {
      if ( tid < half )
         red[tid] = fmax(red[tid], red[tid + half]);
      __syncthreads();
   }
   if ( tid == 0 )
      res[(long long) cc * nblk + c] = red[0];
}

}

int hs_cm_form_z(hipStream_t st, int nblk, int nmax, int m, int cc, const hs_ec_job* jobs, const hs_cm_blk* blks, const double* Yg)
{
   if ( nblk < 1 || cc < 1 || nmax < 1 || m < 0 || jobs == NULL || blks == NULL || Yg == NULL )
      return HS_ERR_ARG;
   const int groups = (cc + HS_CM_G - 1) / HS_CM_G;
   if ( nblk > 65535 )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_cm_form_z, dim3((unsigned) (((long long) nmax * nmax + EC_NT - 1) / EC_NT), nblk, groups < 65535 ? groups : 65535),
      dim3(EC_NT), 0, st, m, cc, jobs, blks, Yg);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_cm_result(hipStream_t st, int nblk, int cc, int m, int q, const double* Dext, const hs_cm_blk* blks, const double* Yg, double* res)
{
   if ( nblk < 0 || cc < 1 || m < 0 || q < 0 || (q > 0 && Dext == NULL) || (nblk > 0 && blks == NULL) || Yg == NULL || res == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_cm_result, dim3(cc), dim3(EC_NT), 0, st, nblk, cc, m, q, Dext, blks, Yg, res);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
