/* hs_ec_sweep.h - the sweep over one constraint matrix that the dense eigenvector cuts share: k_ec_cuts (eigcuts.hip, blocks of at most
 * 128 rows, vectors of a full decomposition) and k_ecl_cuts (eigcuts_large.hip, blocks of 129 .. 512 rows, vectors of the batched
 * selection of syevx.hip).  One body, so that the three storage forms are read, weighted and summed in one way: the packed and the
 * nonzero form count an off-diagonal entry twice, as hs_pack_weighted and cons_sdp.c:826-865 do.  Both kernels run EC_NT threads and
 * reduce the partial sums in the same fixed order (wavefront butterfly, then the wavefronts in index order). */
#ifndef HS_EC_SWEEP_H
#define HS_EC_SWEEP_H

#include "hs_kernels.h"
#include "hs_round_plan.h"     /* hs_rf_weight: the weight of a stored entry, shared with rounding.hip */

#define EC_NT 256
#define EC_CH 8            /* cuts swept together (accumulators in registers); more cuts of a block: further sweeps out of L2 */

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
         const double av = hs_rf_weight(r, c) * a[p];
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
         const double av = hs_rf_weight(r, c) * job.sp.vval[e];
#pragma unroll
         for (int u = 0; u < EC_CH; ++u)
            if ( c0 + u < k )
               acc[u] += av * vs[(c0 + u) * n + r] * vs[(c0 + u) * n + c];
      }
   }
}

/* One block's sweeps for the k vectors in vs (k x n, LDS) over matrix i of the block, all threads of the workgroup: the partial sums of
 * EC_CH cuts at a time, the wavefront butterfly, then thread u < EC_CH adds the wavefronts' sums in index order and stores cut c0 + u -
 * into lhs (i == 0, the constant matrix) or into coef[(slot0 + c) m + i - 1].  part: EC_NT / 64 rows of EC_CH doubles of LDS. */
__device__ __forceinline__ void ec_sweep_store(const hs_ec_job& job, int i, int n, int k, int m, long long slot0, const double* vs,
   double (*part)[EC_CH], double* __restrict__ r_lhs, double* __restrict__ r_coef)
{
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   for (int c0 = 0; c0 < k; c0 += EC_CH)
   {
      double acc[EC_CH];
#pragma unroll
      for (int u = 0; u < EC_CH; ++u)
         acc[u] = 0.0;
      if ( job.form == HS_EC_PACKED )
         ec_sweep<HS_EC_PACKED>(job, i, n, k, c0, vs, acc);
      else if ( job.form == HS_EC_SPARSE && i > 0 )
         ec_sweep<HS_EC_SPARSE>(job, i, n, k, c0, vs, acc);
      else
         ec_sweep<HS_EC_DENSE>(job, i, n, k, c0, vs, acc);      /* (the constant matrix of a sparse block is its dense row 0) */
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

#endif
