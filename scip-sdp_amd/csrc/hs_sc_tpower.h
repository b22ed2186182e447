/* hs_sc_tpower.h - ONE run of the truncated power method (TPower, cons_sdp.c:1140-1234) by a workgroup of SC_NT threads, thread i =
 * row i, on M = maxeig I - Z explicit in LDS: what k_sc_tpower (sparsecuts.hip: the whole loop over cuts in one launch) and
 * k_scr_tpower (sparsecuts_rounds.hip: one run per launch) have in common, so that both take the same decisions with the same bits.
 * One product per iteration: the M x behind the Rayleigh quotient of an iteration is the w of the next one.  A product walks the
 * support of x in ascending index order - the skipped summands are exact zeros.  The truncation keeps entry i when fewer than `size`
 * entries j have |w_j| > |w_i|, or |w_j| == |w_i| and j < i: of two equal absolute values the smaller index stays.  All sums over the
 * threads run in a fixed order (hs_wave_sum_dpp, then the wavefronts in index order).  The loop condition is false for a NaN and
 * bounded by maxit. */
#ifndef HS_SC_TPOWER_H
#define HS_SC_TPOWER_H

#include "hs_wave.h"

#define SC_NT 128          /* one thread per row, HS_SC_MAXN rows at most */

/* Sum over the workgroup, the same bits in every thread: hs_wave_sum_dpp per wavefront, then the wavefronts in index order.  ONE
 * barrier, behind the stores to red - red must not be written again before the next barrier of the caller. */
__device__ __forceinline__ double sc_block_sum(double v, double* red)
{
   v = hs_wave_sum_dpp(v);
   if ( (threadIdx.x & 63) == 0 )
      red[threadIdx.x >> 6] = v;
   __syncthreads();
   double s = red[0];
#pragma unroll
   for (int w = 1; w < SC_NT / 64; ++w)
      s += red[w];
   return s;
}

/* (M x)_i over the support of x in ascending index order: sup[p] the indices, xc[p] the values */
__device__ __forceinline__ double sc_row_product(const double* mrow, const double* xc, const int* sup, int ns)
{
   double acc = 0.0;
#pragma unroll 4
   for (int p = 0; p < ns; ++p)
      acc += mrow[sup[p]] * xc[p];
   return acc;
}

/* what a run leaves in every thread: x its entry of the last iterate (an exact zero off the support), newv, oldv the last two Rayleigh
 * quotients, it the iterations, dead: a truncated iterate had norm 0.  In LDS: sup[size] the ascending support, xc[size] x on it. */
struct sc_run { double x, newv, oldv; int it; bool dead; };

/* mrow: this thread's row of M (row 0 for a thread without a row); v0s[n] the start vector; aw[n], xc[n], sup[n], wkept[SC_NT / 64],
 * red[SC_NT / 64]: LDS.  Starts with a barrier (M, v0s, and the last reads of x and the support by the caller). */
__device__ __forceinline__ sc_run sc_tpower_run(int n, int size, bool row, const double* mrow, const double* v0s, double* aw, double* xc,
   int* sup, int* wkept, double* red, double convtol, int maxit)
{
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   __syncthreads();
   double x = 0.0, u = 0.0;
   if ( row )
   {
      x = v0s[tid];
#pragma unroll 4
      for (int j = 0; j < n; ++j)
         u += mrow[j] * v0s[j];
   }
   double newv = -1.0, oldv = -2.0;
   int it = 0;
   bool dead = false;
   while ( newv - oldv > convtol && it < maxit )
   {
      oldv = newv;
      const double w = u, awi = fabs(w);
      if ( row )
         aw[tid] = awi;
      __syncthreads();
      int above = 0;
#pragma unroll 4
      for (int j = 0; j < n; ++j)
      {
         const double a = aw[j];
         above += (int) (a > awi) | ((int) (a == awi) & (int) (j < tid));
      }
      const bool kept = row && above < size;
      const unsigned long long mask = __ballot(kept);
      const int before = __popcll(mask & ((1ull << lane) - 1ull));
      if ( lane == 0 )
         wkept[wave] = __popcll(mask);
      const double nrm = sqrt(sc_block_sum(kept ? w * w : 0.0, red));
      if ( nrm == 0.0 )
      {
         dead = true;
         break;
      }
      const int pos = (wave == 0 ? 0 : wkept[0]) + before;
      x = kept ? w / nrm : 0.0;
      if ( kept )
      {
         sup[pos] = tid;
         xc[pos] = x;
      }
      __syncthreads();
      u = row ? sc_row_product(mrow, xc, sup, size) : 0.0;
      newv = sc_block_sum(x * u, red);
      ++it;
   }
   sc_run r;
   r.x = x; r.newv = newv; r.oldv = oldv; r.it = it; r.dead = dead;
   return r;
}

#endif
