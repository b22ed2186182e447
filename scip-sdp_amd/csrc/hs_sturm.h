/* hs_sturm.h - the Sturm count of a symmetric tridiagonal matrix in product form, shared by the one-launch eigenvalue kernels
 * (eigi.hip) and the two tridiagonal paths above 128 rows (syevx.hip, syevr.hip). */
#ifndef HS_STURM_H
#define HS_STURM_H

#include <hip/hip_runtime.h>

/* Number of eigenvalues below x of the symmetric tridiagonal matrix scaled to norm <= 1: ds[i] = d_i / norm, es[i] = (e_i / norm)^2,
 * both padded behind the matrix (ds: eight entries 4.0, es: zeros from n - 1 on: rows without coupling that cannot change a sign
 * while |x| <= 1); nb = (n - 1 + 3) >> 2 blocks of four steps.  Sturm sequence in PRODUCT form: p_0 = 1, p_1 = d_0 - x,
 * p_{i+1} = (d_i - x) p_i - e_{i-1}^2 p_{i-1}; a sign change = an eigenvalue below x, a zero takes the sign opposite to its
 * predecessor; rescaled every fourth step; the entries of the next block are on their way while the four steps of this one run.
 * Two dependent operations per step where the quotient form t_i = d_i - x - e_{i-1}^2 / t_{i-1} has a division: 260 cycles per step
 * (the division in double precision is a chain of a dozen dependent instructions) against about 60.
 * LIMIT: the count for the leading `rows` rows alone, nb = (rows - 1 + 3) >> 2 - the steps of the last block of four that lie behind
 * row `rows` are computed and not counted. */
template<bool LIMIT>
__device__ __forceinline__ int ei_sturm_count_t(const double* ds, const double* es, int nb, int rows, double x)
{
   double pp_ = 1.0, pc = ds[0] - x;
   if ( pc == 0.0 ) pc = -1e-290;
   bool posc = pc > 0.0;
   int cnt = posc ? 0 : 1;
   double dn[4], en[4];
#pragma unroll
   for (int u = 0; u < 4; ++u)
   {
      dn[u] = ds[1 + u];
      en[u] = es[u];
   }
   for (int b = 0; b < nb; ++b)
   {
      double dc[4], ec[4];
#pragma unroll
      for (int u = 0; u < 4; ++u)
      {
         dc[u] = dn[u];
         ec[u] = en[u];
      }
      const int nx = (b + 1 < nb) ? 5 + 4 * b : 1;
#pragma unroll
      for (int u = 0; u < 4; ++u)
      {
         dn[u] = ds[nx + u];
         en[u] = es[nx - 1 + u];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
      {
         double pn = fma(dc[u] - x, pc, -ec[u] * pp_);
         if ( pn == 0.0 ) pn = -copysign(1e-290, pc);
         const bool posn = pn > 0.0;
         cnt += (posn != posc && (!LIMIT || 1 + 4 * b + u < rows)) ? 1 : 0;
         pp_ = pc; pc = pn; posc = posn;
      }
      const int ex = -max(__builtin_amdgcn_frexp_exp(pc), __builtin_amdgcn_frexp_exp(pp_));
      pc = ldexp(pc, ex);
      pp_ = ldexp(pp_, ex);
   }
   return cnt;
}

__device__ __forceinline__ int ei_sturm_count(const double* ds, const double* es, int nb, double x)
{
   return ei_sturm_count_t<false>(ds, es, nb, 0, x);
}

/* The same count for the leading `rows` rows alone (a block of a matrix that splits, syevr.hip).  ds, es as above; they are read up
 * to three rows behind the block (the next block of the matrix or the padding). */
__device__ __forceinline__ int ei_sturm_count_rows(const double* ds, const double* es, int rows, double x)
{
   return ei_sturm_count_t<true>(ds, es, (rows - 1 + 3) >> 2, rows, x);
}

#endif
