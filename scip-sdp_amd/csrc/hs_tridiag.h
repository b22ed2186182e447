/* hs_tridiag.h - the numerical rules of the eigen-solvers of a symmetric tridiagonal matrix T = (d, e), stated once: the Gershgorin
 * bracket and its widening, the padding the Sturm count asks for, the stopping rule and the multisection of syevx.hip / syevr.hip,
 * the hashed start vectors, their inverse-iteration chain and the tail of their back-transformations.  Device-only; the Sturm
 * count itself is in hs_sturm.h, the sums over lanes in hs_wave.h.
 *
 * HS_SYEVX_MAXK = 32 (hs_kernels.h) is "vectors of a panel", SX_K of syevx.hip and SR_P of syevr.hip alike: the slots of cntb in
 * hs_td_multisect and the thread mapping of the callers of hs_td_invit (vector lane << 3 | wave: four lanes of each of the eight
 * wavefronts) rely on it.
 *
 * DELIBERATELY NOT HERE - do not "finish" this blind, each would change bits or put a predicate into an inner loop:
 *   - the inverse-iteration chains of eigi.hip (d_syevi_small, k_syevi_mid, d_syev_mid): hs_rcp2 / hs_rsqrt2 for the divisions, two
 *     factor arrays plus a swap bitmask, a transposed Z;
 *   - their multisections: per wavefront, sums by DPP, other round counts;
 *   - the Gram-Schmidt loops: k_syevx_tvec runs over the contiguous range cstart[k] .. k - 1, k_syevr_ortho_panel selects by cluster
 *     id among interleaved blocks;
 *   - k_syevx_col, k_syevr_order, k_syevr_ortho_prev and the bodies of the two _back kernels;
 *   - which path serves which size (host_entries.hip, psd.hip, ipm.hip). */
#ifndef HS_TRIDIAG_H
#define HS_TRIDIAG_H

#include "hs_kernels.h"
#include "hs_sturm.h"
#include "hs_wave.h"

/* Results come back BY VALUE (small structs), not through references: a loop variable of the caller whose address a helper takes is
 * promoted to a register later in the compiler's pipeline, and kernels of eig.hip came out with their instructions in another
 * order.  For the same reason hs_td_widen returns three fields and not the four of hs_td_gersh (k_lmin_tiny). */
struct hs_td_interval { double lo, hi; };
struct hs_td_bracket { double lo, hi, span0; };                 /* a widened bracket (hs_td_widen) */
struct hs_td_gersh { double lo, hi, span0, tnorm; };            /* ... with the norm bound of T */

/* The Gershgorin bracket [lo, hi] widened by 1e-12 of its span (and 1e-300, for the matrix of zeros) on either side, so that no
 * eigenvalue sits on an end; span0 = max(hi - lo, 1e-300) of the bracket BEFORE the widening.  Any thread; no LDS, no barrier. */
__device__ __forceinline__ hs_td_bracket hs_td_widen(double lo, double hi)
{
   const double span0 = fmax(hi - lo, 1e-300);
   lo -= 1e-12 * span0 + 1e-300;
   hi += 1e-12 * span0 + 1e-300;
   return { lo, hi, span0 };
}

/* The stopping rule of a search: the interval is down to two ulps of the eigenvalue (it cannot get shorter than one), but not below
 * half an ulp of the norm - lo, hi belong to the matrix scaled to norm <= 1, whose 0.25 is that floor.  Any thread; no LDS, no barrier. */
__device__ __forceinline__ bool hs_td_converged(double lo, double hi)
{
   return hi - lo <= 4.5e-16 * fmax(fmax(fabs(lo), fabs(hi)), 0.25);
}

/* Gershgorin bracket (widened: hs_td_widen) and norm bound of T, serial: lo = min (d_i - r_i), hi = max (d_i + r_i), tnorm =
 * max (|d_i| + r_i) with r_i = |e_{i-1}| + |e_i| and i ascending; e[n - 1] is not read; tnorm may be zero.  Every thread that needs
 * the result runs the loop itself (d, e in LDS: the reads are broadcasts); no LDS of its own, no barrier. */
__device__ __forceinline__ hs_td_gersh hs_td_gershgorin(int n, const double* d, const double* e)
{
   double lo = 1e300, hi = -1e300, tnorm = 0.0;
   for (int i = 0; i < n; ++i)
   {
      const double rad = (i > 0 ? fabs(e[i - 1]) : 0.0) + (i + 1 < n ? fabs(e[i]) : 0.0);
      lo = fmin(lo, d[i] - rad);
      hi = fmax(hi, d[i] + rad);
      tnorm = fmax(tnorm, fabs(d[i]) + rad);
   }
   const hs_td_bracket b = hs_td_widen(lo, hi);
   return { b.lo, b.hi, b.span0, tnorm };
}

/* The same over a workgroup of NT threads, thread i holding row i's lo = d_i - r_i, hi = d_i + r_i, tn = |d_i| + r_i (a thread
 * without a row: 1e300, -1e300, 0).  ALL NT threads call it.  Minimum and maximum by the butterfly lane ^ 1, 2, .., 32 in every
 * wavefront, lane 0 to red[0 .. 2][wave], ONE barrier, then every thread folds the wavefronts in ascending order (minima and
 * maxima: the order does not change the result).  Returns the widened bracket (hs_td_widen) with tnorm >= 1e-300, the same in every
 * thread; the callers scale by sinv = 1 / tnorm.  Whatever else the caller stores to LDS before the call is visible after it; red
 * must not be written again before the caller's next barrier. */
template<int NT>
__device__ __forceinline__ hs_td_gersh hs_td_bounds(double lo, double hi, double tn, double (*red)[NT / 64])
{
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
   for (int m = 1; m < 64; m <<= 1)
   {
      lo = fmin(lo, __shfl_xor(lo, m, 64));
      hi = fmax(hi, __shfl_xor(hi, m, 64));
      tn = fmax(tn, __shfl_xor(tn, m, 64));
   }
   if ( lane == 0 )
   {
      red[0][wave] = lo; red[1][wave] = hi; red[2][wave] = tn;
   }
   __syncthreads();
   double glo = red[0][0], ghi = red[1][0], tnorm = red[2][0];
#pragma unroll
   for (int w = 1; w < NT / 64; ++w)
   {
      glo = fmin(glo, red[0][w]); ghi = fmax(ghi, red[1][w]); tnorm = fmax(tnorm, red[2][w]);
   }
   const hs_td_bracket b = hs_td_widen(glo, ghi);
   return { b.lo, b.hi, b.span0, fmax(tnorm, 1e-300) };
}

/* What ei_sturm_count reads behind the scaled matrix ds[0 .. n - 1], es[0 .. n - 2]: it runs in blocks of four steps and fetches the
 * next block ahead, up to ds[n + 2] and es[n + 1], and wants rows there that cannot change a sign while |x| <= 1 - diagonal 4.0,
 * no coupling, es zero from n - 1 on.  Thread t of eight (t = 0 .. 7; others return at once) writes ds[n + t] and es[n - 1 + t];
 * ds and es need n + 8 entries.  No barrier: the caller puts one between this and the first count.  A caller that itself stores
 * es[n - 1] = 0 before the same barrier stores the same value. */
__device__ __forceinline__ void hs_td_pad(double* ds, double* es, int n, int t)
{
   if ( t < 8 )
   {
      ds[n + t] = 4.0;
      es[n - 1 + t] = 0.0;
   }
}

/* Sturm multisection for up to HS_SYEVX_MAXK eigenvalues at once, each with S shifts per round (S * slots <= blockDim.x).  ALL
 * threads of the workgroup call it; thread = (slot kk, shift sh), act = the slot searches, ith = the (1-based) index it wants,
 * idle = the count an inactive thread reports.  lo, hi: the bracket (scaled matrix); returned: the interval of eigenvalue ith.
 * count(x) = eigenvalues below x.  Per round the S + 1 subintervals of [lo, hi]: b = number of the slot's shifts with fewer than
 * ith eigenvalues below them = the subinterval that holds it; b is summed with an integer atomicAdd in LDS (the only atomic of the
 * solvers: integer, so the order of the additions does not matter).  cntb[2][HS_SYEVX_MAXK] must be ZERO on entry with a barrier
 * behind the clearing; the rounds alternate between its halves, the idle half is cleared for the next round.  TWO barriers per
 * round (one behind the additions, one in __syncthreads_and); at most 48 rounds, all slots stop together (hs_td_converged). */
template<class COUNT>
__device__ __forceinline__ hs_td_interval hs_td_multisect(int S, int kk, int sh, bool act, int ith, int idle, double lo, double hi,
   int (*cntb)[HS_SYEVX_MAXK], COUNT count)
{
   const int tid = threadIdx.x;
   const double rS1 = 1.0 / (double) (S + 1);
   for (int round = 0; round < 48; ++round)
   {
      const double w = (hi - lo) * rS1;
      const double x = lo + w * (double) (sh + 1);
      const int c = act ? count(x) : idle;
      if ( tid < HS_SYEVX_MAXK )
         cntb[(round + 1) & 1][tid] = 0;
      if ( act && c < ith )
         atomicAdd(&cntb[round & 1][kk], 1);
      __syncthreads();
      const int b = act ? cntb[round & 1][kk] : 0;
      const double nlo = lo + w * (double) b;
      const double nhi = (b < S) ? lo + w * (double) (b + 1) : hi;
      lo = nlo; hi = nhi;
      if ( __syncthreads_and((!act || hs_td_converged(lo, hi)) ? 1 : 0) )
         break;
   }
   return { lo, hi };
}

/* Entry i of the start vector of eigenvector k: in [0.5, 1.5) from a hash of (i, k) - different from vector to vector, so that a
 * multiple eigenvalue gets a basis of its space out of them.  Any thread; no LDS, no barrier. */
__device__ __forceinline__ double hs_td_start(int i, int k)
{
   unsigned h = (unsigned) (i * 2654435761u) ^ (unsigned) ((k + 1) * 40503u);
   h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
   return 0.5 + (double) (h & 0xFFFF) * (1.0 / 65536.0);
}

/* One step of inverse iteration for ONE vector by ONE thread: solves (T - theta I) x = z on the rows r0 .. r1 - 1 (r1 - r0 >= 2) of
 * T = (d, e) and leaves x / ||x|| in z; rows outside are not touched.  Gaussian elimination with partial pivoting, the factors
 * (1 / pivot, the two superdiagonals of U) to G0, G1, G2 at [row * PITCH + col] - col = the thread's vector among the PITCH of its
 * workgroup, so the threads of a wavefront store side by side -, then the backward sweep with the factors of eight rows on
 * their way while the recurrence runs.  A pivot below tiny = 1e-14 max(span0, |theta|) is replaced by tiny; x is scaled by 1e-140
 * whenever its squared norm passes 1e280; a norm that is zero or not finite gives the unit vector of row kglobal (BLOCKS = false)
 * or r0 + kglobal % (r1 - r0) (BLOCKS = true: the vector's own block of a matrix that splits; the flag keeps the integer modulo
 * out of the other kernel).  Everything in plain sequence, nrm = x_{r1-1}^2 + x_{r1-2}^2 + .. in descending rows.
 * d, e, z in LDS, read and written by this thread alone between two barriers of the caller; no barrier inside. */
template<int PITCH, bool BLOCKS>
__device__ __forceinline__ void hs_td_invit(double* z, const double* d, const double* e, int r0, int r1, double theta, double span0,
   double* __restrict__ G0, double* __restrict__ G1, double* __restrict__ G2, int col, int kglobal)
{
   const double tiny = 1e-14 * fmax(span0, fmax(fabs(theta), 1e-300));
   double dd = d[r0] - theta, du = e[r0];
   double cur = z[r0];
   for (int i = r0; i < r1 - 1; ++i)
   {
      const double dl = e[i];
      const double dn = d[i + 1] - theta;
      const double un = (i + 2 < r1) ? e[i + 1] : 0.0;
      const double nxt = z[i + 1];
      if ( fabs(dd) >= fabs(dl) || fabs(dl) < tiny )
      {
         if ( fabs(dd) < tiny ) dd = tiny;
         const double rinv = 1.0 / dd;
         const double mlt = dl * rinv;
         G0[i * PITCH + col] = rinv; G1[i * PITCH + col] = du; G2[i * PITCH + col] = 0.0;
         z[i] = cur;
         cur = nxt - mlt * cur;
         dd = dn - mlt * du;
         du = un;
      }
      else
      {
         const double rinv = 1.0 / dl;
         const double mlt = dd * rinv;
         G0[i * PITCH + col] = rinv; G1[i * PITCH + col] = dn; G2[i * PITCH + col] = un;
         z[i] = nxt;
         cur = cur - mlt * nxt;
         dd = du - mlt * dn;
         du = -mlt * un;
      }
   }
   if ( fabs(dd) < tiny ) dd = tiny;
   double x1 = cur / dd, x2 = 0.0;
   double nrm = x1 * x1;
   z[r1 - 1] = x1;
   for (int i0 = r1 - 2; i0 >= r0; i0 -= 8)
   {
      double g0[8], g1[8], g2[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
      {
         const int i = (i0 - u >= r0) ? i0 - u : r0;
         g0[u] = G0[i * PITCH + col];
         g1[u] = G1[i * PITCH + col];
         g2[u] = G2[i * PITCH + col];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
      {
         const int i = i0 - u;
         if ( i >= r0 )
         {
            const double xi = (z[i] - g1[u] * x1 - g2[u] * x2) * g0[u];
            z[i] = xi;
            nrm += xi * xi;
            x2 = x1; x1 = xi;
            if ( !(nrm < 1e280) )
            {
               const double sc1 = 1e-140;
               for (int q = i; q < r1; ++q)
                  z[q] *= sc1;
               x1 *= sc1; x2 *= sc1; nrm *= sc1 * sc1;
            }
         }
      }
   }
   double rn = 1.0 / sqrt(fmax(nrm, 1e-300));
   if ( !(nrm > 0.0) || !(nrm < 1e300) )
   {
      const int one = BLOCKS ? r0 + kglobal % (r1 - r0) : kglobal;
      for (int i = r0; i < r1; ++i)
         z[i] = (i == one) ? 1.0 : 0.0;
      rn = 1.0;
   }
   for (int i = r0; i < r1; ++i)
      z[i] *= rn;
}

/* The tail of a back-transformation, one wavefront per vector, lane l holding the entries z[m] of the rows l + 64 m: the vector
 * scaled to norm one (left as it is when it is zero) to dst[0 .. n - 1].  All 64 lanes call it.  nr = fma over m ascending, then
 * hs_xsum<64>; no LDS, no barrier. */
template<int NJ>
__device__ __forceinline__ void hs_td_store_unit(const double (&z)[NJ], int n, int lane, double* __restrict__ dst)
{
   double nr = 0.0;
#pragma unroll
   for (int m = 0; m < NJ; ++m)
      nr = fma(z[m], z[m], nr);
   nr = hs_xsum<64>(nr);
   const double rn = nr > 0.0 ? 1.0 / sqrt(nr) : 1.0;
   dst += lane;
#pragma unroll
   for (int m = 0; m < NJ; ++m)
      if ( lane + 64 * m < n )
         dst[64 * m] = z[m] * rn;
}

#endif
