/* hs_scl_tpower.h - the truncated power method on a matrix of 129 .. 512 rows that does not fit into LDS, as device functions: what
 * k_sc_tpower_large (sparsecuts_large.hip: ONE block per call, hipsdp_sparsecuts) and the kernels of sparsecuts_large_rounds.hip (all
 * such blocks of a solver per launch, hipsdp_sparsecuts_all_large) instantiate.  One workgroup of SCL_NT = 512 threads works on one
 * block, thread i = row i, eight wavefronts.
 *
 * M = maxeig I - Z stays EXPLICIT (m_ii = maxeig - z_ii, m_ij = -z_ij), in a global workspace of n^2 doubles, stored TRANSPOSED:
 * MT[c n + r] = M[r][c].  The product (M x)_i = sum_p M[i][s_p] x_p over the ascending support s then reads `size` contiguous rows
 * of MT, one coalesced load per support entry with thread i at column i, and keeps the summands and their order of the row-major
 * product of the reference.  The diagonal of Z, x on its support, |w|, v0, the two lists and the partial sums are in LDS (about
 * 23 KB: SCL_LDS_DECL in the kernel, handed on as scl_lds).  The truncation keeps entry i when fewer than `size` entries j have
 * |w_j| > |w_i|, or |w_j| == |w_i| and j < i.  The ascending support list comes from a ballot per wavefront and the kept counts of the
 * wavefronts before it.  All sums: hs_wave_sum_dpp per wavefront, then the eight wavefronts in index order.
 *
 * HAZARD RULE: MT is read and written by its workgroup alone, and SCL_STORES_DONE with a workgroup barrier stands between its global
 * stores to MT (the fill, every deflation, every new diagonal) and its later loads.  Every loop condition is false for a NaN, and
 * every loop is bounded by maxit or maxcuts. */
#ifndef HS_SCL_TPOWER_H
#define HS_SCL_TPOWER_H

#include "hs_kernels.h"
#include "hs_wave.h"

#ifndef SCL_NT
#define SCL_NT 512         /* one thread per row, HS_SCL_MAXN rows at most (sparsecuts_large.hip names it in front of its launches) */
#endif
#define SCL_NW (SCL_NT / 64)
#define SCL_CT 256         /* the coefficient kernels */

/* the LDS of a workgroup that runs scl_tpower_run */
struct scl_lds
{
   long long* keys;        /* [SCL_NT]      |w| as ordered integers; rows n .. 511 hold -1 */
   long long* ckey;        /* [SCL_NT + 2]  the keys of the candidates, in index order */
   double* zd;             /* [SCL_NT]      the diagonal of Z: M's is formed from it again after every cut */
   double* xc;             /* [SCL_NT]      x on its support: xc[p] = x[sup[p]] */
   double* v0s;            /* [SCL_NT]      the start vector */
   double* red;            /* [SCL_NW] */
   int* sup;               /* [SCL_NT] */
   int* wkept;             /* [SCL_NW] */
   int* wcand;             /* [SCL_NW] */
};
#define SCL_LDS_DECL(L) \
   __shared__ __attribute__((aligned(16))) long long scl_keys[SCL_NT]; \
   __shared__ __attribute__((aligned(16))) long long scl_ckey[SCL_NT + 2]; \
   __shared__ double scl_zd[SCL_NT]; \
   __shared__ double scl_xc[SCL_NT]; \
   __shared__ double scl_v0s[SCL_NT]; \
   __shared__ double scl_red[SCL_NW]; \
   __shared__ int scl_sup[SCL_NT]; \
   __shared__ int scl_wkept[SCL_NW], scl_wcand[SCL_NW]; \
   const scl_lds L = {scl_keys, scl_ckey, scl_zd, scl_xc, scl_v0s, scl_red, scl_sup, scl_wkept, scl_wcand}

/* Sum over the workgroup, the same bits in every thread.  ONE barrier, behind the stores to red - red must not be written again
 * before the next barrier of the caller. */
__device__ __forceinline__ double scl_block_sum(double v, double* red)
{
   v = hs_wave_sum_dpp(v);
   if ( (threadIdx.x & 63) == 0 )
      red[threadIdx.x >> 6] = v;
   __syncthreads();
   double s = red[0];
#pragma unroll
   for (int w = 1; w < SCL_NW; ++w)
      s += red[w];
   return s;
}

/* (M x)_i = sum_p M[i][s_p] x_p in the order of p, mcol = MT + i: M[i][c] lies at mcol[c n].  LIST: s_p = sup[p] (x on its ascending
 * support), otherwise s_p = p (a dense x).  The loads of eight summands are in flight together - one round trip to the L2 per eight
 * instead of one per summand -, the additions keep their order. */
template<bool LIST>
__device__ __forceinline__ double scl_row_product(const double* mcol, int n, const double* xv, const int* sup, int cnt)
{
   double acc = 0.0;
   int p = 0;
   for (; p + 8 <= cnt; p += 8)
   {
      double mv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)
         mv[k] = mcol[(size_t) (LIST ? sup[p + k] : p + k) * n];
#pragma unroll
      for (int k = 0; k < 8; ++k)
         acc += mv[k] * xv[p + k];
   }
   for (; p < cnt; ++p)
      acc += mcol[(size_t) (LIST ? sup[p] : p) * n] * xv[p];
   return acc;
}

/* the global stores of this wavefront to MT have left it: with the barrier that follows, the workgroup's later loads see them */
#define SCL_STORES_DONE() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")

/* MT[c n + r] = M[r][c] of M = maxeig I - Z, and the diagonal of Z to zd: Z is read in memory order, as k_sc_tpower reads it */
__device__ __forceinline__ void scl_fill_mt(int n, const double* __restrict__ Z, double maxeig, double* MT, double* zd)
{
   const int tid = threadIdx.x;
   for (int e0 = tid; e0 < n * n; e0 += 8 * SCL_NT)
   {
      double zv[8];
#pragma unroll
      for (int k = 0; k < 8; ++k)             /* (eight loads in flight, as in scl_row_product) */
         zv[k] = e0 + k * SCL_NT < n * n ? Z[e0 + k * SCL_NT] : 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k)
      {
         const int e = e0 + k * SCL_NT;
         if ( e < n * n )
         {
            const int r = e / n, c = e - r * n;
            MT[(size_t) c * n + r] = r == c ? maxeig - zv[k] : -zv[k];
            if ( r == c )
               zd[r] = zv[k];
         }
      }
   }
}

/* what a TPower run leaves: this thread's entry of the last iterate (an exact zero off the support), the last two Rayleigh quotients,
 * the iterations, dead: a truncated iterate had norm 0; the support and the values on it stay in L.sup / L.xc */
struct scl_run { double x, newv, oldv; int it; bool dead; };

/* ONE TPower run from L.v0s on the M that lies in MT (mcol = MT + this thread's row), by all threads of the workgroup.  Starts with the
 * wait for the workgroup's stores to MT and a barrier (which also ends the last reads of x and the support of the run before). */
__device__ __forceinline__ scl_run scl_tpower_run(int n, int size, bool row, const double* mcol, const scl_lds& L, double convtol, int maxit)
{
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const bool prune = size < 64;             /* (with 64 and more every row is a candidate) */
   long long* keys = L.keys;
   long long* ckey = L.ckey;
   double *xc = L.xc, *red = L.red;
   int *sup = L.sup, *wkept = L.wkept, *wcand = L.wcand;
   SCL_STORES_DONE();
   __syncthreads();           /* MT (first run: filled, later: after the cut) and the last reads of x and the support */
   double x = 0.0, u = 0.0;
   if ( row )
   {
      x = L.v0s[tid];
      u = scl_row_product<false>(mcol, n, L.v0s, sup, n);
   }
   double newv = -1.0, oldv = -2.0;
   int it = 0;
   bool dead = false;
   while ( newv - oldv > convtol && it < maxit )
   {
      oldv = newv;
      const double w = u;
      /* The truncation: entry i stays when fewer than `size` entries lie ABOVE it - j above i: |w_j| > |w_i|, or |w_j| == |w_i|
       * and j < i.  Non-negative doubles order as their bit patterns read as signed integers (+0 is 0; a NaN lies above every
       * number, so the order stays total, exactly `size` entries stay and the lists stay inside their arrays).  Ranking every
       * entry among all n is n^2 comparisons on one compute unit; instead
       *   1. every entry is ranked inside its own wavefront of 64 rows; with `size` entries above it there it cannot stay.  The
       *      others are the CANDIDATES, at most `size` per wavefront, listed in index order (ballot and the counts of the
       *      wavefronts before, as for the support);
       *   2. a candidate is ranked among the candidates alone.  That decides exactly as the full ranking: the `size` entries
       *      that stay have fewer than `size` entries above them in their wavefront too, so all of them are candidates, and
       *      they lie above every entry that does not stay; an entry that stays has fewer than `size` entries above it at all.
       * In the list the order of the positions is the order of the indices: the tie rule reads the positions. */
      const long long key = __double_as_longlong(fabs(w));
      if ( row )
         keys[tid] = key;
      __syncthreads();
      bool cand = row;
      if ( prune )
      {
         const long long* kw = keys + (wave << 6);
         int loc = 0;
#pragma unroll 4
         for (int j = 0; j < 64; j += 2)
         {
            const longlong2 a = *reinterpret_cast<const longlong2*>(kw + j);
            loc += (int) (a.x > key) | ((int) (a.x == key) & (int) (j < lane));
            loc += (int) (a.y > key) | ((int) (a.y == key) & (int) (j + 1 < lane));
         }
         cand = row && loc < size;
      }
      const unsigned long long cmask = __ballot(cand);
      if ( lane == 0 )
         wcand[wave] = __popcll(cmask);
      __syncthreads();
      int cpos = __popcll(cmask & ((1ull << lane) - 1ull)), ncand = 0;
#pragma unroll
      for (int v = 0; v < SCL_NW; ++v)
      {
         cpos += v < wave ? wcand[v] : 0;
         ncand += wcand[v];
      }
      if ( cand )
         ckey[cpos] = key;
      if ( tid == 0 )
         ckey[ncand] = -1;              /* (the list is read in pairs) */
      __syncthreads();
      int above = 0;
      if ( cand )
      {
#pragma unroll 4
         for (int j = 0; j < ncand; j += 2)
         {
            const longlong2 a = *reinterpret_cast<const longlong2*>(ckey + j);
            above += (int) (a.x > key) | ((int) (a.x == key) & (int) (j < cpos));
            above += (int) (a.y > key) | ((int) (a.y == key) & (int) (j + 1 < cpos));
         }
      }
      const bool kept = cand && above < size;
      const unsigned long long mask = __ballot(kept);
      const int before = __popcll(mask & ((1ull << lane) - 1ull));
      if ( lane == 0 )
         wkept[wave] = __popcll(mask);
      const double nrm = sqrt(scl_block_sum(kept ? w * w : 0.0, red));
      if ( nrm == 0.0 )
      {
         dead = true;
         break;
      }
      int pos = before;
      for (int v = 0; v < wave; ++v)
         pos += wkept[v];
      x = kept ? w / nrm : 0.0;
      if ( kept )
      {
         sup[pos] = tid;
         xc[pos] = x;
      }
      __syncthreads();
      u = row ? scl_row_product<true>(mcol, n, xc, sup, size) : 0.0;
      newv = scl_block_sum(x * u, red);
      ++it;
   }
   scl_run r;
   r.x = x; r.newv = newv; r.oldv = oldv; r.it = it; r.dead = dead;
   return r;
}

/* The whole loop over cuts and iterations of the default configuration on ONE block, by all threads of its workgroup: Z (n x n), lmin,
 * maxeig and the start vector v0[n] in device memory, MT: n^2 doubles that only this workgroup touches.  The results go to index 0 of
 * out (slots 0 .. maxcuts - 1, vectors from out.vec, supports with pitch out.smax): the caller hands over the view of its block.  A cut
 * (Z -= scalar x x^T, maxeig -= scalar) adds scalar x_p x_q to MT[s_q n + s_p] for the size^2 pairs of the support - the expression of
 * k_sc_tpower for M[s_p][s_q] - and forms the diagonal again. */
__device__ __forceinline__ void scl_tpower_loop(int n, int size, const double* __restrict__ Z, double lmin, double maxeig,
   const double* __restrict__ v0, double* MT, const hs_sc_par& par, const hs_sc_out& out, const scl_lds& L)
{
   const int tid = threadIdx.x;
   if ( n < 1 || n > SCL_NT || !(lmin < -par.tol) || size > n || size < 1 || par.maxcuts <= 0 )
   {
      if ( tid == 0 )
      {
         out.ncuts[0] = 0; out.iters[0] = 0; out.flags[0] = 0;
         out.lmin[0] = lmin;
      }
      return;
   }
   const bool row = tid < n;
   double *zd = L.zd, *xc = L.xc;
   int* sup = L.sup;
   scl_fill_mt(n, Z, maxeig, MT, zd);
   L.v0s[tid] = row ? v0[tid] : 0.0;
   L.keys[tid] = -1;
   sup[tid] = 0;
   const double* mcol = MT + (row ? tid : 0);          /* M[tid][c] at mcol[c n] */
   int nc = 0, iters = 0, flags = 0;
   for (;;)
   {
      /* ---- one TPower run from v0 on M (as in the reference, one more follows the last cut) ---- */
      const scl_run run = scl_tpower_run(n, size, row, mcol, L, par.convtol, par.maxit);
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
         out.eig[nc] = scalar;
      if ( row )
         out.vec[(long long) nc * n + tid] = x;
      if ( tid < size )
         out.sup[(long long) nc * out.smax + tid] = sup[tid];
      for (int e = tid; e < size * size; e += SCL_NT)
      {
         const int p = e / size, q = e - p * size;
         const double t = scalar * xc[p] * xc[q];
         if ( p == q )
            zd[sup[p]] -= t;
         else
            MT[(size_t) sup[q] * n + sup[p]] += t;
      }
      maxeig -= scalar;
      SCL_STORES_DONE();
      __syncthreads();
      if ( row )
         MT[(size_t) tid * n + tid] = maxeig - zd[tid];
      ++nc;
   }
   if ( tid == 0 )
   {
      out.ncuts[0] = nc; out.iters[0] = iters; out.flags[0] = flags;
      out.lmin[0] = lmin;
   }
}

/* x_c^T A_i x_c of every cut c of ONE block over the pairs of its support (a block kept as nonzeros: over the variable's nonzeros),
 * by a workgroup of SCL_CT threads for matrix i (0: the constant matrix, to lhs): the support and the values of a cut (nonzeros: the
 * dense vector) in LDS.  out: the view of the block (index 0, slots 0 .. maxcuts - 1). */
__device__ __forceinline__ void scl_coefs_block(int m, int maxcuts, int size, int i, const hs_ec_job& job, const hs_sc_out& out, double* xs,
   int* sup, double* part)
{
   const int n = job.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int nc = out.ncuts[0];
   if ( nc <= 0 || nc > maxcuts || size > n || size < 1 || n > HS_SCL_MAXN )
      return;
   const bool walk = job.form == HS_EC_SPARSE && i > 0;       /* (the constant matrix of a sparse block is its dense row 0) */
   const double* __restrict__ a = job.A + (walk ? 0LL : (long long) i * job.ld);
   const int np = size * (size + 1) / 2;
   for (int c = 0; c < nc; ++c)
   {
      const double* __restrict__ v = out.vec + (long long) c * n;
      if ( walk )
      {
         for (int t = tid; t < n; t += SCL_CT)
            xs[t] = v[t];
      }
      else
      {
         for (int t = tid; t < size; t += SCL_CT)
         {
            const int s = out.sup[(long long) c * out.smax + t];
            sup[t] = s;
            xs[t] = v[s];
         }
      }
      __syncthreads();
      double acc = 0.0;
      if ( walk )
      {
         for (int e = job.sp.voff[i - 1] + tid; e < job.sp.voff[i]; e += SCL_CT)
         {
            const int r = job.sp.vrow[e], q = job.sp.vcol[e];
            acc += (r == q ? 1.0 : 2.0) * job.sp.vval[e] * xs[r] * xs[q];
         }
      }
      else
      {
         for (int t = tid; t < np; t += SCL_CT)
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
         for (int w = 0; w < SCL_CT / 64; ++w)
            t += part[w];
         if ( i == 0 )
            out.lhs[c] = t;
         else
            out.coef[(long long) c * m + (i - 1)] = t;
      }
      __syncthreads();
   }
}

/* the view of block blk of a result over many blocks (slots blk maxcuts + c, vectors from vecoff on) as the index-0 view above */
__device__ __forceinline__ hs_sc_out scl_block_view(const hs_sc_out& out, int blk, int maxcuts, int m, long long vecoff)
{
   const long long slot = (long long) blk * maxcuts;
   hs_sc_out o = out;
   o.ncuts = out.ncuts + blk; o.iters = out.iters + blk; o.flags = out.flags + blk; o.lmin = out.lmin + blk;
   o.eig = out.eig + slot; o.lhs = out.lhs + slot; o.coef = out.coef + slot * m; o.vec = out.vec + vecoff;
   o.sup = out.sup + slot * out.smax;
   return o;
}

#endif
