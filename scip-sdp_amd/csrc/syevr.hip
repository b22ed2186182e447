/* syevr.hip - ALL eigenpairs of a symmetric matrix of 129 .. 512 rows through the tridiagonal form (what DSYEVR does for RANGE = 'A'):
 * the full-decomposition counterpart of syevx.hip, whose stage 1 it uses unchanged.
 *
 *   1. Householder tridiagonalisation: hs_syevx_tridiag_dev (syevx.hip), one launch per column; d, e, the reflectors and tau are
 *      reached through hs_syevx_tridiag_view.
 *   2. All n eigenvalues and the structure of T, two launches:
 *        k_syevr_values, ceil(n / 32) workgroups: every workgroup finds the places where T splits (SPLIT TABLE: row i belongs to
 *          the block [bs, be) of rows between two negligible off-diagonal entries) and computes the eigenvalues of 32 SLOTS: slot p
 *          is eigenvalue p - bs + 1 of the block that holds row p, found by Sturm multisection ON THAT BLOCK (ei_sturm_count_rows,
 *          16 shifts per slot and round: hs_td_multisect of hs_tridiag.h, as k_syevx_values).  An eigenvalue therefore belongs to its
 *          block by construction, also when several blocks have it in common; a block of one row returns its diagonal entry.
 *        k_syevr_order, one workgroup: rank of every slot among all n (ties in the order of the slots) -> the ascending eigenvalues,
 *          and per eigenvalue its block and its CLUSTER: the run of eigenvalues OF THE SAME BLOCK each closer than 1e-3 ||T|| to
 *          its predecessor, named by the (ascending) index of its first member.
 *      Both tables stay in the workspace; nothing is read back.
 *   3. The eigenvectors of T, three rounds of
 *        k_syevr_step, ceil(n / 32) workgroups of 32 vectors: one step of inverse iteration per vector on the vector's block of T,
 *          one thread per elimination chain (partial pivoting, factors in device memory as [row][vector]): hs_td_invit of
 *          hs_tridiag.h, the chain of k_syevx_tvec on a range of rows;
 *        then per panel p of 32 consecutive eigenvalue indices, in the order of the panels,
 *        k_syevr_ortho_prev (A(p)), one workgroup per vector: classical Gram-Schmidt, twice, against the members of the vector's
 *          cluster in the panels before p - those are final for this round;
 *        k_syevr_ortho_panel (B(p)), one workgroup: Gram-Schmidt among the members of a cluster inside the panel, normalisation.
 *      Vectors of different blocks have disjoint supports and are never orthogonalised against each other.  A vector without
 *      earlier members of its cluster leaves A(p) at once, a panel without a cluster that started before its vectors leaves B(p).
 *   4. Back-transformation x = H_0 ... H_{n-3} z of all n vectors (k_syevr_back): one wavefront per vector, eight to a workgroup,
 *      which reads every reflector once into LDS for its eight vectors; a reflector that lies below the support of z is skipped.
 * HAZARD RULE: inside one launch no workgroup reads what another workgroup writes; the kernel boundary is the only
 * synchronisation between workgroups.  Every reduction runs in a fixed order, no floating-point atomics: same input, same bits.
 * Launches: n for stage 1, 2 for stage 2, 3 + 6 ceil(n / 32) for stage 3, 1 for stage 4.
 * Each of stages 2 to 4 is a __device__ body (d_syevr_values, _order, _step, _ortho_prev, _ortho_panel, _back) with two kernels around
 * it: the one of a single matrix and the one of MANY matrices per launch (k_syevr_*_many, hs_syevr_many_*: hipsdp_psd_project_many_large). */
#include "hs_common.h"
#include "hs_kernels.h"
#include "hs_tridiag.h"
#include <cmath>

#define SR_N   HS_SYEVX_MAXN
#define SR_P   HS_SYEVX_MAXK        /* vectors of a panel, slots of a workgroup of the eigenvalue kernel */
#define SR_T   512                  /* threads of the kernels of stages 2 and 3 */
#define SR_BW  8                    /* wavefronts (= vectors) of a workgroup of the back-transformation */
#define SR_BC  8                    /* reflectors staged in LDS at a time */

namespace {

/* the part of the workspace behind that of syevx.hip */
struct sr_ws
{
   double* lamU; double* lam; double* meta; int* bsU; int* beU; int* vlo; int* vhi; int* cid; double* Z; double* G0; double* G1; double* G2;
};

__host__ __device__ inline size_t sr_even(size_t v) { return (v + 1) & ~(size_t) 1; }
__host__ __device__ inline size_t sr_npad(int n) { return (size_t) SR_P * ((n + SR_P - 1) / SR_P); }

__host__ __device__ inline sr_ws sr_layout(int n, double* base)
{
   const size_t nl = sr_even((size_t) n), n2 = sr_even((size_t) n * n), ng = sr_even((size_t) n * sr_npad(n));
   sr_ws w;
   w.lamU = base; w.lam = w.lamU + nl; w.meta = w.lam + nl;
   int* ip = reinterpret_cast<int*>(w.meta + 8);
   w.bsU = ip; w.beU = ip + nl; w.vlo = ip + 2 * nl; w.vhi = ip + 3 * nl; w.cid = ip + 4 * nl;
   w.Z = w.meta + 8 + 3 * nl;
   w.G0 = w.Z + n2; w.G1 = w.G0 + ng; w.G2 = w.G1 + ng;
   return w;
}

size_t sr_ws_doubles(int n)
{
   const size_t nl = sr_even((size_t) n), n2 = sr_even((size_t) n * n), ng = sr_even((size_t) n * sr_npad(n));
   return 5 * nl + 8 + n2 + 3 * ng;
}

/* ---- stage 2a: split table and the eigenvalues of 32 slots per workgroup.  meta[0] = Gershgorin span, meta[1] = norm bound of T */
__device__ __forceinline__ void d_syevr_values(int n, int blk, const double* __restrict__ d, const double* __restrict__ e, double* __restrict__ lamU,
   int* __restrict__ bsU, int* __restrict__ beU, double* __restrict__ meta)
{
   __shared__ double ds[SR_N + 8], es[SR_N + 8], red[3][SR_T / 64];
   __shared__ int spl[SR_N], cntb[2][SR_P];
   const int tid = threadIdx.x;
   double lo = 1e300, hi = -1e300, tn = 0.0, dt = 0.0, et = 0.0;
   if ( tid < n )
   {
      dt = d[tid];
      et = (tid + 1 < n) ? e[tid] : 0.0;
      const double rad = (tid > 0 ? fabs(e[tid - 1]) : 0.0) + fabs(et);
      lo = dt - rad;
      hi = dt + rad;
      tn = fabs(dt) + rad;
   }
   if ( tid < 2 * SR_P )
      cntb[tid / SR_P][tid % SR_P] = 0;
   const hs_td_gersh g = hs_td_bounds<SR_T>(lo, hi, tn, red);
   const double glo = g.lo, ghi = g.hi, span0 = g.span0, tnorm = g.tnorm, sinv = 1.0 / tnorm;
   /* T splits behind row j where |e_j| <= eps (|d_j| + |d_{j+1}|) (DSTEIN's test) or |e_j| <= 4 eps ||T|| (the absolute test of the
    * QR routines: the eigenvalues are asked for to a multiple of eps ||T||, and only this one separates the rows that the reduction
    * of a low-rank matrix leaves coupled by its rounding errors).  The scaled matrix has e_j = 0 there. */
   if ( tid < n )
   {
      const double eps = 2.220446049250313e-16;
      const double dn = (tid + 1 < n) ? d[tid + 1] : 0.0;
      const int s = (tid + 1 >= n || fabs(et) <= eps * (fabs(dt) + fabs(dn)) || fabs(et) <= 4.0 * eps * tnorm) ? 1 : 0;
      spl[tid] = s;
      ds[tid] = dt * sinv;
      es[tid] = s ? 0.0 : (et * sinv) * (et * sinv);
   }
   hs_td_pad(ds, es, n, tid);
   __syncthreads();
   /* thread = (slot kk of this workgroup, one of 16 shifts) */
   const int S = SR_T / SR_P;
   const int kk = tid / S, sh = tid % S;
   const int slot = blk * SR_P + kk;
   int bs = 0, be = 1;
   if ( slot < n )
   {
      bs = slot;
      while ( bs > 0 && !spl[bs - 1] )
         --bs;
      be = slot;
      while ( !spl[be] )
         ++be;
      ++be;
   }
   const int rows = be - bs, ith = slot - bs + 1;
   const bool act = slot < n && rows > 1;
   const hs_td_interval iv = hs_td_multisect(S, kk, sh, act, ith, n, glo * sinv, ghi * sinv, cntb,
      [=](double x) { return ei_sturm_count_rows(ds + bs, es + bs, rows, x); });
   if ( slot < n && sh == 0 )
   {
      lamU[slot] = act ? 0.5 * (iv.lo + iv.hi) * tnorm : d[slot];
      bsU[slot] = bs;
      beU[slot] = be;
   }
   if ( blk == 0 && tid == 0 )
   {
      meta[0] = span0;
      meta[1] = tnorm;
   }
}

__global__ void __launch_bounds__(SR_T) k_syevr_values(int n, const double* __restrict__ d, const double* __restrict__ e, double* __restrict__ lamU,
   int* __restrict__ bsU, int* __restrict__ beU, double* __restrict__ meta)
{
   d_syevr_values(n, (int) blockIdx.x, d, e, lamU, bsU, beU, meta);
}

/* ---- stage 2b: ascending order and the cluster table.  For the eigenvalue of ascending index k: lam[k] (also to out), vlo / vhi =
 * its block of rows, cid = ascending index of the first member of its cluster (cid[k] <= k; == k: first member). */
__device__ __forceinline__ void d_syevr_order(int n, const double* __restrict__ lamU, const int* __restrict__ bsU, const int* __restrict__ beU,
   const double* __restrict__ meta, double* __restrict__ lam, int* __restrict__ vlo, int* __restrict__ vhi, int* __restrict__ cid, double* __restrict__ out)
{
   __shared__ double lu[SR_N];
   __shared__ int head[SR_N], rk[SR_N];
   const int p = threadIdx.x;
   const double ortol = 1e-3 * meta[1];
   double v = 0.0;
   int bs = 0;
   if ( p < n )
   {
      v = lamU[p];
      bs = bsU[p];
      lu[p] = v;
   }
   __syncthreads();
   if ( p < n )
   {
      int r = 0;
      for (int q = 0; q < n; ++q)
      {
         const double u = lu[q];
         r += (u < v || (u == v && q < p)) ? 1 : 0;
      }
      rk[p] = r;
      head[p] = (p == bs || !(v - lu[p - 1] <= ortol)) ? 1 : 0;
   }
   __syncthreads();
   if ( p < n )
   {
      int h = p;
      while ( !head[h] )
         --h;
      const int r = rk[p];
      lam[r] = v;
      out[r] = v;
      vlo[r] = bs;
      vhi[r] = beU[p];
      cid[r] = rk[h];
   }
}

__global__ void __launch_bounds__(SR_T) k_syevr_order(int n, const double* __restrict__ lamU, const int* __restrict__ bsU, const int* __restrict__ beU,
   const double* __restrict__ meta, double* __restrict__ lam, int* __restrict__ vlo, int* __restrict__ vhi, int* __restrict__ cid, double* __restrict__ out)
{
   d_syevr_order(n, lamU, bsU, beU, meta, lam, vlo, vhi, cid, out);
}

/* ---- stage 3, the step: vector k = 32 blockIdx + t on the rows [vlo[k], vhi[k]) of T.  Dynamic LDS: Z[32][n | 1].  iter == 0: start
 * vectors hashed per vector and row; later: the vectors of the previous round from Zg.  G0 .. G2: this workgroup's slab, [row][t]. */
__device__ __forceinline__ void d_syevr_step(int n, int iter, int blk, const double* __restrict__ dg, const double* __restrict__ eg,
   const double* __restrict__ lam, const int* __restrict__ vlo, const int* __restrict__ vhi, const double* __restrict__ meta, double* __restrict__ Zg,
   double* __restrict__ G0g, double* __restrict__ G1g, double* __restrict__ G2g, double* __restrict__ Z)
{
   __shared__ double d[SR_N], e[SR_N], th[SR_P];
   __shared__ int blo[SR_P], bhi[SR_P];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int ld = n | 1;
   const int k0 = blk * SR_P;
   const int cnt = min(SR_P, n - k0);
   const double span0 = meta[0];
   double* __restrict__ G0 = G0g + (size_t) blk * SR_P * n;
   double* __restrict__ G1 = G1g + (size_t) blk * SR_P * n;
   double* __restrict__ G2 = G2g + (size_t) blk * SR_P * n;
   if ( tid < n )
   {
      d[tid] = dg[tid];
      e[tid] = eg[tid];
   }
   if ( tid < cnt )
   {
      th[tid] = lam[k0 + tid];
      blo[tid] = vlo[k0 + tid];
      bhi[tid] = vhi[k0 + tid];
   }
   __syncthreads();
   for (int idx = tid; idx < cnt * n; idx += SR_T)
   {
      const int t = idx / n, i = idx - t * n, k = k0 + t;
      double z;
      if ( i < blo[t] || i >= bhi[t] )
         z = 0.0;
      else if ( bhi[t] - blo[t] == 1 )
         z = 1.0;
      else if ( iter > 0 )
         z = Zg[(size_t) k * n + i];
      else
         z = hs_td_start(i, k);
      Z[t * ld + i] = z;
   }
   __syncthreads();
   /* thread (wavefront t mod 8, lane t / 8) owns vector t: the 32 serial chains spread over the wavefronts */
   if ( lane < SR_P / 8 && (lane << 3 | wave) < cnt && bhi[lane << 3 | wave] - blo[lane << 3 | wave] > 1 )
   {
      const int t = lane << 3 | wave;
      hs_td_invit<SR_P, true>(Z + t * ld, d, e, blo[t], bhi[t], th[t], span0, G0, G1, G2, t, k0 + t);
   }
   __syncthreads();
   for (int idx = tid; idx < cnt * n; idx += SR_T)
   {
      const int t = idx / n, i = idx - t * n;
      Zg[(size_t) (k0 + t) * n + i] = Z[t * ld + i];
   }
}

__global__ void __launch_bounds__(SR_T) k_syevr_step(int n, int iter, const double* __restrict__ dg, const double* __restrict__ eg, const double* __restrict__ lam,
   const int* __restrict__ vlo, const int* __restrict__ vhi, const double* __restrict__ meta, double* __restrict__ Zg, double* __restrict__ G0g,
   double* __restrict__ G1g, double* __restrict__ G2g)
{
   extern __shared__ __attribute__((aligned(16))) double Z[];
   d_syevr_step(n, iter, (int) blockIdx.x, dg, eg, lam, vlo, vhi, meta, Zg, G0g, G1g, G2g, Z);
}

/* ---- stage 3, A(p): vector k = 32 p + blockIdx against the members of its cluster in the panels before p, twice.  The
 * coefficients one wavefront per earlier vector, the correction one thread per row with the earlier vectors in ascending order. */
__device__ __forceinline__ void d_syevr_ortho_prev(int n, int p, int t, const int* __restrict__ vlo, const int* __restrict__ vhi, const int* __restrict__ cid,
   double* __restrict__ Zg)
{
   __shared__ double zs[SR_N], coef[SR_N];
   __shared__ int mate[SR_N];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int kend = SR_P * p;
   const int k = kend + t;
   if ( k >= n )
      return;
   const int c = cid[k];
   if ( c >= kend )
      return;
   const int r0 = vlo[k], rows = vhi[k] - r0;
   const int nm = kend - c;                                 /* candidates c .. kend - 1; members of the cluster have cid == c */
   if ( tid < nm )
      mate[tid] = (cid[c + tid] == c) ? 1 : 0;
   if ( tid < rows )
      zs[tid] = Zg[(size_t) k * n + r0 + tid];
   __syncthreads();
   for (int pass = 0; pass < 2; ++pass)
   {
      for (int q = wave; q < nm; q += SR_T / 64)
      {
         double acc = 0.0;
         if ( mate[q] )
         {
            const double* __restrict__ zq = Zg + (size_t) (c + q) * n + r0;
            for (int i = lane; i < rows; i += 64)
               acc = fma(zq[i], zs[i], acc);
            acc = hs_xsum<64>(acc);
         }
         if ( lane == 0 )
            coef[q] = acc;
      }
      __syncthreads();
      if ( tid < rows )
      {
         const double* __restrict__ zc = Zg + (size_t) c * n + r0 + tid;
         double v = zs[tid];
         int q = 0;
         for (; q + 4 <= nm; q += 4)
         {
            /* (four loads on their way; a row that is no member is read and not used) */
            const double a0 = zc[(size_t) q * n], a1 = zc[(size_t) (q + 1) * n], a2 = zc[(size_t) (q + 2) * n], a3 = zc[(size_t) (q + 3) * n];
            if ( mate[q] ) v = fma(-coef[q], a0, v);
            if ( mate[q + 1] ) v = fma(-coef[q + 1], a1, v);
            if ( mate[q + 2] ) v = fma(-coef[q + 2], a2, v);
            if ( mate[q + 3] ) v = fma(-coef[q + 3], a3, v);
         }
         for (; q < nm; ++q)
            if ( mate[q] )
               v = fma(-coef[q], zc[(size_t) q * n], v);
         zs[tid] = v;
      }
      __syncthreads();
   }
   if ( tid < rows )
      Zg[(size_t) k * n + r0 + tid] = zs[tid];
}

__global__ void __launch_bounds__(SR_T) k_syevr_ortho_prev(int n, int p, const int* __restrict__ vlo, const int* __restrict__ vhi, const int* __restrict__ cid,
   double* __restrict__ Zg)
{
   d_syevr_ortho_prev(n, p, (int) blockIdx.x, vlo, vhi, cid, Zg);
}

/* ---- stage 3, B(p): the panel finished - Gram-Schmidt, twice, among the members of a cluster inside the panel, then the norm of
 * every vector that has earlier members at all.  Dynamic LDS: Z[32][n | 1]. */
__device__ __forceinline__ void d_syevr_ortho_panel(int n, int p, const int* __restrict__ cid, double* __restrict__ Zg, double* __restrict__ Z)
{
   __shared__ double coef[SR_P], red[2][SR_T / 64];
   __shared__ int cs[SR_P];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int ld = n | 1;
   const int k0 = SR_P * p;
   const int cnt = min(SR_P, n - k0);
   int mine = 0;
   if ( tid < cnt )
   {
      cs[tid] = cid[k0 + tid];
      mine = (cs[tid] != k0 + tid) ? 1 : 0;
   }
   if ( !__syncthreads_or(mine) )
      return;
   for (int idx = tid; idx < cnt * n; idx += SR_T)
   {
      const int t = idx / n, i = idx - t * n;
      Z[t * ld + i] = Zg[(size_t) (k0 + t) * n + i];
   }
   __syncthreads();
   for (int t = 0; t < cnt; ++t)
   {
      const int c = cs[t];
      if ( c == k0 + t )
         continue;                                         /* (the same in every thread) */
      for (int pass = 0; pass < 2; ++pass)
      {
         for (int q = wave; q < t; q += SR_T / 64)
         {
            double acc = 0.0;
            if ( cs[q] == c )
            {
               for (int i = lane; i < n; i += 64)
                  acc = fma(Z[q * ld + i], Z[t * ld + i], acc);
               acc = hs_xsum<64>(acc);
            }
            if ( lane == 0 )
               coef[q] = acc;
         }
         __syncthreads();
         if ( tid < n )
         {
            double v = Z[t * ld + tid];
            for (int q = 0; q < t; ++q)
               if ( cs[q] == c )
                  v = fma(-coef[q], Z[q * ld + tid], v);
            Z[t * ld + tid] = v;
         }
         __syncthreads();
      }
      const double v = (tid < n) ? Z[t * ld + tid] : 0.0;
      const double nr = hs_block_sum<SR_T / 64>(v * v, red[t & 1]);
      if ( tid < n )
         Z[t * ld + tid] = v / sqrt(fmax(nr, 1e-300));
      __syncthreads();
   }
   for (int idx = tid; idx < cnt * n; idx += SR_T)
   {
      const int t = idx / n, i = idx - t * n;
      if ( cs[t] != k0 + t )
         Zg[(size_t) (k0 + t) * n + i] = Z[t * ld + i];
   }
}

__global__ void __launch_bounds__(SR_T) k_syevr_ortho_panel(int n, int p, const int* __restrict__ cid, double* __restrict__ Zg)
{
   extern __shared__ __attribute__((aligned(16))) double Z[];
   d_syevr_ortho_panel(n, p, cid, Zg, Z);
}

/* ---- stage 4: x = H_0 H_1 ... H_{n-3} z for all n vectors.  Wavefront w of workgroup g owns vector 8 g + w, lane l holds the entries
 * l + 64 m.  The reflectors come through LDS eight at a time, read once from L2 per workgroup (wavefront w fetches reflector w of
 * the next eight into registers while the current eight are applied).  H_j acts on the rows j + 1 .. n - 1: a vector whose support ends at or before
 * row j + 1 is not changed by it and skips it, as it skips tau_j = 0. */
__device__ __forceinline__ void d_syevr_back(int n, int blk, const double* __restrict__ R, const double* __restrict__ tau, const double* __restrict__ Zg,
   const int* __restrict__ vhi, double* __restrict__ out)
{
   __shared__ double vs[SR_BC][SR_N], ts[SR_N];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int k = blk * SR_BW + wave;
   const bool have = k < n;
   for (int i = tid; i < n; i += SR_BW * 64)
      ts[i] = tau[i];
   double z[SR_N / 64];
#pragma unroll
   for (int m = 0; m < SR_N / 64; ++m)
      z[m] = (have && lane + 64 * m < n) ? Zg[(size_t) k * n + lane + 64 * m] : 0.0;
   const int top = have ? vhi[k] : 0;                       /* reflectors j with j + 1 < top touch the support */
   /* chunk ch holds the reflectors jt - 8 ch - u, u = 0 .. 7, jt = n - 3 */
   const int jt = n - 3;
   const int nch = (jt + 1 + SR_BC - 1) / SR_BC;
   double nx[SR_N / 64];
   {
      const int j = jt - wave;
#pragma unroll
      for (int m = 0; m < SR_N / 64; ++m)
         vs[wave][lane + 64 * m] = (j >= 0 && lane + 64 * m < n) ? R[(size_t) j * n + lane + 64 * m] : 0.0;
   }
   __syncthreads();
   for (int ch = 0; ch < nch; ++ch)
   {
      const int jn = jt - SR_BC * (ch + 1) - wave;
#pragma unroll
      for (int m = 0; m < SR_N / 64; ++m)
         nx[m] = (ch + 1 < nch && jn >= 0 && lane + 64 * m < n) ? R[(size_t) jn * n + lane + 64 * m] : 0.0;
#pragma unroll
      for (int u = 0; u < SR_BC; ++u)
      {
         const int j = jt - SR_BC * ch - u;
         if ( j >= 0 && j + 1 < top && ts[j] != 0.0 )      /* (the same in every lane of the wavefront) */
         {
            double dot = 0.0;
#pragma unroll
            for (int m = 0; m < SR_N / 64; ++m)
               dot = fma(vs[u][lane + 64 * m], z[m], dot);
            dot = ts[j] * hs_xsum<64>(dot);
#pragma unroll
            for (int m = 0; m < SR_N / 64; ++m)
               z[m] = fma(-dot, vs[u][lane + 64 * m], z[m]);
         }
      }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < SR_N / 64; ++m)
         vs[wave][lane + 64 * m] = nx[m];
      __syncthreads();
   }
   if ( !have )
      return;
   hs_td_store_unit(z, n, lane, out + (size_t) k * n);
}

__global__ void __launch_bounds__(SR_BW * 64) k_syevr_back(int n, const double* __restrict__ R, const double* __restrict__ tau, const double* __restrict__ Zg,
   const int* __restrict__ vhi, double* __restrict__ out)
{
   d_syevr_back(n, (int) blockIdx.x, R, tau, Zg, vhi, out);
}

/* ---- the same stages for MANY matrices per launch (hs_syevr_many_*; caller: hipsdp_psd_project_many_large, psd_large.hip): matrix
 * blockIdx.y of the table, its n and its arrays from its hs_srm_job; the bodies are those of the single matrix, so the bits of a
 * matrix are those of hs_syevr_dev on it alone.  The grids are sized by the largest matrix of the table: a workgroup whose slots,
 * panel or vectors lie beyond its matrix's n leaves at once (uniform per workgroup). */
__global__ void __launch_bounds__(SR_T) k_syevr_values_many(const hs_srm_job* __restrict__ jobs)
{
   const hs_srm_job J = jobs[blockIdx.y];
   if ( (int) blockIdx.x * SR_P >= J.n )
      return;
   const sr_ws w = sr_layout(J.n, J.sr);
   d_syevr_values(J.n, (int) blockIdx.x, J.d, J.e, w.lamU, w.bsU, w.beU, w.meta);
}

__global__ void __launch_bounds__(SR_T) k_syevr_order_many(const hs_srm_job* __restrict__ jobs)
{
   const hs_srm_job J = jobs[blockIdx.y];
   const sr_ws w = sr_layout(J.n, J.sr);
   d_syevr_order(J.n, w.lamU, w.bsU, w.beU, w.meta, w.lam, w.vlo, w.vhi, w.cid, J.out);
}

/* dynamic LDS: 32 x (nmax | 1) doubles */
__global__ void __launch_bounds__(SR_T) k_syevr_step_many(int iter, const hs_srm_job* __restrict__ jobs)
{
   extern __shared__ __attribute__((aligned(16))) double Z[];
   const hs_srm_job J = jobs[blockIdx.y];
   if ( (int) blockIdx.x * SR_P >= J.n )
      return;
   const sr_ws w = sr_layout(J.n, J.sr);
   d_syevr_step(J.n, iter, (int) blockIdx.x, J.d, J.e, w.lam, w.vlo, w.vhi, w.meta, w.Z, w.G0, w.G1, w.G2, Z);
}

__global__ void __launch_bounds__(SR_T) k_syevr_ortho_prev_many(int p, const hs_srm_job* __restrict__ jobs)
{
   const hs_srm_job J = jobs[blockIdx.y];
   if ( SR_P * p + (int) blockIdx.x >= J.n )
      return;
   const sr_ws w = sr_layout(J.n, J.sr);
   d_syevr_ortho_prev(J.n, p, (int) blockIdx.x, w.vlo, w.vhi, w.cid, w.Z);
}

/* dynamic LDS: 32 x (nmax | 1) doubles */
__global__ void __launch_bounds__(SR_T) k_syevr_ortho_panel_many(int p, const hs_srm_job* __restrict__ jobs)
{
   extern __shared__ __attribute__((aligned(16))) double Z[];
   const hs_srm_job J = jobs[blockIdx.y];
   if ( SR_P * p >= J.n )
      return;
   const sr_ws w = sr_layout(J.n, J.sr);
   d_syevr_ortho_panel(J.n, p, w.cid, w.Z, Z);
}

__global__ void __launch_bounds__(SR_BW * 64) k_syevr_back_many(const hs_srm_job* __restrict__ jobs)
{
   const hs_srm_job J = jobs[blockIdx.y];
   if ( (int) blockIdx.x * SR_BW >= J.n )
      return;
   const sr_ws w = sr_layout(J.n, J.sr);
   d_syevr_back(J.n, (int) blockIdx.x, J.R, J.tau, w.Z, w.vhi, J.out + HS_SYEVR_OUT_VEC(J.n));
}

}

size_t hs_syevr_ws(int n) { return (n < 2 || n > SR_N) ? 0 : hs_syevx_ws(n) + sr_ws_doubles(n); }

/* stages 2 and 3 on the (d, e) that lie in the workspace (hs_syevx_tridiag_view): eigenvalues to dOut[0 .. n - 1], the eigenvectors of T
 * as rows of hs_syevr_tvec_view(n, ws) */
int hs_syevr_tvec_dev(hipStream_t st, int n, int vectors, double* dOut, double* ws)
{
   if ( n < 2 || n > SR_N || dOut == NULL || ws == NULL )
      return HS_ERR_ARG;
   double* d; double* e; double* R; double* tau;
   hs_syevx_tridiag_view(n, ws, &d, &e, &R, &tau);
   const sr_ws w = sr_layout(n, ws + hs_syevx_ws(n));
   const int np = (n + SR_P - 1) / SR_P;
   hipLaunchKernelGGL(k_syevr_values, dim3(np), dim3(SR_T), 0, st, n, d, e, w.lamU, w.bsU, w.beU, w.meta);
   hipLaunchKernelGGL(k_syevr_order, dim3(1), dim3(SR_T), 0, st, n, w.lamU, w.bsU, w.beU, w.meta, w.lam, w.vlo, w.vhi, w.cid, dOut);
   if ( vectors )
   {
      static hs_attr_mask step_done, panel_done;
      const int ldsmax = SR_P * (SR_N + 1) * (int) sizeof(double);
      const size_t lds = (size_t) SR_P * (n | 1) * sizeof(double);
      HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_syevr_step), ldsmax, &step_done) );
      HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_syevr_ortho_panel), ldsmax, &panel_done) );
      for (int iter = 0; iter < 3; ++iter)
      {
         hipLaunchKernelGGL(k_syevr_step, dim3(np), dim3(SR_T), lds, st, n, iter, d, e, w.lam, w.vlo, w.vhi, w.meta, w.Z, w.G0, w.G1, w.G2);
         for (int p = 0; p < np; ++p)
         {
            hipLaunchKernelGGL(k_syevr_ortho_prev, dim3(SR_P), dim3(SR_T), 0, st, n, p, w.vlo, w.vhi, w.cid, w.Z);
            hipLaunchKernelGGL(k_syevr_ortho_panel, dim3(1), dim3(SR_T), lds, st, n, p, w.cid, w.Z);
         }
      }
   }
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

double* hs_syevr_tvec_view(int n, double* ws) { return sr_layout(n, ws + hs_syevx_ws(n)).Z; }

int hs_syevr_dev(hipStream_t st, int n, const double* dA, int vectors, double* dOut, double* ws)
{
   if ( n < 2 || n > SR_N || dA == NULL || dOut == NULL || ws == NULL )
      return HS_ERR_ARG;
   HS_CALL( hs_syevx_tridiag_dev(st, n, dA, ws) );
   HS_CALL( hs_syevr_tvec_dev(st, n, vectors, dOut, ws) );
   if ( vectors )
   {
      double* d; double* e; double* R; double* tau;
      hs_syevx_tridiag_view(n, ws, &d, &e, &R, &tau);
      const sr_ws w = sr_layout(n, ws + hs_syevx_ws(n));
      hipLaunchKernelGGL(k_syevr_back, dim3((n + SR_BW - 1) / SR_BW), dim3(SR_BW * 64), 0, st, n, R, tau, w.Z, w.vhi, dOut + HS_SYEVR_OUT_VEC(n));
      HS_HIP( hipGetLastError() );
   }
   return HS_OK;
}

/* ---- many matrices per launch.  hs_syevr_many_job: the table entry of a matrix of n rows with its workspace (hs_syevr_ws(n) doubles,
 * its head the workspace hs_syevx_many_job takes) and its output (HS_SYEVR_OUT(n) doubles, the layout of hs_syevr_dev). */
int hs_syevr_many_job(int n, double* ws, double* out, hs_srm_job* J)
{
   if ( n < 2 || n > SR_N || ws == NULL || out == NULL || J == NULL )
      return HS_ERR_ARG;
   J->n = n; J->pad = 0;
   hs_syevx_tridiag_view(n, ws, &J->d, &J->e, &J->R, &J->tau);
   J->sr = ws + hs_syevx_ws(n);
   J->out = out;
   return HS_OK;
}

/* stages 2 and 3 of every matrix on the forms hs_syevx_many_cols leaves: 5 + 6 ceil(nmax / 32) launches, whatever the matrices are */
int hs_syevr_many_tvec(hipStream_t st, int count, int nmax, const hs_srm_job* djobs)
{
   if ( count < 1 || nmax < 2 || nmax > SR_N || djobs == NULL )
      return HS_ERR_ARG;
   const int np = (nmax + SR_P - 1) / SR_P;
   static hs_attr_mask step_done, panel_done;
   const int ldsmax = SR_P * (SR_N + 1) * (int) sizeof(double);
   const size_t lds = (size_t) SR_P * (nmax | 1) * sizeof(double);
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_syevr_step_many), ldsmax, &step_done) );
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_syevr_ortho_panel_many), ldsmax, &panel_done) );
   hipLaunchKernelGGL(k_syevr_values_many, dim3(np, count), dim3(SR_T), 0, st, djobs);
   hipLaunchKernelGGL(k_syevr_order_many, dim3(1, count), dim3(SR_T), 0, st, djobs);
   for (int iter = 0; iter < 3; ++iter)
   {
      hipLaunchKernelGGL(k_syevr_step_many, dim3(np, count), dim3(SR_T), lds, st, iter, djobs);
      for (int p = 0; p < np; ++p)
      {
         hipLaunchKernelGGL(k_syevr_ortho_prev_many, dim3(SR_P, count), dim3(SR_T), 0, st, p, djobs);
         hipLaunchKernelGGL(k_syevr_ortho_panel_many, dim3(1, count), dim3(SR_T), lds, st, p, djobs);
      }
   }
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

/* stage 4 of every matrix: all vectors of all matrices in one launch */
int hs_syevr_many_back(hipStream_t st, int count, int nmax, const hs_srm_job* djobs)
{
   if ( count < 1 || nmax < 2 || nmax > SR_N || djobs == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_syevr_back_many, dim3((nmax + SR_BW - 1) / SR_BW, count), dim3(SR_BW * 64), 0, st, djobs);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
