/* syevx.hip - selected eigenpairs of a symmetric matrix of up to 512 rows WITHOUT a full decomposition: what DSYEVR does for
 * RANGE = 'I' (eigenpairs il .. iu) and RANGE = 'V' (those below a bound), the requests behind SCIPlapackComputeIthEigenvalue,
 * SCIPlapackComputeEigenvectorsNegative, the feasibility check and the eigenvector cuts (lapack_interface.c:178-288, 290-396).
 * Up to 128 rows one launch serves them (eigi.hip); above, the only device path was the block-Jacobi decomposition (eig.hip):
 * several O(n^3) sweeps and all n vectors to return one or five.  Here:
 *
 *   1. Householder tridiagonalisation over G workgroups, ONE LAUNCH PER COLUMN (k_syevx_col).  The matrix sits in the workspace
 *      with full symmetric storage (2 MB at 512 rows: resident in L2), row i belongs to workgroup i mod G - cyclic, so the shrinking
 *      trailing block stays balanced.  The launch of column j
 *        - applies reflector j-1's rank-2 update A <- A - v w^T - w v^T to the workgroup's own rows below row j; w = p - (tau/2)(p.v) v
 *          is recomputed by every workgroup from v_{j-1} and the p_{j-1} of the previous launch (O(n), the same bits everywhere);
 *        - forms the updated row j (= column j: the storage is symmetric to the bit) from the OLD row j and from it v_j, tau_j, d_j,
 *          e_j, again in every workgroup; workgroup 0 stores them;
 *        - computes p_j[i] = tau_j (row_i . v_j) for its rows in the same pass that updates them.
 *      A row holds all its columns, so no sum crosses workgroups: the kernel boundary is the only synchronisation (1.5-2 us
 *      for a dependent launch against 4 us and more for the cheapest grid barrier, and a boundary cannot hang).
 *      HAZARD RULE: inside one launch no workgroup reads a matrix entry another workgroup writes.  Row j is read by everybody and
 *      is therefore NOT updated in place by its owner (nobody needs it again: its content lives on as d_j, e_j and v_j in the
 *      reflector array); every other entry is read and written by its owner alone; p alternates between two buffers.
 *   2. The wanted eigenvalues by Sturm multisection on (d, e) in LDS (k_syevx_values): one workgroup, every thread counts at its own
 *      shift (ei_sturm_count), 512 / k shifts per wanted index and round, all intervals shrink together (hs_td_multisect,
 *      hs_tridiag.h).  For a bound: the count at the bound first, then the indices 1 .. min(count, maxk).
 *   3. Their eigenvectors of the tridiagonal matrix by inverse iteration (k_syevx_tvec): one workgroup, one thread per vector for
 *      the elimination (spread over the wavefronts), three rounds of { one step (hs_td_invit, hs_tridiag.h), Gram-Schmidt twice
 *      inside the clusters of eigenvalues closer than 1e-3 ||T|| }; only the RETURNED vectors are made orthonormal, so an index inside a
 *      cluster of hundreds of equal eigenvalues (low-rank matrices) costs what the k <= 32 wanted vectors cost.
 *   4. Back-transformation through the reflectors (k_syevx_back): one wavefront per vector, the reflectors read four ahead.
 * Every reduction runs in a fixed order (no floating-point atomics): the same input gives the same bits.
 * Each stage is a __device__ body (d_syevx_col, d_syevx_values, d_syevx_tvec, d_syevx_back) with two kernels around it: the one of a
 * single matrix and the one of MANY matrices per launch (k_syevx_*_many, hs_syevx_many_*: the rounds of hipsdp_onevar_bounds_large;
 * k_syevx_*_below_many, hs_syevx_many_below: several pairs per matrix, hipsdp_eigencuts_all_large). */
#include "hs_common.h"
#include "hs_kernels.h"
#include "hs_tridiag.h"
#include <cmath>

#define SX_N   HS_SYEVX_MAXN
#define SX_K   HS_SYEVX_MAXK
#define SX_CT  256                  /* threads of a column launch: four wavefronts, one row each at a time */
#define SX_VT  512                  /* threads of the eigenvalue and the eigenvector kernel */

namespace {

/* a b + c d with both products rounded: symmetric under (a, b) <-> (d, c), so the update keeps A[i][c] == A[c][i] to the bit */
__device__ __forceinline__ double sx_sym2(double a, double b, double c, double d)
{
#pragma clang fp contract(off)
   const double p = a * b;
   const double q = c * d;
   return p + q;
}

/* the workspace: matrix, reflectors (row j = v_j, entries 0 .. j zero, entry j + 1 one), the two p buffers, tau, d, e, the
 * eigenvectors of T (k x n) and the three factor arrays of the elimination ([row][vector]) */
struct sx_ws
{
   double* A; double* R; double* P; double* tau; double* d; double* e; double* Zt; double* G0; double* G1; double* G2;
};

__host__ __device__ inline sx_ws sx_layout(int n, double* ws)
{
   const size_t n2 = ((size_t) n * n + 1) & ~(size_t) 1, nl = ((size_t) n + 1) & ~(size_t) 1;
   sx_ws w;
   w.A = ws; w.R = w.A + n2; w.P = w.R + n2; w.tau = w.P + 2 * nl; w.d = w.tau + nl; w.e = w.d + nl;
   w.Zt = w.e + nl; w.G0 = w.Zt + (size_t) SX_K * nl; w.G1 = w.G0 + (size_t) SX_K * nl; w.G2 = w.G1 + (size_t) SX_K * nl;
   return w;
}

size_t sx_ws_doubles(int n)
{
   const size_t n2 = ((size_t) n * n + 1) & ~(size_t) 1, nl = ((size_t) n + 1) & ~(size_t) 1;
   return 2 * n2 + 5 * nl + 4 * (size_t) SX_K * nl;
}

/* Workgroups of the column launches: four rows per workgroup - each of its four wavefronts takes ONE row per launch (at 512 rows:
 * eight loads per lane, one pass) -, at most 128: half the compute units, every workgroup resident at once, and the redundant O(n)
 * part of a launch (w, the reflector) stays a small share of what the dispatcher starts. */
__host__ __device__ inline int sx_groups(int n) { const int g = (n + 3) / 4; return g < 128 ? g : 128; }

/* the symmetric matrix from the triangle the callers fill (memory positions [j n + i], i >= j), reflector array cleared */
__global__ void __launch_bounds__(256) k_syevx_init(int n, const double* __restrict__ in, double* __restrict__ A, double* __restrict__ R)
{
   for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < n * n; idx += gridDim.x * blockDim.x)
   {
      const int i = idx / n, c = idx - i * n;
      A[idx] = (c <= i) ? in[(size_t) c * n + i] : in[(size_t) i * n + c];
      R[idx] = 0.0;
   }
}

/* column j of the reduction, 0 <= j <= n - 2 (see the head of the file); workgroup g of the G of the matrix owns the rows g, g + G,
 * g + 2 G, ...  The body of k_syevx_col and of k_syevx_col_many (one matrix per blockIdx.y): the same arithmetic for both, and no sum
 * crosses workgroups, so the bits do not depend on G */
__device__ __forceinline__ void d_syevx_col(int n, int j, int G, int g, double* __restrict__ A, double* __restrict__ R, double* __restrict__ P,
   double* __restrict__ tau, double* __restrict__ d, double* __restrict__ e)
{
   __shared__ double vp[SX_N], wp[SX_N], xs[SX_N], red[2][SX_CT / 64];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const double* __restrict__ pprev = P + (size_t) ((j + 1) & 1) * n;
   double* __restrict__ pcur = P + (size_t) (j & 1) * n;
   const double tprev = (j > 0) ? tau[j - 1] : 0.0;

   /* ---- w of reflector j - 1 and the updated row j, columns j .. n - 1 (the same in every workgroup) */
   if ( tprev != 0.0 )
   {
      double part = 0.0;
      for (int c = j + tid; c < n; c += SX_CT)
      {
         const double v = R[(size_t) (j - 1) * n + c], p = pprev[c];
         vp[c] = v;
         wp[c] = p;
         part = fma(p, v, part);
      }
      const double al = -0.5 * tprev * hs_block_sum<SX_CT / 64>(part, red[0]);
      for (int c = j + tid; c < n; c += SX_CT)
         wp[c] = fma(al, vp[c], wp[c]);                   /* (each thread its own entries) */
      __syncthreads();
      const double vj = vp[j], wj = wp[j];
      for (int c = j + tid; c < n; c += SX_CT)
         xs[c] = A[(size_t) j * n + c] - sx_sym2(vj, wp[c], vp[c], wj);
   }
   else
   {
      for (int c = j + tid; c < n; c += SX_CT)
         xs[c] = A[(size_t) j * n + c];
   }
   __syncthreads();

   /* ---- reflector j from x = xs[j + 1 .. n - 1] (DLARFG: v_0 = 1, H x = beta e_0), into xs */
   double s2p = 0.0;
   for (int c = j + 2 + tid; c < n; c += SX_CT)
      s2p = fma(xs[c], xs[c], s2p);
   const double s2 = hs_block_sum<SX_CT / 64>(s2p, red[1]);
   const double x0 = xs[j + 1], dj = xs[j];
   double beta = x0, t = 0.0, scale = 0.0;
   if ( s2 > 0.0 )
   {
      beta = -copysign(sqrt(x0 * x0 + s2), x0);
      t = (beta - x0) / beta;
      scale = 1.0 / (x0 - beta);
   }
   __syncthreads();                                        /* (everybody has read xs[j], xs[j + 1]) */
   for (int c = j + 1 + tid; c < n; c += SX_CT)
   {
      const double v = (c == j + 1) ? 1.0 : xs[c] * scale;
      xs[c] = v;
      if ( g == 0 && t != 0.0 )
         R[(size_t) j * n + c] = v;
   }
   if ( g == 0 && tid == 0 )
   {
      tau[j] = t;
      d[j] = dj;
      e[j] = beta;
      if ( j == n - 2 )
         e[n - 1] = 0.0;
   }
   __syncthreads();

   /* ---- own rows below row j: the pending update and p_j in one pass, one wavefront per row (n <= 512: eight entries per lane) */
   if ( tprev == 0.0 && t == 0.0 && j != n - 2 )
      return;
   const int k0 = (j + 1 > g) ? (j + 1 - g + G - 1) / G : 0;
   for (int i = g + (k0 + wave) * G; i < n; i += (SX_CT / 64) * G)
   {
      double* __restrict__ row = A + (size_t) i * n;
      double a[SX_N / 64];
#pragma unroll
      for (int m = 0; m < SX_N / 64; ++m)
      {
         const int c = j + 1 + lane + 64 * m;
         a[m] = (c < n) ? row[c] : 0.0;
      }
      double acc = 0.0;
      if ( tprev != 0.0 )
      {
         const double vi = vp[i], wi = wp[i];
#pragma unroll
         for (int m = 0; m < SX_N / 64; ++m)
         {
            const int c = j + 1 + lane + 64 * m;
            if ( c < n )
            {
               a[m] -= sx_sym2(vi, wp[c], vp[c], wi);
               row[c] = a[m];
            }
         }
      }
      if ( t != 0.0 )
      {
#pragma unroll
         for (int m = 0; m < SX_N / 64; ++m)
         {
            const int c = j + 1 + lane + 64 * m;
            if ( c < n )
               acc = fma(a[m], xs[c], acc);
         }
         acc = hs_xsum<64>(acc);
         if ( lane == 0 )
            pcur[i] = t * acc;
      }
      if ( j == n - 2 && lane == 0 )                        /* (i = n - 1, c = n - 1: the last diagonal entry) */
         d[n - 1] = a[0];
   }
}

__global__ void __launch_bounds__(SX_CT) k_syevx_col(int n, int j, double* __restrict__ A, double* __restrict__ R, double* __restrict__ P,
   double* __restrict__ tau, double* __restrict__ d, double* __restrict__ e)
{
   d_syevx_col(n, j, (int) gridDim.x, (int) blockIdx.x, A, R, P, tau, d, e);
}

/* ---- stage 2: the wanted eigenvalues.  out[0] = how many pairs are returned, out[1] = eigenvalues below the bound (-1 for an index
 * range), out[2] = Gershgorin span, out[3] = norm bound of T, out[HS_SYEVX_OUT_LAM + k] = k-th returned eigenvalue */
__device__ __forceinline__ void d_syevx_values(int n, int below, int il, int iu, double bound, int maxk, const double* __restrict__ d,
   const double* __restrict__ e, double* __restrict__ out)
{
   __shared__ double ds[SX_N + 8], es[SX_N + 8], red[3][SX_VT / 64];
   __shared__ int cntb[2][SX_K], sh_cnt, sh_nbelow;
   const int tid = threadIdx.x;
   double lo = 1e300, hi = -1e300, tn = 0.0;
   if ( tid < n )
   {
      const double rad = (tid > 0 ? fabs(e[tid - 1]) : 0.0) + (tid + 1 < n ? fabs(e[tid]) : 0.0);
      lo = d[tid] - rad;
      hi = d[tid] + rad;
      tn = fabs(d[tid]) + rad;
   }
   if ( tid < 2 * SX_K )
      cntb[tid / SX_K][tid % SX_K] = 0;
   const hs_td_gersh g = hs_td_bounds<SX_VT>(lo, hi, tn, red);
   const double glo = g.lo, ghi = g.hi, span0 = g.span0, tnorm = g.tnorm, sinv = 1.0 / tnorm;
   /* the matrix scaled to norm <= 1 for the counts in product form */
   if ( tid < n )
   {
      ds[tid] = d[tid] * sinv;
      es[tid] = (tid + 1 < n) ? (e[tid] * sinv) * (e[tid] * sinv) : 0.0;
   }
   hs_td_pad(ds, es, n, tid);
   __syncthreads();
   const int nb = (n - 1 + 3) >> 2;
   if ( tid == 0 )
   {
      int cnt = iu - il + 1, nbel = -1;
      if ( below )
      {
         nbel = (bound >= ghi) ? n : ((bound < glo) ? 0 : ei_sturm_count(ds, es, nb, bound * sinv));
         cnt = min(nbel, maxk);
      }
      sh_cnt = cnt;
      sh_nbelow = nbel;
   }
   __syncthreads();
   const int cnt = sh_cnt;
   const int k0 = below ? 1 : il;                          /* index (1-based) of the first wanted eigenvalue */
   if ( tid == 0 )
   {
      out[0] = (double) cnt;
      out[1] = (double) sh_nbelow;
      out[2] = span0;
      out[3] = tnorm;
   }
   if ( cnt <= 0 )
      return;
   /* thread = (wanted index kk, one of S shifts), S = 512 / (power of two >= cnt): 16 shifts per index for 32 of them (4.1 bits
    * per round), all 512 for one (9 bits) */
   int lgK = 0;
   while ( (1 << lgK) < cnt )
      ++lgK;
   const int lgS = 9 - lgK, S = 1 << lgS;
   const int kk = tid >> lgS, sh = tid & (S - 1);
   const bool act = kk < cnt;
   const int ith = k0 + kk;
   const hs_td_interval iv = hs_td_multisect(S, kk, sh, act, ith, n, glo * sinv, ghi * sinv, cntb,
      [=](double x) { return ei_sturm_count(ds, es, nb, x); });
   /* every index is searched in an interval of its own: the midpoints of a multiple eigenvalue may differ in the last place, in either
    * order.  Ascending as promised: the running maximum (changes nothing where the values ascend already; ds is free by now) */
   __syncthreads();
   if ( act && sh == 0 )
      ds[kk] = 0.5 * (iv.lo + iv.hi) * tnorm;
   __syncthreads();
   if ( tid < cnt )
   {
      double lmax = ds[tid];
      for (int j = 0; j < tid; ++j)
         lmax = fmax(lmax, ds[j]);
      out[HS_SYEVX_OUT_LAM + tid] = lmax;
   }
}

__global__ void __launch_bounds__(SX_VT) k_syevx_values(int n, int below, int il, int iu, double bound, int maxk, const double* __restrict__ d,
   const double* __restrict__ e, double* __restrict__ out)
{
   d_syevx_values(n, below, il, iu, bound, maxk, d, e, out);
}

/* ---- stage 3: eigenvectors of T for the returned eigenvalues, Zt[k][i].  Dynamic LDS: Z[SX_K][n | 1] (the batched launch asks for one
 * vector per matrix: Z[1][nmax | 1]). */
__device__ __forceinline__ void d_syevx_tvec(int n, const double* __restrict__ dg, const double* __restrict__ eg, const double* __restrict__ out,
   double* __restrict__ Zt, double* __restrict__ G0, double* __restrict__ G1, double* __restrict__ G2, double* Z)
{
   __shared__ double d[SX_N], e[SX_N], th[SX_K], coef[SX_K], red[2][SX_VT / 64];
   __shared__ int cstart[SX_K];
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   const int ld = n | 1;
   const int cnt = (int) out[0];
   if ( cnt <= 0 )
      return;
   const double span0 = out[2], tnorm = out[3];
   const double ortol = 1e-3 * tnorm;                      /* DSTEIN's criterion, as in k_syev_mid */
   if ( tid < n )
   {
      d[tid] = dg[tid];
      e[tid] = eg[tid];
   }
   if ( tid < cnt )
      th[tid] = out[HS_SYEVX_OUT_LAM + tid];
   __syncthreads();
   if ( tid == 0 )
   {
      /* clusters among the RETURNED eigenvalues: cstart[k] = first vector of the cluster of vector k */
      cstart[0] = 0;
      for (int k = 1; k < cnt; ++k)
         cstart[k] = (th[k] - th[k - 1] <= ortol) ? cstart[k - 1] : k;
   }
   /* start vectors that differ from vector to vector: a multiple eigenvalue gets a basis of its space out of them */
   for (int idx = tid; idx < cnt * n; idx += SX_VT)
   {
      const int k = idx / n, i = idx - k * n;
      Z[k * ld + i] = hs_td_start(i, k);
   }
   __syncthreads();

   for (int iter = 0; iter < 3; ++iter)
   {
      /* one step of inverse iteration per vector (hs_td_invit): thread (wavefront k mod 8, lane k / 8) owns vector k - the 32 serial
       * chains spread over the wavefronts; factors in device memory as [row][vector] */
      if ( lane < SX_K / 8 && (lane << 3 | wave) < cnt )
      {
         const int k = lane << 3 | wave;
         hs_td_invit<SX_K, false>(Z + k * ld, d, e, 0, n, th[k], span0, G0, G1, G2, k, k);
      }
      __syncthreads();

      /* classical Gram-Schmidt, twice, against the earlier vectors of the same cluster: the coefficients one wavefront per earlier
       * vector, the correction one thread per component with the earlier vectors in a fixed order */
      for (int k = 1; k < cnt; ++k)
      {
         const int c0 = cstart[k];
         if ( c0 == k )
            continue;                                      /* (the same in every thread) */
         for (int pass = 0; pass < 2; ++pass)
         {
            for (int p = c0 + wave; p < k; p += SX_VT / 64)
            {
               double acc = 0.0;
               for (int i = lane; i < n; i += 64)
                  acc = fma(Z[p * ld + i], Z[k * ld + i], acc);
               acc = hs_xsum<64>(acc);
               if ( lane == 0 )
                  coef[p] = acc;
            }
            __syncthreads();
            if ( tid < n )
            {
               double v = Z[k * ld + tid];
               for (int p = c0; p < k; ++p)
                  v = fma(-coef[p], Z[p * ld + tid], v);
               Z[k * ld + tid] = v;
            }
            __syncthreads();
         }
         const double v = (tid < n) ? Z[k * ld + tid] : 0.0;
         const double nr = hs_block_sum<SX_VT / 64>(v * v, red[k & 1]);
         if ( tid < n )
            Z[k * ld + tid] = v / sqrt(fmax(nr, 1e-300));
         __syncthreads();
      }
   }
   for (int idx = tid; idx < cnt * n; idx += SX_VT)
   {
      const int k = idx / n, i = idx - k * n;
      Zt[(size_t) k * n + i] = Z[k * ld + i];
   }
}

__global__ void __launch_bounds__(SX_VT) k_syevx_tvec(int n, const double* __restrict__ dg, const double* __restrict__ eg, const double* __restrict__ out,
   double* __restrict__ Zt, double* __restrict__ G0, double* __restrict__ G1, double* __restrict__ G2)
{
   extern __shared__ __attribute__((aligned(16))) double Z[];
   d_syevx_tvec(n, dg, eg, out, Zt, G0, G1, G2, Z);
}

/* ---- stage 4: x = H_0 H_1 ... H_{n-3} z, one wavefront per vector: lane l holds the entries l + 64 m; a reflector is a dot product
 * and an axpy over the wavefront, and the reflectors are read four ahead of their use (they do not depend on z).
 * k 2 n^2 multiply-adds bound by the latency of the reduction: nothing for the matrix cores at k <= 32. */
__device__ __forceinline__ void d_syevx_back(int n, int k, const double* __restrict__ R, const double* __restrict__ tau, const double* __restrict__ Zt,
   double* __restrict__ out)
{
   __shared__ double ts[SX_N];
   const int lane = threadIdx.x;
   if ( k >= (int) out[0] )
      return;
   for (int i = lane; i < n; i += 64)
      ts[i] = tau[i];
   double z[SX_N / 64];
#pragma unroll
   for (int m = 0; m < SX_N / 64; ++m)
      z[m] = (lane + 64 * m < n) ? Zt[(size_t) k * n + lane + 64 * m] : 0.0;
   __syncthreads();
   double vb[4][SX_N / 64];
#pragma unroll
   for (int u = 0; u < 4; ++u)
   {
      const int j = n - 3 - u;
#pragma unroll
      for (int m = 0; m < SX_N / 64; ++m)
         vb[u][m] = (j >= 0 && lane + 64 * m < n) ? R[(size_t) j * n + lane + 64 * m] : 0.0;
   }
   for (int jj = n - 3; jj >= 0; jj -= 4)
   {
#pragma unroll
      for (int u = 0; u < 4; ++u)
      {
         const int j = jj - u;
         if ( j >= 0 )
         {
            const double t = ts[j];
            double dot = 0.0;
#pragma unroll
            for (int m = 0; m < SX_N / 64; ++m)
               dot = fma(vb[u][m], z[m], dot);
            dot = t * hs_xsum<64>(dot);
#pragma unroll
            for (int m = 0; m < SX_N / 64; ++m)
               z[m] = fma(-dot, vb[u][m], z[m]);
            const int jn = j - 4;
#pragma unroll
            for (int m = 0; m < SX_N / 64; ++m)
               vb[u][m] = (jn >= 0 && lane + 64 * m < n) ? R[(size_t) jn * n + lane + 64 * m] : 0.0;
         }
      }
   }
   hs_td_store_unit(z, n, lane, out + HS_SYEVX_OUT_VEC + (size_t) k * n);
}

__global__ void __launch_bounds__(64) k_syevx_back(int n, const double* __restrict__ R, const double* __restrict__ tau, const double* __restrict__ Zt,
   double* __restrict__ out)
{
   d_syevx_back(n, (int) blockIdx.x, R, tau, Zt, out);
}

/* ---- the same four stages for MANY matrices per launch (hs_syevx_many_*; caller: hipsdp_onevar_bounds_large, onevar_large.hip): matrix
 * blockIdx.y of the table, its workspace and its n from its hs_sxm_job, act[job] == 0: the matrix takes no part in this round.  Both
 * conditions at the top of a kernel are uniform per workgroup.  A matrix gets min(sx_groups(n), gridDim.x) workgroups of a column
 * launch.  Selection: eigenvalue 1, with HS_SXM_BOTH also eigenvalue n (to out2), with HS_SXM_VEC the vector of eigenvalue 1. */
__global__ void __launch_bounds__(SX_CT) k_syevx_col_many(int j, const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act)
{
   const int job = blockIdx.y;
   const int n = jobs[job].n;
   if ( act[job] == 0 || j > n - 2 )
      return;
   const int G = min(sx_groups(n), (int) gridDim.x);
   if ( (int) blockIdx.x >= G )
      return;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   d_syevx_col(n, j, G, (int) blockIdx.x, w.A, w.R, w.P, w.tau, w.d, w.e);
}

__global__ void __launch_bounds__(SX_VT) k_syevx_values_many(const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act)
{
   const int job = blockIdx.x, which = blockIdx.y;
   const int a = act[job];
   if ( a == 0 || (which == 1 && !(a & HS_SXM_BOTH)) )
      return;
   const int n = jobs[job].n;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   const int ith = which == 0 ? 1 : n;
   d_syevx_values(n, 0, ith, ith, 0.0, 0, w.d, w.e, which == 0 ? jobs[job].out : jobs[job].out2);
}

__global__ void __launch_bounds__(SX_VT) k_syevx_tvec_many(const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act)
{
   extern __shared__ __attribute__((aligned(16))) double Z[];
   const int job = blockIdx.x;
   if ( !(act[job] & HS_SXM_VEC) )
      return;
   const int n = jobs[job].n;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   d_syevx_tvec(n, w.d, w.e, jobs[job].out, w.Zt, w.G0, w.G1, w.G2, Z);
}

__global__ void __launch_bounds__(64) k_syevx_back_many(const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act)
{
   const int job = blockIdx.x;
   if ( !(act[job] & HS_SXM_VEC) )
      return;
   const int n = jobs[job].n;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   d_syevx_back(n, 0, w.R, w.tau, w.Zt, jobs[job].out);
}

/* ---- the BELOW selection for many matrices per launch (k_syevx_*_below_many; host side: hs_syevx_many_below further down): wrappers of
 * the same kind around the bodies of stages 2 to 4, kept in a file of their own */
#include "hs_syevx_below_many.h"
/* ---- the several-indices values launch for many matrices (k_syevx_values_index_many; host side: hs_syevx_many_index further down): a
 * wrapper of the same kind around the body of stage 2 */
#include "hs_syevx_index_many.h"

}

size_t hs_syevx_ws(int n) { return (n < 2 || n > SX_N) ? 0 : sx_ws_doubles(n); }

/* ---- many matrices per launch.  hs_syevx_many_job: the table entry of a matrix of n rows with its workspace (hs_syevx_ws(n) doubles)
 * and its selection output (HS_SXM_OUT(n) doubles); A and R are where the caller's own kernel writes the symmetric matrix (n x n, no
 * pitch) and clears the reflector array before hs_syevx_many_cols - in place of k_syevx_init. */
int hs_syevx_many_job(int n, double* ws, double* out, hs_sxm_job* J)
{
   if ( n < 2 || n > SX_N || ws == NULL || out == NULL || J == NULL )
      return HS_ERR_ARG;
   const sx_ws w = sx_layout(n, ws);
   J->n = n; J->pad = 0; J->ws = ws; J->A = w.A; J->R = w.R;
   J->out = out; J->out2 = out + HS_SYEVX_OUT_VEC + (((size_t) n + 1) & ~(size_t) 1);
   return HS_OK;
}

/* nmax - 1 launches: column j of every matrix with act != 0 and n - 2 >= j; cap: workgroups per matrix at most (1 .. 128) */
int hs_syevx_many_cols(hipStream_t st, int count, int nmax, int cap, const hs_sxm_job* djobs, const int* dact)
{
   if ( count < 1 || nmax < 2 || nmax > SX_N || cap < 1 || djobs == NULL || dact == NULL )
      return HS_ERR_ARG;
   const int G = sx_groups(nmax) < cap ? sx_groups(nmax) : cap;
   for (int j = 0; j + 1 < nmax; ++j)
      hipLaunchKernelGGL(k_syevx_col_many, dim3(G, count), dim3(SX_CT), 0, st, j, djobs, dact);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

/* the `cap` of a call that names none: about four workgroups per compute unit over all `count` matrices, at least 8 (a matrix of 512
 * rows then has 16 rows per wavefront and launch), at most the 128 of a matrix alone */
int hs_syevx_many_cap(int count)
{
   const int cus = hs_device_cus();
   const int g = (4 * (cus > 0 ? cus : 256)) / count;
   return g < 8 ? 8 : (g > 128 ? 128 : g);
}

/* three launches, whatever the flags say: the values (both: a second row of workgroups for eigenvalue n), the vector of T, its
 * back-transformation */
int hs_syevx_many_select(hipStream_t st, int count, int nmax, int both, const hs_sxm_job* djobs, const int* dact)
{
   if ( count < 1 || nmax < 2 || nmax > SX_N || djobs == NULL || dact == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_syevx_values_many, dim3(count, both ? 2 : 1), dim3(SX_VT), 0, st, djobs, dact);
   hipLaunchKernelGGL(k_syevx_tvec_many, dim3(count), dim3(SX_VT), (size_t) (nmax | 1) * sizeof(double), st, djobs, dact);
   hipLaunchKernelGGL(k_syevx_back_many, dim3(count), dim3(64), 0, st, djobs, dact);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

/* ONE launch, values only: eigenvalue 1 of every matrix with act != 0 to out[HS_SYEVX_OUT_LAM], eigenvalues n - 1 and n to
 * out2[HS_SYEVX_OUT_LAM], out2[HS_SYEVX_OUT_LAM + 1] */
int hs_syevx_many_index(hipStream_t st, int count, int nmax, const hs_sxm_job* djobs, const int* dact)
{
   if ( count < 1 || nmax < 2 || nmax > SX_N || djobs == NULL || dact == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_syevx_values_index_many, dim3(count, 2), dim3(SX_VT), 0, st, djobs, dact);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

/* the entry of a matrix for hs_syevx_many_below: as hs_syevx_many_job, with out = HS_SXB_OUT(n) doubles - the selection in the layout
 * HS_SYEVX_OUT(n), and behind it the HS_SYEVX_OUT_VEC doubles of eigenvalue 1 (out2) */
int hs_syevx_many_below_job(int n, double* ws, double* out, hs_sxm_job* J)
{
   HS_CALL( hs_syevx_many_job(n, ws, out, J) );
   J->out2 = out + HS_SYEVX_OUT(n);
   return HS_OK;
}

/* one launch for the values (a second row of workgroups for the eigenvalues below the bound when maxk > 0) and, with maxk > 0, two more:
 * the vectors of T and their back-transformation - whatever the counts turn out to be */
int hs_syevx_many_below(hipStream_t st, int count, int nmax, double bound, int maxk, const hs_sxm_job* djobs, const int* dact)
{
   if ( count < 1 || nmax < 2 || nmax > SX_N || maxk < 0 || maxk > SX_K || djobs == NULL || dact == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_syevx_values_below_many, dim3(count, maxk > 0 ? 2 : 1), dim3(SX_VT), 0, st, djobs, dact, bound, maxk);
   if ( maxk > 0 )
   {
      static hs_attr_mask attr_done;
      HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_syevx_tvec_below_many), SX_K * (SX_N + 1) * (int) sizeof(double), &attr_done) );
      hipLaunchKernelGGL(k_syevx_tvec_below_many, dim3(count), dim3(SX_VT), (size_t) maxk * (nmax | 1) * sizeof(double), st, djobs, dact);
      hipLaunchKernelGGL(k_syevx_back_below_many, dim3(count, maxk), dim3(64), 0, st, djobs, dact);
   }
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

/* stage 1 alone: d, e, tau and the reflector array in the workspace (hs_syevx_tridiag_view) */
int hs_syevx_tridiag_dev(hipStream_t st, int n, const double* dA, double* ws)
{
   if ( n < 2 || n > SX_N || dA == NULL || ws == NULL )
      return HS_ERR_ARG;
   const sx_ws w = sx_layout(n, ws);
   hipLaunchKernelGGL(k_syevx_init, dim3((n * n + 255) / 256 < 256 ? (n * n + 255) / 256 : 256), dim3(256), 0, st, n, dA, w.A, w.R);
   const int G = sx_groups(n);
   for (int j = 0; j + 1 < n; ++j)
      hipLaunchKernelGGL(k_syevx_col, dim3(G), dim3(SX_CT), 0, st, n, j, w.A, w.R, w.P, w.tau, w.d, w.e);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

void hs_syevx_tridiag_view(int n, double* ws, double** d, double** e, double** R, double** tau)
{
   const sx_ws w = sx_layout(n, ws);
   *d = w.d; *e = w.e; *R = w.R; *tau = w.tau;
}

/* stages 2 to 4 alone on the tridiagonal form that lies in ws (hs_syevx_tridiag_dev): one launch for the values, two more for the
 * vectors.  May be called several times on one form, each time with a dOut of its own. */
int hs_syevx_select_dev(hipStream_t st, int n, int mode, int il, int iu, double bound, int maxk, double* dOut, double* ws)
{
   const int below = (mode & HS_SYEVX_BELOW) ? 1 : 0;
   if ( n < 2 || n > SX_N || dOut == NULL || ws == NULL )
      return HS_ERR_ARG;
   if ( below ? (maxk < 0 || maxk > SX_K) : (il < 1 || iu > n || il > iu || iu - il + 1 > SX_K) )
      return HS_ERR_ARG;
   const sx_ws w = sx_layout(n, ws);
   hipLaunchKernelGGL(k_syevx_values, dim3(1), dim3(SX_VT), 0, st, n, below, il, iu, bound, maxk, w.d, w.e, dOut);
   const int kmax = below ? maxk : iu - il + 1;
   if ( !(mode & HS_SYEVX_NOVEC) && kmax > 0 )
   {
      static hs_attr_mask attr_done;
      HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_syevx_tvec), SX_K * (SX_N + 1) * (int) sizeof(double), &attr_done) );
      hipLaunchKernelGGL(k_syevx_tvec, dim3(1), dim3(SX_VT), (size_t) SX_K * (n | 1) * sizeof(double), st, n, w.d, w.e, dOut, w.Zt, w.G0, w.G1, w.G2);
      hipLaunchKernelGGL(k_syevx_back, dim3(kmax), dim3(64), 0, st, n, w.R, w.tau, w.Zt, dOut);
   }
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_syevx_dev(hipStream_t st, int n, const double* dA, int mode, int il, int iu, double bound, int maxk, double* dOut, double* ws)
{
   const int below = (mode & HS_SYEVX_BELOW) ? 1 : 0;
   if ( n < 2 || n > SX_N || dA == NULL || dOut == NULL || ws == NULL )
      return HS_ERR_ARG;
   if ( below ? (maxk < 0 || maxk > SX_K) : (il < 1 || iu > n || il > iu || iu - il + 1 > SX_K) )
      return HS_ERR_ARG;
   HS_CALL( hs_syevx_tridiag_dev(st, n, dA, ws) );
   return hs_syevx_select_dev(st, n, mode, il, iu, bound, maxk, dOut, ws);
}
