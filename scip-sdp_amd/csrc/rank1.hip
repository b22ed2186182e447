/* rank1.hip - the rank-1 constraints of the constraint handler for MANY candidate points in a fixed number of launches
 * (hipsdp_rank1_check_many; host side: cut_calls.hip).
 *
 * The reference checks a rank-1 constraint per solution (consCheckSdp, cons_sdp.c:7735-7865): isMatrixRankOne (:733-823) forms Z_b(y),
 * asks for eigenvalue n - 1 and, when that is not zero, scans all n (n - 1) / 2 principal 2 x 2 minors for the largest smaller
 * eigenvalue; with quadconsrank1, checkRank1QuadConss (:3712-3785) scans the determinants of the same minors against feastol.  Here Z of
 * all blocks and candidates comes from hs_cm_form_z (check_many.hip), the eigenvalues 1, n - 1 and n from ONE reduction per matrix
 * (eigi.hip: k_lsel_many_small / k_lsel_many_mid; syevx.hip: the column launches and hs_syevx_many_index), and two kernels stand here:
 *
 *    k_r1_minors   grid (candidates, blocks), ONE launch   both scans in one pass over the lower triangle of Z - behind hs_cm_form_z and
 *                                                          IN FRONT of the column launches of the 129 .. 512 class, which consume the
 *                                                          matrix they are given (no second copy of Z)
 *    k_r1_result   grid (candidates), the last launch      the three eigenvalues of every (candidate, block) into the result block
 * and for hipsdp_rank1_approx (the device part of the best rank-1 approximation heuristic, cons_sdp.c:7869-8185: ONE eigenpair is used)
 *    k_r1_negate   grid (tiles, blocks of 129 .. 512 rows) A = -A, R = 0 in the jobs of the batched tridiagonal path
 *    k_r1_rhs      grid (tiles, blocks), the last launch   lmax, its vector and rhsmatrix (:8058-8092) of every asked-for block
 *
 * A pair (i, k), k < i, has the position i (i - 1) / 2 + k: the reference's order, i ascending and then k ascending.  Thread t of a
 * workgroup takes the positions t, t + T, ...: consecutive lanes read consecutive words of a row of Z; the diagonal is staged in LDS.
 * REDUCTION RULE: a thread keeps its best (value, position) - it walks ascending positions and replaces on a strict >, so of equal values
 * its first stays; two results merge by value first and then by the smaller position, a total order, so the tree over the workgroup gives
 * the first pair of the largest value whatever the number of threads.  No atomic operation, no flag: every word of the result is written
 * by one thread of one launch.  The bits of (candidate, block) depend on that matrix alone.
 *
 * Smaller eigenvalue of [[a, b], [b, c]]: h - sqrt(g g + b b) with h = (a + c) / 2, g = (a - c) / 2, every operation rounded on its own
 * (absolute error: a few ulp of |a| + |b| + |c|).  Determinant: a c - b b, both products rounded, then the difference - no contraction. */
#include "hs_kernels.h"

#define R1_NOPOS 0x7fffffff

namespace {

struct r1_best { double ev; int evpos; double det; int detpos; };

__device__ __forceinline__ void r1_merge(r1_best& a, const r1_best& b)
{
   if ( b.ev > a.ev || (b.ev == a.ev && b.evpos < a.evpos) )
   {
      a.ev = b.ev;
      a.evpos = b.evpos;
   }
   a.det = fmax(a.det, b.det);
   a.detpos = b.detpos < a.detpos ? b.detpos : a.detpos;
}

/* (i, k), k < i, of position p >= 0 */
__device__ __forceinline__ void r1_pair(int p, int* i, int* k)
{
   int r = (int) ((1.0 + sqrt(1.0 + 8.0 * (double) p)) * 0.5);
   while ( (long long) r * (r - 1) / 2 > p ) --r;
   while ( (long long) (r + 1) * r / 2 <= p ) ++r;
   *i = r;
   *k = p - (int) ((long long) r * (r - 1) / 2);
}

/* the whole workgroup (blockDim.x a power of two, at most R1_NT): both scans of the n x n matrix Z (the lower triangle at [i n + k] is
 * read) - o[0] = minorev, o[1] = minordet, ind[0 .. 3] = minorind, detind */
#define R1_NT 512
__device__ __forceinline__ void r1_scan(int n, const double* __restrict__ Z, double feastol, double* __restrict__ o, int* __restrict__ ind)
{
#pragma clang fp contract(off)                              /* every product and sum below is rounded on its own: the bits are numpy's */
   __shared__ double diag[R1_NT];
   __shared__ double rev[R1_NT], rdet[R1_NT];
   __shared__ int revpos[R1_NT], rdetpos[R1_NT];
   const int tid = threadIdx.x, T = (int) blockDim.x;
   for (int i = tid; i < n; i += T)
      diag[i] = Z[(long long) i * n + i];
   __syncthreads();
   r1_best best = { 0.0, R1_NOPOS, 0.0, R1_NOPOS };
   const int npairs = n * (n - 1) / 2;                      /* (n <= 512: 130816 at most) */
   if ( tid < npairs )
   {
      int i, k;
      r1_pair(tid, &i, &k);
      for (int p = tid; p < npairs; p += T)
      {
         const double a = diag[i], c = diag[k], b = Z[(long long) i * n + k];
         const double h = 0.5 * (a + c), g = 0.5 * (a - c);
         const double gg = g * g, bb = b * b;
         const double ev = h - sqrt(gg + bb);
         if ( ev > best.ev )
         {
            best.ev = ev;
            best.evpos = p;
         }
         const double ac = a * c;
         const double minor = ac - bb;
         best.det = fmax(best.det, fabs(minor));
         if ( (minor < -feastol || minor > feastol) && p < best.detpos )
            best.detpos = p;
         k += T;
         while ( k >= i )
         {
            k -= i;
            ++i;
         }
      }
   }
   rev[tid] = best.ev; revpos[tid] = best.evpos; rdet[tid] = best.det; rdetpos[tid] = best.detpos;
   __syncthreads();
   for (int half = T >> 1; half > 0; half >>= 1)
   {
      if ( tid < half )
      {
         r1_best x = { rev[tid], revpos[tid], rdet[tid], rdetpos[tid] };
         const r1_best y = { rev[tid + half], revpos[tid + half], rdet[tid + half], rdetpos[tid + half] };
         r1_merge(x, y);
         rev[tid] = x.ev; revpos[tid] = x.evpos; rdet[tid] = x.det; rdetpos[tid] = x.detpos;
      }
      __syncthreads();
   }
   if ( tid == 0 )
   {
      o[0] = rev[0];
      o[1] = rdet[0];
      ind[0] = ind[1] = ind[2] = ind[3] = -1;
      if ( revpos[0] != R1_NOPOS )
         r1_pair(revpos[0], &ind[0], &ind[1]);
      if ( rdetpos[0] != R1_NOPOS )
         r1_pair(rdetpos[0], &ind[2], &ind[3]);
   }
}

/* matrix (block blockIdx.y, candidate blockIdx.x) of the tables of check_many.hip; its row of the result: HS_R1_RESW doubles at
 * res + (c nblk + b) HS_R1_RESW - [3] minorev, [4] minordet, [5], [6]: minorind and detind as four ints */
__global__ void __launch_bounds__(R1_NT) k_r1_minors(double feastol, const hs_ec_job* __restrict__ jobs, const hs_cm_blk* __restrict__ blks,
   double* __restrict__ res)
{
   const hs_cm_blk B = blks[blockIdx.y];
   const long long c = blockIdx.x;
   double* __restrict__ row = res + (c * gridDim.y + blockIdx.y) * HS_R1_RESW;
   r1_scan(jobs[blockIdx.y].n, B.Z + c * B.zstride, feastol, row + 3, reinterpret_cast<int*>(row + 5));
}

/* the unit form: matrix blockIdx.x of n[.] rows at Z + off[.], its results to o + 2 blockIdx.x and ind + 4 blockIdx.x */
__global__ void __launch_bounds__(R1_NT) k_r1_minors_unit(const int* __restrict__ n, const long long* __restrict__ off, const double* __restrict__ Z,
   double feastol, double* __restrict__ o, int* __restrict__ ind)
{
   r1_scan(n[blockIdx.x], Z + off[blockIdx.x], feastol, o + 2LL * blockIdx.x, ind + 4LL * blockIdx.x);
}

/* where the eigenvalues of a matrix of block b lie from blks[b].lam + c lstride on: up to 128 rows the four doubles of k_lsel_many_*
 * (value 1, half width, value n - 1, value n), above that the selection outputs of hs_syevx_many_job - lam points at out[HS_SYEVX_OUT_LAM],
 * out2 starts HS_SYEVX_OUT_VEC + even(n) doubles behind out */
__global__ void __launch_bounds__(256) k_r1_result(int nblk, const hs_ec_job* __restrict__ jobs, const hs_cm_blk* __restrict__ blks, double* __restrict__ res)
{
   const long long c = blockIdx.x;
   for (int b = threadIdx.x; b < nblk; b += 256)
   {
      const int n = jobs[b].n;
      const double* __restrict__ lam = blks[b].lam + c * blks[b].lstride;
      double* __restrict__ row = res + (c * nblk + b) * HS_R1_RESW;
      const double l1 = lam[0];
      double l2, l3;
      if ( n <= 2 )
      {
         l2 = n == 1 ? 0.0 : l1;
         l3 = n == 1 ? l1 : lam[3];
      }
      else if ( n <= HS_SC_MAXN )
      {
         l2 = lam[2];
         l3 = lam[3];
      }
      else
      {
         const long long o2 = HS_SYEVX_OUT_VEC + (((long long) n + 1) & ~1LL);
         l2 = lam[o2];
         l3 = lam[o2 + 1];
      }
      row[0] = l1; row[1] = l2; row[2] = l3;
   }
}

/* hipsdp_rank1_approx, blocks of 129 .. 512 rows: Z(y) was formed into the matrix of the block's tridiagonal job; eigenvalue 1 of -Z
 * with its vector is pair n of Z */
__global__ void __launch_bounds__(256) k_r1_negate(const hs_sxm_job* __restrict__ sx)
{
   const hs_sxm_job J = sx[blockIdx.y];
   const long long nn = (long long) J.n * J.n;
   for (long long e = (long long) blockIdx.x * 256 + threadIdx.x; e < nn; e += (long long) gridDim.x * 256)
   {
      J.A[e] = -J.A[e];
      J.R[e] = 0.0;
   }
}

/* block blockIdx.y: entry e = i (i + 1) / 2 + k of its packed right-hand side per thread; the first n threads of the block's first
 * workgroup store the vector, thread 0 the eigenvalue */
__global__ void __launch_bounds__(256) k_r1_rhs(const hs_ec_job* __restrict__ jobs, const hs_r1a_job* __restrict__ tab, double* __restrict__ res_lmax,
   double* __restrict__ res_vec, double* __restrict__ res_rhs)
{
#pragma clang fp contract(off)                              /* (lam v_i) v_k, then the sum: every operation rounded on its own */
   const hs_ec_job job = jobs[blockIdx.y];
   const hs_r1a_job T = tab[blockIdx.y];
   const int n = job.n;
   const long long nent = (long long) n * (n + 1) / 2;
   const double lam = T.sign * T.lam[0];
   if ( blockIdx.x == 0 )
   {
      for (int i = threadIdx.x; i < n; i += 256)
         res_vec[T.voff + i] = T.vec[i];
      if ( threadIdx.x == 0 )
         res_lmax[blockIdx.y] = lam;
   }
   for (long long e = (long long) blockIdx.x * 256 + threadIdx.x; e < nent; e += (long long) gridDim.x * 256)
   {
      int i = (int) ((sqrt(8.0 * (double) e + 1.0) - 1.0) * 0.5);
      while ( (long long) i * (i + 1) / 2 > e ) --i;
      while ( (long long) (i + 1) * (i + 2) / 2 <= e ) ++i;
      const int k = (int) (e - (long long) i * (i + 1) / 2);
      const double a0 = job.form == HS_EC_PACKED ? job.A[e] : job.A[(long long) i * n + k];
      const double lv = lam * T.vec[i];
      const double t = lv * T.vec[k];
      res_rhs[T.roff + e] = a0 + t;
   }
}

}

int hs_r1_negate(hipStream_t st, int count, int nmax, const hs_sxm_job* sx)
{
   if ( count < 1 || count > 65535 || nmax < 2 || nmax > R1_NT || sx == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_r1_negate, dim3((unsigned) (((long long) nmax * nmax + 255) / 256), count), dim3(256), 0, st, sx);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_r1_rhs(hipStream_t st, int count, int nmax, const hs_ec_job* jobs, const hs_r1a_job* tab, double* res_lmax, double* res_vec, double* res_rhs)
{
   if ( count < 1 || count > 65535 || nmax < 1 || nmax > R1_NT || jobs == NULL || tab == NULL || res_lmax == NULL || res_vec == NULL || res_rhs == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_r1_rhs, dim3((unsigned) (((long long) nmax * (nmax + 1) / 2 + 255) / 256), count), dim3(256), 0, st, jobs, tab, res_lmax,
      res_vec, res_rhs);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

/* threads of a workgroup of the minors launch: a power of two, by the largest matrix of the launch */
static int hs_r1_block_threads(int nmax) { return nmax <= 32 ? 64 : (nmax <= HS_SC_MAXN ? 256 : R1_NT); }

int hs_r1_minors(hipStream_t st, int nblk, int cc, int nmax, double feastol, const hs_ec_job* jobs, const hs_cm_blk* blks, double* res)
{
   if ( nblk < 1 || nblk > 65535 || cc < 1 || nmax < 1 || nmax > R1_NT || jobs == NULL || blks == NULL || res == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_r1_minors, dim3(cc, nblk), dim3(hs_r1_block_threads(nmax)), 0, st, feastol, jobs, blks, res);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_r1_minors_unit(hipStream_t st, int count, int nmax, const int* n, const long long* off, const double* Z, double feastol, double* o, int* ind)
{
   if ( count < 1 || nmax < 1 || nmax > R1_NT || n == NULL || off == NULL || Z == NULL || o == NULL || ind == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_r1_minors_unit, dim3(count), dim3(hs_r1_block_threads(nmax)), 0, st, n, off, Z, feastol, o, ind);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_r1_result(hipStream_t st, int nblk, int cc, const hs_ec_job* jobs, const hs_cm_blk* blks, double* res)
{
   if ( nblk < 1 || cc < 1 || jobs == NULL || blks == NULL || res == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_r1_result, dim3(cc), dim3(256), 0, st, nblk, jobs, blks, res);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
