/* kernels.hip - the bandwidth-bound pieces of the interior-point iteration: the two passes over the packed constraint
 * matrices A (row i = vec(A_i), the "svec-free" full storage used by the MFMA Schur assembly),
 *
 *    A(X)_i   = <A_i, X>                 hs_gemv_n   (one coalesced pass, up to four X at once)
 *    A^T(y)   = sum_i y_i A_i            hs_gemv_t   (one coalesced pass)
 *
 * plus reductions and element-wise updates.  These replace work that the reference leaves to DSDP/SDPA
 * (sdpisolver_dsdp.c:1503, sdpisolver_sdpa.cpp:1620).  All are HBM-bound: 8 bytes of A per 2 flops.
 * Reductions are two-stage with a fixed combination order, so results are bitwise reproducible run to run.
 */
#include "hs_kernels.h"
#include <string.h>
#include <stdio.h>
#include <stdlib.h>

/* recorders of the deferred batch (defined with it below): 1 = recorded; 0 = not recorded, pending records have been launched, the
 * caller launches its kernel */
static int hs_rec_dir_block_small(hipStream_t s, int n, double c, const double* X, const double* R, const double* E, const double* Zinv,
   double s1, double* out);
static int hs_rec_lp_dir(hipStream_t s, int q, double sigmu, double eta, const double* x, const double* z, const double* r, const double* elp,
   double* out);
static int hs_rec_vec_mul(hipStream_t s, long long n, const double* a, const double* b, double* out);
static int hs_rec_axpy3(hipStream_t s, double a, long long n1, const double* x1, double* y1, long long n2, const double* x2, double* y2,
   long long n3, const double* x3, double* y3);
static int hs_rec_gemv_t(hipStream_t s, int R, long long E, const double* A, long long lda, const double* coef, double sa, const double* add,
   double* out);

struct __attribute__((aligned(16))) dbl2 { double x, y; };
/* 16 bytes of a row that is read once per sweep (the constraint matrices): the load does not allocate in the caches, so that what the
 * sweep runs beside - the factorization of M on the other queue, the vectors of the sweep itself - stays in L2 */
__device__ __forceinline__ dbl2 load_stream2(const double* p)
{
   typedef double gv2 __attribute__((ext_vector_type(2)));
   const gv2 t = __builtin_nontemporal_load(reinterpret_cast<const gv2*>(p));
   dbl2 r; r.x = t.x; r.y = t.y;
   return r;
}

static inline int hs_launch_ok(void)
{
   return hipGetLastError() == hipSuccess ? HS_OK : HS_ERR_HIP;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* element-wise                                                                                                       */
/* ---------------------------------------------------------------------------------------------------------------- */

__global__ void k_fill(double* p, long long n, double v)
{
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
      p[i] = v;
}

__global__ void k_identity(double* A, int n, double v)
{
   const long long total = (long long) n * n;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / n);
      const int c = (int) (i - (long long) r * n);
      A[i] = (r == c) ? v : 0.0;
   }
}

__global__ void k_scale_add(long long n, double a, const double* __restrict__ x, double b, const double* __restrict__ y,
   double* __restrict__ out)
{
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
   {
      double v = a * x[i];
      if ( y != NULL )
         v += b * y[i];
      out[i] = v;
   }
}

__global__ void k_mirror_lower(double* A, int n, long long lda)
{
   const long long total = (long long) n * n;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / n);
      const int c = (int) (i - (long long) r * n);
      if ( r < c )
         A[(long long) r * lda + c] = A[(long long) c * lda + r];
   }
}

__global__ void k_mirror_upper(double* A, int n, long long lda)
{
   const long long total = (long long) n * n;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / n);
      const int c = (int) (i - (long long) r * n);
      if ( r > c )
         A[(long long) r * lda + c] = A[(long long) c * lda + r];
   }
}

/* packed lower storage: entry (r, c), r >= c, at t = r (r + 1) / 2 + c; rows padded to an even length Lp */
__global__ void k_pack_rows(int m1, int n, long long Lp, const double* __restrict__ A, double* __restrict__ Apk)
{
   const long long n2 = (long long) n * n;
   const long long total = (long long) m1 * n2;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const long long i = e / n2;
      const long long rc = e - i * n2;
      const int r = (int) (rc / n), c = (int) (rc - (long long) r * n);
      if ( c <= r )
         Apk[i * Lp + (long long) r * (r + 1) / 2 + c] = A[e];
   }
}

/* D[i][r] = A_i[r][r] out of the packed rows (entry (r, r) at t = r (r + 3) / 2); rows of D have ldd >= n entries, those behind n are
 * set to zero */
__global__ void k_packed_diag(int m1, int n, int ldd, long long Lp, const double* __restrict__ Apk, double* __restrict__ D)
{
   const long long total = (long long) m1 * ldd;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const long long i = e / ldd;
      const int r = (int) (e - i * ldd);
      D[e] = r < n ? Apk[i * Lp + (long long) r * (r + 3) / 2] : 0.0;
   }
}

/* C[r][c] -= S[r][c] on the lower triangle (c <= r) of two n x n matrices */
__global__ void k_sub_lower(int n, const double* __restrict__ S, double* __restrict__ C)
{
   const long long total = (long long) n * n;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (e / n), c = (int) (e - (long long) r * n);
      if ( c <= r )
         C[e] -= S[e];
   }
}

/* pk[t] = w * V[r][c] with w = 1 on the diagonal, 2 off it: <A_i, V> = sum_t Apk[i][t] pk[t] for symmetric V */
__global__ void k_pack_weighted(int n, const double* __restrict__ V, double* __restrict__ pk)
{
   const long long total = (long long) n * n;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (e / n), c = (int) (e - (long long) (e / n) * n);
      if ( c <= r )
         pk[(long long) r * (r + 1) / 2 + c] = (r == c ? 1.0 : 2.0) * V[e];
   }
}

/* out[r][c] = pk[t(max(r,c), min(r,c))] + sa * add[r][c] */
__global__ void k_unpack_sym(int n, const double* __restrict__ pk, double sa, const double* __restrict__ add, double* __restrict__ out)
{
   const long long total = (long long) n * n;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const int r0 = (int) (e / n), c0 = (int) (e - (long long) (e / n) * n);
      const int r = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
      double v = pk[(long long) r * (r + 1) / 2 + c];
      if ( add != NULL )
         v += sa * add[e];
      out[e] = v;
   }
}

/* up to three k_unpack_sym of the same order in one launch (blockIdx.y selects; add == NULL in all of them): the three results of the
 * three-vector sweep over the packed rows */
struct unpack3_args { const double* pk[3]; double* out[3]; };
__global__ void k_unpack_sym3(int n, unpack3_args U)
{
   const double* __restrict__ pk = U.pk[blockIdx.y];
   double* __restrict__ out = U.out[blockIdx.y];
   const long long total = (long long) n * n;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const int r0 = (int) (e / n), c0 = (int) (e - (long long) (e / n) * n);
      const int r = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
      out[e] = pk[(long long) r * (r + 1) / 2 + c];
   }
}

/* k_unpack_sym (add == NULL) into dZ followed by ipm.hip's k_dz_combine on it, element for element: dZ = (P1 - dtau P2) + eta Rd with
 * P1 out of the packed vector and dtau = sc[idtau] */
__global__ void k_unpack_dz_combine(int n, const double* __restrict__ pk, const double* __restrict__ P2, const double* __restrict__ sc, int idtau,
   double eta, const double* __restrict__ Rd, double* __restrict__ dZ)
{
   const double dtau = sc[idtau];
   const long long total = (long long) n * n;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const int r0 = (int) (e / n), c0 = (int) (e - (long long) (e / n) * n);
      const int r = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
      const double p1 = pk[(long long) r * (r + 1) / 2 + c];
      dZ[e] = (p1 - dtau * P2[e]) + eta * Rd[e];
   }
}

/* k_dirmat that also leaves the packed, weighted copy of its result (k_pack_weighted of H): the element (r, c), c <= r, is stored to
 * both places by the thread that formed it */
__global__ void k_dirmat_pack(int n, double s1, const double* __restrict__ Zinv, const double* __restrict__ X,
   const double* __restrict__ GZ, double* __restrict__ H, double* __restrict__ pk)
{
   const long long total = (long long) n * n;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / n);
      const int c = (int) (i - (long long) r * n);
      const double g = 0.5 * (GZ[i] + GZ[(long long) c * n + r]);
      const double h = s1 * Zinv[i] - X[i] - g;
      H[i] = h;
      if ( c <= r )
         pk[(long long) r * (r + 1) / 2 + c] = (r == c ? 1.0 : 2.0) * h;
   }
}

__global__ void k_zero_upper(double* A, int n)
{
   const long long total = (long long) n * n;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / n);
      const int c = (int) (i - (long long) r * n);
      if ( r < c )
         A[i] = 0.0;
   }
}

__global__ void k_symmetrize(double* A, int n)
{
   const long long total = (long long) n * n;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / n);
      const int c = (int) (i - (long long) r * n);
      if ( r > c )
      {
         const double v = 0.5 * (A[(long long) r * n + c] + A[(long long) c * n + r]);
         A[(long long) r * n + c] = v;
         A[(long long) c * n + r] = v;
      }
   }
}

__global__ void k_dirmat(int n, double s1, const double* __restrict__ Zinv, const double* __restrict__ X,
   const double* __restrict__ GZ, double* __restrict__ H)
{
   const long long total = (long long) n * n;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / n);
      const int c = (int) (i - (long long) r * n);
      const double g = 0.5 * (GZ[i] + GZ[(long long) c * n + r]);
      H[i] = s1 * Zinv[i] - X[i] - g;
   }
}

__global__ void k_lp_dir(int q, double sigmu, double eta, const double* __restrict__ x, const double* __restrict__ z,
   const double* __restrict__ r, const double* __restrict__ elp, double* __restrict__ out)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i < q )
   {
      double t = eta * x[i] * r[i];
      if ( elp != NULL )
         t += elp[i];
      out[i] = sigmu / z[i] - x[i] - t / z[i];
   }
}

__global__ void k_lp_scale_rows(int q, int cols, const double* __restrict__ x, const double* __restrict__ z,
   const double* __restrict__ D, double* __restrict__ S)
{
   const long long total = (long long) q * cols;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (i / cols);
      S[i] = (x[r] / z[r]) * D[i];
   }
}

__global__ void k_vec_mul(long long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out)
{
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
      out[i] = a[i] * b[i];
}

static inline int grid_for(long long n, int block, int cap)
{
   long long g = (n + block - 1) / block;
   if ( g > cap ) g = cap;
   if ( g < 1 ) g = 1;
   return (int) g;
}

int hs_fill(hipStream_t s, double* p, long long n, double v)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 0 ) return HS_OK;
   hipLaunchKernelGGL(k_fill, dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, p, n, v);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_set_identity(hipStream_t s, double* A, int n, double v)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 0 ) return HS_OK;
   hipLaunchKernelGGL(k_identity, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, A, n, v);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

__global__ void k_copy(long long n, const double* __restrict__ src, double* __restrict__ dst)
{
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
      dst[i] = src[i];
}

/* ---- the lanes of hipsdp_solve_objectives (hs_kernels.h) */
long long hs_objs_lane_layout(int m, int q, int nblk, const int* n, int gap, long long* off)
{
   long long t = 0;
   int i = 0;
   auto put = [&](long long len) { off[i++] = t; t += ((len + 1) & ~1LL) + gap; };
   put(m); put(m); put(q); put(q);
   for (int k = 0; k < nblk; ++k)
   {
      put((long long) n[k] * n[k]);
      put((long long) n[k] * n[k]);
   }
   return t;
}

/* blockIdx.y: the segment, blockIdx.x (and on from there in steps of the grid): the lane; a copy in 16-byte pieces */
__global__ void __launch_bounds__(256) k_objs_fanout(const hs_fan_plan P, double* __restrict__ lanes, long long lane_stride, int nlanes)
{
   typedef double fan_v2 __attribute__((ext_vector_type(2)));
   const hs_fan_seg& S = P.seg[blockIdx.y];
   const long long nv = S.len >> 1;
   for (long long j = blockIdx.x; j < nlanes; j += gridDim.x)
   {
      const double* __restrict__ src = (j == 0) ? S.src0 : S.src + (j - 1) * S.stride;
      double* __restrict__ dst = lanes + j * lane_stride + S.dst;
      for (long long e = threadIdx.x; e < nv; e += 256)
         reinterpret_cast<fan_v2*>(dst)[e] = reinterpret_cast<const fan_v2*>(src)[e];
      if ( (S.len & 1) && threadIdx.x == 0 )
         dst[S.len - 1] = src[S.len - 1];
   }
}

int hs_objs_fanout(hipStream_t st, const hs_fan_plan* plan, double* lanes, long long lane_stride, int nlanes)
{
   if ( plan->nseg <= 0 || nlanes <= 0 )
      return HS_OK;
   if ( plan->nseg > HS_FAN_MAXSEG || (lane_stride & 1) || (reinterpret_cast<size_t>(lanes) & 15) )
      return HS_ERR_ARG;
   for (int i = 0; i < plan->nseg; ++i)
   {
      const hs_fan_seg& S = plan->seg[i];
      if ( S.len <= 0 || (S.dst & 1) || (S.stride & 1) || (reinterpret_cast<size_t>(S.src0) & 15) || (reinterpret_cast<size_t>(S.src) & 15) )
         return HS_ERR_ARG;
   }
   const int gx = nlanes < (1 << 20) ? nlanes : (1 << 20);
   hipLaunchKernelGGL(k_objs_fanout, dim3(gx, plan->nseg), dim3(256), 0, st, *plan, lanes, lane_stride, nlanes);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_copy(hipStream_t s, double* dst, const double* src, long long n)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 0 ) return HS_OK;
   if ( n <= (1LL << 16) )
   {
      /* small vectors / blocks: a kernel launch costs the host about half of what the copy engine path does, and the
       * small-problem regime is bound by exactly that */
      hipLaunchKernelGGL(k_copy, dim3(grid_for(n, 256, 256)), dim3(256), 0, s, n, src, dst);
      HS_LAUNCH_CHECK();
      return HS_OK;
   }
   HS_HIP( hipMemcpyAsync(dst, src, (size_t) n * sizeof(double), hipMemcpyDeviceToDevice, s) );
   return HS_OK;
}

/* y_k += a * x_k for three vectors in one launch (the iterate update y, x, z) */
__global__ void k_axpy3(double a, long long n1, const double* __restrict__ x1, double* __restrict__ y1, long long n2,
   const double* __restrict__ x2, double* __restrict__ y2, long long n3, const double* __restrict__ x3, double* __restrict__ y3)
{
   const long long total = n1 + n2 + n3;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long) gridDim.x * blockDim.x)
   {
      if ( i < n1 )
         y1[i] += a * x1[i];
      else if ( i < n1 + n2 )
         y2[i - n1] += a * x2[i - n1];
      else
         y3[i - n1 - n2] += a * x3[i - n1 - n2];
   }
}

int hs_axpy3(hipStream_t s, double a, long long n1, const double* x1, double* y1, long long n2, const double* x2, double* y2,
   long long n3, const double* x3, double* y3)
{
   if ( n1 < 0 ) n1 = 0;
   if ( n2 < 0 ) n2 = 0;
   if ( n3 < 0 ) n3 = 0;
   if ( n1 + n2 + n3 == 0 ) return HS_OK;
   if ( hs_rec_axpy3(s, a, n1, x1, y1, n2, x2, y2, n3, x3, y3) )
      return HS_OK;
   hipLaunchKernelGGL(k_axpy3, dim3(grid_for(n1 + n2 + n3, 256, 2048)), dim3(256), 0, s, a, n1, x1, y1, n2, x2, y2, n3, x3, y3);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_scale_add(hipStream_t s, long long n, double a, const double* x, double b, const double* y, double* out)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 0 ) return HS_OK;
   hipLaunchKernelGGL(k_scale_add, dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, n, a, x, b, y, out);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* blockIdx.y = 0: X, 1: Z.  The value is formed by the statements of k_scale_add (b arrives as an argument there and here, so the
 * compiler contracts both alike); on the first attempt V is read and written by the same thread at the same index */
__global__ void k_trial_pair(long long n, double a, double b, int first, hs_trial_job J0, hs_trial_job J1)
{
   const hs_trial_job J = blockIdx.y ? J1 : J0;
   const double* base = first ? J.V : J.Vs;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
   {
      const double y = base[i];
      double v = a * J.dV[i];
      v += b * y;
      if ( first )
         J.Vs[i] = y;
      J.V[i] = v;
      J.L[i] = v;
   }
}

int hs_trial_pair(hipStream_t s, long long n, double alpha, int first, const hs_trial_job* jobs)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 0 ) return HS_OK;
   hipLaunchKernelGGL(k_trial_pair, dim3(grid_for(n, 256, 2048), 2), dim3(256), 0, s, n, alpha, 1.0, first, jobs[0], jobs[1]);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_axpy(hipStream_t s, long long n, double a, const double* x, double* y)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   return hs_scale_add(s, n, a, x, 1.0, y, y);
}

int hs_mirror_lower(hipStream_t s, double* A, int n, long long lda)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 1 ) return HS_OK;
   hipLaunchKernelGGL(k_mirror_lower, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, A, n, lda);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_mirror_upper(hipStream_t s, double* A, int n, long long lda)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 1 ) return HS_OK;
   hipLaunchKernelGGL(k_mirror_upper, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, A, n, lda);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_pack_rows(hipStream_t s, int m1, int n, long long Lp, const double* A, double* Apk)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   HS_HIP( hipMemsetAsync(Apk, 0, (size_t) m1 * (size_t) Lp * sizeof(double), s) );
   hipLaunchKernelGGL(k_pack_rows, dim3(grid_for((long long) m1 * n * n, 256, 65536)), dim3(256), 0, s, m1, n, Lp, A, Apk);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_packed_diag(hipStream_t s, int m1, int n, int ldd, long long Lp, const double* Apk, double* D)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( ldd < n )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_packed_diag, dim3(grid_for((long long) m1 * ldd, 256, 2048)), dim3(256), 0, s, m1, n, ldd, Lp, Apk, D);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_sub_lower(hipStream_t s, int n, const double* S, double* C)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   hipLaunchKernelGGL(k_sub_lower, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, n, S, C);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_pack_weighted(hipStream_t s, int n, const double* V, double* pk)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   hipLaunchKernelGGL(k_pack_weighted, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, n, V, pk);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_unpack_sym(hipStream_t s, int n, const double* pk, double sa, const double* add, double* out)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   hipLaunchKernelGGL(k_unpack_sym, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, n, pk, sa, add, out);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_unpack_sym3(hipStream_t s, int n, int cnt, const double* const* pk, double* const* out)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( cnt < 1 || cnt > 3 )
      return HS_ERR_ARG;
   unpack3_args U = {{NULL, NULL, NULL}, {NULL, NULL, NULL}};
   for (int k = 0; k < cnt; ++k)
   {
      U.pk[k] = pk[k]; U.out[k] = out[k];
   }
   hipLaunchKernelGGL(k_unpack_sym3, dim3(grid_for((long long) n * n, 256, 2048), cnt), dim3(256), 0, s, n, U);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_unpack_dz_combine(hipStream_t s, int n, const double* pk, const double* P2, const double* sc, int idtau, double eta, const double* Rd,
   double* dZ)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   hipLaunchKernelGGL(k_unpack_dz_combine, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, n, pk, P2, sc, idtau, eta, Rd, dZ);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_zero_upper(hipStream_t s, double* A, int n)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 1 ) return HS_OK;
   hipLaunchKernelGGL(k_zero_upper, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, A, n);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* dst = src^T through 32 x 32 LDS tiles (both sides coalesced) */
__global__ void __launch_bounds__(256) k_transpose(int n, const double* __restrict__ src, double* __restrict__ dst)
{
   __shared__ double tile[32][33];
   const int bx = blockIdx.x * 32, by = blockIdx.y * 32;
   const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
   for (int r = ty; r < 32; r += 8)
      if ( by + r < n && bx + tx < n )
         tile[r][tx] = src[(long long) (by + r) * n + bx + tx];
   __syncthreads();
   for (int r = ty; r < 32; r += 8)
      if ( bx + r < n && by + tx < n )
         dst[(long long) (bx + r) * n + by + tx] = tile[tx][r];
}

int hs_transpose(hipStream_t s, int n, const double* src, double* dst)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 0 ) return HS_OK;
   const int t = (n + 31) / 32;
   hipLaunchKernelGGL(k_transpose, dim3(t, t), dim3(256), 0, s, n, src, dst);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_symmetrize(hipStream_t s, double* A, int n)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 1 ) return HS_OK;
   hipLaunchKernelGGL(k_symmetrize, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, A, n);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* small blocks (n <= HS_SMALL_N): the whole chain  out = s1 Zinv - X - sym((c X R + E) Zinv)  in one workgroup, operands in LDS.
 * Same products as the three-launch path (gemm, gemm, k_dirmat), one launch: the B&B-sized problems are bound by the launch
 * count. */
#include "hs_lds_product.h"

__device__ void d_dir_block_small(int n, double c, const double* __restrict__ X, const double* __restrict__ R,
   const double* __restrict__ E, const double* __restrict__ Zinv, double s1, double* __restrict__ out, double* db_smem)
{
   const int ld = n + 1;
   double* sx = db_smem;
   double* sr = sx + n * ld;
   double* sz = sr + n * ld;
   double* sg = sz + n * ld;
   const int tid = threadIdx.x;
   const int n2 = n * n;
   if ( n2 <= 256 )
   {
      /* at most one entry per thread (n <= 16): nothing to interleave, the short form is the fast one (1.8 us at n = 10) */
      const int e = tid;
      const bool in = e < n2;
      const int r = in ? e / n : 0, cc = in ? e - r * n : 0;
      const double evv = (in && E != NULL) ? E[e] : 0.0;
      if ( in )
      {
         sx[r * ld + cc] = X[e];
         sr[r * ld + cc] = R[e];
         sz[r * ld + cc] = Zinv[e];
      }
      __syncthreads();
      if ( in )
      {
         double acc = 0.0;
         for (int k = 0; k < n; ++k)
            acc = fma(sx[r * ld + k], sr[k * ld + cc], acc);
         double g = acc * c;
         if ( E != NULL )
            g = __dadd_rn(g, evv);
         sg[r * ld + cc] = g;
      }
      __syncthreads();
      double gz = 0.0;
      if ( in )
      {
         for (int k = 0; k < n; ++k)
            gz = fma(sg[r * ld + k], sz[k * ld + cc], gz);
      }
      __syncthreads();
      if ( in )
         sr[r * ld + cc] = gz;
      __syncthreads();
      if ( in )
         out[e] = s1 * sz[r * ld + cc] - sx[r * ld + cc] - 0.5 * (sr[r * ld + cc] + sr[cc * ld + r]);
      return;
   }
   /* all global loads of the thread first (independent ones in flight together), then the LDS stores: everything in this regime
    * waits for memory, and a loop of load - store - load pays the latency once per trip */
   double ev[DB_PR][DB_PC];
   {
      const int tc = (n + DB_PC - 1) / DB_PC;
      const int pr = tid / tc, pc = tid - pr * tc;
#pragma unroll
      for (int i = 0; i < DB_PR; ++i)
#pragma unroll
         for (int j = 0; j < DB_PC; ++j)
         {
            const int r = min(DB_PR * pr + i, n - 1), cc = min(DB_PC * pc + j, n - 1);
            ev[i][j] = (E != NULL) ? E[r * n + cc] : 0.0;
         }
      const int ueff = (n2 + 255) >> 8;
      double xv[DB_U], rv[DB_U], zv[DB_U];
#pragma unroll
      for (int u = 0; u < DB_U; ++u)
         if ( u < ueff )
         {
            const int e = min(tid + 256 * u, n2 - 1);
            xv[u] = X[e];
            rv[u] = R[e];
            zv[u] = Zinv[e];
         }
#pragma unroll
      for (int u = 0; u < DB_U; ++u)
      {
         const int e = tid + 256 * u;
         if ( u < ueff && e < n2 )
         {
            const int r = e / n, cc = e - r * n;
            sx[r * ld + cc] = xv[u];
            sr[r * ld + cc] = rv[u];
            sz[r * ld + cc] = zv[u];
         }
      }
   }
   __syncthreads();
   /* G = c X R (+ E): the product is rounded, scaled, then E is added - three roundings, spelled out so that every kernel this body
    * is compiled into does the same */
   db_product(n, ld, sx, sr, [&](int i, int j, int r, int cc, double acc)
   {
      double g = acc * c;
      if ( E != NULL )
         g = __dadd_rn(g, ev[i][j]);
      sg[r * ld + cc] = g;
   });
   __syncthreads();
   /* GZ into sr (R is no longer needed) */
   db_product(n, ld, sg, sz, [&](int, int, int r, int cc, double acc) { sr[r * ld + cc] = acc; });
   __syncthreads();
   for (int e = tid; e < n2; e += 256)
   {
      const int r = e / n, cc = e - r * n;
      out[e] = s1 * sz[r * ld + cc] - sx[r * ld + cc] - 0.5 * (sr[r * ld + cc] + sr[cc * ld + r]);
   }
}

__global__ void __launch_bounds__(256) k_dir_block_small(int n, double c, const double* __restrict__ X, const double* __restrict__ R,
   const double* __restrict__ E, const double* __restrict__ Zinv, double s1, double* __restrict__ out)
{
   extern __shared__ double db_smem_k[];
   d_dir_block_small(n, c, X, R, E, Zinv, s1, out, db_smem_k);
}

int hs_dir_block_small(hipStream_t s, int n, double c, const double* X, const double* R, const double* E, const double* Zinv,
   double s1, double* out)
{
   if ( n <= 0 ) return HS_OK;
   if ( n > HS_SMALL_N ) return HS_ERR_ARG;
   if ( hs_rec_dir_block_small(s, n, c, X, R, E, Zinv, s1, out) )
      return HS_OK;
   static hs_attr_mask attr_done;
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_dir_block_small), 4 * HS_SMALL_N * (HS_SMALL_N + 1) * (int) sizeof(double), &attr_done) );
   hipLaunchKernelGGL(k_dir_block_small, dim3(1), dim3(256), (size_t) 4 * n * (n + 1) * sizeof(double), s, n, c, X, R, E, Zinv, s1, out);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_dirmat(hipStream_t s, int n, double s1, const double* Zinv, const double* X, const double* GZ, double* H)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( n <= 0 ) return HS_OK;
   hipLaunchKernelGGL(k_dirmat, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, n, s1, Zinv, X, GZ, H);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_dirmat_pack(hipStream_t s, int n, double s1, const double* Zinv, const double* X, const double* GZ, double* H, double* pk)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   hipLaunchKernelGGL(k_dirmat_pack, dim3(grid_for((long long) n * n, 256, 2048)), dim3(256), 0, s, n, s1, Zinv, X, GZ, H, pk);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_lp_dir(hipStream_t s, int q, double sigmu, double eta, const double* x, const double* z, const double* r,
   const double* elp, double* out)
{
   if ( q <= 0 ) return HS_OK;
   if ( hs_rec_lp_dir(s, q, sigmu, eta, x, z, r, elp, out) )
      return HS_OK;
   hipLaunchKernelGGL(k_lp_dir, dim3((q + 255) / 256), dim3(256), 0, s, q, sigmu, eta, x, z, r, elp, out);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_lp_scale_rows(hipStream_t s, int q, int cols, const double* x, const double* z, const double* D, double* S)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( q <= 0 ) return HS_OK;
   hipLaunchKernelGGL(k_lp_scale_rows, dim3(grid_for((long long) q * cols, 256, 2048)), dim3(256), 0, s, q, cols, x, z, D, S);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_vec_mul(hipStream_t s, long long n, const double* a, const double* b, double* out)
{
   if ( n <= 0 ) return HS_OK;
   if ( hs_rec_vec_mul(s, n, a, b, out) )
      return HS_OK;
   hipLaunchKernelGGL(k_vec_mul, dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, n, a, b, out);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* block reduction helpers (wave = 64 lanes)                                                                          */
/* ---------------------------------------------------------------------------------------------------------------- */

struct OpSum { __device__ static double id() { return 0.0; } __device__ static double f(double a, double b) { return a + b; } };
struct OpMax { __device__ static double id() { return 0.0; } __device__ static double f(double a, double b) { return a > b ? a : b; } };
struct OpMin { __device__ static double id() { return 1e300; } __device__ static double f(double a, double b) { return a < b ? a : b; } };

template<class OP>
__device__ __forceinline__ double wave_reduce(double v)
{
#pragma unroll
   for (int off = 32; off > 0; off >>= 1)
      v = OP::f(v, __shfl_down(v, off, 64));
   return v;
}

/* reduces over the 256 threads of a block; result valid in thread 0 */
template<class OP>
__device__ __forceinline__ double block_reduce_256(double v, double* sh)
{
   v = wave_reduce<OP>(v);
   const int lane = threadIdx.x & 63;
   const int wave = threadIdx.x >> 6;
   if ( lane == 0 )
      sh[wave] = v;
   __syncthreads();
   double r = OP::id();
   if ( threadIdx.x == 0 )
   {
      r = sh[0];
      for (int w = 1; w < (int) (blockDim.x >> 6); ++w)
         r = OP::f(r, sh[w]);
   }
   __syncthreads();
   return r;
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* generic two-stage reductions                                                                                       */
/* ---------------------------------------------------------------------------------------------------------------- */

#define RED_DOT      0
#define RED_ABSMAX   1
#define RED_RATIOMIN 2
#define RED_LPS0     3
#define RED_STAGE_N  2048   /* entries per workgroup of the first stage; up to that many, one workgroup writes the result itself */

template<int KIND> struct RedTraits;
template<> struct RedTraits<RED_DOT>      { typedef OpSum OP; };
template<> struct RedTraits<RED_ABSMAX>   { typedef OpMax OP; };
template<> struct RedTraits<RED_RATIOMIN> { typedef OpMin OP; };
template<> struct RedTraits<RED_LPS0>     { typedef OpSum OP; };

template<int KIND>
__device__ __forceinline__ double red_elem(long long i, const double* a, const double* b, const double* c)
{
   if ( KIND == RED_DOT )
      return a[i] * b[i];
   if ( KIND == RED_ABSMAX )
      return fabs(a[i]);
   if ( KIND == RED_RATIOMIN )
   {
      const double d = b[i];
      return d < 0.0 ? -a[i] / d : 1e300;
   }
   /* RED_LPS0: (x / z) * beta^2 */
   return (a[i] / b[i]) * c[i] * c[i];
}

template<int KIND>
__global__ void __launch_bounds__(256) k_reduce_stage1(long long n, const double* __restrict__ a, const double* __restrict__ b,
   const double* __restrict__ c, double* __restrict__ part, double* __restrict__ out, int accumulate, int direct)
{
   typedef typename RedTraits<KIND>::OP OP;
   __shared__ double sh[4];
   double v = OP::id();
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
      v = OP::f(v, red_elem<KIND>(i, a, b, c));
   v = block_reduce_256<OP>(v, sh);
   if ( threadIdx.x == 0 )
   {
      if ( direct )
         *out = accumulate ? OP::f(*out, v) : v;
      else
         part[blockIdx.x] = v;
   }
}

template<int KIND>
__global__ void __launch_bounds__(256) k_reduce_stage2(int nparts, const double* __restrict__ part, double* __restrict__ out,
   int accumulate)
{
   typedef typename RedTraits<KIND>::OP OP;
   __shared__ double sh[4];
   double v = OP::id();
   for (int i = threadIdx.x; i < nparts; i += blockDim.x)
      v = OP::f(v, part[i]);
   v = block_reduce_256<OP>(v, sh);
   if ( threadIdx.x == 0 )
      *out = accumulate ? OP::f(*out, v) : v;
}

/* ---- deferred reductions -------------------------------------------------------------------------------------------
 * The small-problem regime is bound by the number of launches, and an interior-point iteration contains runs of scalar
 * reductions (dot products, maxima, ratio tests, zeroing of scalar slots) whose inputs are not touched again until the
 * host reads the scalars.  Between hs_red_batch_begin and hs_red_batch_end such calls (vectors of at most
 * RB_MAXN entries) are only recorded; the end launches ONE single-workgroup kernel that executes the records in order
 * (so accumulation into a common slot keeps its order).  A call that does not fit flushes the records first. */
#define RB_MAX   24
#define RB_MAXN  16384
#define RB_ROWS  64       /* rows / matrices of a staged pass of RB_LPROWS / RB_APPLYA: 64 x 65 resp. 32 x 4 x 65 doubles of LDS */
#define RB_MATS  32
#define RB_MAXWORK 16384  /* multiply-adds of one recorded vector operation: above that its multi-workgroup launch is the faster form */
#define RB_FILL  100
#define RB_COPY1 101
#define RB_SOLVE 102      /* out[0:n] <- inv(L)^T inv(L) out[0:n] with a = inv(L) as 64 x 64, b = L as n x n (single-block factor, n <= 64); accumulate = number of right-hand sides, v = stride in doubles */
#define RB_FINISH 103     /* the direction's closing element-wise kernel (k_finish_dir of ipm.hip) with its parameters in fin */
#define RB_STAGE2 105     /* (105 & 31 = 9: a slot of the developer timing table that no other kind maps to) k_reduce_stage2<RED_DOT> of a dot whose first stage was launched on its own (hs_dot_deferred): p[0] = the partial
                           * sums, i[0] = their number, p[3] = out */
/* Round 3: the B&B-sized regime is bound by its launches (example_TT: 37 per iteration, 26 of them a few microseconds of work), so
 * the small single-workgroup kernels of an iteration can be recorded as well.  Every one of them does the arithmetic of its own
 * launch in the same order (element-wise kernels: any thread mapping gives the same bits; row sums of the passes: one thread /
 * one wavefront per output as in the launch; the block reduction of k_apply_A_small is re-enacted by one wavefront with four
 * accumulators per lane), so iterates do not depend on whether an operation was recorded. */
#define RB_DIRBLK  110    /* k_dir_block_small: p = X, R, E, Zinv, out; i0 = n; d0 = c, d1 = s1 */
#define RB_LPDIR   111    /* k_lp_dir: p = x, z, r, elp, out; i0 = q; d0 = sigmu, d1 = eta */
#define RB_VECMUL  112    /* k_vec_mul: p = a, b, out; i0 = n */
#define RB_AXPY3   113    /* k_axpy3: p = x1, y1, x2, y2, x3, y3; i0, i1, i2 = lengths; d0 = a */
#define RB_MAKEEXT 114    /* k_make_ext: p = v, ext; i0 = m; d0 = s0, d1 = s1 */
#define RB_GEMVT   115    /* k_gemv_t: p = A, coef, add, out; i0 = R, i1 = E, i2 = lda; d0 = sa */
#define RB_LPROWS  116    /* k_lp_rows_small: p = Dext, v, x, z, rd, elp, out1, out2; i0 = q, i1 = m1, i2 = mode; d0 = eta, d1 = sigmu */
#define RB_APPLYA  117    /* k_apply_A_small (at most two blocks): p = A0, V0, A1, V1, Dext, vlp, out, vin, vout; i0 = m1, i1 = nblk,
                           * i2, i3 = n^2 of the blocks, i4 = q, i5 = epi; d0 = scal */

struct rb_desc { int kind; int accumulate; int i[6]; double d[4]; const void* p[10]; };
struct rb_finish { int m; double eta, rg, sigmu, tau, kappa, etk; const double* u1; const double* u2; double* dy; double* dyt; double* sc;
   int s0, bub, bh, wrp, bu1, dtau, dkappa, den; };
/* pub_*: after the records, copy pub_n doubles to host-visible memory and raise the sequence number there (the host waits for
 * the number instead of a copy + stream synchronisation) */
struct rb_args { int cnt; rb_desc d[RB_MAX]; rb_finish fin; int pub_n; const double* pub_src; double* pub_dst;
   unsigned long long pub_seq; unsigned long long* pub_flag;
   unsigned long long* dbg; };         /* developer switch HIPSDP_BATCH_TIMES=1: [kind & 31][2] = wall-clock ticks (100 MHz), records */
/* hold: depth of the regions (hs_red_batch_hold / _release) inside which begin / end do not launch; smem: dynamic LDS the records need */
static_assert(sizeof(rb_args) <= 4096, "the records travel as kernel arguments");
static thread_local struct { bool open; hipStream_t s; int hold; size_t smem; rb_args args; } g_rb = {false, NULL, 0, 0, {0, {}}};

/* a launched reduction of more than RED_STAGE_N entries takes two stages (reduce_launch): k_reduce_stage1 on g = ceil(n / RED_STAGE_N)
 * workgroups, thread t of workgroup k over the entries 256 k + t, 256 (g + k) + t, ..., then k_reduce_stage2 over the g partial results.
 * Its record re-enacts both: the one workgroup keeps the g partial results of a thread position in registers (each over the same
 * entries in the same order; one pass, so the loads of the g virtual workgroups are in flight together), reduces each as its
 * workgroup would, and combines them as the second stage does - the same bits as the launch (tests/test_gpu_small_path.py,
 * red_workgroup_form at 2049 and 16 384 entries: before, the record summed in the one-workgroup order at every length). */
#define RB_STAGES (RB_MAXN / RED_STAGE_N)
static_assert(RB_STAGES * RED_STAGE_N == RB_MAXN && RB_STAGES <= 256, "rb_run keeps one partial result per first-stage workgroup");

template<int KIND>
__device__ __forceinline__ double rb_run(const rb_desc& D, double* sh, double* part)
{
   typedef typename RedTraits<KIND>::OP OP;
   const double* a = (const double*) D.p[0];
   const double* b = (const double*) D.p[1];
   const double* c = (const double*) D.p[2];
   double* out = (double*) D.p[3];
   const int n = D.i[0];
   const int g = (n + RED_STAGE_N - 1) / RED_STAGE_N;
   double v = OP::id();
   if ( g <= 1 )
   {
      for (long long i = threadIdx.x; i < n; i += 256)
         v = OP::f(v, red_elem<KIND>(i, a, b, c));
      v = block_reduce_256<OP>(v, sh);
   }
   else
   {
      double w[RB_STAGES];
#pragma unroll
      for (int k = 0; k < RB_STAGES; ++k)
         w[k] = OP::id();
      for (int base = threadIdx.x; base < n; base += 256 * g)
      {
#pragma unroll
         for (int k = 0; k < RB_STAGES; ++k)
         {
            const int i = base + 256 * k;
            if ( k < g && i < n )
               w[k] = OP::f(w[k], red_elem<KIND>(i, a, b, c));
         }
      }
#pragma unroll
      for (int k = 0; k < RB_STAGES; ++k)
      {
         if ( k < g )
         {
            const double r = block_reduce_256<OP>(w[k], sh);
            if ( threadIdx.x == 0 )
               part[k] = r;
         }
      }
      __syncthreads();
      /* k_reduce_stage2 with nparts = g <= 256: one term per thread */
      if ( (int) threadIdx.x < g )
         v = OP::f(v, part[threadIdx.x]);
      v = block_reduce_256<OP>(v, sh);
   }
   if ( threadIdx.x == 0 )
      *out = D.accumulate ? OP::f(*out, v) : v;
   return v;
}

/* what lane 0 holds after "for off = 32 .. 1: v += shfl_down(v, off)" over the 64 lanes of a wavefront, computed by ONE thread that
 * has the 64 lane values in registers: the same additions in the same association (lane l of a level adds lanes l and l + off of the
 * level before) */
__device__ __forceinline__ double d_tree64(double (&p)[64])
{
#pragma unroll
   for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int l = 0; l < off; ++l)
         p[l] += p[l + off];
   return p[0];
}

/* rb_run by ONE wavefront: lane l keeps the partial results of the threads l, 64 + l, 128 + l, 192 + l of the workgroup form, reduces
 * each as that thread's wavefront would and combines the four in the order thread 0 does - the same bits, no barrier, so up to four
 * reductions that do not depend on each other run side by side (each one is a round trip to memory: 1.06 us) */
template<int KIND>
__device__ __forceinline__ void rb_run_wave(const rb_desc& D)
{
   typedef typename RedTraits<KIND>::OP OP;
   const double* a = (const double*) D.p[0];
   const double* b = (const double*) D.p[1];
   const double* c = (const double*) D.p[2];
   double* out = (double*) D.p[3];
   const int lane = threadIdx.x & 63;
   double v[4];
#pragma unroll
   for (int g = 0; g < 4; ++g)
   {
      double x = OP::id();
      for (long long i = 64 * g + lane; i < D.i[0]; i += 256)
         x = OP::f(x, red_elem<KIND>(i, a, b, c));
      v[g] = x;
   }
#pragma unroll
   for (int g = 0; g < 4; ++g)
      v[g] = wave_reduce<OP>(v[g]);
   if ( lane == 0 )
   {
      double r = v[0];
      r = OP::f(r, v[1]); r = OP::f(r, v[2]); r = OP::f(r, v[3]);
      *out = D.accumulate ? OP::f(*out, r) : r;
   }
}

__global__ void __launch_bounds__(256) k_red_batch(rb_args A)
{
   extern __shared__ double rb_dyn[];
   __shared__ double sh[4];
   __shared__ double sh_part[RB_STAGES];
   for (int t = 0; t < A.cnt; ++t)
   {
      {
         /* a run of reductions with distinct results: up to four at a time, one per wavefront */
         int g = 0;
         /* (short vectors only: a wavefront alone takes four times as long over a long one as the workgroup does - 45 instead of 19 us
          * per batch at n = 128, where the dots run over 16 384 entries) */
         while ( g < 4 && t + g < A.cnt && A.d[t + g].kind <= RED_LPS0 && A.d[t + g].i[0] <= 1024 )
         {
            bool fresh = true;
            for (int h = 0; h < g; ++h)
               fresh = fresh && A.d[t + h].p[3] != A.d[t + g].p[3];
            if ( !fresh )
               break;
            ++g;
         }
         if ( g > 1 )
         {
            const unsigned long long tg_begin = (A.dbg != NULL) ? wall_clock64() : 0ULL;
            const int w = threadIdx.x >> 6;
            if ( w < g )
            {
               const rb_desc& G = A.d[t + w];
               switch ( G.kind )
               {
               case RED_DOT:      rb_run_wave<RED_DOT>(G); break;
               case RED_ABSMAX:   rb_run_wave<RED_ABSMAX>(G); break;
               case RED_RATIOMIN: rb_run_wave<RED_RATIOMIN>(G); break;
               default:           rb_run_wave<RED_LPS0>(G); break;
               }
            }
            __threadfence_block();
            __syncthreads();
            if ( A.dbg != NULL && threadIdx.x == 0 )
            {
               atomicAdd(A.dbg + 2 * 8, wall_clock64() - tg_begin);            /* slot 8: groups of reductions */
               atomicAdd(A.dbg + 2 * 8 + 1, 1ULL);
            }
            t += g - 1;
            continue;
         }
      }
      const rb_desc& D = A.d[t];
      const unsigned long long t_begin = (A.dbg != NULL) ? wall_clock64() : 0ULL;
      const unsigned long long c_begin = (A.dbg != NULL) ? clock64() : 0ULL;
      switch ( D.kind )
      {
      case RED_DOT:      rb_run<RED_DOT>(D, sh, sh_part); break;
      case RED_ABSMAX:   rb_run<RED_ABSMAX>(D, sh, sh_part); break;
      case RED_RATIOMIN: rb_run<RED_RATIOMIN>(D, sh, sh_part); break;
      case RED_LPS0:     rb_run<RED_LPS0>(D, sh, sh_part); break;
      case RB_FILL:      if ( threadIdx.x == 0 ) *(double*) D.p[3] = D.d[0]; break;
      case RB_COPY1:     if ( threadIdx.x == 0 ) *(double*) D.p[3] = *(const double*) D.p[0]; break;
      case RB_STAGE2:
      {
         /* the statements of k_reduce_stage2 (256 threads there as here): the partial sums are combined in its order */
         const double* part = (const double*) D.p[0];
         double* out = (double*) D.p[3];
         double v = OpSum::id();
         for (int i = threadIdx.x; i < D.i[0]; i += 256)
            v = OpSum::f(v, part[i]);
         v = block_reduce_256<OpSum>(v, sh);
         if ( threadIdx.x == 0 )
            *out = D.accumulate ? OpSum::f(*out, v) : v;
         break;
      }
      case RB_DIRBLK:
         d_dir_block_small(D.i[0], D.d[0], (const double*) D.p[0], (const double*) D.p[1], (const double*) D.p[2], (const double*) D.p[3],
            D.d[1], (double*) D.p[4], rb_dyn);
         break;
      case RB_LPDIR:
      {
         const double* x = (const double*) D.p[0]; const double* z = (const double*) D.p[1]; const double* r = (const double*) D.p[2];
         const double* elp = (const double*) D.p[3]; double* out = (double*) D.p[4];
         const double sigmu = D.d[0], eta = D.d[1];
         for (int i = threadIdx.x; i < D.i[0]; i += 256)
         {
            double t = eta * x[i] * r[i];
            if ( elp != NULL )
               t += elp[i];
            out[i] = sigmu / z[i] - x[i] - t / z[i];
         }
         break;
      }
      case RB_VECMUL:
      {
         const double* a = (const double*) D.p[0]; const double* b = (const double*) D.p[1]; double* out = (double*) D.p[2];
         for (int i = threadIdx.x; i < D.i[0]; i += 256)
            out[i] = a[i] * b[i];
         break;
      }
      case RB_AXPY3:
      {
         const double a = D.d[0];
         for (int v = 0; v < 3; ++v)
         {
            const double* x = (const double*) D.p[2 * v]; double* y = (double*) D.p[2 * v + 1];
            for (int i = threadIdx.x; i < D.i[v]; i += 256)
               y[i] += a * x[i];
         }
         break;
      }
      case RB_MAKEEXT:
      {
         const double* v = (const double*) D.p[0]; double* ext = (double*) D.p[1];
         if ( threadIdx.x == 0 )
            ext[0] = D.d[0];
         for (int i = threadIdx.x; i < D.i[0]; i += 256)
            ext[1 + i] = D.d[1] * v[i];
         break;
      }
      case RB_GEMVT:
      {
         const double* Am = (const double*) D.p[0]; const double* coef = (const double*) D.p[1]; const double* add = (const double*) D.p[2];
         double* out = (double*) D.p[3];
         const int R = D.i[0], E = D.i[1];
         const long long lda = D.i[2];
         const double sa = D.d[0];
         /* everything in this kernel waits for memory: eight rows are requested before the first is used (same summation order) */
         for (int e = threadIdx.x; e < E; e += 256)
         {
            double s0 = 0.0;
            const double* a = Am + e;
            const double ad = (add != NULL) ? add[e] : 0.0;
            int i = 0;
            for (; i + 8 <= R; i += 8)
            {
               double x[8], cq[8];
#pragma unroll
               for (int u = 0; u < 8; ++u)
               {
                  x[u] = a[(long long) (i + u) * lda];
                  cq[u] = coef[i + u];
               }
#pragma unroll
               for (int u = 0; u < 8; ++u)
                  s0 += cq[u] * x[u];
            }
            for (; i < R; ++i)
               s0 += coef[i] * a[(long long) i * lda];
            if ( add != NULL )
               s0 += sa * ad;
            out[e] = s0;
         }
         break;
      }
      case RB_LPROWS:
      {
         const double* Dext = (const double*) D.p[0]; const double* v = (const double*) D.p[1]; const double* x = (const double*) D.p[2];
         const double* z = (const double*) D.p[3]; const double* rd = (const double*) D.p[4]; const double* elp = (const double*) D.p[5];
         double* out1 = (double*) D.p[6]; double* out2 = (double*) D.p[7];
         const int q = D.i[0], m1 = D.i[1], mode = D.i[2];
         const double eta = D.d[0], sigmu = D.d[1];
         /* the launch gives a row to a wavefront: lane l sums the products i = l, l + 64, .., the lanes are added by the shuffle
          * tree.  Here: first all lane sums of up to RB_ROWS rows, one per thread and step, into LDS (everything in this kernel waits
          * for memory: the loads of a step are independent), then one THREAD per row adds its 64 lane sums in the order of the
          * tree (d_tree64).  8.8 -> 2 us at q = 85 against one wavefront per row and pass. */
         for (int rb = 0; rb < q; rb += RB_ROWS)
         {
            const int nr = min(RB_ROWS, q - rb);
            if ( m1 <= 64 )
            {
               /* at most one product per lane sum: straight-line, the loads of several steps in flight */
               const int l = threadIdx.x & 63;
               const bool has = l < m1;
               const double vl = has ? v[l] : 0.0;
               const double* dl = Dext + (has ? l : 0);
               for (int r4 = threadIdx.x >> 6; r4 < nr; r4 += 32)
               {
                  double xd[8];
#pragma unroll
                  for (int u = 0; u < 8; ++u)
                     xd[u] = dl[(long long) (rb + min(r4 + 4 * u, nr - 1)) * m1];
#pragma unroll
                  for (int u = 0; u < 8; ++u)
                     if ( r4 + 4 * u < nr )
                     {
                        double a = 0.0;
                        if ( has )
                           a += xd[u] * vl;
                        rb_dyn[(r4 + 4 * u) * 65 + l] = a;
                     }
               }
            }
            else
            {
               for (int idx = threadIdx.x; idx < nr * 64; idx += 256)
               {
                  const int r = rb + (idx >> 6), l = idx & 63;
                  const double* dr = Dext + (long long) r * m1;
                  double a = 0.0;
                  for (int i = l; i < m1; i += 64)
                     a += dr[i] * v[i];
                  rb_dyn[(idx >> 6) * 65 + l] = a;
               }
            }
            __syncthreads();
            for (int rr = threadIdx.x; rr < nr; rr += 256)
            {
               const int r = rb + rr;
               double pl[64];
#pragma unroll
               for (int l = 0; l < 64; ++l)
                  pl[l] = rb_dyn[rr * 65 + l];        /* (odd pitch: the threads of a wavefront read different banks) */
               const double t = d_tree64(pl);
               if ( mode == 0 )
                  out1[r] = t - z[r];
               else
               {
                  const double dzr = t + eta * rd[r];
                  out1[r] = dzr;
                  double tt = x[r] * dzr;
                  if ( elp != NULL )
                     tt += elp[r];
                  out2[r] = sigmu / z[r] - x[r] - tt / z[r];
               }
            }
            __syncthreads();
         }
         break;
      }
      case RB_APPLYA:
      {
         const int m1 = D.i[0], epi = D.i[5];
         double* out = (double*) D.p[6]; const double* vin = (const double*) D.p[7]; double* vout = (double*) D.p[8];
         const double scal = D.d[0];
         /* the launch: thread t of workgroup i sums the products e = t, t + 256, .. of every block and of the LP rows, the wavefronts
          * reduce by the shuffle tree, thread 0 adds the four results in order.  Here: thread t forms those sums for up to RB_MATS
          * matrices, one after the other (independent loads), into LDS; then thread (i, g) re-enacts wavefront g of workgroup i from
          * its 64 values (d_tree64) and the four of a matrix, neighbours in a wavefront, are added in the launch's order */
         const int nblk = D.i[1], n2a = D.i[2], n2b = D.i[3], q = D.i[4];
         const double* A0 = (const double*) D.p[0]; const double* V0 = (const double*) D.p[1];
         const double* A1 = (const double*) D.p[2]; const double* V1 = (const double*) D.p[3];
         const double* Dext = (const double*) D.p[4]; const double* vlp = (const double*) D.p[5];
         for (int base = 0; base < m1; base += RB_MATS)
         {
            const int nm = min(RB_MATS, m1 - base);
            const int t = threadIdx.x;
            if ( nblk == 1 && n2a <= 256 && q <= 256 )
            {
               /* at most one product of the block and one of the LP rows per thread and matrix: straight-line, eight matrices in flight */
               const bool hs = t < n2a, hl = t < q;
               const double v0 = hs ? V0[t] : 0.0, vl = hl ? vlp[t] : 0.0;
               const double* ap = A0 + (hs ? t : 0);
               const double* dp = Dext + (long long) (hl ? t : 0) * m1;
               for (int ii = 0; ii < nm; ii += 8)
               {
                  double xa[8], xd[8];
#pragma unroll
                  for (int u = 0; u < 8; ++u)
                  {
                     const int i = base + min(ii + u, nm - 1);
                     xa[u] = ap[(long long) i * n2a];
                     xd[u] = hl ? dp[i] : 0.0;         /* (q = 0: Dext has no row to read in place of a thread's own - tests/small_path_cases.py, applya_straight with q = 0) */
                  }
#pragma unroll
                  for (int u = 0; u < 8; ++u)
                     if ( ii + u < nm )
                     {
                        double a = 0.0;
                        if ( hs )
                           a += xa[u] * v0;
                        if ( hl )
                           a += xd[u] * vl;
                        rb_dyn[((ii + u) * 4 + (t >> 6)) * 65 + (t & 63)] = a;
                     }
               }
            }
            else
            for (int ii = 0; ii < nm; ++ii)
            {
               const int i = base + ii;
               double a = 0.0;
               {
                  const double* ap = A0 + (long long) i * n2a;
                  for (int e = t; e < n2a; e += 256)
                     a += ap[e] * V0[e];
               }
               if ( nblk > 1 )
               {
                  const double* ap = A1 + (long long) i * n2b;
                  for (int e = t; e < n2b; e += 256)
                     a += ap[e] * V1[e];
               }
               for (int r = t; r < q; r += 256)
                  a += Dext[(long long) r * m1 + i] * vlp[r];
               rb_dyn[(ii * 4 + (t >> 6)) * 65 + (t & 63)] = a;
            }
            __syncthreads();
            for (int jj = threadIdx.x; jj < 4 * ((nm + 15) / 16) * 16; jj += 256)      /* whole quads of threads */
            {
               const int ii = min(jj >> 2, nm - 1), g = jj & 3;
               double pl[64];
#pragma unroll
               for (int l = 0; l < 64; ++l)
                  pl[l] = rb_dyn[(ii * 4 + g) * 65 + l];
               const double sg = d_tree64(pl);
               /* sh[0] + sh[1] + sh[2] + sh[3], left to right */
               const double s1v = __shfl_down(sg, 1, 64), s2v = __shfl_down(sg, 2, 64), s3v = __shfl_down(sg, 3, 64);
               const double v = ((sg + s1v) + s2v) + s3v;
               const int i = base + (jj >> 2);
               if ( g == 0 && (jj >> 2) < nm )
               {
                  out[i] = v;
                  if ( i >= 1 )
                  {
                     if ( epi == 1 )
                        vout[i - 1] = v - scal * vin[i - 1];
                     else if ( epi == 2 )
                        vout[i - 1] = vin[i - 1] * scal - v;
                  }
               }
            }
            __syncthreads();
         }
         break;
      }
      case RB_SOLVE:
      {
         /* vec <- inv(L)^T inv(L) vec for `accumulate` right-hand sides, m <= 64, with one correction per triangular solve by the
          * factor itself: x = Y r (Y = inv(L) as computed) leaves r - L x of the order cond(L) eps |r|, and that residual is the
          * primal infeasibility the step leaves behind; x += Y (r - L x) brings it down to that of a substitution (on nodes whose
          * optimum is not attained cond(L) reaches 1e8 and the uncorrected solves stall the iteration at an infeasibility of
          * 1e-6).  Y sits in the lower triangle of an LDS tile (odd pitch), the strict lower triangle of L transposed above it,
          * the diagonal of L beside; every row of a product is split over four adjacent lanes. */
         __shared__ double sL[64 * 65];
         __shared__ double tv[64], tw[64], tr[64], ldg[64];
         const int m = D.i[0];
         const long long stride = (long long) D.d[0];
         const double* Da = (const double*) D.p[0];
         const double* Db = (const double*) D.p[1];
         const int row = threadIdx.x >> 2, part = threadIdx.x & 3;
         if ( D.i[1] )
         {
            /* round 6 (HIPSDP_SMALL_SOLVE=subst): substitution with the factor itself in the oracle's order (hs_kernels.h: hs_wl_msolve),
             * one right-hand side per wavefront */
            for (int e = threadIdx.x; e < m * m; e += 256)
            {
               const int i = e / m, j = e - i * m;
               if ( j <= i )
                  sL[i * 65 + j] = Db[(long long) i * m + j];
            }
            __syncthreads();
            const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
            for (int k = wv; k < D.accumulate; k += 4)
            {
               double* vec = (double*) D.p[3] + k * stride;
               const double x = hs_wl_msolve(sL, m, ln, ln < m ? vec[ln] : 0.0);
               if ( ln < m )
                  vec[ln] = x;
            }
            __syncthreads();
            break;
         }
         for (int e = threadIdx.x; e < m * m; e += 256)
         {
            const int i = e / m, j = e - i * m;
            if ( j <= i )
               sL[i * 65 + j] = Da[i * 64 + j];
            if ( j < i )
               sL[j * 65 + i] = Db[(long long) i * m + j];
            if ( j == i )
               ldg[i] = Db[(long long) i * m + i];
         }
         for (int k = 0; k < D.accumulate; ++k)
         {
            double* vec = (double*) D.p[3] + k * stride;
            if ( threadIdx.x < m )
               tv[threadIdx.x] = vec[threadIdx.x];
            __syncthreads();
            /* forward: tw = Y tv, tr = tv - L tw, tw += Y tr */
            double x0 = 0.0;
            {
               double acc = 0.0;
               if ( row < m )
               {
#pragma unroll 4
                  for (int j = part; j <= row; j += 4)
                     acc += sL[row * 65 + j] * tv[j];
               }
               acc += __shfl_xor(acc, 1, 64);
               acc += __shfl_xor(acc, 2, 64);
               x0 = acc;
               if ( row < m && part == 0 )
                  tw[row] = acc;
            }
            __syncthreads();
            {
               double acc = 0.0;
               if ( row < m )
               {
#pragma unroll 4
                  for (int j = part; j < row; j += 4)
                     acc += sL[j * 65 + row] * tw[j];
               }
               acc += __shfl_xor(acc, 1, 64);
               acc += __shfl_xor(acc, 2, 64);
               if ( row < m && part == 0 )
                  tr[row] = tv[row] - (acc + ldg[row] * x0);
            }
            __syncthreads();
            {
               double acc = 0.0;
               if ( row < m )
               {
#pragma unroll 4
                  for (int j = part; j <= row; j += 4)
                     acc += sL[row * 65 + j] * tr[j];
               }
               acc += __shfl_xor(acc, 1, 64);
               acc += __shfl_xor(acc, 2, 64);
               if ( row < m && part == 0 )
                  tw[row] = x0 + acc;
            }
            __syncthreads();
            /* backward: tv = Y^T tw, tr = tw - L^T tv, result = tv + Y^T tr */
            {
               double acc = 0.0;
               if ( row < m )
               {
#pragma unroll 4
                  for (int i = row + part; i < m; i += 4)
                     acc += sL[i * 65 + row] * tw[i];
               }
               acc += __shfl_xor(acc, 1, 64);
               acc += __shfl_xor(acc, 2, 64);
               x0 = acc;
               if ( row < m && part == 0 )
                  tv[row] = acc;
            }
            __syncthreads();
            {
               double acc = 0.0;
               if ( row < m )
               {
#pragma unroll 4
                  for (int i = row + 1 + part; i < m; i += 4)
                     acc += sL[row * 65 + i] * tv[i];
               }
               acc += __shfl_xor(acc, 1, 64);
               acc += __shfl_xor(acc, 2, 64);
               if ( row < m && part == 0 )
                  tr[row] = tw[row] - (acc + ldg[row] * x0);
            }
            __syncthreads();
            {
               double acc = 0.0;
               if ( row < m )
               {
#pragma unroll 4
                  for (int i = row + part; i < m; i += 4)
                     acc += sL[i * 65 + row] * tr[i];
               }
               acc += __shfl_xor(acc, 1, 64);
               acc += __shfl_xor(acc, 2, 64);
               if ( row < m && part == 0 )
                  vec[row] = x0 + acc;
            }
            __syncthreads();
         }
         break;
      }
      default:      /* RB_FINISH */
      {
         const rb_finish& F = A.fin;
         const double den = F.sc[F.s0] + F.kappa / F.tau + F.sc[F.bub];
         const double num = -F.eta * F.rg + (F.sigmu - F.tau * F.kappa - F.etk) / F.tau - F.sc[F.bh] - F.eta * F.sc[F.wrp] + F.sc[F.bu1];
         const double dtau = num / den;
         __syncthreads();
         if ( threadIdx.x == 0 )
         {
            F.sc[F.dtau] = dtau;
            F.sc[F.dkappa] = (F.sigmu - F.tau * F.kappa - F.etk - F.kappa * dtau) / F.tau;
            F.sc[F.den] = den;
            F.dyt[0] = -dtau;
         }
         for (int i = threadIdx.x; i < F.m; i += 256)
         {
            const double v = F.u1[i] - F.u2[i] * dtau;
            F.dy[i] = v;
            F.dyt[1 + i] = v;
         }
         break;
      }
      }
      /* the next record may read what this one wrote (same workgroup, global memory) */
      __threadfence_block();
      __syncthreads();
      if ( A.dbg != NULL && threadIdx.x == 0 )
      {
         const unsigned long long dt = wall_clock64() - t_begin;
         atomicAdd(A.dbg + 2 * (D.kind & 31), dt);
         atomicAdd(A.dbg + 2 * (D.kind & 31) + 1, 1ULL);
         atomicAdd(A.dbg + 64, dt);                    /* all records: wall-clock ticks and shader-clock cycles */
         atomicAdd(A.dbg + 65, (unsigned long long) clock64() - c_begin);
      }
   }
   if ( A.pub_n > 0 )
   {
      for (int i = threadIdx.x; i < A.pub_n; i += 256)
         __builtin_nontemporal_store(A.pub_src[i], A.pub_dst + i);
      __threadfence_system();
      __syncthreads();
      if ( threadIdx.x == 0 )
         __hip_atomic_store(A.pub_flag, A.pub_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
   }
}

/* HIPSDP_BATCH_TIMES=1: time per kind of record, printed when the process ends (developer switch) */
static unsigned long long* g_rb_dbg = NULL;
static void rb_dbg_report(void)
{
   unsigned long long h[66];
   if ( g_rb_dbg == NULL || hipMemcpy(h, g_rb_dbg, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess )
      return;
   if ( h[64] > 0 )
      fprintf(stderr, "batch records: shader clock while they ran %.0f MHz\n", (double) h[65] / ((double) h[64] * 0.01));
   for (int k = 0; k < 32; ++k)
      if ( h[2 * k + 1] > 0 )
         fprintf(stderr, "batch records of kind %%32 = %2d: %10llu records, %8.3f us each\n", k, h[2 * k + 1],
            (double) h[2 * k] / (double) h[2 * k + 1] * 0.01);
}
static unsigned long long* rb_dbg_buffer(void)
{
   static int on = -1;
   if ( on < 0 )
   {
      const char* env = getenv("HIPSDP_BATCH_TIMES");
      on = (env != NULL && env[0] == '1') ? 1 : 0;
      if ( on && hipMalloc((void**) &g_rb_dbg, 66 * sizeof(unsigned long long)) == hipSuccess
         && hipMemset(g_rb_dbg, 0, 66 * sizeof(unsigned long long)) == hipSuccess )
         atexit(rb_dbg_report);
      else
         g_rb_dbg = NULL;
   }
   return g_rb_dbg;
}

static int rb_flush(void)
{
   if ( g_rb.args.cnt > 0 || g_rb.args.pub_n > 0 )
   {
      if ( g_rb.smem > 0 )
      {
         static hs_attr_mask attr_done;
         HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_red_batch), 4 * HS_SMALL_N * (HS_SMALL_N + 1) * (int) sizeof(double), &attr_done) );
         static_assert(4 * HS_SMALL_N * (HS_SMALL_N + 1) >= RB_MATS * 4 * 65 && RB_MATS * 4 * 65 >= RB_ROWS * 65, "dynamic LDS of the batch kernel");
      }
      g_rb.args.dbg = rb_dbg_buffer();
      hipLaunchKernelGGL(k_red_batch, dim3(1), dim3(256), g_rb.smem, g_rb.s, g_rb.args);
      g_rb.args.cnt = 0;
      g_rb.args.pub_n = 0;
      g_rb.smem = 0;
      HS_LAUNCH_CHECK();
   }
   return HS_OK;
}

void hs_red_batch_begin(hipStream_t s)
{
   if ( g_rb.hold > 0 && g_rb.open && g_rb.s == s )
      return;                         /* inside a held region: keep recording */
   if ( g_rb.open )
      (void) rb_flush();
   g_rb.open = true;
   g_rb.s = s;
   g_rb.args.cnt = 0;
   g_rb.smem = 0;
}

/* A held region: from here to the matching release everything recordable on the stream is recorded - begin / end inside it do
 * not launch - and whatever is not recordable flushes the records first (hs_red_batch_flush in its wrapper), so the order of the
 * program is the order of execution.  Regions nest. */
void hs_red_batch_hold(hipStream_t s)
{
   if ( g_rb.hold == 0 )
      hs_red_batch_begin(s);
   ++g_rb.hold;
}

int hs_red_batch_release(void)
{
   if ( g_rb.hold > 0 && --g_rb.hold > 0 )
      return HS_OK;
   return hs_red_batch_end();
}

/* launches what is recorded and keeps recording: in front of every launch that is not recorded */
int hs_red_batch_flush(void)
{
   return (g_rb.open && g_rb.hold > 0) ? rb_flush() : HS_OK;
}

/* records waiting for the batch's launch (the unit entries: whether a call was recorded or declined) */
int hs_red_batch_pending(void)
{
   return g_rb.args.cnt;
}

/* drops whatever is recorded (an earlier call may have left a batch open on an error path) */
void hs_red_batch_reset(void)
{
   g_rb.open = false;
   g_rb.hold = 0;
   g_rb.smem = 0;
   g_rb.args.cnt = 0;
   g_rb.args.pub_n = 0;
}

int hs_red_batch_end(void)
{
   if ( g_rb.hold > 0 )
      return HS_OK;                   /* the region's release launches */
   const int rc = g_rb.open ? rb_flush() : HS_OK;
   g_rb.open = false;
   return rc;
}

/* ends every held region and the batch: before the host reads results by any other way than hs_red_batch_end_publish */
int hs_red_batch_end_all(void)
{
   g_rb.hold = 0;
   return hs_red_batch_end();
}

/* closes the batch (if one is open) and makes its kernel - or a kernel of its own when nothing is recorded - copy n doubles
 * from src (device) to dst (device view of coherent host memory) and then store seq to flag (same kind of memory) */
int hs_red_batch_end_publish(hipStream_t s, int n, const double* src, double* dst, unsigned long long seq, unsigned long long* flag)
{
   if ( g_rb.open && g_rb.s != s )
   {
      g_rb.hold = 0;
      HS_CALL( hs_red_batch_end() );
   }
   g_rb.hold = 0;                     /* a read-back ends every region */
   g_rb.s = s;
   g_rb.args.pub_n = n; g_rb.args.pub_src = src; g_rb.args.pub_dst = dst; g_rb.args.pub_seq = seq; g_rb.args.pub_flag = flag;
   if ( !g_rb.open )
      g_rb.args.cnt = 0;
   g_rb.open = false;
   return rb_flush();
}

/* 1: recorded; 0: not recordable (the caller launches normally, after the records were flushed to keep the order) */
static int rb_record(hipStream_t s, int kind, long long n, const double* a, const double* b, const double* c, double* out,
   int accumulate, double v)
{
   if ( !g_rb.open )
      return 0;
   if ( s != g_rb.s || n > RB_MAXN )
   {
      (void) rb_flush();
      return 0;
   }
   if ( g_rb.args.cnt == RB_MAX )
      (void) rb_flush();
   rb_desc& D = g_rb.args.d[g_rb.args.cnt++];
   memset(&D, 0, sizeof(D));
   D.kind = kind; D.accumulate = accumulate; D.i[0] = (int) n; D.p[0] = a; D.p[1] = b; D.p[2] = c; D.p[3] = out; D.d[0] = v;
   return 1;
}

/* a record of the round-3 kinds: NULL when no batch is open on this stream (the caller launches; pending records are flushed first) */
static rb_desc* rb_record_ext(hipStream_t s, int kind, size_t smem)
{
   /* only inside a held region: a batch opened by begin alone keeps its round-2 meaning (reductions whose inputs nobody touches
    * before the read-back; the launches between them are not recorded and run first) */
   if ( !g_rb.open || g_rb.hold == 0 )
      return NULL;
   if ( s != g_rb.s )
   {
      (void) rb_flush();
      return NULL;
   }
   if ( g_rb.args.cnt == RB_MAX )
      (void) rb_flush();
   rb_desc& D = g_rb.args.d[g_rb.args.cnt++];
   memset(&D, 0, sizeof(D));
   D.kind = kind;
   if ( smem > g_rb.smem )
      g_rb.smem = smem;
   return &D;
}

/* any other kernel launched on the stream while a batch is open must see the records executed first when it depends on
 * them; the engine only opens batches around runs where that is not the case, but scalar fills / copies of one element
 * are part of such runs and are recorded too */
int hs_fill_scalar(hipStream_t s, double* p, double v)
{
   if ( rb_record(s, RB_FILL, 1, NULL, NULL, NULL, p, 0, v) )
      return HS_OK;
   return hs_fill(s, p, 1, v);
}

int hs_copy_scalar(hipStream_t s, double* dst, const double* src)
{
   if ( rb_record(s, RB_COPY1, 1, src, NULL, NULL, dst, 0, 0.0) )
      return HS_OK;
   return hs_copy(s, dst, src, 1);
}

/* HIPSDP_SMALL_SOLVE=subst: the solves with the factor of M for m <= 128 substitute in the oracle's order (hs_kernels.h: hs_wl_msolve,
 * hs_wl2_msolve; chol.hip: k_msolve_sub64 / 128) instead of multiplying by explicitly inverted diagonal blocks with one correction per
 * triangular solve (the default since round 2).  Round 6 built it to test the reading that the general path parts from the oracle on
 * singular Schur complements BECAUSE of the inverted blocks - it does not hold up: on 24 fuzz shapes where the
 * one-launch kernel and the general path disagree, status agreement WITH THE ORACLE is 17 (substitution) against 18 (inverse) of 24, and on a fresh slice of 400
 * shapes the two paths disagree on 6 (substitution) against 4 (inverse) - profiles/r06_small_solve_substitution.txt.  Kept as a switch
 * (read at every call: tests flip it), not as the default. */
int hs_small_solve_by_substitution(void)
{
   const char* e = getenv("HIPSDP_SMALL_SOLVE");
   return (e != NULL && e[0] == 's') ? 1 : 0;
}

/* records  vec[k] <- inv(L)^T inv(L) vec[k]  (k < nrhs, vectors ld apart) for a single-block factor (m <= 64, dinv = inv(L) as
 * 64 x 64, L = the factor itself as m x m: each triangular solve is corrected once with it); 1: recorded, 0: no batch open */
int hs_red_batch_solve(hipStream_t s, int m, const double* dinv, const double* L, int nrhs, double* vec, long long ld)
{
   if ( m > 64 )
      return 0;
   if ( !rb_record(s, RB_SOLVE, m, dinv, L, NULL, vec, nrhs, (double) ld) )
      return 0;
   g_rb.args.d[g_rb.args.cnt - 1].i[1] = hs_small_solve_by_substitution();
   return 1;
}

/* records the closing kernel of a direction; the parameter block is copied.  1: recorded, 0: no batch open */
int hs_red_batch_finish(hipStream_t s, const void* fin, size_t bytes)
{
   if ( !g_rb.open || s != g_rb.s || bytes != sizeof(rb_finish) )
      return 0;
   if ( g_rb.args.cnt == RB_MAX )
      (void) rb_flush();
   memcpy(&g_rb.args.fin, fin, sizeof(rb_finish));
   rb_desc& D = g_rb.args.d[g_rb.args.cnt++];
   memset(&D, 0, sizeof(D));
   D.kind = RB_FINISH;
   return 1;
}

/* ---- recorders of the round-3 kinds.  Not recordable (no batch, other stream, too much work for one workgroup): the records so far
 * are launched - the caller's kernel must run behind them - and 0 is returned. */
static int rb_decline(void)
{
   if ( g_rb.open && g_rb.hold > 0 )
      (void) rb_flush();
   return 0;
}

static int hs_rec_dir_block_small(hipStream_t s, int n, double c, const double* X, const double* R, const double* E, const double* Zinv,
   double s1, double* out)
{
   rb_desc* D = rb_record_ext(s, RB_DIRBLK, (size_t) 4 * n * (n + 1) * sizeof(double));
   if ( D == NULL )
      return 0;
   D->i[0] = n; D->d[0] = c; D->d[1] = s1; D->p[0] = X; D->p[1] = R; D->p[2] = E; D->p[3] = Zinv; D->p[4] = out;
   return 1;
}

static int hs_rec_lp_dir(hipStream_t s, int q, double sigmu, double eta, const double* x, const double* z, const double* r, const double* elp,
   double* out)
{
   if ( q > RB_MAXN )
      return rb_decline();
   rb_desc* D = rb_record_ext(s, RB_LPDIR, 0);
   if ( D == NULL )
      return 0;
   D->i[0] = q; D->d[0] = sigmu; D->d[1] = eta; D->p[0] = x; D->p[1] = z; D->p[2] = r; D->p[3] = elp; D->p[4] = out;
   return 1;
}

static int hs_rec_vec_mul(hipStream_t s, long long n, const double* a, const double* b, double* out)
{
   if ( n > RB_MAXN )
      return rb_decline();
   rb_desc* D = rb_record_ext(s, RB_VECMUL, 0);
   if ( D == NULL )
      return 0;
   D->i[0] = (int) n; D->p[0] = a; D->p[1] = b; D->p[2] = out;
   return 1;
}

static int hs_rec_axpy3(hipStream_t s, double a, long long n1, const double* x1, double* y1, long long n2, const double* x2, double* y2,
   long long n3, const double* x3, double* y3)
{
   if ( n1 > RB_MAXN || n2 > RB_MAXN || n3 > RB_MAXN )
      return rb_decline();
   rb_desc* D = rb_record_ext(s, RB_AXPY3, 0);
   if ( D == NULL )
      return 0;
   D->d[0] = a; D->i[0] = (int) n1; D->i[1] = (int) n2; D->i[2] = (int) n3;
   D->p[0] = x1; D->p[1] = y1; D->p[2] = x2; D->p[3] = y2; D->p[4] = x3; D->p[5] = y3;
   return 1;
}

static int hs_rec_gemv_t(hipStream_t s, int R, long long E, const double* A, long long lda, const double* coef, double sa, const double* add,
   double* out)
{
   if ( E > RB_MAXN || lda > 0x7fffffffLL || (long long) R * E > RB_MAXWORK )
      return rb_decline();
   rb_desc* D = rb_record_ext(s, RB_GEMVT, 0);
   if ( D == NULL )
      return 0;
   D->i[0] = R; D->i[1] = (int) E; D->i[2] = (int) lda; D->d[0] = sa; D->p[0] = A; D->p[1] = coef; D->p[2] = add; D->p[3] = out;
   return 1;
}

/* ext = [s0; s1 v] (the coefficient vector of a pass over A with the constant matrix in front) */
__global__ void k_make_ext(int m, double s0, double s1, const double* __restrict__ v, double* __restrict__ ext)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i == 0 )
      ext[0] = s0;
   if ( i < m )
      ext[1 + i] = s1 * v[i];
}

int hs_make_ext(hipStream_t s, int m, double s0, double s1, const double* v, double* ext)
{
   if ( m <= RB_MAXN )
   {
      rb_desc* D = rb_record_ext(s, RB_MAKEEXT, 0);
      if ( D != NULL )
      {
         D->i[0] = m; D->d[0] = s0; D->d[1] = s1; D->p[0] = v; D->p[1] = ext;
         return HS_OK;
      }
   }
   else
      (void) rb_decline();
   hipLaunchKernelGGL(k_make_ext, dim3((unsigned) ((m + 1 + 255) / 256)), dim3(256), 0, s, m, s0, s1, v, ext);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* small problems, LP rows: t_r = Dext[r, :] . v, then the element-wise kernels that follow, in one launch (one wavefront per row).
 * mode 0: out1 = t - z (the residual rd);  mode 1: out1 = t + eta * rd (dz), out2 = sigmu / z - x - (x * out1 + elp) / z (dx) */
__global__ void __launch_bounds__(256) k_lp_rows_small(int q, int m1, const double* __restrict__ Dext, const double* __restrict__ v,
   int mode, double eta, double sigmu, const double* __restrict__ x, const double* __restrict__ z, const double* __restrict__ rd,
   const double* __restrict__ elp, double* __restrict__ out1, double* __restrict__ out2)
{
   const int lane = threadIdx.x & 63;
   const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
   if ( r >= q )
      return;
   const double* d = Dext + (long long) r * m1;
   double t = 0.0;
   for (int i = lane; i < m1; i += 64)
      t += d[i] * v[i];
   t = hs_wave_sum_down(t);
   if ( lane == 0 )
   {
      if ( mode == 0 )
         out1[r] = t - z[r];
      else
      {
         const double dzr = t + eta * rd[r];
         out1[r] = dzr;
         double tt = x[r] * dzr;
         if ( elp != NULL )
            tt += elp[r];
         out2[r] = sigmu / z[r] - x[r] - tt / z[r];
      }
   }
}

int hs_lp_rows_small(hipStream_t s, int q, int m1, const double* Dext, const double* v, int mode, double eta, double sigmu, const double* x,
   const double* z, const double* rd, const double* elp, double* out1, double* out2)
{
   if ( q <= 0 )
      return HS_OK;
   if ( (long long) q * m1 <= RB_MAXWORK )
   {
      rb_desc* D = rb_record_ext(s, RB_LPROWS, (size_t) RB_ROWS * 65 * sizeof(double));
      if ( D != NULL )
      {
         D->i[0] = q; D->i[1] = m1; D->i[2] = mode; D->d[0] = eta; D->d[1] = sigmu;
         D->p[0] = Dext; D->p[1] = v; D->p[2] = x; D->p[3] = z; D->p[4] = rd; D->p[5] = elp; D->p[6] = out1; D->p[7] = out2;
         return HS_OK;
      }
   }
   else
      (void) rb_decline();
   hipLaunchKernelGGL(k_lp_rows_small, dim3((q + 3) / 4), dim3(256), 0, s, q, m1, Dext, v, mode, eta, sigmu, x, z, rd, elp, out1, out2);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* small problems: A(V) over all blocks + LP part + the element-wise kernel that always follows, in one launch.
 * epi 0: out only; 1: h[i] = out[1 + i] - eta * rp[i] (k_h); 2: rp[i] = b[i] * tau - out[1 + i] (k_rp) */
__global__ void __launch_bounds__(256) k_apply_A_small(int m1, hs_as_args B, int q, const double* __restrict__ Dext,
   const double* __restrict__ vlp, double* __restrict__ out, int epi, double scal, const double* __restrict__ vin,
   double* __restrict__ vout)
{
   __shared__ double sh[4];
   const int i = blockIdx.x;
   const int tid = threadIdx.x;
   double acc = 0.0;
   for (int k = 0; k < B.nblk; ++k)
   {
      const double* a = B.A[k] + (long long) i * B.n2[k];
      const double* v = B.V[k];
      for (int e = tid; e < B.n2[k]; e += 256)
         acc += a[e] * v[e];
   }
   for (int r = tid; r < q; r += 256)
      acc += Dext[(long long) r * m1 + i] * vlp[r];
   for (int off = 32; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, 64);
   if ( (tid & 63) == 0 )
      sh[tid >> 6] = acc;
   __syncthreads();
   if ( tid == 0 )
   {
      const double v = sh[0] + sh[1] + sh[2] + sh[3];
      out[i] = v;
      if ( i >= 1 )
      {
         if ( epi == 1 )
            vout[i - 1] = v - scal * vin[i - 1];
         else if ( epi == 2 )
            vout[i - 1] = vin[i - 1] * scal - v;
      }
   }
}

int hs_apply_A_small(hipStream_t s, int m1, const hs_as_args* B, int q, const double* Dext, const double* vlp, double* out, int epi,
   double scal, const double* vin, double* vout)
{
   long long tot = q;
   for (int k = 0; k < B->nblk; ++k)
      tot += B->n2[k];
   if ( B->nblk >= 1 && B->nblk <= 2 && tot * m1 <= RB_MAXWORK )
   {
      rb_desc* D = rb_record_ext(s, RB_APPLYA, (size_t) RB_MATS * 4 * 65 * sizeof(double));
      if ( D != NULL )
      {
         D->i[0] = m1; D->i[1] = B->nblk; D->i[2] = B->n2[0]; D->i[3] = B->nblk > 1 ? B->n2[1] : 0; D->i[4] = q; D->i[5] = epi;
         D->d[0] = scal;
         D->p[0] = B->A[0]; D->p[1] = B->V[0]; D->p[2] = B->nblk > 1 ? B->A[1] : NULL; D->p[3] = B->nblk > 1 ? B->V[1] : NULL;
         D->p[4] = Dext; D->p[5] = vlp; D->p[6] = out; D->p[7] = vin; D->p[8] = vout;
         return HS_OK;
      }
   }
   else
      (void) rb_decline();
   hipLaunchKernelGGL(k_apply_A_small, dim3(m1), dim3(256), 0, s, m1, *B, q, Dext, vlp, out, epi, scal, vin, vout);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

template<int KIND>
static int reduce_launch(hipStream_t s, long long n, const double* a, const double* b, const double* c, double* out,
   int accumulate, double* ws)
{
   if ( n > 0 && rb_record(s, KIND, n, a, b, c, out, accumulate, 0.0) )
      return HS_OK;
   if ( n <= 0 )
   {
      if ( !accumulate )
      {
         const double idv = (KIND == RED_RATIOMIN) ? 1e300 : 0.0;
         HS_CALL( hs_fill_scalar(s, out, idv) );
      }
      return HS_OK;
   }
   const int g = grid_for(n, RED_STAGE_N, 256);
   (void) hs_red_batch_flush();
   if ( g == 1 )
   {
      hipLaunchKernelGGL((k_reduce_stage1<KIND>), dim3(1), dim3(256), 0, s, n, a, b, c, ws, out, accumulate, 1);
      HS_LAUNCH_CHECK();
      return HS_OK;
   }
   hipLaunchKernelGGL((k_reduce_stage1<KIND>), dim3(g), dim3(256), 0, s, n, a, b, c, ws, out, accumulate, 0);
   HS_LAUNCH_CHECK();
   hipLaunchKernelGGL((k_reduce_stage2<KIND>), dim3(1), dim3(256), 0, s, g, ws, out, accumulate);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_dot(hipStream_t s, long long n, const double* a, const double* b, double* out, int accumulate, double* ws)
{
   return reduce_launch<RED_DOT>(s, n, a, b, NULL, out, accumulate, ws);
}

/* hs_dot of a long vector inside a batch opened by hs_red_batch_begin alone (no held region): the first stage is launched at once,
 * in front of the records - it reads a and b and writes its partial sums, so no record of the batch may write a or b or read the
 * partial sums: the engine's batches of this kind hold scalar fills and reductions only - and the second stage becomes a record:
 * the batch's one launch then combines the partial sums in the order of k_reduce_stage2, behind the records before it (the fill of
 * a slot that several dots accumulate into) and in front of those behind it (the direction's closing record reads the result).
 * Two launches where a flush of the records so far, the two stages and a later batch launch were four.  slot: which 256 doubles of
 * ws (at least 1024) hold the partial sums until the batch is launched - distinct for the deferred dots of one batch.  Anything else
 * (no such batch, short vector, slot out of range) is hs_dot. */
int hs_dot_deferred(hipStream_t s, long long n, const double* a, const double* b, double* out, int accumulate, double* ws, int slot)
{
   const int g = n > 0 ? grid_for(n, 2048, 256) : 0;
   /* (a call that falls back after deferred ones is safe: hs_dot launches the records - the pending second stages - before its own first
    * stage writes ws from offset 0) */
   if ( !g_rb.open || g_rb.hold > 0 || s != g_rb.s || n <= RB_MAXN || g <= 1 || g > HS_DOT_SLOT_DOUBLES || slot < 0 || slot >= HS_DOT_SLOTS )
      return hs_dot(s, n, a, b, out, accumulate, ws);
   double* part = ws + HS_DOT_SLOT_DOUBLES * slot;
   hipLaunchKernelGGL((k_reduce_stage1<RED_DOT>), dim3(g), dim3(256), 0, s, n, a, b, (const double*) NULL, part, out, accumulate, 0);
   HS_LAUNCH_CHECK();
   if ( g_rb.args.cnt == RB_MAX )
      HS_CALL( rb_flush() );
   rb_desc& D = g_rb.args.d[g_rb.args.cnt++];
   memset(&D, 0, sizeof(D));
   D.kind = RB_STAGE2; D.accumulate = accumulate; D.i[0] = g; D.p[0] = part; D.p[3] = out;
   return HS_OK;
}

int hs_absmax(hipStream_t s, long long n, const double* a, double* out, int accumulate, double* ws)
{
   return reduce_launch<RED_ABSMAX>(s, n, a, NULL, NULL, out, accumulate, ws);
}

int hs_ratio_min(hipStream_t s, long long n, const double* x, const double* d, double* out, int accumulate, double* ws)
{
   return reduce_launch<RED_RATIOMIN>(s, n, x, d, NULL, out, accumulate, ws);
}

int hs_lp_s0(hipStream_t s, int q, const double* x, const double* z, const double* beta, double* out, int accumulate, double* ws)
{
   return reduce_launch<RED_LPS0>(s, q, x, z, beta, out, accumulate, ws);
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* A(X): row-wise dot products, one pass over A for up to four vectors                                                */
/* ---------------------------------------------------------------------------------------------------------------- */

struct gemvn_vecs { const double* v[4]; };

template<int NV, bool VEC>
__global__ void __launch_bounds__(256) k_gemv_n(int R, long long E, const double* __restrict__ A, long long lda,
   gemvn_vecs V, double* __restrict__ out, long long ldo, int nsplit, long long chunk)
{
   __shared__ double sh[4];
   const int row = blockIdx.x;
   const int sp = blockIdx.y;
   const long long e0 = sp * chunk;
   long long e1 = e0 + chunk;
   if ( e1 > E ) e1 = E;
   const double* a = A + (long long) row * lda;
   double acc[NV];
#pragma unroll
   for (int v = 0; v < NV; ++v)
      acc[v] = 0.0;

   if ( VEC )
   {
      /* chunk and e0 are even, all bases 16-byte aligned.  [Round 6, measured and not kept: four 16-byte pieces of the row in flight
       * per thread as non-allocating loads - 185 against 169 us per sweep at the bench size, and a block column of the factorization of
       * M on the other queue waited 130 us for compute units beside it (profiles/r06_sweep_streaming_loads.txt).  The column sweeps
       * k_gemv_t / k_gemv_t3 do take the non-allocating loads: 155 -> 145 us.] */
      long long e = e0 + 2 * threadIdx.x;
      for (; e + 1 < e1; e += 512)
      {
         const dbl2 x = *reinterpret_cast<const dbl2*>(a + e);
#pragma unroll
         for (int v = 0; v < NV; ++v)
         {
            const dbl2 w = *reinterpret_cast<const dbl2*>(V.v[v] + e);
            acc[v] += x.x * w.x;
            acc[v] += x.y * w.y;
         }
      }
      if ( ((e1 - e0) & 1) && threadIdx.x == 0 )
      {
#pragma unroll
         for (int v = 0; v < NV; ++v)
            acc[v] += a[e1 - 1] * V.v[v][e1 - 1];
      }
   }
   else
   {
      for (long long e = e0 + threadIdx.x; e < e1; e += 256)
      {
         const double x = a[e];
#pragma unroll
         for (int v = 0; v < NV; ++v)
            acc[v] += x * V.v[v][e];
      }
   }
#pragma unroll
   for (int v = 0; v < NV; ++v)
   {
      const double r = block_reduce_256<OpSum>(acc[v], sh);
      if ( threadIdx.x == 0 )
         out[((long long) sp * NV + v) * ldo + row] = r;
   }
}

/* one vector, many rows: four rows per workgroup, so that the vector (which every row needs and which does not stay in the
 * L2 next to the streaming A once it is a few MB) is read a quarter as often */
__global__ void __launch_bounds__(256) k_gemv_n_rows4(int R, long long E, const double* __restrict__ A, long long lda,
   const double* __restrict__ v, double* __restrict__ out)
{
   __shared__ double sh[4];
   const int row0 = blockIdx.x * 4;
   const double* a0 = A + (long long) row0 * lda;
   const double* a1 = a0 + (row0 + 1 < R ? lda : 0);
   const double* a2 = a0 + (row0 + 2 < R ? 2 * lda : 0);
   const double* a3 = a0 + (row0 + 3 < R ? 3 * lda : 0);
   double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
   /* E even, all bases 16-byte aligned (checked by the caller) */
   for (long long e = 2 * threadIdx.x; e + 1 < E; e += 512)
   {
      const dbl2 w = *reinterpret_cast<const dbl2*>(v + e);
      const dbl2 x0 = *reinterpret_cast<const dbl2*>(a0 + e);
      const dbl2 x1 = *reinterpret_cast<const dbl2*>(a1 + e);
      const dbl2 x2 = *reinterpret_cast<const dbl2*>(a2 + e);
      const dbl2 x3 = *reinterpret_cast<const dbl2*>(a3 + e);
      acc0 += x0.x * w.x; acc0 += x0.y * w.y;
      acc1 += x1.x * w.x; acc1 += x1.y * w.y;
      acc2 += x2.x * w.x; acc2 += x2.y * w.y;
      acc3 += x3.x * w.x; acc3 += x3.y * w.y;
   }
   if ( (E & 1) && threadIdx.x == 0 )
   {
      const double w = v[E - 1];
      acc0 += a0[E - 1] * w; acc1 += a1[E - 1] * w; acc2 += a2[E - 1] * w; acc3 += a3[E - 1] * w;
   }
   const double r0 = block_reduce_256<OpSum>(acc0, sh);
   const double r1 = block_reduce_256<OpSum>(acc1, sh);
   const double r2 = block_reduce_256<OpSum>(acc2, sh);
   const double r3 = block_reduce_256<OpSum>(acc3, sh);
   if ( threadIdx.x == 0 )
   {
      out[row0] = r0;
      if ( row0 + 1 < R ) out[row0 + 1] = r1;
      if ( row0 + 2 < R ) out[row0 + 2] = r2;
      if ( row0 + 3 < R ) out[row0 + 3] = r3;
   }
}

__global__ void k_gemv_n_combine(int R, int nv, int nsplit, const double* __restrict__ part, long long ldp,
   double* __restrict__ out, long long ldo)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i >= R )
      return;
   for (int v = 0; v < nv; ++v)
   {
      double s = 0.0;
      for (int k = 0; k < nsplit; ++k)
         s += part[((long long) k * nv + v) * ldp + i];
      out[(long long) v * ldo + i] = s;
   }
}

template<int NV>
static int gemv_n_launch(hipStream_t s, int R, long long E, const double* A, long long lda, const double* const* V,
   double* out, long long ldo, double* ws, long long wsdoubles)
{
   gemvn_vecs vv;
   bool vec = ((lda & 1) == 0) && ((reinterpret_cast<uintptr_t>(A) & 15) == 0);
   for (int v = 0; v < 4; ++v)
   {
      vv.v[v] = v < NV ? V[v] : V[0];
      if ( v < NV && (reinterpret_cast<uintptr_t>(V[v]) & 15) != 0 )
         vec = false;
   }
   if ( NV == 1 && vec && R >= 1024 && E >= (1LL << 18) )
   {
      hipLaunchKernelGGL(k_gemv_n_rows4, dim3((R + 3) / 4), dim3(256), 0, s, R, E, A, lda, vv.v[0], out);
      HS_LAUNCH_CHECK();
      return HS_OK;
   }
   /* enough workgroups to cover the chip: split long rows when there are few of them */
   int nsplit = 1;
   if ( R < 512 && E >= 16384 )
   {
      nsplit = (int) ((1024 + R - 1) / R);
      const long long maxs = E / 8192;
      if ( nsplit > maxs ) nsplit = (int) maxs;
      if ( nsplit < 1 ) nsplit = 1;
      if ( (long long) nsplit * NV * R > wsdoubles ) nsplit = 1;
   }
   long long chunk = (E + nsplit - 1) / nsplit;
   chunk = (chunk + 1) & ~1LL;
   double* dst = nsplit > 1 ? ws : out;
   const long long ldd = nsplit > 1 ? R : ldo;
   dim3 grid(R, nsplit);
   if ( vec )
      hipLaunchKernelGGL((k_gemv_n<NV, true>), grid, dim3(256), 0, s, R, E, A, lda, vv, dst, ldd, nsplit, chunk);
   else
      hipLaunchKernelGGL((k_gemv_n<NV, false>), grid, dim3(256), 0, s, R, E, A, lda, vv, dst, ldd, nsplit, chunk);
   HS_LAUNCH_CHECK();
   if ( nsplit > 1 )
   {
      hipLaunchKernelGGL(k_gemv_n_combine, dim3((R + 255) / 256), dim3(256), 0, s, R, NV, nsplit, ws, (long long) R, out, ldo);
      HS_LAUNCH_CHECK();
   }
   return HS_OK;
}

int hs_gemv_n(hipStream_t s, int R, long long E, const double* A, long long lda, int nv, const double* const* V,
   double* out, long long ldo, double* ws, long long wsdoubles)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( R <= 0 )
      return HS_OK;
   if ( nv < 1 || nv > 4 )
      return HS_ERR_ARG;
   if ( E <= 0 )
   {
      for (int v = 0; v < nv; ++v)
         HS_CALL( hs_fill(s, out + (long long) v * ldo, R, 0.0) );
      return HS_OK;
   }
   switch ( nv )
   {
   case 1: return gemv_n_launch<1>(s, R, E, A, lda, V, out, ldo, ws, wsdoubles);
   case 2: return gemv_n_launch<2>(s, R, E, A, lda, V, out, ldo, ws, wsdoubles);
   case 3: return gemv_n_launch<3>(s, R, E, A, lda, V, out, ldo, ws, wsdoubles);
   default: return gemv_n_launch<4>(s, R, E, A, lda, V, out, ldo, ws, wsdoubles);
   }
}

/* ---------------------------------------------------------------------------------------------------------------- */
/* A^T(y): column-wise linear combination, one pass over A                                                            */
/* ---------------------------------------------------------------------------------------------------------------- */

template<bool VEC>
__global__ void __launch_bounds__(256) k_gemv_t(int R, long long E, const double* __restrict__ A, long long lda,
   const double* __restrict__ coef, double sa, const double* __restrict__ add, double* __restrict__ out)
{
   if ( VEC )
   {
      const long long e = 2 * ((long long) blockIdx.x * blockDim.x + threadIdx.x);
      if ( e >= E )
         return;
      if ( e + 1 < E )
      {
         double s0 = 0.0, s1 = 0.0;
         const double* a = A + e;
         int i = 0;
         /* eight rows requested before the first is used (16 KB per row and workgroup in flight); same summation order */
         for (; i + 8 <= R; i += 8)
         {
            dbl2 x[8];
#pragma unroll
            for (int q = 0; q < 8; ++q)
               x[q] = load_stream2(a + (long long) (i + q) * lda);
#pragma unroll
            for (int q = 0; q < 8; ++q)
            {
               const double cq = coef[i + q];
               s0 += cq * x[q].x; s1 += cq * x[q].y;
            }
         }
         for (; i + 4 <= R; i += 4)
         {
            const dbl2 x0 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 0) * lda);
            const dbl2 x1 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 1) * lda);
            const dbl2 x2 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 2) * lda);
            const dbl2 x3 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 3) * lda);
            const double c0 = coef[i], c1 = coef[i + 1], c2 = coef[i + 2], c3 = coef[i + 3];
            s0 += c0 * x0.x; s1 += c0 * x0.y;
            s0 += c1 * x1.x; s1 += c1 * x1.y;
            s0 += c2 * x2.x; s1 += c2 * x2.y;
            s0 += c3 * x3.x; s1 += c3 * x3.y;
         }
         for (; i < R; ++i)
         {
            const dbl2 x0 = *reinterpret_cast<const dbl2*>(a + (long long) i * lda);
            const double c0 = coef[i];
            s0 += c0 * x0.x; s1 += c0 * x0.y;
         }
         if ( add != NULL )
         {
            s0 += sa * add[e];
            s1 += sa * add[e + 1];
         }
         out[e] = s0;
         out[e + 1] = s1;
      }
      else
      {
         double s0 = 0.0;
         for (int i = 0; i < R; ++i)
            s0 += coef[i] * A[(long long) i * lda + e];
         if ( add != NULL )
            s0 += sa * add[e];
         out[e] = s0;
      }
   }
   else
   {
      const long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x;
      if ( e >= E )
         return;
      double s0 = 0.0;
      for (int i = 0; i < R; ++i)
         s0 += coef[i] * A[(long long) i * lda + e];
      if ( add != NULL )
         s0 += sa * add[e];
      out[e] = s0;
   }
}

/* three linear combinations of the rows in ONE sweep over A: out_v[e] = sum_i coef_v[i] A[i][e], v = 0, 1, 2 (same summation order
 * per output as k_gemv_t: identical bits).  E even, lda even, 16-byte aligned bases. */
__global__ void __launch_bounds__(256) k_gemv_t3(int R, long long E, const double* __restrict__ A, long long lda,
   const double* __restrict__ c0, const double* __restrict__ c1, const double* __restrict__ c2, double* __restrict__ o0,
   double* __restrict__ o1, double* __restrict__ o2)
{
   const long long e = 2 * ((long long) blockIdx.x * blockDim.x + threadIdx.x);
   if ( e >= E )
      return;
   double s00 = 0.0, s01 = 0.0, s10 = 0.0, s11 = 0.0, s20 = 0.0, s21 = 0.0;
   const double* a = A + e;
   int i = 0;
   for (; i + 8 <= R; i += 8)
   {
      dbl2 xx[8];
#pragma unroll
      for (int q = 0; q < 8; ++q)
         xx[q] = load_stream2(a + (long long) (i + q) * lda);
#pragma unroll
      for (int q = 0; q < 8; ++q)
      {
         const dbl2 x = xx[q];
         const double a0 = c0[i + q], a1 = c1[i + q], a2 = c2[i + q];
         s00 += a0 * x.x; s01 += a0 * x.y;
         s10 += a1 * x.x; s11 += a1 * x.y;
         s20 += a2 * x.x; s21 += a2 * x.y;
      }
   }
   for (; i + 4 <= R; i += 4)
   {
      const dbl2 x0 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 0) * lda);
      const dbl2 x1 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 1) * lda);
      const dbl2 x2 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 2) * lda);
      const dbl2 x3 = *reinterpret_cast<const dbl2*>(a + (long long) (i + 3) * lda);
#pragma unroll
      for (int q = 0; q < 4; ++q)
      {
         const dbl2 x = q == 0 ? x0 : (q == 1 ? x1 : (q == 2 ? x2 : x3));
         const double a0 = c0[i + q], a1 = c1[i + q], a2 = c2[i + q];
         s00 += a0 * x.x; s01 += a0 * x.y;
         s10 += a1 * x.x; s11 += a1 * x.y;
         s20 += a2 * x.x; s21 += a2 * x.y;
      }
   }
   for (; i < R; ++i)
   {
      const dbl2 x = *reinterpret_cast<const dbl2*>(a + (long long) i * lda);
      const double a0 = c0[i], a1 = c1[i], a2 = c2[i];
      s00 += a0 * x.x; s01 += a0 * x.y;
      s10 += a1 * x.x; s11 += a1 * x.y;
      s20 += a2 * x.x; s21 += a2 * x.y;
   }
   o0[e] = s00; o0[e + 1] = s01;
   o1[e] = s10; o1[e + 1] = s11;
   o2[e] = s20; o2[e + 1] = s21;
}

/* 1: done in one sweep; 0: shapes / alignment do not qualify (the caller makes three hs_gemv_t calls) */
int hs_gemv_t3(hipStream_t s, int R, long long E, const double* A, long long lda, const double* c0, const double* c1, const double* c2,
   double* o0, double* o1, double* o2)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   if ( E <= 0 || R <= 0 || (E & 1) || (lda & 1) || (reinterpret_cast<uintptr_t>(A) & 15) || (reinterpret_cast<uintptr_t>(o0) & 15)
      || (reinterpret_cast<uintptr_t>(o1) & 15) || (reinterpret_cast<uintptr_t>(o2) & 15) )
      return 0;
   const long long nthreads = E / 2;
   hipLaunchKernelGGL(k_gemv_t3, dim3((unsigned) ((nthreads + 255) / 256)), dim3(256), 0, s, R, E, A, lda, c0, c1, c2, o0, o1, o2);
   if ( hipGetLastError() != hipSuccess )
      return -HS_ERR_HIP;
   return 1;
}

/* few output entries, many rows (a block of 50 - 300 rows with hundreds of variables: E = 2 500 .. 45 000 entries, 10 .. 90 workgroups
 * of k_gemv_t, each walking all rows: 1 TB/s): the rows are cut into chunks, workgroup (x, c) forms the partial sums of chunk c, a
 * second launch adds the chunks in order (and the additive term).  Deterministic; not the summation order of k_gemv_t, which is
 * why the recorded form (RB_GEMVT, tiny problems) and this one never apply to the same size. */
__global__ void __launch_bounds__(256) k_gemv_t_part(int R, int rc, long long E, const double* __restrict__ A, long long lda,
   const double* __restrict__ coef, double* __restrict__ part)
{
   const long long e = 2 * ((long long) blockIdx.x * blockDim.x + threadIdx.x);
   if ( e >= E )
      return;
   const int i0 = blockIdx.y * rc;
   const int i1 = min(R, i0 + rc);
   double s0 = 0.0, s1 = 0.0;
   const bool two = e + 1 < E;
   const double* a = A + e;
   int i = i0;
   for (; i + 8 <= i1; i += 8)
   {
      double x0[8], x1[8];
#pragma unroll
      for (int q = 0; q < 8; ++q)
      {
         const double* p = a + (long long) (i + q) * lda;
         x0[q] = p[0];
         x1[q] = two ? p[1] : 0.0;
      }
#pragma unroll
      for (int q = 0; q < 8; ++q)
      {
         const double cq = coef[i + q];
         s0 += cq * x0[q]; s1 += cq * x1[q];
      }
   }
   for (; i < i1; ++i)
   {
      const double* p = a + (long long) i * lda;
      const double cq = coef[i];
      s0 += cq * p[0];
      if ( two )
         s1 += cq * p[1];
   }
   double* o = part + (long long) blockIdx.y * E + e;
   o[0] = s0;
   if ( two )
      o[1] = s1;
}

__global__ void __launch_bounds__(256) k_gemv_t_comb(int C, long long E, const double* __restrict__ part, double sa,
   const double* __restrict__ add, double* __restrict__ out)
{
   const long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x;
   if ( e >= E )
      return;
   double s0 = 0.0;
   for (int c = 0; c < C; ++c)
      s0 += part[(long long) c * E + e];
   if ( add != NULL )
      s0 += sa * add[e];
   out[e] = s0;
}

/* chunks the split form would use (0: the plain kernel is the right one); workspace: chunks * E doubles */
int hs_gemv_t_chunks(int R, long long E)
{
   if ( E > 65536 || R < 128 || (long long) R * E < (1LL << 20) )
      return 0;
   const long long wg = (E + 511) / 512;
   long long c = (512 + wg - 1) / wg;
   if ( c > 32 ) c = 32;
   if ( c > R / 32 ) c = R / 32;
   return c >= 2 ? (int) c : 0;
}

int hs_gemv_t_ws(hipStream_t s, int R, long long E, const double* A, long long lda, const double* coef, double sa,
   const double* add, double* out, double* ws, long long wsdoubles)
{
   const int C = hs_gemv_t_chunks(R, E);
   if ( C == 0 || ws == NULL || (long long) C * E > wsdoubles )
      return hs_gemv_t(s, R, E, A, lda, coef, sa, add, out);
   (void) hs_red_batch_flush();
   int rc = (R + C - 1) / C;
   rc = (rc + 7) & ~7;
   const int Cu = (R + rc - 1) / rc;
   hipLaunchKernelGGL(k_gemv_t_part, dim3((unsigned) ((E + 511) / 512), (unsigned) Cu), dim3(256), 0, s, R, rc, E, A, lda, coef, ws);
   hipLaunchKernelGGL(k_gemv_t_comb, dim3((unsigned) ((E + 255) / 256)), dim3(256), 0, s, Cu, E, ws, sa, add, out);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_gemv_t(hipStream_t s, int R, long long E, const double* A, long long lda, const double* coef, double sa,
   const double* add, double* out)
{
   if ( E <= 0 )
      return HS_OK;
   if ( hs_rec_gemv_t(s, R, E, A, lda, coef, sa, add, out) )
      return HS_OK;
   const bool vec = ((lda & 1) == 0) && ((reinterpret_cast<uintptr_t>(A) & 15) == 0) && R > 0;
   if ( vec )
   {
      const long long nthreads = (E + 1) / 2;
      hipLaunchKernelGGL((k_gemv_t<true>), dim3((unsigned) ((nthreads + 255) / 256)), dim3(256), 0, s, R, E, A, lda, coef, sa, add, out);
   }
   else
      hipLaunchKernelGGL((k_gemv_t<false>), dim3((unsigned) ((E + 255) / 256)), dim3(256), 0, s, R, E, A, lda, coef, sa, add, out);
   HS_LAUNCH_CHECK();
   return HS_OK;
}
