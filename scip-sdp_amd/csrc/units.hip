/* units.hip - TEST entry points around single device kernels for the per-kernel parity tests in tests/ (self-checks of the GEMM
 * kernels, single factorizations, single Schur assemblies, ...).  Each call: H2D, kernel(s) on the default stream, D2H, with
 * per-call allocations - fine for tests, not for the product: what lapack_interface_hip.c calls (hipsdp_dgemm, hipsdp_gemv_*,
 * hipsdp_syev) lives in host_entries.hip.  Nothing here has a CPU code path. */
#include "hs_kernels.h"
#include "hs_chunks.h"
#include "hs_gram_cache.h"
#include "../../include/hipsdp.h"
#include "../../include/hipsdp_units.h"
#include <vector>
#include <algorithm>
#include <cstring>
#include <cstdlib>

namespace {

struct DevBuf
{
   double* p;
   DevBuf() : p(NULL) {}
   ~DevBuf() { if ( p ) (void) hipFree(p); }
   int alloc(long long n) { if ( n <= 0 ) n = 1; hipError_t e = hipMalloc((void**) &p, (size_t) n * sizeof(double)); if ( e != hipSuccess ) { hs_record_hip_error(e, "hipMalloc", __FILE__, __LINE__); return e == hipErrorOutOfMemory ? HS_ERR_NOMEM : HS_ERR_HIP; } return HS_OK; }
   int up(const double* h, long long n) { if ( n <= 0 ) return HS_OK; hipError_t e = hipMemcpy(p, h, (size_t) n * sizeof(double), hipMemcpyHostToDevice); if ( e != hipSuccess ) { hs_record_hip_error(e, "H2D", __FILE__, __LINE__); return HS_ERR_HIP; } return HS_OK; }
   int down(double* h, long long n) { if ( n <= 0 ) return HS_OK; hipError_t e = hipMemcpy(h, p, (size_t) n * sizeof(double), hipMemcpyDeviceToHost); if ( e != hipSuccess ) { hs_record_hip_error(e, "D2H", __FILE__, __LINE__); return HS_ERR_HIP; } return HS_OK; }
};

int pick_device(int device)
{
   int nd = 0;
   if ( hipGetDeviceCount(&nd) != hipSuccess || nd <= 0 )
      return HIPSDP_ERR_NODEVICE;
   if ( device < 0 || device >= nd )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(device) );
   return HS_OK;
}

long long span(int rows, int cols, long long ld) { return rows <= 0 ? 0 : (long long) (rows - 1) * ld + cols; }

}

/* fills with reproducible values in [-0.5, 0.5) */
__global__ void k_unit_fill(long long n, unsigned long long seed, double* __restrict__ x)
{
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
   {
      unsigned long long h = (unsigned long long) (i + 1) * 0x9E3779B97F4A7C15ULL + seed;
      h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ULL; h ^= h >> 32; h *= 0x94D049BB133111EBULL; h ^= h >> 29;
      x[i] = (double) (h >> 11) * (1.0 / 9007199254740992.0) - 0.5;
   }
}

__global__ void k_unit_maxdiff(long long n, const double* __restrict__ a, const double* __restrict__ b, unsigned long long* __restrict__ ndiff)
{
   unsigned long long cnt = 0;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
      if ( __double_as_longlong(a[i]) != __double_as_longlong(b[i]) )
         ++cnt;
   if ( cnt )
      atomicAdd(ndiff, cnt);
}

/* max |a - b| (non-negative doubles order like their bit patterns) */
__global__ void k_unit_maxabsdiff(long long n, const double* __restrict__ a, const double* __restrict__ b, unsigned long long* __restrict__ out)
{
   double m = 0.0;
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long) gridDim.x * blockDim.x)
   {
      const double d = fabs(a[i] - b[i]);
      if ( !(d <= m) )            /* a NaN counts as the largest difference */
         m = (d != d) ? 1e300 : d;
   }
   if ( m > 0.0 )
      atomicMax(out, (unsigned long long) __double_as_longlong(m));
}

/* zero the part of an operand that a triangular flag declares zero: mode 0: X[r][c] = 0 for c > r (rows x cols, K contiguous A:
 * k > m), mode 1: X[r][c] = 0 for r < c (B stored [K][N]: k < n) - the same predicate, kept apart for readability */
__global__ void k_unit_tri(int rows, int cols, long long stride, int batch, double* __restrict__ x)
{
   const long long per = (long long) rows * cols;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < per * batch; e += (long long) gridDim.x * blockDim.x)
   {
      const long long b = e / per, w = e - b * per;
      const int r = (int) (w / cols), c = (int) (w - (long long) r * cols);
      if ( c > r )
         x[b * stride + w] = 0.0;
   }
}

/* X[r][c] = 0 for c < r (upper triangular left factor) */
__global__ void k_unit_tri_upper(int rows, int cols, double* __restrict__ x)
{
   const long long per = (long long) rows * cols;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < per; e += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (e / cols), c = (int) (e - (long long) r * cols);
      if ( c < r )
         x[e] = 0.0;
   }
}

/* The same product through both GEMM kernels (dgemm.hip, dgemm2.hip) on device-generated operands: the results must agree
 * bit for bit.  A is K-contiguous; layB, batch, splitk and flags as in hs_gemm_args (C packed, ldc = N).  used_v2 = 1 when
 * the persistent kernel accepted the shape; ndiff = number of differing elements of C (over all batch entries). */
static int dgemm_selfcheck_impl(int device, int M, int N, int K, int layB, int batch, int splitk, int flags, double alpha, double beta,
   int reps, int* used, long long* ndiff, double* ms_tile, double* ms_fast, double* maxdiff = NULL, long long* nrepro = NULL)
{
   HS_CALL( pick_device(device) );
   if ( M <= 0 || N <= 0 || K <= 0 || batch < 1 )
      return HIPSDP_ERR_ARG;
   const long long na = (long long) M * K, nb = (long long) N * K, nc = (long long) M * N;
   const long long sB = (batch > 1) ? nb : 0;
   DevBuf dA, dB, dC1, dC2, dW;
   unsigned long long* dn = NULL;
   HS_CALL( dA.alloc(na) ); HS_CALL( dB.alloc(batch > 1 ? nb * batch : nb) ); HS_CALL( dC1.alloc(nc * batch) ); HS_CALL( dC2.alloc(nc * batch) );
   if ( splitk > 1 )
      HS_CALL( dW.alloc((long long) splitk * nc) );
   HS_HIP( hipMalloc((void**) &dn, sizeof(unsigned long long)) );
   HS_HIP( hipMemset(dn, 0, sizeof(unsigned long long)) );
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, na, 11ULL, dA.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, batch > 1 ? nb * batch : nb, 23ULL, dB.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, nc * batch, 37ULL, dC1.p);
   if ( flags & HS_GEMM_A_LOWTRI )
      hipLaunchKernelGGL(k_unit_tri, dim3(1024), dim3(256), 0, 0, M, K, 0LL, 1, dA.p);
   if ( (flags & HS_GEMM_B_LOWTRI) && layB == HS_MC )
      hipLaunchKernelGGL(k_unit_tri, dim3(1024), dim3(256), 0, 0, K, N, nb, batch, dB.p);
   if ( flags & HS_GEMM_A_UPTRI )
      hipLaunchKernelGGL(k_unit_tri_upper, dim3(1024), dim3(256), 0, 0, M, K, dA.p);
   HS_HIP( hipMemcpy(dC2.p, dC1.p, (size_t) (nc * batch) * sizeof(double), hipMemcpyDeviceToDevice) );
   hs_gemm_args g = {M, N, K, HS_KC, layB, dA.p, K, 0, dB.p, layB == HS_KC ? (long long) K : (long long) N, sB, dC1.p, N, nc, alpha, beta,
      batch, flags, splitk, dW.p};
   hipEvent_t e0 = NULL, e1 = NULL;
   if ( reps > 0 && (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) )
      return HS_ERR_HIP;
   auto timed = [&](double* ms) -> int
   {
      /* beta = 0 only (the product is repeated on the same C) */
      if ( reps <= 0 || ms == NULL || beta != 0.0 )
         return HS_OK;
      int rc = HS_OK;
      for (int w = 0; w < 2 && rc == HS_OK; ++w)
         rc = hs_dgemm(0, &g);
      (void) hipEventRecord(e0, 0);
      for (int r = 0; r < reps && rc == HS_OK; ++r)
         rc = hs_dgemm(0, &g);
      (void) hipEventRecord(e1, 0);
      if ( rc == HS_OK && hipEventSynchronize(e1) != hipSuccess )
         rc = HS_ERR_HIP;
      float t = 0.f;
      if ( rc == HS_OK && hipEventElapsedTime(&t, e0, e1) != hipSuccess )
         rc = HS_ERR_HIP;
      *ms = (double) t / reps;
      return rc;
   };
   int rc = HS_OK;
   /* reference: the one-tile-per-workgroup kernel (dgemm.hip) alone */
   hs_dgemm2_enable(0);
   rc = hs_dgemm(0, &g);
   if ( rc == HS_OK )
      rc = timed(ms_tile);
   const int before = hs_dgemm2_enable(1);
   g.C = dC2.p;
   /* the second run must not inherit the slabs of the first: a slice one kernel never writes would go unnoticed */
   if ( splitk > 1 )
      hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, (long long) splitk * nc, 51ULL, dW.p);
   if ( rc == HS_OK )
      rc = hs_dgemm(0, &g);
   const int after = hs_dgemm2_enable(1);
   if ( rc == HS_OK )
      rc = timed(ms_fast);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess )
      rc = HS_ERR_HIP;
   unsigned long long hn = 0;
   if ( rc == HS_OK )
   {
      hipLaunchKernelGGL(k_unit_maxdiff, dim3(1024), dim3(256), 0, 0, nc * batch, dC1.p, dC2.p, dn);
      if ( hipMemcpy(&hn, dn, sizeof(hn), hipMemcpyDeviceToHost) != hipSuccess )
         rc = HS_ERR_HIP;
   }
   if ( rc == HS_OK && nrepro != NULL )
   {
      /* the default dispatch once more into a third array: the same bits whichever workgroup computed which tile */
      DevBuf dC3;
      unsigned long long hr = 0;
      rc = dC3.alloc(nc * batch);
      if ( rc == HS_OK && hipMemcpy(dC3.p, dC1.p, (size_t) (nc * batch) * sizeof(double), hipMemcpyDeviceToDevice) != hipSuccess )
         rc = HS_ERR_HIP;
      if ( rc == HS_OK && beta != 0.0 )
      {
         /* (beta != 0: C1 holds the tile kernel's result, not the input - regenerate the input) */
         hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, nc * batch, 37ULL, dC3.p);
         hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, nc * batch, 37ULL, dC2.p);
         g.C = dC2.p;
         rc = hs_dgemm(0, &g);
      }
      g.C = dC3.p;
      if ( rc == HS_OK )
         rc = hs_dgemm(0, &g);
      if ( rc == HS_OK && hipMemset(dn, 0, sizeof(unsigned long long)) != hipSuccess )
         rc = HS_ERR_HIP;
      if ( rc == HS_OK )
      {
         hipLaunchKernelGGL(k_unit_maxdiff, dim3(1024), dim3(256), 0, 0, nc * batch, dC2.p, dC3.p, dn);
         if ( hipMemcpy(&hr, dn, sizeof(hr), hipMemcpyDeviceToHost) != hipSuccess )
            rc = HS_ERR_HIP;
      }
      *nrepro = (long long) hr;
      g.C = dC2.p;
   }
   if ( rc == HS_OK && maxdiff != NULL )
   {
      unsigned long long bits = 0;
      if ( hipMemset(dn, 0, sizeof(unsigned long long)) != hipSuccess )
         rc = HS_ERR_HIP;
      hipLaunchKernelGGL(k_unit_maxabsdiff, dim3(1024), dim3(256), 0, 0, nc * batch, dC1.p, dC2.p, dn);
      if ( rc == HS_OK && hipMemcpy(&bits, dn, sizeof(bits), hipMemcpyDeviceToHost) != hipSuccess )
         rc = HS_ERR_HIP;
      memcpy(maxdiff, &bits, sizeof(double));
   }
   (void) hipFree(dn);
   if ( e0 != NULL ) (void) hipEventDestroy(e0);
   if ( e1 != NULL ) (void) hipEventDestroy(e1);
   HS_CALL( rc );
   *used = after - before > 0 ? 1 : 0;
   *ndiff = (long long) hn;
   return HIPSDP_OK;
}

extern "C" int hipsdp_dgemm_selfcheck(int device, int M, int N, int K, int layB, int batch, int splitk, int flags, double beta,
   int* used_v2, long long* ndiff)
{
   int used = 0;
   HS_CALL( dgemm_selfcheck_impl(device, M, N, K, layB, batch, splitk, flags, 1.25, beta, 0, &used, ndiff, NULL, NULL) );
   *used_v2 = used & 1;
   return HIPSDP_OK;
}

/* the same with a free alpha and, for reps > 0 and beta = 0, the average time of one product through the tile kernel alone
 * (ms_tile) and through the default dispatch (ms_fast).  *used: bit 0 a persistent kernel of dgemm2.hip took it */
extern "C" int hipsdp_dgemm_selfcheck2(int device, int M, int N, int K, int layB, int batch, int splitk, int flags, double alpha, double beta,
   int reps, int* used, long long* ndiff, double* ms_tile, double* ms_fast)
{
   return dgemm_selfcheck_impl(device, M, N, K, layB, batch, splitk, flags, alpha, beta, reps, used, ndiff, ms_tile, ms_fast);
}

/* the same with the largest absolute difference between the two results (entries are sums of K products of values in
 * [-0.5, 0.5): the paired-band kernel of the triangular products sums the band in another order than the tile kernel) */
extern "C" int hipsdp_dgemm_selfcheck3(int device, int M, int N, int K, int layB, int batch, int splitk, int flags, double alpha, double beta,
   int reps, int* used, long long* ndiff, double* maxdiff, long long* nrepro, double* ms_tile, double* ms_fast)
{
   return dgemm_selfcheck_impl(device, M, N, K, layB, batch, splitk, flags, alpha, beta, reps, used, ndiff, ms_tile, ms_fast, maxdiff, nrepro);
}

/* One product with a triangular operand from the caller's operands through hs_dgemm, with the instance of the paired-band kernel
 * (csrc/dgemm2.hip) forced: mode 0 its 128 x 128 instance, 1 its wide instance, -1 the default dispatch.  A [M][K] K contiguous
 * (shared by the batch), B [batch][K][N] (layB = HS_MC) or [batch][N][K] (HS_KC), C [batch][crows][ldc] with crows >= M and ldc >= N:
 * passed in and returned whole, so the caller sees what lies outside the M x N results.  alpha = 1, beta = 0.
 * used[2]: products of the call the paired-band kernel took, and of these its wide instance. */
extern "C" int hipsdp_tri_product_unit(int device, int mode, int M, int N, int K, int layB, int batch, int flags, const double* A,
   const double* B, double* Cio, int crows, int ldc, int* used)
{
   HS_CALL( pick_device(device) );
   if ( mode < -1 || mode > 1 || M < 1 || N < 1 || K < 1 || batch < 1 || (layB != HS_MC && layB != HS_KC) || A == NULL || B == NULL || Cio == NULL
      || crows < M || ldc < N || used == NULL )
      return HIPSDP_ERR_ARG;
   const long long na = (long long) M * K, nb = (long long) N * K, nc = (long long) crows * ldc;
   DevBuf dA, dB, dC;
   HS_CALL( dA.alloc(na) ); HS_CALL( dB.alloc(nb * batch) ); HS_CALL( dC.alloc(nc * batch) );
   HS_CALL( dA.up(A, na) ); HS_CALL( dB.up(B, nb * batch) ); HS_CALL( dC.up(Cio, nc * batch) );
   hs_gemm_args g = {M, N, K, HS_KC, layB, dA.p, K, 0, dB.p, layB == HS_KC ? (long long) K : (long long) N, nb, dC.p, ldc, nc, 1.0, 0.0,
      batch, flags, 1, NULL};
   const int t5 = hs_dgemm2_paired_taken();
   const int tw = hs_dgemm2_wide_force(mode);
   int rc = hs_dgemm(0, &g);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   used[1] = hs_dgemm2_wide_force(-1) - tw;
   used[0] = hs_dgemm2_paired_taken() - t5;
   HS_CALL( rc );
   HS_CALL( dC.down(Cio, nc * batch) );
   return HIPSDP_OK;
}

/* test hook of the same choice for the calls that reach these products through the assembly (hipsdp_schur_form_unit): mode as above;
 * returns how many products the wide instance has taken so far */
extern "C" int hipsdp_tri_instance_force(int mode)
{
   return hs_dgemm2_wide_force(mode);
}

/* lower triangle: max |a - b| over r >= c, and the number of elements there whose bits differ */
__global__ void k_unit_lowdiff(int M, const double* __restrict__ a, const double* __restrict__ b, unsigned long long* __restrict__ out)
{
   double m = 0.0;
   unsigned long long cnt = 0;
   const long long MM = (long long) M * M;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < MM; e += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (e / M), c = (int) (e - (long long) r * M);
      if ( c > r )
         continue;
      const double d = fabs(a[e] - b[e]);
      if ( !(d <= m) )
         m = (d != d) ? 1e300 : d;
      if ( __double_as_longlong(a[e]) != __double_as_longlong(b[e]) )
         ++cnt;
   }
   if ( m > 0.0 )
      atomicMax(out, (unsigned long long) __double_as_longlong(m));
   if ( cnt )
      atomicAdd(out + 1, cnt);
}

/* The Gram product of the Schur assembly, C = W W^T + C on the lower triangle with W [M][K] generated on the device, through the
 * K-sliced tile kernels (hs_dgemm, HS_GEMM_LOWER | HS_GEMM_XCD) and through the Gram kernel (gram.hip): *used = 1 when the Gram
 * kernel took the shape, *maxdiff = largest difference over the lower triangle, *nrepro = elements of the lower triangle that
 * differ between two runs of the Gram kernel (must be 0); reps > 0: average times of the two paths */
extern "C" int hipsdp_gram_selfcheck(int device, int M, long long K, int reps, int* used, double* maxdiff, long long* nrepro, double* ms_tile,
   double* ms_gram)
{
   HS_CALL( pick_device(device) );
   if ( M <= 0 || K <= 0 || used == NULL || maxdiff == NULL || nrepro == NULL )
      return HIPSDP_ERR_ARG;
   const long long MM = (long long) M * M;
   const long long tm = (M + 127) / 128;
   int sk = hs_dgemm_pick_xcd_slices(tm * (tm + 1) / 2, K);
   const int nslab = 64;
   DevBuf dW, dC1, dC2, dC3, dS;
   unsigned long long* dn = NULL;
   HS_CALL( dW.alloc((long long) M * K) ); HS_CALL( dC1.alloc(MM) ); HS_CALL( dC2.alloc(MM) ); HS_CALL( dC3.alloc(MM) ); HS_CALL( dS.alloc((long long) nslab * MM) );
   HS_HIP( hipMalloc((void**) &dn, 2 * sizeof(unsigned long long)) );
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, (long long) M * K, 11ULL, dW.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, MM, 37ULL, dC1.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, MM, 37ULL, dC2.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, MM, 37ULL, dC3.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, (long long) nslab * MM, 51ULL, dS.p);
   hs_gemm_args g3 = {M, M, (int) K, HS_KC, HS_KC, dW.p, K, 0, dW.p, K, 0, dC1.p, M, 0, 1.0, 1.0, 1, HS_GEMM_LOWER | HS_GEMM_XCD | HS_GEMM_NOFAST, sk, dS.p};
   int rc = hs_dgemm(0, &g3);
   int r2 = 0;
   double ex = 0.0;
   if ( rc == HS_OK )
   {
      hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, (long long) nslab * MM, 52ULL, dS.p);
      r2 = hs_gram_try(0, M, K, dW.p, K, dC2.p, M, 1.0, 1.0, dS.p, nslab, &ex);
      if ( r2 < 0 ) rc = -r2;
   }
   if ( rc == HS_OK && r2 == 1 )
   {
      hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, (long long) nslab * MM, 53ULL, dS.p);
      r2 = hs_gram_try(0, M, K, dW.p, K, dC3.p, M, 1.0, 1.0, dS.p, nslab, &ex);
      if ( r2 < 0 ) rc = -r2;
   }
   *used = r2 == 1 ? 1 : 0;
   *maxdiff = 0.0; *nrepro = 0;
   unsigned long long h[2] = {0, 0};
   if ( rc == HS_OK && r2 == 1 )
   {
      if ( hipMemset(dn, 0, 2 * sizeof(unsigned long long)) != hipSuccess ) rc = HS_ERR_HIP;
      hipLaunchKernelGGL(k_unit_lowdiff, dim3(1024), dim3(256), 0, 0, M, dC1.p, dC2.p, dn);
      if ( rc == HS_OK && hipMemcpy(h, dn, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
      memcpy(maxdiff, &h[0], sizeof(double));
      if ( rc == HS_OK && hipMemset(dn, 0, 2 * sizeof(unsigned long long)) != hipSuccess ) rc = HS_ERR_HIP;
      hipLaunchKernelGGL(k_unit_lowdiff, dim3(1024), dim3(256), 0, 0, M, dC2.p, dC3.p, dn);
      if ( rc == HS_OK && hipMemcpy(h, dn, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
      *nrepro = (long long) h[1];
   }
   if ( rc == HS_OK && reps > 0 && ms_tile != NULL && ms_gram != NULL )
   {
      hipEvent_t e0, e1;
      HS_HIP( hipEventCreate(&e0) ); HS_HIP( hipEventCreate(&e1) );
      for (int which = 0; which < 2 && rc == HS_OK; ++which)
      {
         for (int it = -2; it < reps && rc == HS_OK; ++it)
         {
            if ( it == 0 )
               (void) hipEventRecord(e0, 0);
            if ( which == 0 )
               rc = hs_dgemm(0, &g3);
            else if ( r2 == 1 )
            {
               const int r = hs_gram_try(0, M, K, dW.p, K, dC2.p, M, 1.0, 1.0, dS.p, nslab, &ex);
               if ( r < 0 ) rc = -r;
            }
         }
         (void) hipEventRecord(e1, 0);
         float t = 0.f;
         if ( rc == HS_OK && (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess) )
            rc = HS_ERR_HIP;
         *(which == 0 ? ms_tile : ms_gram) = (double) t / reps;
      }
      (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
   }
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess )
      rc = HS_ERR_HIP;
   (void) hipFree(dn);
   return rc;
}

/* how csrc/gram.hip cuts the Gram product of a shape: partial tiles per off-diagonal / diagonal tile, items, estimated time in units
 * of one off-diagonal tile over all of K */
extern "C" int hipsdp_gram_plan_info(int device, int M, long long K, int nslab, int* no, int* nd, int* nitems, double* span)
{
   HS_CALL( pick_device(device) );
   return hs_gram_plan_info(M, K, nslab, no, nd, nitems, span) ? HIPSDP_OK : HIPSDP_ERR_ARG;
}

/* One Gram product from the caller's operands through hs_gram_try with the instance of the Gram kernel (csrc/gram.hip) forced: mode 0
 * its 128 x 128 instance, 1 its wide instance, -1 chosen per shape.  W [M][ldw] (ldw >= K, the K first of every row are read),
 * Cio [M][M] in and out: lower triangle = alpha W W^T + beta Cio, the rest comes back as it went in.  nslab: slabs of M x M doubles
 * granted.  used[2]: 1 when the Gram kernel took the product (0: it declined, Cio is unchanged), and 1 when that was its wide instance */
extern "C" int hipsdp_gram_product_unit(int device, int mode, int M, long long K, const double* W, long long ldw, double alpha, double beta,
   double* Cio, int nslab, int* used)
{
   HS_CALL( pick_device(device) );
   if ( mode < -1 || mode > 1 || M < 1 || K < 1 || ldw < K || W == NULL || Cio == NULL || nslab < 1 || nslab > 64 || used == NULL )
      return HIPSDP_ERR_ARG;
   const long long MM = (long long) M * M;
   DevBuf dW, dC, dS;
   HS_CALL( dW.alloc((long long) M * ldw) ); HS_CALL( dC.alloc(MM) ); HS_CALL( dS.alloc((long long) nslab * MM) );
   HS_CALL( dW.up(W, (long long) M * ldw) ); HS_CALL( dC.up(Cio, MM) );
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, (long long) nslab * MM, 52ULL, dS.p);
   const int tg = hs_gram_taken();
   const int tw = hs_gram_instance_force(mode);
   const int r = hs_gram_try(0, M, K, dW.p, ldw, dC.p, M, alpha, beta, dS.p, nslab, NULL);
   int rc = r < 0 ? -r : HS_OK;
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   used[1] = hs_gram_instance_force(-1) - tw;
   used[0] = hs_gram_taken() - tg;
   HS_CALL( rc );
   HS_CALL( dC.down(Cio, MM) );
   return HIPSDP_OK;
}

/* test hook of the same choice for the calls that reach the Gram product through the assembly (hipsdp_schur_form_unit,
 * hipsdp_schur_identity_unit) or through hipsdp_gram_selfcheck: mode as above; returns how many products the wide instance has taken
 * so far */
extern "C" int hipsdp_gram_instance_force(int mode)
{
   return hs_gram_instance_force(mode);
}

/* host only: the plan csrc/gram.hip builds for instance inst (0: 128 x 128 tiles on 512 lists, 1: 256 x 256 on 256) of a shape with
 * nslab slabs granted; forced = 1 as a forced instance gets it.  info[4] = items, lists, partial tiles per off-diagonal / diagonal
 * tile; off[lists + 1] (513 ints are enough); the first cap items as six ints (ti, tj, k0, k1, slab, column half).  HIPSDP_ERR_ARG: no plan */
extern "C" int hipsdp_gram_plan_unit(int inst, int forced, int M, long long K, int nslab, int cap, int* items, int* off, int* info)
{
   if ( items == NULL || off == NULL || info == NULL || cap < 0 )
      return HIPSDP_ERR_ARG;
   return hs_gram_plan_host(inst, forced, M, K, nslab, cap, items, off, info) ? HIPSDP_OK : HIPSDP_ERR_ARG;
}

/* The cold start's first assembly on its own: Mx (m1 x m1, as the caller filled it) += the Gram matrix <A_i, A_j> of the host matrices
 * A[m1][n][n] on the lower tiles.  full_storage = 0: hs_pack_rows + hs_schur_W_identity_packed (2 P P^T - D D^T over the packed lower
 * triangles), 1: hs_schur_W_identity over the full rows.  ws_gbytes > 0: the Schur workspace under that budget (chunked when the
 * T, W pair does not fit), as the engine sizes it.  *flops: FP64 matrix-core flops the call executed. */
extern "C" int hipsdp_schur_identity_unit(int device, int m1, int n, const double* A, double ws_gbytes, int full_storage, double* Mx,
   double* flops)
{
   HS_CALL( pick_device(device) );
   if ( m1 <= 0 || n <= 0 || A == NULL || Mx == NULL )
      return HIPSDP_ERR_ARG;
   const long long n2 = (long long) n * n;
   const long long Lp = (((long long) n * (n + 1) / 2) + 1) & ~1LL;
   DevBuf dA, dP, dM;
   HS_CALL( dA.alloc(m1 * n2) ); HS_CALL( dM.alloc((long long) m1 * m1) );
   HS_CALL( dA.up(A, m1 * n2) ); HS_CALL( dM.up(Mx, (long long) m1 * m1) );
   if ( !full_storage )
      HS_CALL( dP.alloc(m1 * Lp) );
   hs_schur_ws w;
   int rc = hs_schur_ws_alloc(&w, m1, n2, ws_gbytes > 0.0 ? ws_gbytes : 40.0);
   if ( rc != HS_OK )
   {
      hs_schur_ws_free(&w);              /* (what a failed allocation left behind) */
      return rc;
   }
   const double before = hs_mfma_flops_total();
   if ( full_storage )
      rc = hs_schur_W_identity(0, m1, n, dA.p, dM.p, &w);
   else
   {
      rc = hs_pack_rows(0, m1, n, Lp, dA.p, dP.p);
      if ( rc == HS_OK ) rc = hs_schur_W_identity_packed(0, m1, n, dP.p, Lp, dM.p, &w);
   }
   if ( flops != NULL )
      *flops = hs_mfma_flops_total() - before;
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   hs_schur_ws_free(&w);
   HS_CALL( rc );
   HS_CALL( dM.down(Mx, (long long) m1 * m1) );
   return HIPSDP_OK;
}

extern "C" int hipsdp_schur_dense(int device, int m1, int n, const double* A, const double* X, const double* Zinv, double* Mx,
   double ws_gbytes)
{
   /* ws_gbytes > 0: the chunked U formulation with that budget; ws_gbytes <= 0: the W formulation (needs chol X and the
    * inverse Cholesky factor of Z, both formed here on the device from X and Zinv^-1... the caller passes Zinv, so Z^-1 = G^T G
    * is obtained from the Cholesky factor of Zinv: Zinv = C C^T  ->  G = C^T is upper; to stay with lower factors the W
    * path is exercised through hipsdp_schur_w below) */
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   DevBuf dA, dX, dZ, dM;
   HS_CALL( dA.alloc(m1 * n2) ); HS_CALL( dX.alloc(n2) ); HS_CALL( dZ.alloc(n2) ); HS_CALL( dM.alloc((long long) m1 * m1) );
   HS_CALL( dA.up(A, m1 * n2) ); HS_CALL( dX.up(X, n2) ); HS_CALL( dZ.up(Zinv, n2) );
   hs_schur_ws w;
   HS_CALL( hs_schur_ws_alloc(&w, m1, n2, ws_gbytes > 0.0 ? ws_gbytes : 1e9) );
   if ( ws_gbytes > 0.0 && w.chunk_cols > 1 )
   {
      /* allow chunks smaller than the 128 granularity of the engine so that tiny tests exercise the chunk loop */
      long long cols = (long long) (ws_gbytes * 1e9 / (16.0 * (double) n2));
      if ( cols < 1 ) cols = 1;
      if ( cols < w.chunk_cols ) w.chunk_cols = cols;
   }
   HS_CALL( hs_fill(0, dM.p, (long long) m1 * m1, 0.0) );
   int rc = hs_schur_U(0, m1, n, dA.p, dX.p, dZ.p, dM.p, &w, 0, m1);
   if ( rc == HS_OK ) rc = hs_mirror_lower(0, dM.p, m1, m1);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   hs_schur_ws_free(&w);
   HS_CALL( rc );
   HS_CALL( dM.down(Mx, (long long) m1 * m1) );
   return HIPSDP_OK;
}

/* time of the Schur work ONE rank of an nranks-way sharded assembly does (row chunks or a column slice, + mirror), on synthetic operands
 * generated in HBM: lets the per-rank cost at 2/4/8 ranks be measured on a one-GPU machine (tests/devtools/shard_time.py) */
extern "C" int hipsdp_schur_shard_time(int device, int m1, int n, int nranks, int rank, int by_columns, int reps, double ws_gbytes,
   double* ms)
{
   HS_CALL( pick_device(device) );
   if ( m1 < 1 || n < 1 || nranks < 1 || rank < 0 || rank >= nranks || reps < 1 || ms == NULL )
      return HIPSDP_ERR_ARG;
   const long long n2 = (long long) n * n;
   DevBuf dA, dX, dZ, dM;
   HS_CALL( dA.alloc(m1 * n2) ); HS_CALL( dX.alloc(n2) ); HS_CALL( dZ.alloc(n2) ); HS_CALL( dM.alloc((long long) (m1 + 32) * m1) );
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, m1 * n2, 11ULL, dA.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, n2, 23ULL, dX.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, n2, 37ULL, dZ.p);
   hs_schur_ws w;
   int c, b1, b2, c0 = 0, cw = 0;
   hs_shard_rows(m1, nranks, rank, &c, &b1, &b2);
   hs_shard_cols(m1, n, nranks, rank, &c0, &cw);
   HS_CALL( hs_schur_ws_alloc(&w, m1, by_columns ? (long long) n * (cw > 0 ? cw : 1) : n2, ws_gbytes > 0.0 ? ws_gbytes : 40.0) );
   hipEvent_t e0, e1;
   HS_HIP( hipEventCreate(&e0) ); HS_HIP( hipEventCreate(&e1) );
   int rc = HS_OK;
   for (int it = 0; it <= reps && rc == HS_OK; ++it)
   {
      if ( it == 1 )
         rc = hipEventRecord(e0, 0) == hipSuccess ? HS_OK : HS_ERR_HIP;        /* iteration 0 is the warm-up */
      if ( rc == HS_OK ) rc = hs_fill(0, dM.p, (long long) m1 * m1, 0.0);
      if ( by_columns )
      {
         if ( rc == HS_OK ) rc = hs_schur_Wcols(0, m1, n, dA.p, dX.p, dZ.p, dM.p, &w, c0, cw);
         if ( rc == HS_OK ) rc = hs_mirror_lower(0, dM.p, m1, m1);
      }
      else
      {
         if ( rc == HS_OK ) rc = hs_schur_Urows(0, m1, n, dA.p, dX.p, dZ.p, dM.p, &w, b1, b1 + c);
         if ( rc == HS_OK ) rc = hs_schur_Urows(0, m1, n, dA.p, dX.p, dZ.p, dM.p, &w, b2, b2 + c);
         if ( rc == HS_OK ) rc = hs_mirror_upper(0, dM.p, m1, m1);
      }
   }
   float t = 0.f;
   if ( rc == HS_OK && (hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess
         || hipEventElapsedTime(&t, e0, e1) != hipSuccess) )
      rc = HS_ERR_HIP;
   (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
   hs_schur_ws_free(&w);
   HS_CALL( rc );
   *ms = (double) t / (double) reps;
   return HIPSDP_OK;
}

/* the same for the variable-sharded assembly (hs_schur_Wvar): rank `rank` of `nranks` holds only its own rows of A - which is how
 * one rank's share of n = 4000, m = 8000 (128 GB of the 1 TB of A) fits one device.  The all-to-all runs through the measurement
 * transport (nothing but the rank's own piece moves); *a2a_bytes = what the rank would send (= receive) per assembly. */
extern "C" int hipsdp_comm_create_null(int rank, int nranks, void** comm);
extern "C" void hipsdp_comm_destroy(void* comm);
extern "C" int hipsdp_schur_var_share_time(int device, int m1, int n, int nranks, int rank, int cw, int reps, double* ms, double* a2a_bytes)
{
   HS_CALL( pick_device(device) );
   if ( m1 < 1 || n < 1 || nranks < 1 || nranks > 64 || rank < 0 || rank >= nranks || reps < 1 || ms == NULL || cw < 1 )
      return HIPSDP_ERR_ARG;
   if ( cw > n ) cw = n;
   const long long n2 = (long long) n * n;
   int r0, r1, q0, q1;
   hs_var_rows(m1, nranks, rank, &r0, &r1);
   hs_var_wrows(n, nranks, rank, &q0, &q1);
   DevBuf dA, dX, dZ, dM;
   HS_CALL( dA.alloc((long long) (r1 - r0 > 0 ? r1 - r0 : 1) * n2) ); HS_CALL( dX.alloc(n2) ); HS_CALL( dZ.alloc(n2) );
   HS_CALL( dM.alloc((long long) (m1 + 32) * m1) );
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, (long long) (r1 - r0) * n2, 11ULL, dA.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, n2, 23ULL, dX.p);
   hipLaunchKernelGGL(k_unit_fill, dim3(1024), dim3(256), 0, 0, n2, 37ULL, dZ.p);
   void* comm = NULL;
   HS_CALL( hipsdp_comm_create_null(rank, nranks, &comm) );
   hs_schur_ws w;
   int rc = hs_schur_ws_alloc_var(&w, m1, nranks, n, cw);
   hipEvent_t e0, e1;
   HS_HIP( hipEventCreate(&e0) ); HS_HIP( hipEventCreate(&e1) );
   for (int it = 0; it <= reps && rc == HS_OK; ++it)
   {
      if ( it == 1 )
         rc = hipEventRecord(e0, 0) == hipSuccess ? HS_OK : HS_ERR_HIP;        /* iteration 0 is the warm-up */
      if ( rc == HS_OK ) rc = hs_fill(0, dM.p, (long long) m1 * m1, 0.0);
      for (int c0 = 0; c0 < n && rc == HS_OK; c0 += cw)
         rc = hs_schur_Wvar(0, comm, rank, nranks, m1, n, dA.p - (long long) r0 * n2, dX.p, dZ.p, dM.p, &w, c0, n - c0 < cw ? n - c0 : cw);
      if ( rc == HS_OK ) rc = hs_mirror_lower(0, dM.p, m1, m1);
   }
   float t = 0.f;
   if ( rc == HS_OK && (hipEventRecord(e1, 0) != hipSuccess || hipEventSynchronize(e1) != hipSuccess
         || hipEventElapsedTime(&t, e0, e1) != hipSuccess) )
      rc = HS_ERR_HIP;
   (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
   hs_schur_ws_free(&w);
   hipsdp_comm_destroy(comm);
   HS_CALL( rc );
   *ms = (double) t / (double) reps;
   if ( a2a_bytes != NULL )
      *a2a_bytes = 8.0 * (double) (r1 - r0) * (double) (n - (q1 - q0)) * (double) n;
   return HIPSDP_OK;
}

/* W formulation: X and Z (not its inverse) are given; chol(X), chol(Z), inverse factor and the three GEMMs on the device */
extern "C" int hipsdp_schur_w(int device, int m1, int n, const double* A, const double* X, const double* Z, double* Mx)
{
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   DevBuf dA, dX, dZ, dG, dT, dM, dD;
   int* dflag = NULL;
   HS_CALL( dA.alloc(m1 * n2) ); HS_CALL( dX.alloc(n2) ); HS_CALL( dZ.alloc(n2) ); HS_CALL( dG.alloc(n2) ); HS_CALL( dT.alloc(n2) );
   HS_CALL( dM.alloc((long long) m1 * m1) ); HS_CALL( dD.alloc(hs_potrf_dinv_len(n)) );
   HS_HIP( hipMalloc((void**) &dflag, sizeof(int)) );
   HS_HIP( hipMemset(dflag, 0, sizeof(int)) );
   HS_CALL( dA.up(A, m1 * n2) ); HS_CALL( dX.up(X, n2) ); HS_CALL( dZ.up(Z, n2) );
   hs_schur_ws w;
   int rc = hs_schur_ws_alloc(&w, m1, n2, 1e9);
   if ( rc == HS_OK ) rc = hs_potrf(0, n, dZ.p, dD.p, dflag, NULL);
   if ( rc == HS_OK ) rc = hs_trtri(0, n, dZ.p, dD.p, dG.p, dT.p);
   if ( rc == HS_OK ) rc = hs_potrf(0, n, dX.p, dD.p, dflag, NULL);
   if ( rc == HS_OK ) rc = hs_zero_upper(0, dX.p, n);
   if ( rc == HS_OK ) rc = hs_fill(0, dM.p, (long long) m1 * m1, 0.0);
   if ( rc == HS_OK ) rc = hs_schur_W(0, m1, n, dA.p, dX.p, dG.p, dM.p, &w);
   if ( rc == HS_OK ) rc = hs_mirror_lower(0, dM.p, m1, m1);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   hs_schur_ws_free(&w);
   (void) hipFree(dflag);
   HS_CALL( rc );
   HS_CALL( dM.down(Mx, (long long) m1 * m1) );
   return HIPSDP_OK;
}

/* One dense block through ONE form of the assembly, from the caller's operands (nothing is factored here), every part of a sharded
 * form added up on this device in rank order.  The workspace of each form is sized as the engine sizes it: forms 0, 2, 3 for the
 * whole block (3: under ws_gbytes with the small chunks of hipsdp_schur_dense), 1 for its widest slice, 4 by hs_schur_ws_alloc_var.
 * used[3]: products the persistent kernels took during the call, of these the paired-band kernel's, and the Gram kernel's. */
extern "C" int hipsdp_schur_form_unit(int device, int form, int parts, int m1, int n, const double* A, const double* P, const double* Q,
   double ws_gbytes, double* Mx, int* used)
{
   HS_CALL( pick_device(device) );
   if ( form < 0 || form > 4 || m1 < 1 || n < 1 || A == NULL || P == NULL || Q == NULL || Mx == NULL || !(ws_gbytes == ws_gbytes) )
      return HIPSDP_ERR_ARG;
   if ( ((form == 1 || form == 2) && (parts < 1 || parts > 64)) || (form == 4 && parts < 1) )
      return HIPSDP_ERR_ARG;
   const long long n2 = (long long) n * n;
   if ( n2 > 2000000000LL || (long long) m1 * n > 2000000000LL || (long long) m1 * m1 > 2000000000LL )
      return HIPSDP_ERR_ARG;
   DevBuf dA, dP, dQ, dM;
   HS_CALL( dA.alloc(m1 * n2) ); HS_CALL( dP.alloc(n2) ); HS_CALL( dQ.alloc(n2) ); HS_CALL( dM.alloc((long long) m1 * m1) );
   HS_CALL( dA.up(A, m1 * n2) ); HS_CALL( dP.up(P, n2) ); HS_CALL( dQ.up(Q, n2) );
   hs_schur_ws w;
   void* comm = NULL;
   int rc = HS_OK;
   if ( form == 1 )
   {
      long long widest = 1;
      for (int g = 0; g < parts; ++g)
      {
         int c0, cw;
         hs_shard_cols(m1, n, parts, g, &c0, &cw);
         if ( (long long) n * cw > widest ) widest = (long long) n * cw;
      }
      rc = hs_schur_ws_alloc(&w, m1, widest, 40.0);
   }
   else if ( form == 4 )
   {
      if ( parts > n ) parts = n;
      rc = hipsdp_comm_create_null(0, 1, &comm);
      if ( rc != HS_OK )
         return rc;
      rc = hs_schur_ws_alloc_var(&w, m1, 1, n, parts);
   }
   else
   {
      rc = hs_schur_ws_alloc(&w, m1, n2, form == 3 && ws_gbytes > 0.0 ? ws_gbytes : 40.0);
      if ( rc == HS_OK && form == 3 && ws_gbytes > 0.0 && w.chunk_cols > 1 )
      {
         long long cols = (long long) (ws_gbytes * 1e9 / (16.0 * (double) n2));
         if ( cols < 1 ) cols = 1;
         if ( cols < w.chunk_cols ) w.chunk_cols = cols;
      }
   }
   const int t2 = hs_dgemm2_enable(1), t5 = hs_dgemm2_paired_taken(), tg = hs_gram_taken();
   if ( rc == HS_OK ) rc = hs_fill(0, dM.p, (long long) m1 * m1, 0.0);
   switch ( form )
   {
   case 0:
      if ( rc == HS_OK ) rc = hs_schur_W(0, m1, n, dA.p, dP.p, dQ.p, dM.p, &w);
      break;
   case 1:
      for (int g = 0; g < parts && rc == HS_OK; ++g)
      {
         int c0, cw;
         hs_shard_cols(m1, n, parts, g, &c0, &cw);
         rc = hs_schur_Wcols(0, m1, n, dA.p, dP.p, dQ.p, dM.p, &w, c0, cw);
      }
      break;
   case 2:
      for (int g = 0; g < parts && rc == HS_OK; ++g)
      {
         int c, b1, b2;
         hs_shard_rows(m1, parts, g, &c, &b1, &b2);
         rc = hs_schur_Urows(0, m1, n, dA.p, dP.p, dQ.p, dM.p, &w, b1, b1 + c);
         if ( rc == HS_OK ) rc = hs_schur_Urows(0, m1, n, dA.p, dP.p, dQ.p, dM.p, &w, b2, b2 + c);
      }
      break;
   case 3:
      if ( rc == HS_OK ) rc = hs_schur_U(0, m1, n, dA.p, dP.p, dQ.p, dM.p, &w, 0, m1);
      break;
   default:
      if ( rc == HS_OK ) rc = hs_schur_Wvar_all(0, NULL, comm, 0, 1, m1, n, dA.p, dP.p, dQ.p, dM.p, &w, parts, 0);
      break;
   }
   if ( rc == HS_OK ) rc = form == 2 ? hs_mirror_upper(0, dM.p, m1, m1) : hs_mirror_lower(0, dM.p, m1, m1);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   if ( used != NULL )
   {
      used[0] = hs_dgemm2_enable(1) - t2;
      used[1] = hs_dgemm2_paired_taken() - t5;
      used[2] = hs_gram_taken() - tg;
   }
   hs_schur_ws_free(&w);
   if ( comm != NULL )
      hipsdp_comm_destroy(comm);
   HS_CALL( rc );
   HS_CALL( dM.down(Mx, (long long) m1 * m1) );
   return HIPSDP_OK;
}

/* hs_schur_small alone on host operands: block k has ns[k] rows and m1 matrices A[k][m1][ns[k]^2]; outputs are copied back only when
 * the kernel took the shape (*taken = 1), so a refused shape leaves the caller's arrays as they were */
extern "C" int hipsdp_schur_small_unit(int device, int m1, int nblk, const int* ns, const double* const* A, const double* const* X,
   const double* const* Zinv, int q, const double* Dext, const double* x, const double* z, double* Mx, double* Lm, double* diagM, int* taken)
{
   HS_CALL( pick_device(device) );
   if ( m1 < 1 || m1 > 32768 || nblk < 1 || nblk > 64 || ns == NULL || A == NULL || X == NULL || Zinv == NULL || q < 0 || Mx == NULL
      || Lm == NULL || diagM == NULL || taken == NULL || (q > 0 && (Dext == NULL || x == NULL || z == NULL)) )
      return HIPSDP_ERR_ARG;
   for (int k = 0; k < nblk; ++k)
      if ( ns[k] < 1 || ns[k] > 4096 || A[k] == NULL || X[k] == NULL || Zinv[k] == NULL )
         return HIPSDP_ERR_ARG;
   const int m = m1 - 1;
   std::vector<DevBuf> dA(nblk), dX(nblk), dZ(nblk);
   std::vector<const double*> pA(nblk), pX(nblk), pZ(nblk);
   for (int k = 0; k < nblk; ++k)
   {
      const long long n2 = (long long) ns[k] * ns[k];
      HS_CALL( dA[k].alloc(m1 * n2) ); HS_CALL( dX[k].alloc(n2) ); HS_CALL( dZ[k].alloc(n2) );
      HS_CALL( dA[k].up(A[k], m1 * n2) ); HS_CALL( dX[k].up(X[k], n2) ); HS_CALL( dZ[k].up(Zinv[k], n2) );
      pA[k] = dA[k].p; pX[k] = dX[k].p; pZ[k] = dZ[k].p;
   }
   DevBuf dD, dx, dz, dM, dL, dg;
   HS_CALL( dD.alloc((long long) q * m1) ); HS_CALL( dx.alloc(q) ); HS_CALL( dz.alloc(q) );
   HS_CALL( dM.alloc((long long) m1 * m1) ); HS_CALL( dL.alloc((long long) m * m) ); HS_CALL( dg.alloc(m) );
   HS_CALL( dD.up(Dext, (long long) q * m1) ); HS_CALL( dx.up(x, q) ); HS_CALL( dz.up(z, q) );
   HS_CALL( dM.up(Mx, (long long) m1 * m1) ); HS_CALL( dL.up(Lm, (long long) m * m) ); HS_CALL( dg.up(diagM, m) );
   const int r = hs_schur_small(0, m1, nblk, ns, pA.data(), pX.data(), pZ.data(), q, q > 0 ? dD.p : NULL, q > 0 ? dx.p : NULL,
      q > 0 ? dz.p : NULL, dM.p, dL.p, dg.p);
   if ( r < 0 )
      return -r;
   HS_HIP( hipDeviceSynchronize() );
   *taken = r;
   HS_CALL( dM.down(Mx, (long long) m1 * m1) ); HS_CALL( dL.down(Lm, (long long) m * m) ); HS_CALL( dg.down(diagM, m) );
   return HIPSDP_OK;
}

extern "C" int hipsdp_potrf(int device, int n, double* A, int* fail)
{
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   DevBuf dA, dD;
   int* dflag = NULL;
   HS_CALL( dA.alloc(n2) ); HS_CALL( dD.alloc(hs_potrf_dinv_len(n)) );
   HS_HIP( hipMalloc((void**) &dflag, sizeof(int)) );
   HS_HIP( hipMemset(dflag, 0, sizeof(int)) );
   HS_CALL( dA.up(A, n2) );
   int rc = hs_potrf(0, n, dA.p, dD.p, dflag, NULL);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   int hflag = 0;
   if ( rc == HS_OK && hipMemcpy(&hflag, dflag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dflag);
   HS_CALL( rc );
   HS_CALL( dA.down(A, n2) );
   if ( fail != NULL ) *fail = hflag;
   return HIPSDP_OK;
}

int hs_potrf_force_v1(int on);

/* test entry: the blocked factorization in both forms (v1 = 1: diagonal kernel + panel GEMM + mask kernel + trailing GEMM per
 * block column; 0: one fused launch per block column), optionally in semidefinite mode (diag0 = the matrix diagonal, forced
 * pivots reported in regmask[n]); dinv: ceil(n / 64) * 4096 doubles (inverses of the diagonal blocks) */
extern "C" int hipsdp_potrf_ex(int device, int n, double* A, int psd, int v1, double* dinv, int* regmask, int* fail)
{
   HS_CALL( pick_device(device) );
   if ( n <= 0 ) return HIPSDP_ERR_ARG;
   const long long n2 = (long long) n * n;
   const long long nd = (long long) ((n + 63) / 64) * 4096;
   DevBuf dA, dD, dG;
   int* dint = NULL;
   HS_CALL( dA.alloc(n2) ); HS_CALL( dD.alloc(hs_potrf_dinv_len(n)) ); HS_CALL( dG.alloc(n) );
   HS_HIP( hipMalloc((void**) &dint, (size_t) (n + 1) * sizeof(int)) );
   HS_HIP( hipMemset(dint, 0, (size_t) (n + 1) * sizeof(int)) );
   HS_HIP( hipMemset(dD.p, 0, (size_t) nd * sizeof(double)) );
   HS_CALL( dA.up(A, n2) );
   std::vector<double> dg(n);
   for (int i = 0; i < n; ++i) dg[i] = A[(long long) i * n + i];
   HS_CALL( dG.up(dg.data(), n) );
   const int old = hs_potrf_force_v1(v1);
   int rc = hs_potrf_psd(0, n, dA.p, dD.p, dint, psd ? dG.p : NULL, psd ? dint + 1 : NULL, 0);
   (void) hs_potrf_force_v1(old);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   std::vector<int> hint(n + 1, 0);
   if ( rc == HS_OK && hipMemcpy(hint.data(), dint, (size_t) (n + 1) * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dint);
   HS_CALL( rc );
   HS_CALL( dA.down(A, n2) );
   if ( dinv != NULL ) HS_CALL( dD.down(dinv, nd) );
   if ( fail != NULL ) *fail = hint[0];
   if ( regmask != NULL )
      for (int i = 0; i < n; ++i) regmask[i] = hint[1 + i];
   return HIPSDP_OK;
}

extern "C" int hipsdp_potrs(int device, int n, const double* A, int nrhs, double* rhs)
{
   HS_CALL( pick_device(device) );
   if ( nrhs < 1 || nrhs > 4 ) return HIPSDP_ERR_ARG;
   const long long n2 = (long long) n * n;
   DevBuf dA, dD, dR;
   int* dflag = NULL;
   HS_CALL( dA.alloc(n2) ); HS_CALL( dD.alloc(hs_potrf_dinv_len(n)) ); HS_CALL( dR.alloc((long long) nrhs * n) );
   HS_HIP( hipMalloc((void**) &dflag, sizeof(int)) );
   HS_HIP( hipMemset(dflag, 0, sizeof(int)) );
   HS_CALL( dA.up(A, n2) ); HS_CALL( dR.up(rhs, (long long) nrhs * n) );
   /* the solve runs through the multi-workgroup kernels when the factor has at least 3 blocks (as in the engine) */
   int* dsync = NULL;
   int epoch = 0;
   HS_HIP( hipMalloc((void**) &dsync, (size_t) hs_trsv_sync_ws(n) * sizeof(int)) );
   HS_CALL( hs_trsv_sync_init(0, n, dsync, NULL) );
   int rc = hs_potrf(0, n, dA.p, dD.p, dflag, NULL);
   /* mode 7: forward + backward, every diagonal-block solve corrected once with the factor itself, as the engine runs them */
   if ( rc == HS_OK ) rc = hs_trsv_sync(0, n, dA.p, dD.p, nrhs, dR.p, n, 7, dsync, &epoch);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dsync);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   int hflag = 0;
   if ( rc == HS_OK && hipMemcpy(&hflag, dflag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dflag);
   HS_CALL( rc );
   HS_CALL( dR.down(rhs, (long long) nrhs * n) );
   return hflag == 0 ? HIPSDP_OK : HIPSDP_ERR_NUMERIC;
}

/* test entry: ONE factorization (psd = 0: hs_potrf; 1: hs_potrf_psd with diag0 = the matrix diagonal and a mask, as hipsdp_potrf_ex
 * sets it up), ONE workspace of hs_trsv_sync with one epoch counter, then ncalls solves one behind the other on that workspace, as
 * the engine issues them through a whole interior-point solve: call c takes nrhs[c] right-hand sides in mode[c], in place on slab c
 * of rhs (4 rows of n doubles per slab) */
extern "C" int hipsdp_potrs_seq(int device, int n, const double* A, int psd, int ncalls, const int* nrhs, const int* mode, double* rhs,
   int* regmask, int* fail)
{
   if ( n <= 0 || A == NULL || ncalls < 0 || (psd != 0 && psd != 1) || (ncalls > 0 && (nrhs == NULL || mode == NULL || rhs == NULL)) )
      return HIPSDP_ERR_ARG;
   for (int c = 0; c < ncalls; ++c)
      if ( nrhs[c] < 1 || nrhs[c] > 4 || (mode[c] != 3 && mode[c] != 5 && mode[c] != 6 && mode[c] != 7) )
         return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   const long long nr = (long long) ncalls * 4 * n;
   DevBuf dA, dD, dG, dR;
   int* dint = NULL;
   int* dsync = NULL;
   HS_CALL( dA.alloc(n2) ); HS_CALL( dD.alloc(hs_potrf_dinv_len(n)) ); HS_CALL( dG.alloc(n) ); HS_CALL( dR.alloc(nr) );
   HS_CALL( dA.up(A, n2) ); HS_CALL( dR.up(rhs, nr) );
   std::vector<double> dg(n);
   for (int i = 0; i < n; ++i) dg[i] = A[(long long) i * n + i];
   HS_CALL( dG.up(dg.data(), n) );
   std::vector<int> hint(n + 1, 0);
   int gaveup = 0;                   /* the error word of the workspace: a block of a solve left without its predecessors' entries */
   int epoch = 0;
   int rc = HS_OK;
   /* from here on every path goes through the two hipFree below */
   if ( hipMalloc((void**) &dint, (size_t) (n + 1) * sizeof(int)) != hipSuccess
         || hipMalloc((void**) &dsync, (size_t) hs_trsv_sync_ws(n) * sizeof(int)) != hipSuccess
         || hipMemset(dint, 0, (size_t) (n + 1) * sizeof(int)) != hipSuccess )
      rc = HS_ERR_HIP;
   if ( rc == HS_OK ) rc = hs_trsv_sync_init(0, n, dsync, &epoch);
   if ( rc == HS_OK ) rc = hs_potrf_psd(0, n, dA.p, dD.p, dint, psd ? dG.p : NULL, psd ? dint + 1 : NULL, 0);
   for (int c = 0; c < ncalls && rc == HS_OK; ++c)
      rc = hs_trsv_sync(0, n, dA.p, dD.p, nrhs[c], dR.p + (long long) c * 4 * n, n, mode[c], dsync, &epoch);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   if ( rc == HS_OK && hipMemcpy(hint.data(), dint, (size_t) (n + 1) * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   if ( rc == HS_OK && hipMemcpy(&gaveup, dsync, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   if ( rc == HS_OK ) rc = dR.down(rhs, nr);
   (void) hipFree(dsync);
   (void) hipFree(dint);
   HS_CALL( rc );
   if ( fail != NULL ) *fail = hint[0];
   if ( regmask != NULL )
      for (int i = 0; i < n; ++i) regmask[i] = psd ? hint[1 + i] : 0;
   return gaveup == 0 ? HIPSDP_OK : HIPSDP_ERR_NUMERIC;
}

/* test entry: the fused single-block factorization of base + alpha * dir (n <= 64) with all its outputs, through hs_potrf_small_ext
 * (pair = 0) or - two problems of n rows laid one behind the other in every array - through hs_potrf_small_ext_pair (pair = 1).  L, Mout,
 * Linv, Gram: n x n per problem, dinv: 4096 per problem, flag: one word per problem, cleared before the launch; dir, Mout, Linv and Gram
 * may be NULL, Gram is written only when want_gram = 1 (n <= 32) */
extern "C" int hipsdp_potrf_small_unit(int device, int n, int pair, const double* base, const double* dir, double alpha, int set_flag,
   int want_gram, double* L, double* dinv, double* Mout, double* Linv, double* Gram, int* flag)
{
   if ( n < 1 || n > 64 || (pair != 0 && pair != 1) || base == NULL || L == NULL || dinv == NULL || flag == NULL
         || (set_flag != 0 && set_flag != 1) || (want_gram != 0 && want_gram != 1) || (want_gram && (n > 32 || Gram == NULL)) )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const int np = pair ? 2 : 1;
   const long long n2 = (long long) n * n;
   DevBuf dB, dR, dL, dD, dM, dI, dG;
   int* dflag = NULL;
   HS_CALL( dB.alloc(np * n2) ); HS_CALL( dR.alloc(np * n2) ); HS_CALL( dL.alloc(np * n2) ); HS_CALL( dD.alloc(np * 4096) );
   HS_CALL( dM.alloc(np * n2) ); HS_CALL( dI.alloc(np * n2) ); HS_CALL( dG.alloc(np * n2) );
   HS_HIP( hipMalloc((void**) &dflag, 2 * sizeof(int)) );
   HS_HIP( hipMemset(dflag, 0, 2 * sizeof(int)) );
   /* every output starts as NaN: what the kernel does not write shows */
   HS_HIP( hipMemset(dL.p, 0xFF, (size_t) (np * n2) * sizeof(double)) ); HS_HIP( hipMemset(dD.p, 0xFF, (size_t) (np * 4096) * sizeof(double)) );
   HS_HIP( hipMemset(dM.p, 0xFF, (size_t) (np * n2) * sizeof(double)) ); HS_HIP( hipMemset(dI.p, 0xFF, (size_t) (np * n2) * sizeof(double)) );
   HS_HIP( hipMemset(dG.p, 0xFF, (size_t) (np * n2) * sizeof(double)) );
   HS_CALL( dB.up(base, np * n2) );
   if ( dir != NULL ) HS_CALL( dR.up(dir, np * n2) );
   int rc;
   if ( !pair )
      rc = hs_potrf_small_ext(0, n, dL.p, dD.p, dflag, dB.p, dir != NULL ? dR.p : NULL, alpha, Mout != NULL ? dM.p : NULL,
         Linv != NULL ? dI.p : NULL, want_gram ? dG.p : NULL, set_flag);
   else
   {
      double* pL[2] = {dL.p, dL.p + n2};
      double* pD[2] = {dD.p, dD.p + 4096};
      int* pF[2] = {dflag, dflag + 1};
      const double* pB[2] = {dB.p, dB.p + n2};
      const double* pR[2] = {dir != NULL ? dR.p : NULL, dir != NULL ? dR.p + n2 : NULL};
      double* pM[2] = {Mout != NULL ? dM.p : NULL, Mout != NULL ? dM.p + n2 : NULL};
      double* pI[2] = {Linv != NULL ? dI.p : NULL, Linv != NULL ? dI.p + n2 : NULL};
      double* pG[2] = {want_gram ? dG.p : NULL, want_gram ? dG.p + n2 : NULL};
      rc = hs_potrf_small_ext_pair(0, n, pL, pD, pF, pB, pR, alpha, pM, pI, pG, set_flag);
   }
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   int hflag[2] = {0, 0};
   if ( rc == HS_OK && hipMemcpy(hflag, dflag, 2 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dflag);
   HS_CALL( rc );
   HS_CALL( dL.down(L, np * n2) ); HS_CALL( dD.down(dinv, np * 4096) );
   if ( Mout != NULL ) HS_CALL( dM.down(Mout, np * n2) );
   if ( Linv != NULL ) HS_CALL( dI.down(Linv, np * n2) );
   if ( want_gram ) HS_CALL( dG.down(Gram, np * n2) );
   for (int k = 0; k < np; ++k) flag[k] = hflag[k];
   return HIPSDP_OK;
}

/* test entry: strict-mode factorization of two matrices of n rows (one behind the other in A), pair = 1 through hs_potrf_pair, 0 through
 * two calls of hs_potrf.  dinv: hs_potrf_dinv_len(n) doubles per matrix - the staging blocks included - zero where nothing is written;
 * fail[2]: each matrix's own flag */
extern "C" long long hipsdp_potrf_dinv_len(int n) { return hs_potrf_dinv_len(n); }
extern "C" int hipsdp_potrf_pair_unit(int device, int n, int pair, double* A, double* dinv, int* fail)
{
   if ( n < 1 || (pair != 0 && pair != 1) || A == NULL || dinv == NULL || fail == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   const long long nd = hs_potrf_dinv_len(n);
   DevBuf dA, dD;
   int* dflag = NULL;
   HS_CALL( dA.alloc(2 * n2) ); HS_CALL( dD.alloc(2 * nd) );
   HS_HIP( hipMalloc((void**) &dflag, 2 * sizeof(int)) );
   HS_HIP( hipMemset(dflag, 0, 2 * sizeof(int)) );
   HS_HIP( hipMemset(dD.p, 0, (size_t) (2 * nd) * sizeof(double)) );
   HS_CALL( dA.up(A, 2 * n2) );
   const hs_potrf_job jobs[2] = {{dA.p, dD.p, dflag}, {dA.p + n2, dD.p + nd, dflag + 1}};
   int rc;
   if ( pair )
      rc = hs_potrf_pair(0, n, jobs);
   else
   {
      rc = hs_potrf(0, n, jobs[0].A, jobs[0].dinv, jobs[0].flag, NULL);
      if ( rc == HS_OK ) rc = hs_potrf(0, n, jobs[1].A, jobs[1].dinv, jobs[1].flag, NULL);
   }
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   int hflag[2] = {0, 0};
   if ( rc == HS_OK && hipMemcpy(hflag, dflag, 2 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dflag);
   HS_CALL( rc );
   HS_CALL( dA.down(A, 2 * n2) ); HS_CALL( dD.down(dinv, 2 * nd) );
   fail[0] = hflag[0]; fail[1] = hflag[1];
   return HIPSDP_OK;
}

/* test entry: the trial iterates of a step.  io holds eight arrays of n x n, one behind the other: X, Z, dX, dZ, Xs, Zs, Lx, Lz (all of
 * them inputs, so that what a form leaves untouched shows; X, Z, Xs, Zs, Lx, Lz come back).  fused = 1: hs_trial_pair; 0: the launches
 * it replaces - first: hs_copy(Vs, V); then hs_scale_add(alpha, dV, 1.0, Vs, V) and hs_copy(L, V) - for X, then for Z */
extern "C" int hipsdp_trial_pair_unit(int device, int n, int fused, int first, double alpha, double* io)
{
   if ( n < 1 || (fused != 0 && fused != 1) || (first != 0 && first != 1) || io == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   DevBuf d;
   HS_CALL( d.alloc(8 * n2) );
   HS_CALL( d.up(io, 8 * n2) );
   double* X = d.p; double* Z = d.p + n2; double* dX = d.p + 2 * n2; double* dZ = d.p + 3 * n2;
   double* Xs = d.p + 4 * n2; double* Zs = d.p + 5 * n2; double* Lx = d.p + 6 * n2; double* Lz = d.p + 7 * n2;
   const hs_trial_job tj[2] = {{X, dX, Xs, Lx}, {Z, dZ, Zs, Lz}};
   int rc = HS_OK;
   if ( fused )
      rc = hs_trial_pair(0, n2, alpha, first, tj);
   else
      for (int k = 0; k < 2 && rc == HS_OK; ++k)
      {
         if ( first ) rc = hs_copy(0, tj[k].Vs, tj[k].V, n2);
         if ( rc == HS_OK ) rc = hs_scale_add(0, n2, alpha, tj[k].dV, 1.0, tj[k].Vs, tj[k].V);
         if ( rc == HS_OK ) rc = hs_copy(0, tj[k].L, tj[k].V, n2);
      }
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   HS_CALL( rc );
   HS_CALL( d.down(io, 8 * n2) );
   return HIPSDP_OK;
}

/* ---- test entries of the merged launches between two Schur assemblies (general path): fused = 1 the merged launch, 0 the launches it
 * replaces.  Outputs start as NaN on the device, so that what a form does not write shows */
namespace {
int nan_fill(DevBuf& d, long long n) { HS_HIP( hipMemset(d.p, 0xFF, (size_t) (n > 0 ? n : 1) * sizeof(double)) ); return HS_OK; }
long long packed_len(int n) { const long long t = (long long) n * (n + 1) / 2; return t + (t & 1); }
}

/* k_after_solve2 + hs_make_ext twice: rhs2[2 m], u1[m] -> u2[m], wt[m + 1], e2[m + 1] = [1; u2], e1[m + 1] = [0; u1] */
extern "C" int hipsdp_tail_after_solve2_unit(int device, int m, int fused, const double* rhs2, const double* u1, double* u2, double* wt,
   double* e2, double* e1)
{
   if ( m < 1 || (fused != 0 && fused != 1) || rhs2 == NULL || u1 == NULL || u2 == NULL || wt == NULL || e2 == NULL || e1 == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   DevBuf dR, dU1, dU2, dW, dE2, dE1;
   HS_CALL( dR.alloc(2 * m) ); HS_CALL( dU1.alloc(m) ); HS_CALL( dU2.alloc(m) ); HS_CALL( dW.alloc(m + 1) ); HS_CALL( dE2.alloc(m + 1) );
   HS_CALL( dE1.alloc(m + 1) );
   HS_CALL( nan_fill(dU2, m) ); HS_CALL( nan_fill(dW, m + 1) ); HS_CALL( nan_fill(dE2, m + 1) ); HS_CALL( nan_fill(dE1, m + 1) );
   HS_CALL( dR.up(rhs2, 2 * m) ); HS_CALL( dU1.up(u1, m) );
   int rc = hs_ipm_after_solve2(0, m, dR.p, dU2.p, dW.p, dU1.p, dE2.p, dE1.p, fused);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   HS_CALL( rc );
   HS_CALL( dU2.down(u2, m) ); HS_CALL( dW.down(wt, m + 1) ); HS_CALL( dE2.down(e2, m + 1) ); HS_CALL( dE1.down(e1, m + 1) );
   return HIPSDP_OK;
}

/* three hs_unpack_sym: pk[3][Lp] (Lp = n (n + 1) / 2 rounded up to even) -> out[3][n][n] */
extern "C" int hipsdp_tail_unpack3_unit(int device, int n, int fused, const double* pk, double* out)
{
   if ( n < 1 || (fused != 0 && fused != 1) || pk == NULL || out == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n, Lp = packed_len(n);
   DevBuf dP, dO;
   HS_CALL( dP.alloc(3 * Lp) ); HS_CALL( dO.alloc(3 * n2) ); HS_CALL( nan_fill(dO, 3 * n2) );
   HS_CALL( dP.up(pk, 3 * Lp) );
   int rc = HS_OK;
   if ( fused )
   {
      const double* p3[3] = {dP.p, dP.p + Lp, dP.p + 2 * Lp};
      double* o3[3] = {dO.p, dO.p + n2, dO.p + 2 * n2};
      rc = hs_unpack_sym3(0, n, 3, p3, o3);
   }
   else
      for (int k = 0; k < 3 && rc == HS_OK; ++k)
         rc = hs_unpack_sym(0, n, dP.p + k * Lp, 0.0, NULL, dO.p + k * n2);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   HS_CALL( rc );
   return dO.down(out, 3 * n2);
}

/* hs_unpack_sym into dZ + the engine's k_dz_combine: pk[Lp], P2[n][n], Rd[n][n], dtau, eta -> dZ[n][n] */
extern "C" int hipsdp_tail_dz_unit(int device, int n, int fused, const double* pk, const double* P2, const double* Rd, double dtau, double eta,
   double* dZ)
{
   if ( n < 1 || (fused != 0 && fused != 1) || pk == NULL || P2 == NULL || Rd == NULL || dZ == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n, Lp = packed_len(n);
   const int nsc = hs_ipm_sc_len(1);
   DevBuf dP, dP2, dR, dZd, dS;
   HS_CALL( dP.alloc(Lp) ); HS_CALL( dP2.alloc(n2) ); HS_CALL( dR.alloc(n2) ); HS_CALL( dZd.alloc(n2) ); HS_CALL( dS.alloc(nsc) );
   HS_CALL( nan_fill(dZd, n2) );
   std::vector<double> sc((size_t) nsc, 0.0);
   sc[hs_ipm_sc_dtau()] = dtau;
   HS_CALL( dS.up(sc.data(), nsc) ); HS_CALL( dP.up(pk, Lp) ); HS_CALL( dP2.up(P2, n2) ); HS_CALL( dR.up(Rd, n2) );
   int rc;
   if ( fused )
      rc = hs_unpack_dz_combine(0, n, dP.p, dP2.p, dS.p, hs_ipm_sc_dtau(), eta, dR.p, dZd.p);
   else
   {
      rc = hs_unpack_sym(0, n, dP.p, 0.0, NULL, dZd.p);
      if ( rc == HS_OK ) rc = hs_ipm_dz_combine(0, n2, dZd.p, dP2.p, dS.p, eta, dR.p);
   }
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   HS_CALL( rc );
   return dZd.down(dZ, n2);
}

/* hs_dirmat + hs_pack_weighted of its result: Zinv, X, GZ [n][n], s1 -> H[n][n], pk[Lp] (the padding entry, if any, is not written) */
extern "C" int hipsdp_tail_dirmat_unit(int device, int n, int fused, double s1, const double* Zinv, const double* X, const double* GZ, double* H,
   double* pk)
{
   if ( n < 1 || (fused != 0 && fused != 1) || Zinv == NULL || X == NULL || GZ == NULL || H == NULL || pk == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n, Lp = packed_len(n);
   DevBuf dZ, dX, dG, dH, dP;
   HS_CALL( dZ.alloc(n2) ); HS_CALL( dX.alloc(n2) ); HS_CALL( dG.alloc(n2) ); HS_CALL( dH.alloc(n2) ); HS_CALL( dP.alloc(Lp) );
   HS_CALL( nan_fill(dH, n2) ); HS_CALL( nan_fill(dP, Lp) );
   HS_CALL( dZ.up(Zinv, n2) ); HS_CALL( dX.up(X, n2) ); HS_CALL( dG.up(GZ, n2) );
   int rc;
   if ( fused )
      rc = hs_dirmat_pack(0, n, s1, dZ.p, dX.p, dG.p, dH.p, dP.p);
   else
   {
      rc = hs_dirmat(0, n, s1, dZ.p, dX.p, dG.p, dH.p);
      if ( rc == HS_OK ) rc = hs_pack_weighted(0, n, dH.p, dP.p);
   }
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   HS_CALL( rc );
   HS_CALL( dH.down(H, n2) );
   return dP.down(pk, Lp);
}

/* the scalars of a direction and its closing kernel for one block of n rows and m variables (hs_ipm_dir_tail, the engine's own function):
 * fused = 0: fill, the two stages of <B, H>, the dots over m, k_finish_dir as launches of their own; 1: first stage + one batch launch.
 * B, H [n][n]; rhs2, rp, b, u1, u2 [m]; par = eta, rg, sigmu, tau, kappa, etk; sc: the scalar block (hipsdp_tail_sc_len() doubles,
 * read and written); dy[m], dyt[m + 1] */
extern "C" int hipsdp_tail_sc_len(void) { return hs_ipm_sc_len(1); }
extern "C" int hipsdp_tail_dir_unit(int device, int m, int n, int fused, const double* B, const double* H, const double* rhs2, const double* rp,
   const double* b, const double* u1, const double* u2, const double* par, double* sc, double* dy, double* dyt)
{
   if ( m < 1 || n < 1 || (fused != 0 && fused != 1) || B == NULL || H == NULL || rhs2 == NULL || rp == NULL || b == NULL || u1 == NULL
         || u2 == NULL || par == NULL || sc == NULL || dy == NULL || dyt == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   const int nsc = hs_ipm_sc_len(1);
   DevBuf dB, dH, dR, dRp, db, dU1, dU2, dS, dY, dYt, dW;
   HS_CALL( dB.alloc(n2) ); HS_CALL( dH.alloc(n2) ); HS_CALL( dR.alloc(m) ); HS_CALL( dRp.alloc(m) ); HS_CALL( db.alloc(m) );
   HS_CALL( dU1.alloc(m) ); HS_CALL( dU2.alloc(m) ); HS_CALL( dS.alloc(nsc) ); HS_CALL( dY.alloc(m) ); HS_CALL( dYt.alloc(m + 1) );
   HS_CALL( dW.alloc(HS_RED_WS_DOUBLES) );
   HS_CALL( nan_fill(dY, m) ); HS_CALL( nan_fill(dYt, m + 1) ); HS_CALL( nan_fill(dW, HS_RED_WS_DOUBLES) );
   HS_CALL( dB.up(B, n2) ); HS_CALL( dH.up(H, n2) ); HS_CALL( dR.up(rhs2, m) ); HS_CALL( dRp.up(rp, m) ); HS_CALL( db.up(b, m) );
   HS_CALL( dU1.up(u1, m) ); HS_CALL( dU2.up(u2, m) ); HS_CALL( dS.up(sc, nsc) );
   const double* pB = dB.p; const double* pH = dH.p;
   const hs_dir_tail_args ta = {m, 0, 1, &n, &pB, &pH, NULL, NULL, dR.p, dRp.p, db.p, dU1.p, dU2.p, dY.p, dYt.p, dS.p, dW.p, NULL, NULL,
      par[0], par[1], par[2], par[3], par[4], par[5]};
   hs_red_batch_reset();
   int rc = hs_ipm_dir_tail(0, &ta, fused, 0);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   hs_red_batch_reset();
   HS_CALL( rc );
   HS_CALL( dS.down(sc, nsc) ); HS_CALL( dY.down(dy, m) );
   return dYt.down(dyt, m + 1);
}

/* the reductions of the solves with M and of the residual pass: inside one batch  out[0] = 0;  out[0] += <a0, a1>;  out[1] = <a2, a2>;
 * out[0] += <a0, a2>  (vectors of n^2 entries; several sums into one slot, slots of their own for the partial sums)  and
 * out[2] = <v0, v1> (m entries); fused = 0: hs_dot, 1: hs_dot_deferred.  a[3][n^2], v[2][m], out[3] */
extern "C" int hipsdp_tail_dots_unit(int device, int m, int n, int fused, const double* a, const double* v, double* out)
{
   if ( m < 1 || n < 1 || (fused != 0 && fused != 1) || a == NULL || v == NULL || out == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   DevBuf dA, dV, dO, dW;
   HS_CALL( dA.alloc(3 * n2) ); HS_CALL( dV.alloc(2 * m) ); HS_CALL( dO.alloc(3) ); HS_CALL( dW.alloc(HS_RED_WS_DOUBLES) );
   HS_CALL( nan_fill(dO, 3) ); HS_CALL( nan_fill(dW, HS_RED_WS_DOUBLES) );
   HS_CALL( dA.up(a, 3 * n2) ); HS_CALL( dV.up(v, 2 * m) );
   const double* a0 = dA.p; const double* a1 = dA.p + n2; const double* a2 = dA.p + 2 * n2;
   hs_red_batch_reset();
   hs_red_batch_begin(0);
   int rc = hs_fill_scalar(0, dO.p, 0.0);
   if ( fused )
   {
      if ( rc == HS_OK ) rc = hs_dot_deferred(0, n2, a0, a1, dO.p, 1, dW.p, 0);
      if ( rc == HS_OK ) rc = hs_dot_deferred(0, n2, a2, a2, dO.p + 1, 0, dW.p, 1);
      if ( rc == HS_OK ) rc = hs_dot_deferred(0, n2, a0, a2, dO.p, 1, dW.p, 2);
   }
   else
   {
      if ( rc == HS_OK ) rc = hs_dot(0, n2, a0, a1, dO.p, 1, dW.p);
      if ( rc == HS_OK ) rc = hs_dot(0, n2, a2, a2, dO.p + 1, 0, dW.p);
      if ( rc == HS_OK ) rc = hs_dot(0, n2, a0, a2, dO.p, 1, dW.p);
   }
   if ( rc == HS_OK ) rc = hs_dot(0, m, dV.p, dV.p + m, dO.p + 2, 0, dW.p);
   if ( rc == HS_OK ) rc = hs_red_batch_end();
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   hs_red_batch_reset();
   HS_CALL( rc );
   return dO.down(out, 3);
}

extern "C" int hipsdp_trtri(int device, int n, const double* A, double* Linv)
{
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   DevBuf dA, dD, dL, dT;
   int* dflag = NULL;
   HS_CALL( dA.alloc(n2) ); HS_CALL( dD.alloc(hs_potrf_dinv_len(n)) ); HS_CALL( dL.alloc(n2) ); HS_CALL( dT.alloc(n2) );
   HS_HIP( hipMalloc((void**) &dflag, sizeof(int)) );
   HS_HIP( hipMemset(dflag, 0, sizeof(int)) );
   HS_CALL( dA.up(A, n2) );
   int rc = hs_potrf(0, n, dA.p, dD.p, dflag, NULL);
   if ( rc == HS_OK ) rc = hs_trtri(0, n, dA.p, dD.p, dL.p, dT.p);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   int hflag = 0;
   if ( rc == HS_OK && hipMemcpy(&hflag, dflag, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dflag);
   HS_CALL( rc );
   HS_CALL( dL.down(Linv, n2) );
   return hflag == 0 ? HIPSDP_OK : HIPSDP_ERR_NUMERIC;
}

extern "C" int hipsdp_lambda_min(int device, int n, const double* W, int steps, double* theta, double* resid)
{
   HS_CALL( pick_device(device) );
   if ( n <= 0 ) return HIPSDP_ERR_ARG;
   if ( steps <= 0 ) steps = n < 250 ? n : 250;
   if ( steps > 250 ) steps = 250;
   const long long n2 = (long long) n * n;
   DevBuf dW, dR, dS;
   HS_CALL( dW.alloc(n2) ); HS_CALL( dR.alloc(8) ); HS_CALL( dS.alloc(hs_lanczos_ws(n, steps)) );
   HS_CALL( dW.up(W, n2) );
   HS_CALL( hs_lanczos_lmin(0, n, dW.p, steps, dR.p, dS.p) );
   HS_HIP( hipDeviceSynchronize() );
   double h[3];
   HS_CALL( dR.down(h, 3) );
   *theta = h[0];
   if ( resid != NULL ) *resid = h[1];
   return HIPSDP_OK;
}

/* hs_lanczos_lmin2 as the engine calls it where no solver's exchange vectors exist (rot = dsync = NULL): one or two matrices per
 * launch (W1 may be NULL) - k_lmin_tiny up to 16 rows, k_lanczos_fused up to 8192, a launch per step and matrix above; steps <= 0:
 * min(n, 250).  theta[2], resid[2], steps_done[2] = res[0 .. 2] of both matrices; the slot of a matrix that is not given keeps
 * NaN, NaN, -1. */
extern "C" int hipsdp_lambda_min2_unit(int device, int n, const double* W0, const double* W1, int steps, double* theta, double* resid,
   int* steps_done)
{
   HS_CALL( pick_device(device) );
   if ( n <= 0 || W0 == NULL || theta == NULL || resid == NULL || steps_done == NULL ) return HIPSDP_ERR_ARG;
   if ( steps <= 0 ) steps = n < 250 ? n : 250;
   if ( steps > 250 ) steps = 250;
   const long long n2 = (long long) n * n;
   DevBuf dW0, dW1, dR, dS0, dS1;
   double h[16];
   for (int i = 0; i < 16; ++i)
      h[i] = (i & 7) == 2 ? -1.0 : NAN;
   HS_CALL( dW0.alloc(n2) ); HS_CALL( dR.alloc(16) ); HS_CALL( dS0.alloc(hs_lanczos_ws(n, steps)) );
   HS_CALL( dW0.up(W0, n2) ); HS_CALL( dR.up(h, 16) );
   if ( W1 != NULL )
   {
      HS_CALL( dW1.alloc(n2) ); HS_CALL( dS1.alloc(hs_lanczos_ws(n, steps)) );
      HS_CALL( dW1.up(W1, n2) );
   }
   HS_CALL( hs_lanczos_lmin2(0, n, dW0.p, W1 != NULL ? dW1.p : NULL, steps, dR.p, dR.p + 8, dS0.p, dS1.p, NULL, NULL, 0) );
   HS_HIP( hipDeviceSynchronize() );
   HS_CALL( dR.down(h, 16) );
   for (int j = 0; j < 2; ++j)
   {
      theta[j] = h[8 * j];
      resid[j] = h[8 * j + 1];
      steps_done[j] = (int) h[8 * j + 2];
   }
   return HIPSDP_OK;
}

/* lambda_min(L D L^T) as the step-length code computes it for small blocks: theta and the residual bound, for the X-side and the
 * Z-side slot at once (same operands) */
extern "C" int hipsdp_lambda_min_scaled(int device, int n, const double* L, const double* D, int steps, double* theta, double* resid)
{
   HS_CALL( pick_device(device) );
   if ( n <= 0 || n > 64 || theta == NULL ) return HIPSDP_ERR_ARG;
   const long long n2 = (long long) n * n;
   DevBuf dL, dD, dR;
   HS_CALL( dL.alloc(n2) ); HS_CALL( dD.alloc(n2) ); HS_CALL( dR.alloc(16) );
   HS_CALL( dL.up(L, n2) ); HS_CALL( dD.up(D, n2) );
   /* through the launch the engine uses: all blocks of a size class at once (here: the same operands as two blocks, whose results
    * must agree bit for bit); n <= 16 exact (k_lmin_tiny), 17 .. 48 exact by reduction + multisection (k_lmin_exact_multi), above
    * Lanczos (k_lanczos_small) */
   DevBuf dR2;
   HS_CALL( dR2.alloc(16) );
   hs_step_jobs J;
   J.nblk = 2;
   for (int j = 0; j < 2; ++j)
   {
      J.n[j] = n; J.L0[j] = dL.p; J.D0[j] = dD.p; J.L1[j] = dL.p; J.D1[j] = dD.p;
      J.res0[j] = (j == 0 ? dR.p : dR2.p); J.res1[j] = (j == 0 ? dR.p : dR2.p) + 8;
   }
   HS_CALL( hs_steplen_small_multi(0, &J, steps > 0 ? steps : 24) );
   HS_HIP( hipDeviceSynchronize() );
   double h[16], h2[16];
   HS_CALL( dR.down(h, 16) );
   HS_CALL( dR2.down(h2, 16) );
   if ( h[0] != h2[0] || h[8] != h2[8] || h[1] != h2[1] || h[9] != h2[9] )
      return HIPSDP_ERR_NUMERIC;
   theta[0] = h[0]; theta[1] = h[8];
   if ( resid != NULL ) { resid[0] = h[1]; resid[1] = h[9]; }
   return HIPSDP_OK;
}

/* out[e] = sum_i coef[i] A[i][e] + sa add[e] (the pass A^T of the engine): 0 = the plain kernel (one thread walks all rows of its
 * entries), 1 = as the engine calls it for blocks with few entries (row chunks side by side + a second launch that adds them in
 * order, when hs_gemv_t_chunks says so: *chunks returns how many).  Two calls with the same operands give the same bits. */
extern "C" int hipsdp_pass_at_unit(int device, int R, long long E, const double* A, const double* coef, double sa, const double* add, int split,
   double* out, int* chunks)
{
   HS_CALL( pick_device(device) );
   if ( R <= 0 || E <= 0 || A == NULL || coef == NULL || out == NULL )
      return HIPSDP_ERR_ARG;
   DevBuf dA, dc, dadd, dout, dws;
   const int C = hs_gemv_t_chunks(R, E);
   if ( chunks != NULL )
      *chunks = C;
   HS_CALL( dA.alloc((long long) R * E) ); HS_CALL( dc.alloc(R) ); HS_CALL( dadd.alloc(E) ); HS_CALL( dout.alloc(E) );
   HS_CALL( dws.alloc((long long) (C > 0 ? C : 1) * E) );
   HS_CALL( dA.up(A, (long long) R * E) ); HS_CALL( dc.up(coef, R) );
   if ( add != NULL )
      HS_CALL( dadd.up(add, E) );
   if ( split )
      HS_CALL( hs_gemv_t_ws(0, R, E, dA.p, E, dc.p, sa, add != NULL ? dadd.p : NULL, dout.p, dws.p, (long long) (C > 0 ? C : 1) * E) );
   else
      HS_CALL( hs_gemv_t(0, R, E, dA.p, E, dc.p, sa, add != NULL ? dadd.p : NULL, dout.p) );
   HS_HIP( hipDeviceSynchronize() );
   HS_CALL( dout.down(out, E) );
   return HIPSDP_OK;
}

/* unit entry of the sparse block mode (csrc/sparse.hip): the Schur entries tr(A_i X A_j Zinv), i, j = 1 .. m, of matrices given as
 * triplets (var 1 .. m; an entry may name either triangle, and of several with the same (var, row, col) the last one counts - what
 * hs_sp_build makes of them), assembled by hs_sp_schur exactly as the engine calls it; Mx: (m + 1) x (m + 1), only the lower
 * triangle of the rows / columns 1 .. m is written (the rest is returned zero) */
static int schur_sparse_unit(int device, int n, int m, long long nnz, const int* var, const int* row, const int* col,
   const double* val, const double* X, const double* Zinv, double* Mx, bool ex, int kernel, int* took)
{
   HS_CALL( pick_device(device) );
   if ( n <= 0 || m <= 0 || nnz < 0 || X == NULL || Zinv == NULL || Mx == NULL )
      return HIPSDP_ERR_ARG;
   hs_sparse* sp = NULL;
   HS_CALL( hs_sp_build(&sp, n, m, nnz, var, row, col, val) );
   const long long n2 = (long long) n * n, mm = (long long) (m + 1) * (m + 1);
   DevBuf dX, dZ, dM;
   int rc = dX.alloc(n2);
   if ( rc == HS_OK ) rc = dZ.alloc(n2);
   if ( rc == HS_OK ) rc = dM.alloc(mm);
   if ( rc == HS_OK ) rc = dX.up(X, n2);
   if ( rc == HS_OK ) rc = dZ.up(Zinv, n2);
   if ( rc == HS_OK && hipMemset(dM.p, 0, (size_t) mm * sizeof(double)) != hipSuccess ) rc = HS_ERR_HIP;
   if ( rc == HS_OK ) rc = ex ? hs_sp_schur_ex(0, sp, dX.p, dZ.p, dM.p, kernel, took) : hs_sp_schur(0, sp, dX.p, dZ.p, dM.p);
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   if ( rc == HS_OK ) rc = dM.down(Mx, mm);
   hs_sp_free(sp);
   return rc;
}

extern "C" int hipsdp_schur_sparse_unit(int device, int n, int m, long long nnz, const int* var, const int* row, const int* col,
   const double* val, const double* X, const double* Zinv, double* Mx)
{
   return schur_sparse_unit(device, n, m, nnz, var, row, col, val, X, Zinv, Mx, false, -1, NULL);
}

/* the same with the kernel in the caller's hand: kernel = -1 the engine's rule, 0 k_sp_schur_t (one thread per pair), 1 k_sp_schur (one
 * wavefront per pair) on whatever input; *took (may be NULL): the kernel that ran */
extern "C" int hipsdp_schur_sparse_unit2(int device, int n, int m, long long nnz, const int* var, const int* row, const int* col,
   const double* val, const double* X, const double* Zinv, double* Mx, int kernel, int* took)
{
   if ( kernel < -1 || kernel > 1 )
      return HIPSDP_ERR_ARG;
   return schur_sparse_unit(device, n, m, nnz, var, row, col, val, X, Zinv, Mx, true, kernel, took);
}

/* the two passes over a block kept as nonzeros (csrc/sparse.hip) on a structure hs_sp_build makes of the caller's triplets:
 * outA[m] = <A_v, V>, v = 1 .. m, by hs_sp_apply_A (V[n][n] need not be symmetric: an off-diagonal entry reads V[r][c] and V[c][r]);
 * outAT[n][n] = base + sum_{v >= 1} coef[v] A_v by hs_sp_apply_AT on a copy of base (coef[m + 1]; coef[0] belongs to the constant
 * matrix and is not used).  Either pair (V, outA) / (coef, base, outAT) may be NULL: that half is skipped. */
extern "C" int hipsdp_sparse_ops_unit(int device, int n, int m, long long nnz, const int* var, const int* row, const int* col,
   const double* val, const double* V, const double* coef, const double* base, double* outA, double* outAT)
{
   HS_CALL( pick_device(device) );
   const bool doA = V != NULL && outA != NULL, doAT = coef != NULL && base != NULL && outAT != NULL;
   if ( n <= 0 || m <= 0 || nnz < 0 || (!doA && !doAT) )
      return HIPSDP_ERR_ARG;
   hs_sparse* sp = NULL;
   HS_CALL( hs_sp_build(&sp, n, m, nnz, var, row, col, val) );
   const long long n2 = (long long) n * n;
   DevBuf dV, dA, dc, dO;
   int rc = HS_OK;
   if ( doA )
   {
      rc = dV.alloc(n2);
      if ( rc == HS_OK ) rc = dA.alloc(m);
      if ( rc == HS_OK ) rc = dV.up(V, n2);
      if ( rc == HS_OK && hipMemset(dA.p, 0, (size_t) m * sizeof(double)) != hipSuccess ) rc = HS_ERR_HIP;
      if ( rc == HS_OK ) rc = hs_sp_apply_A(0, sp, dV.p, dA.p);
   }
   if ( rc == HS_OK && doAT )
   {
      rc = dc.alloc(m + 1);
      if ( rc == HS_OK ) rc = dO.alloc(n2);
      if ( rc == HS_OK ) rc = dc.up(coef, m + 1);
      if ( rc == HS_OK ) rc = dO.up(base, n2);
      if ( rc == HS_OK ) rc = hs_sp_apply_AT(0, sp, dc.p, dO.p);
   }
   if ( rc == HS_OK && hipDeviceSynchronize() != hipSuccess ) rc = HS_ERR_HIP;
   if ( rc == HS_OK && doA ) rc = dA.down(outA, m);
   if ( rc == HS_OK && doAT ) rc = dO.down(outAT, n2);
   hs_sp_free(sp);
   return rc;
}

/* ---- measured FP64 matrix peak of THIS device ("peak values are measured on the box"): every wavefront of a
 * chip-filling launch issues independent v_mfma_f64_16x16x4_f64 out of registers, nothing else - no memory traffic, no barriers -
 * for about `ms` milliseconds; *tflops = matrix flops / HIP-event time, *ghz = shader clocks / 100 MHz ticks inside the kernel (the
 * frequency the firmware grants under pure matrix load).  The roofline of bench.py is priced against the vendor figure AND this. */
typedef double up_v4d __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_mfma_peak(long long iters, double* __restrict__ sink, unsigned long long* __restrict__ clk)
{
   up_v4d a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0, a4 = a0, a5 = a0, a6 = a0, a7 = a0;
   const double x = 1.0 + 1e-9 * (double) threadIdx.x, y = 1.0 - 1e-9 * (double) threadIdx.x;
   unsigned long long c0 = 0, w0 = 0;
   if ( blockIdx.x == 0 && threadIdx.x == 0 )
   {
      c0 = clock64();
      w0 = wall_clock64();
   }
   /* (tied inline asm: with the builtin the register allocator moved the 64 accumulator registers between the two register files in
    * every trip - 128 copies around 8 matrix instructions, 60 % of the rate) */
#define UP_MFMA(acc, p, q) asm volatile("v_mfma_f64_16x16x4_f64 %0, %1, %2, %0" : "+v"(acc) : "v"(p), "v"(q))
   for (long long i = 0; i < iters; ++i)
   {
      UP_MFMA(a0, x, y); UP_MFMA(a1, y, x); UP_MFMA(a2, x, x); UP_MFMA(a3, y, y);
      UP_MFMA(a4, x, y); UP_MFMA(a5, y, x); UP_MFMA(a6, x, x); UP_MFMA(a7, y, y);
   }
   asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
   if ( blockIdx.x == 0 && threadIdx.x == 0 )
   {
      clk[0] = clock64() - c0;
      clk[1] = wall_clock64() - w0;
   }
   const up_v4d t = ((a0 + a1) + (a2 + a3)) + ((a4 + a5) + (a6 + a7));
   if ( t[0] + t[1] + t[2] + t[3] == 12345.678 )          /* (never: keeps the accumulators alive) */
      sink[threadIdx.x] = t[0];
}

extern "C" int hipsdp_mfma_peak(int device, double ms, double* tflops, double* ghz)
{
   HS_CALL( pick_device(device) );
   if ( !(ms > 0.0) ) ms = 20.0;
   DevBuf sink, clk;
   HS_CALL( sink.alloc(256) ); HS_CALL( clk.alloc(2) );
   const int cus = hs_device_cus() > 0 ? hs_device_cus() : 256;
   hipEvent_t e0, e1;
   HS_HIP( hipEventCreate(&e0) ); HS_HIP( hipEventCreate(&e1) );
   double best = 0.0, bestghz = 0.0;
   /* one, two and four workgroups of four wavefronts per compute unit: the best of them is the figure (which occupancy feeds the
    * matrix pipes best is the device's business) */
   for (int wgpc = 1; wgpc <= 4; wgpc *= 2)
   {
      const int grid = cus * wgpc;
      long long iters = 20000;
      float t = 0.f;
      for (int pass = 0; pass < 3; ++pass)                         /* pass 0 warms up and calibrates the trip count */
      {
         HS_HIP( hipEventRecord(e0, 0) );
         hipLaunchKernelGGL(k_mfma_peak, dim3(grid), dim3(256), 0, 0, iters, sink.p, reinterpret_cast<unsigned long long*>(clk.p));
         HS_HIP( hipEventRecord(e1, 0) );
         HS_HIP( hipEventSynchronize(e1) );
         HS_HIP( hipEventElapsedTime(&t, e0, e1) );
         if ( pass == 0 && t > 0.f )
         {
            iters = (long long) ((double) iters * ms / (double) t);
            if ( iters < 1000 ) iters = 1000;
         }
      }
      unsigned long long h[2] = {0, 0};
      HS_HIP( hipMemcpy(h, clk.p, sizeof(h), hipMemcpyDeviceToHost) );
      const double flops = (double) iters * 8.0 * 2048.0 * 4.0 * (double) grid;      /* 2048 flops per instruction, 4 wavefronts per workgroup */
      const double tf = flops / ((double) t * 1e-3) / 1e12;
      if ( tf > best )
      {
         best = tf;
         bestghz = h[1] > 0 ? (double) h[0] / ((double) h[1] * 10.0) : 0.0;      /* wall ticks are 10 ns */
      }
   }
   (void) hipEventDestroy(e0); (void) hipEventDestroy(e1);
   if ( tflops != NULL ) *tflops = best;
   if ( ghz != NULL ) *ghz = bestghz;
   return HIPSDP_OK;
}

/* the one-launch kernel's admission rule (csrc/solve1_body.h: hs_solve1_fits) and size class (csrc/solve1.hip: hs_solve1_class) for a
 * shape: the tests pick "the largest block that fits" and one row more from the rule itself */
extern "C" int hipsdp_solve1_fits(int m, int q, int nblk, const int* ns)
{
   if ( ns == NULL || nblk < 1 || nblk > HS_S1_MAXBLK )
      return 0;
   return hs_solve1_fits(m, q, nblk, ns);
}

extern "C" unsigned long long hipsdp_gram_gen_next(unsigned long long* counter)
{
   return counter != NULL ? hs_gen_next(counter) : 0;
}

extern "C" int hipsdp_gram_key_match_unit(int m_a, int nblk_a, const int* n_a, const int* form_a, const unsigned long long* gen_a,
   const long long* ws_a, int m_b, int nblk_b, const int* n_b, const int* form_b, const unsigned long long* gen_b, const long long* ws_b)
{
   hs_gram_key a, b;
   if ( n_a == NULL || form_a == NULL || gen_a == NULL || ws_a == NULL || n_b == NULL || form_b == NULL || gen_b == NULL || ws_b == NULL )
      return 0;
   (void) hs_gram_key_make(&a, m_a, nblk_a, n_a, form_a, gen_a, ws_a[0], ws_a[1], (int) ws_a[2]);
   (void) hs_gram_key_make(&b, m_b, nblk_b, n_b, form_b, gen_b, ws_b[0], ws_b[1], (int) ws_b[2]);
   return hs_gram_key_match(&a, &b);
}

extern "C" int hipsdp_solve1_class(int m, int nblk, const int* ns)
{
   if ( ns == NULL || nblk < 1 || nblk > HS_S1_MAXBLK )
      return -1;
   hs_solve1_args a;
   memset(&a, 0, sizeof(a));
   a.m = m; a.nblk = nblk;
   for (int k = 0; k < nblk; ++k)
      a.n[k] = ns[k];
   return hs_solve1_class(&a);
}

/* the batched full decomposition of hipsdp_eigencuts_all (csrc/eigi.hip: hs_syev_small_many) on `count` host matrices: matrix j has
 * ns[j] <= 128 rows and follows matrix j - 1 in A; lam receives the eigenvalues (ns[j] each, ascending), V the eigenvectors
 * (ns[j] x ns[j] each, row k = k-th eigenvector); *launches = kernel launches issued (at most 3 whatever count is) */
extern "C" int hipsdp_syev_many_unit(int device, int count, const int* ns, const double* A, double* lam, double* V, int* launches)
{
   HS_CALL( pick_device(device) );
   if ( count < 1 || ns == NULL || A == NULL || lam == NULL || V == NULL )
      return HIPSDP_ERR_ARG;
   long long tot = 0, wslen = 0;
   for (int j = 0; j < count; ++j)
   {
      if ( ns[j] < 1 || ns[j] > 128 )
         return HIPSDP_ERR_ARG;
      tot += (long long) ns[j] * ns[j];
      wslen += hs_syev_small_scratch(ns[j]);
   }
   DevBuf din, dws, dtab;
   HS_CALL( din.alloc(tot) ); HS_CALL( dws.alloc(wslen) );
   HS_CALL( din.up(A, tot) );
   /* jobs in the order of the size classes; where[j]: the job of matrix j */
   std::vector<hs_eig_job> jobs;
   std::vector<int> where((size_t) count, -1);
   std::vector<long long> aoff((size_t) count + 1, 0), woff((size_t) count + 1, 0);
   for (int j = 0; j < count; ++j)
   {
      aoff[j + 1] = aoff[j] + (long long) ns[j] * ns[j];
      woff[j + 1] = woff[j] + hs_syev_small_scratch(ns[j]);
   }
   for (int cls = 0; cls < 3; ++cls)
      for (int j = 0; j < count; ++j)
         if ( hs_syev_many_class(ns[j]) == cls )
         {
            hs_eig_job J;
            memset(&J, 0, sizeof(J));
            J.n = ns[j]; J.in = din.p + aoff[j]; J.ws = dws.p + woff[j];
            where[j] = (int) jobs.size();
            jobs.push_back(J);
         }
   HS_CALL( dtab.alloc((long long) ((jobs.size() * sizeof(hs_eig_job) + 7) / 8)) );
   HS_HIP( hipMemcpy(dtab.p, jobs.data(), jobs.size() * sizeof(hs_eig_job), hipMemcpyHostToDevice) );
   int nl = 0;
   HS_CALL( hs_syev_small_many(0, count, jobs.data(), reinterpret_cast<const hs_eig_job*>(dtab.p), &nl) );
   HS_HIP( hipDeviceSynchronize() );
   long long lo = 0;
   for (int j = 0; j < count; ++j)
   {
      const int n = ns[j];
      HS_HIP( hipMemcpy(lam + lo, dws.p + woff[j], (size_t) n * sizeof(double), hipMemcpyDeviceToHost) );
      HS_HIP( hipMemcpy(V + aoff[j], dws.p + woff[j] + hs_syev_many_vecpos(n), (size_t) n * n * sizeof(double), hipMemcpyDeviceToHost) );
      lo += n;
   }
   if ( launches != NULL )
      *launches = nl;
   return HIPSDP_OK;
}

/* k_sc_tpower alone (csrc/sparsecuts.hip) on `count` host matrices with given start vectors and largest eigenvalues: the slab of a
 * job holds maxeig in all ns[j] eigenvalue slots and v0 behind them, and the launch gets tol = -infinity, so every matrix takes part */
extern "C" int hipsdp_sparsecuts_unit(int device, int count, const int* ns, const double* Z, const double* v0, const double* maxeig,
   const int* sizes, const hipsdp_sparsecut_opts* opts, int* ncuts, double* eigvals, double* vecs, int* iters, int* flags)
{
   HS_CALL( pick_device(device) );
   if ( count < 1 || ns == NULL || Z == NULL || v0 == NULL || maxeig == NULL || sizes == NULL || opts == NULL || opts->maxcuts < 1
      || ncuts == NULL || eigvals == NULL || vecs == NULL || iters == NULL || flags == NULL )
      return HIPSDP_ERR_ARG;
   const int maxcuts = opts->maxcuts;
   std::vector<long long> zoff((size_t) count + 1, 0), woff((size_t) count + 1, 0), vecoff((size_t) count + 1, 0);
   int nmax = 0, smax = 1;
   for (int j = 0; j < count; ++j)
   {
      if ( ns[j] < 1 || ns[j] > HS_SC_MAXN || sizes[j] < 1 )
         return HIPSDP_ERR_ARG;
      zoff[j + 1] = zoff[j] + (long long) ns[j] * ns[j];
      woff[j + 1] = woff[j] + 2LL * ns[j];
      vecoff[j + 1] = vecoff[j] + (long long) maxcuts * ns[j];
      nmax = ns[j] > nmax ? ns[j] : nmax;
      if ( sizes[j] <= ns[j] && sizes[j] > smax )
         smax = sizes[j];
   }
   std::vector<double> slab((size_t) woff[count]);
   for (int j = 0; j < count; ++j)
      for (int i = 0; i < ns[j]; ++i)
      {
         slab[(size_t) woff[j] + i] = maxeig[j];
         slab[(size_t) woff[j] + ns[j] + i] = v0[woff[j] / 2 + i];
      }
   /* results: lmin | eigvals | vecs | ncuts, iters, flags (int) | supports (int) | sizes (int) */
   const long long slots = (long long) count * maxcuts;
   const long long ipos = count + slots + vecoff[count], spos = ipos + (3LL * count + 1) / 2, zpos = spos + (slots * smax + 1) / 2;
   const long long reslen = zpos + ((long long) count + 1) / 2;
   DevBuf dz, dws, dres, dtab;
   HS_CALL( dz.alloc(zoff[count]) ); HS_CALL( dws.alloc(woff[count]) ); HS_CALL( dres.alloc(reslen) );
   HS_CALL( dz.up(Z, zoff[count]) ); HS_CALL( dws.up(slab.data(), woff[count]) );
   HS_HIP( hipMemcpy(dres.p + zpos, sizes, (size_t) count * sizeof(int), hipMemcpyHostToDevice) );
   std::vector<hs_ec_job> jobs((size_t) count);
   for (int j = 0; j < count; ++j)
   {
      hs_ec_job& J = jobs[j];
      memset(&J, 0, sizeof(J));
      J.n = ns[j]; J.blk = j; J.form = HS_EC_DENSE; J.ld = (long long) ns[j] * ns[j];
      J.Z = dz.p + zoff[j]; J.ws = dws.p + woff[j]; J.vpos = ns[j]; J.vecoff = vecoff[j];
   }
   HS_CALL( dtab.alloc((long long) ((jobs.size() * sizeof(hs_ec_job) + 7) / 8)) );
   HS_HIP( hipMemcpy(dtab.p, jobs.data(), jobs.size() * sizeof(hs_ec_job), hipMemcpyHostToDevice) );
   hs_sc_out out;
   memset(&out, 0, sizeof(out));
   out.lmin = dres.p; out.eig = dres.p + count; out.vec = out.eig + slots;
   out.ncuts = reinterpret_cast<int*>(dres.p + ipos); out.iters = out.ncuts + count; out.flags = out.iters + count;
   out.sup = reinterpret_cast<int*>(dres.p + spos); out.smax = smax;
   hs_sc_par par;
   par.tol = -HUGE_VAL; par.feastol = opts->feastol;
   par.convtol = opts->convtol > 0.0 ? opts->convtol : 1e-6;
   par.maxcuts = maxcuts;
   par.maxit = opts->maxit > 0 ? opts->maxit : HIPSDP_SPARSECUTS_MAXIT;
   HS_CALL( hs_sc_tpower(0, count, nmax, reinterpret_cast<const hs_ec_job*>(dtab.p), reinterpret_cast<const int*>(dres.p + zpos), &par, &out) );
   HS_HIP( hipDeviceSynchronize() );
   std::vector<double> h((size_t) spos);
   HS_CALL( dres.down(h.data(), spos) );
   const int* hi = reinterpret_cast<const int*>(h.data() + ipos);
   for (int j = 0; j < count; ++j)
   {
      const int k = hi[j];
      if ( k < 0 || k > maxcuts )
         return HIPSDP_ERR_NUMERIC;
      ncuts[j] = k; iters[j] = hi[count + j]; flags[j] = hi[2 * count + j];
      memcpy(eigvals + (size_t) j * maxcuts, h.data() + count + (size_t) j * maxcuts, (size_t) k * sizeof(double));
      memcpy(vecs + vecoff[j], h.data() + count + slots + vecoff[j], (size_t) k * ns[j] * sizeof(double));
   }
   return HIPSDP_OK;
}

/* the Newton kernel of hipsdp_onevar_bounds alone (csrc/eigi.hip: k_onevar_small / k_onevar_mid) on host matrices: Z and one dense
 * A per job */
extern "C" int hipsdp_onevar_unit(int device, int n, int count, const double* Z, const double* A, const double* shift, const int* kind,
   const double* lb, const double* ub, double feastol, int maxevals, int* status, double* optval, double* lmin, double* grad, int* evals)
{
   HS_CALL( pick_device(device) );
   if ( n < 1 || n > HS_OV_MAXN || count < 1 || Z == NULL || A == NULL || shift == NULL || lb == NULL || ub == NULL || !(feastol >= 0.0)
      || status == NULL || optval == NULL )
      return HIPSDP_ERR_ARG;
   const long long n2 = (long long) n * n;
   std::vector<double> tab((size_t) count * HS_OV_TAB);
   for (int j = 0; j < count; ++j)
   {
      if ( kind != NULL && kind[j] != HIPSDP_ONEVAR_NEWTON && kind[j] != HIPSDP_ONEVAR_TWOPOINT )
         return HIPSDP_ERR_ARG;
      double* t = tab.data() + (size_t) j * HS_OV_TAB;
      t[0] = (double) j; t[1] = (double) (kind != NULL ? kind[j] : HIPSDP_ONEVAR_NEWTON); t[2] = lb[j]; t[3] = ub[j]; t[4] = shift[j];
   }
   DevBuf dz, da, dtab, dres, dslab;
   HS_CALL( dz.alloc(n2) ); HS_CALL( da.alloc(n2 * count) ); HS_CALL( dtab.alloc((long long) tab.size()) );
   HS_CALL( dres.alloc((long long) count * HS_OV_RES) );
   if ( hs_onevar_slab(n, count) > 0 )
      HS_CALL( dslab.alloc(hs_onevar_slab(n, count)) );
   HS_CALL( dz.up(Z, n2) ); HS_CALL( da.up(A, n2 * count) ); HS_CALL( dtab.up(tab.data(), (long long) tab.size()) );
   hs_ov_par P;
   memset(&P, 0, sizeof(P));
   P.n = n; P.count = count; P.maxevals = maxevals > 0 ? maxevals : 100;
   P.feastol = feastol; P.infinity = 1e20;
   P.Z = dz.p; P.A = da.p; P.tab = dtab.p; P.slab = dslab.p; P.res = dres.p;
   HS_CALL( hs_onevar_newton(0, &P) );
   HS_HIP( hipDeviceSynchronize() );
   std::vector<double> h((size_t) count * HS_OV_RES);
   HS_CALL( dres.down(h.data(), (long long) h.size()) );
   for (int j = 0; j < count; ++j)
   {
      const double* r = h.data() + (size_t) j * HS_OV_RES;
      if ( !(r[0] >= 0.0 && r[0] <= (double) HIPSDP_ONEVAR_GAVEUP) )
         return HIPSDP_ERR_NUMERIC;
      status[j] = (int) r[0];
      optval[j] = r[1];
      if ( lmin != NULL ) lmin[j] = r[2];
      if ( grad != NULL ) grad[j] = r[3];
      if ( evals != NULL ) evals[j] = (int) r[4];
   }
   return HIPSDP_OK;
}

/* the launches of hipsdp_onevar_bounds_all alone (csrc/eigi.hip: k_onevar_all_small / k_onevar_all_mid) on host matrices per job: every
 * job is a block of its own in the table of hs_ec_job - dense rows, row 0 (the constant matrix, never read here) and row 1 = A_j,
 * the job's variable index 0 - so the kernels take the path they take in the product call */
extern "C" int hipsdp_onevar_all_unit(int device, int count, const int* n, const double* Z, const double* A, const double* shift,
   const int* kind, const double* lb, const double* ub, double feastol, int maxevals, int mid_cap,
   int* status, double* optval, double* lmin, double* grad, int* evals)
{
   HS_CALL( pick_device(device) );
   if ( count < 1 || n == NULL || Z == NULL || A == NULL || shift == NULL || lb == NULL || ub == NULL || !(feastol >= 0.0) || mid_cap < 1
      || status == NULL || optval == NULL )
      return HIPSDP_ERR_ARG;
   std::vector<long long> off((size_t) count + 1, 0);
   std::vector<int> small, mid;
   for (int j = 0; j < count; ++j)
   {
      if ( n[j] < 1 || n[j] > HS_OV_MAXN )
         return HIPSDP_ERR_ARG;
      if ( kind != NULL && (kind[j] < 0 || kind[j] > HS_OV_KIND_EXTREMES) )
         return HIPSDP_ERR_ARG;
      off[j + 1] = off[j] + (long long) n[j] * n[j];
      (n[j] <= 64 ? small : mid).push_back(j);
   }
   std::stable_sort(mid.begin(), mid.end(), [&](int a, int c) { return n[a] > n[c]; });
   const long long tot = off[count];
   DevBuf dz, da, dtab, dres, dslab, djobs;
   HS_CALL( dz.alloc(tot) ); HS_CALL( da.alloc(2 * tot) ); HS_CALL( dtab.alloc((long long) count * HS_OVA_TAB) );
   HS_CALL( dres.alloc((long long) count * HS_OV_RES) );
   HS_CALL( djobs.alloc((long long) ((size_t) count * sizeof(hs_ec_job) + sizeof(double) - 1) / (long long) sizeof(double)) );
   /* the two rows of job j at da + 2 off[j] */
   std::vector<double> ha((size_t) (2 * tot), 0.0), tab((size_t) count * HS_OVA_TAB, 0.0);
   std::vector<hs_ec_job> jobs((size_t) count);
   for (int j = 0; j < count; ++j)
   {
      const long long n2 = (long long) n[j] * n[j];
      memcpy(ha.data() + 2 * off[j] + n2, A + off[j], (size_t) n2 * sizeof(double));
      memset(&jobs[j], 0, sizeof(hs_ec_job));
      jobs[j].n = n[j]; jobs[j].form = HS_EC_DENSE; jobs[j].blk = j; jobs[j].ld = n2;
      jobs[j].A = da.p + 2 * off[j];
      jobs[j].Z = dz.p + off[j];
   }
   int nsmall = 0, row = 0;
   for (int cls = 0; cls < 2; ++cls)
   {
      const std::vector<int>& list = cls == 0 ? small : mid;
      for (size_t k = 0; k < list.size(); ++k, ++row)
      {
         const int j = list[k];
         double* t = tab.data() + (size_t) row * HS_OVA_TAB;
         t[0] = 0.0; t[1] = (double) (kind != NULL ? kind[j] : HIPSDP_ONEVAR_NEWTON); t[2] = lb[j]; t[3] = ub[j]; t[4] = shift[j];
         t[5] = (double) j; t[6] = (double) j;
         if ( cls == 0 )
            nsmall = n[j] > nsmall ? n[j] : nsmall;
      }
   }
   const int nmid = mid.empty() ? 0 : n[mid[0]];
   const int grid = (int) mid.size() < mid_cap ? (int) mid.size() : mid_cap;
   if ( grid > 0 )
      HS_CALL( dslab.alloc(2LL * grid * nmid * nmid) );
   HS_CALL( dz.up(Z, tot) ); HS_CALL( da.up(ha.data(), 2 * tot) ); HS_CALL( dtab.up(tab.data(), (long long) tab.size()) );
   HS_HIP( hipMemcpy(djobs.p, jobs.data(), (size_t) count * sizeof(hs_ec_job), hipMemcpyHostToDevice) );
   hs_ova_par P;
   memset(&P, 0, sizeof(P));
   P.maxevals = maxevals > 0 ? maxevals : 100;
   P.feastol = feastol; P.infinity = 1e20;
   P.jobs = reinterpret_cast<const hs_ec_job*>(djobs.p); P.res = dres.p;
   P.count = (int) small.size(); P.grid = P.count; P.nmax = nsmall; P.tab = dtab.p;
   HS_CALL( hs_onevar_all(0, 0, &P) );
   P.count = (int) mid.size(); P.grid = grid; P.nmax = nmid; P.tab = dtab.p + (long long) small.size() * HS_OVA_TAB; P.slab = dslab.p;
   HS_CALL( hs_onevar_all(0, 1, &P) );
   HS_HIP( hipDeviceSynchronize() );
   std::vector<double> h((size_t) count * HS_OV_RES);
   HS_CALL( dres.down(h.data(), (long long) h.size()) );
   for (int j = 0; j < count; ++j)
   {
      const double* r = h.data() + (size_t) j * HS_OV_RES;
      if ( !(r[0] >= 0.0 && r[0] <= (double) HIPSDP_ONEVAR_DONE) )
         return HIPSDP_ERR_NUMERIC;
      status[j] = (int) r[0];
      optval[j] = r[1];
      if ( lmin != NULL ) lmin[j] = r[2];
      if ( grad != NULL ) grad[j] = r[3];
      if ( evals != NULL ) evals[j] = (int) r[4];
   }
   return HIPSDP_OK;
}

/* the rounds of hipsdp_onevar_bounds_large alone (csrc/onevar_large.hip: hs_onevar_large_chunk, the function the product call runs per
 * chunk) on host matrices per job: every job is a block of its own - dense rows, row 1 = A_j, variable index 0 - whose Z is uploaded
 * where k_ec_form_z would have put it */
extern "C" int hipsdp_onevar_large_unit(int device, int count, const int* n, const double* Z, const double* A, const double* shift,
   const int* kind, const double* lb, const double* ub, double feastol, int maxevals, int wg_cap, int chunk,
   int* status, double* optval, double* lmin, double* grad, int* evals, int* rounds)
{
   HS_CALL( pick_device(device) );
   if ( count < 1 || n == NULL || Z == NULL || A == NULL || shift == NULL || lb == NULL || ub == NULL || !(feastol >= 0.0)
      || status == NULL || optval == NULL )
      return HIPSDP_ERR_ARG;
   std::vector<long long> off((size_t) count + 1, 0);
   std::vector<int> list;
   for (int j = 0; j < count; ++j)
   {
      if ( n[j] < 2 || n[j] > HS_SYEVX_MAXN )
         return HIPSDP_ERR_ARG;
      if ( kind != NULL && (kind[j] < 0 || kind[j] > HS_OV_KIND_EXTREMES) )
         return HIPSDP_ERR_ARG;
      off[j + 1] = off[j] + (long long) n[j] * n[j];
   }
   if ( rounds != NULL )
      *rounds = 0;
   for (int j = 0; j < count; ++j)
   {
      const int kd = kind != NULL ? kind[j] : HIPSDP_ONEVAR_NEWTON;
      if ( hs_onevar_large_declined(kd, lb[j], ub[j], 1e20) )
      {
         status[j] = HIPSDP_ONEVAR_DECLINED; optval[j] = 0.0;
         if ( lmin != NULL ) lmin[j] = 0.0;
         if ( grad != NULL ) grad[j] = 0.0;
         if ( evals != NULL ) evals[j] = 0;
      }
      else
         list.push_back(j);
   }
   std::stable_sort(list.begin(), list.end(), [&](int a, int c) { return n[a] > n[c]; });
   const int total = (int) list.size();
   std::vector<long long> job_len((size_t) total);
   for (int k = 0; k < total; ++k)
      job_len[k] = hs_onevar_large_job_len(n[list[k]]);
   /* the dense rows of every job: row 0 (never read) and row 1 = A_j */
   DevBuf da;
   const long long tot = off[count];
   HS_CALL( da.alloc(2 * tot) );
   {
      std::vector<double> ha((size_t) (2 * tot), 0.0);
      for (int j = 0; j < count; ++j)
         memcpy(ha.data() + 2 * off[j] + (long long) n[j] * n[j], A + off[j], (size_t) n[j] * n[j] * sizeof(double));
      HS_CALL( da.up(ha.data(), 2 * tot) );
   }
   /* one chunk: jobs start .. end - 1 of the list (chunk <= 0: no budget, all jobs at once) */
   auto run = [&](int start, int end) -> int
   {
      const int cnt = end - start;
      std::vector<hs_ovl_row> rows((size_t) cnt);
      long long zlen = 0;
      std::vector<long long> zoff((size_t) cnt);
      for (int k = 0; k < cnt; ++k)
      {
         const int j = list[start + k];
         hs_ovl_row& r = rows[k];
         r.n = n[j]; r.var = 0; r.kind = kind != NULL ? kind[j] : HIPSDP_ONEVAR_NEWTON; r.entry = k;
         r.lb = lb[j]; r.ub = ub[j]; r.shift = shift[j];
         zoff[k] = zlen;
         zlen += hs_cut_mat_len(n[j]);
      }
      hs_ovl_layout L;
      std::vector<long long> wso, outo;
      hs_onevar_large_plan(0, cnt, rows.data(), zlen, &L, &wso, &outo);
      DevBuf dev, djobs;
      HS_CALL( dev.alloc(L.len.dev_len) );
      HS_CALL( djobs.alloc((long long) ((size_t) cnt * sizeof(hs_ec_job) + sizeof(double) - 1) / (long long) sizeof(double)) );
      std::vector<double> pin((size_t) L.len.pin_len, 0.0);
      std::vector<hs_ec_job> jobs((size_t) cnt);
      for (int k = 0; k < cnt; ++k)
      {
         const int j = list[start + k];
         const long long n2 = (long long) n[j] * n[j];
         memset(&jobs[k], 0, sizeof(hs_ec_job));
         jobs[k].n = n[j]; jobs[k].form = HS_EC_DENSE; jobs[k].blk = k; jobs[k].ld = n2;
         jobs[k].A = da.p + 2 * off[j];
         jobs[k].Z = dev.p + L.Z + zoff[k];
         HS_HIP( hipMemcpy(jobs[k].Z, Z + off[j], (size_t) n2 * sizeof(double), hipMemcpyHostToDevice) );
      }
      HS_HIP( hipMemcpy(djobs.p, jobs.data(), (size_t) cnt * sizeof(hs_ec_job), hipMemcpyHostToDevice) );
      hs_ovl_chunk c;
      memset(&c, 0, sizeof(c));
      c.m = 0; c.count = cnt; c.nz = 0; c.nzmax = 0; c.cap = wg_cap; c.maxevals = maxevals > 0 ? maxevals : 100;
      c.feastol = feastol; c.infinity = 1e20;
      c.u = NULL; c.rows = rows.data(); c.dblocks = reinterpret_cast<const hs_ec_job*>(djobs.p); c.dev = dev.p; c.pin = pin.data();
      long long launches = 0, readbacks = 0;
      int r = 0;
      HS_CALL( hs_onevar_large_chunk(0, &c, L, wso, outo, &launches, &readbacks, &r) );
      if ( rounds != NULL )
         *rounds += r;
      for (int k = 0; k < cnt; ++k)
      {
         const int j = list[start + k];
         const double* q = pin.data() + L.res + (long long) k * HS_OV_RES;
         if ( !(q[0] >= 0.0 && q[0] <= (double) HIPSDP_ONEVAR_DONE) )
            return HIPSDP_ERR_NUMERIC;
         status[j] = (int) q[0];
         optval[j] = q[1];
         if ( lmin != NULL ) lmin[j] = q[2];
         if ( grad != NULL ) grad[j] = q[3];
         if ( evals != NULL ) evals[j] = (int) q[4];
      }
      return HIPSDP_OK;
   };
   return hs_chunks_run(job_len.data(), total, 1LL << 40, chunk > 0 ? chunk : 0, run);
}

/* k_sc_tpower_large alone (csrc/sparsecuts_large.hip) on one host matrix: lmin is given as -1 with tol = -infinity, so the matrix
 * takes part */
extern "C" int hipsdp_sparsecuts_large_unit(int device, int n, const double* Z, const double* v0, double maxeig, int size,
   const hipsdp_sparsecut_opts* opts, int* ncuts, double* eigvals, double* vecs, int* iters, int* flags)
{
   HS_CALL( pick_device(device) );
   if ( n <= HS_SC_MAXN || n > HS_SCL_MAXN || Z == NULL || v0 == NULL || size < 1 || opts == NULL || opts->maxcuts < 1 || ncuts == NULL
      || eigvals == NULL || vecs == NULL || iters == NULL || flags == NULL )
      return HIPSDP_ERR_ARG;
   const int maxcuts = opts->maxcuts, smax = size <= n ? size : 1;
   const long long n2 = (long long) n * n, slots = maxcuts;
   /* input: lmin, maxeig | v0;  results: lmin | eigvals | vecs | ncuts, iters, flags (int) | supports (int) */
   const long long inlen = 2 + (((long long) n + 1) & ~1LL);
   const long long ipos = 1 + slots + slots * n, spos = ipos + 2, reslen = spos + (slots * smax + 1) / 2;
   std::vector<double> hin((size_t) inlen, 0.0);
   hin[0] = -1.0; hin[1] = maxeig;
   memcpy(hin.data() + 2, v0, (size_t) n * sizeof(double));
   DevBuf dz, dmt, din, dres;
   HS_CALL( dz.alloc(n2) ); HS_CALL( dmt.alloc(n2) ); HS_CALL( din.alloc(inlen) ); HS_CALL( dres.alloc(reslen) );
   HS_CALL( dz.up(Z, n2) ); HS_CALL( din.up(hin.data(), inlen) );
   hs_sc_out out;
   memset(&out, 0, sizeof(out));
   out.lmin = dres.p; out.eig = dres.p + 1; out.vec = out.eig + slots;
   out.ncuts = reinterpret_cast<int*>(dres.p + ipos); out.iters = out.ncuts + 1; out.flags = out.iters + 1;
   out.sup = reinterpret_cast<int*>(dres.p + spos); out.smax = smax;
   hs_sc_par par;
   par.tol = -HUGE_VAL; par.feastol = opts->feastol;
   par.convtol = opts->convtol > 0.0 ? opts->convtol : 1e-6;
   par.maxcuts = maxcuts;
   par.maxit = opts->maxit > 0 ? opts->maxit : HIPSDP_SPARSECUTS_MAXIT;
   HS_CALL( hs_scl_tpower(0, n, size, dz.p, din.p, din.p + 1, din.p + 2, dmt.p, &par, &out) );
   HS_HIP( hipDeviceSynchronize() );
   std::vector<double> h((size_t) spos);
   HS_CALL( dres.down(h.data(), spos) );
   const int* hi = reinterpret_cast<const int*>(h.data() + ipos);
   const int k = hi[0];
   if ( k < 0 || k > maxcuts )
      return HIPSDP_ERR_NUMERIC;
   *ncuts = k; *iters = hi[1]; *flags = hi[2];
   memcpy(eigvals, h.data() + 1, (size_t) k * sizeof(double));
   memcpy(vecs, h.data() + 1 + slots, (size_t) k * n * sizeof(double));
   return HIPSDP_OK;
}

/* the batched BELOW selection (hs_syevx_many_below, csrc/syevx.hip) on `count` host matrices of mixed sizes through the staging of
 * hipsdp_eigencuts_all_large: the symmetric matrix into the head of its workspace, the reflector arrays cleared by hs_ecl_clear, the
 * column launches with `cap` workgroups per matrix at most, the selection */
extern "C" int hipsdp_syevx_many_below_unit(int device, int count, const int* n, const double* A, double bound, int maxk, int cap, int* cnt,
   double* lam, double* V)
{
   HS_CALL( pick_device(device) );
   if ( count < 1 || n == NULL || A == NULL || maxk < 0 || maxk > HS_SYEVX_MAXK || cap < 1 || cap > 128 || cnt == NULL || lam == NULL
      || bound != bound )
      return HIPSDP_ERR_ARG;
   int nmax = 0;
   std::vector<long long> off((size_t) count + 1, 0), wso((size_t) count), outo((size_t) count);
   long long len = 0;
   for (int j = 0; j < count; ++j)
   {
      if ( n[j] < 2 || n[j] > HS_SYEVX_MAXN )
         return HIPSDP_ERR_ARG;
      nmax = n[j] > nmax ? n[j] : nmax;
      off[j + 1] = off[j] + (long long) n[j] * n[j];
      const hs_ecl_block B = hs_ecl_block_make((long long) hs_syevx_ws(n[j]), HS_SXB_OUT(n[j]));
      wso[j] = len + B.ws; outo[j] = len + B.out;
      len += B.len;
   }
   static_assert(sizeof(hs_sxm_job) == 6 * sizeof(double), "job table in doubles");
   DevBuf dev, djobs, dact;
   HS_CALL( dev.alloc(len) ); HS_CALL( djobs.alloc(6LL * count) ); HS_CALL( dact.alloc(((long long) count + 1) / 2) );
   std::vector<hs_sxm_job> jobs((size_t) count);
   std::vector<int> act((size_t) count, HS_SXM_ACTIVE);
   std::vector<double> sym;
   for (int j = 0; j < count; ++j)
   {
      HS_CALL( hs_syevx_many_below_job(n[j], dev.p + wso[j], dev.p + outo[j], &jobs[j]) );
      /* the matrix the single-matrix path builds from the triangle at [c n + i], i >= c */
      const int nn = n[j];
      const double* in = A + off[j];
      sym.resize((size_t) nn * nn);
      for (int i = 0; i < nn; ++i)
         for (int c = 0; c < nn; ++c)
            sym[(size_t) i * nn + c] = (c <= i) ? in[(size_t) c * nn + i] : in[(size_t) i * nn + c];
      HS_HIP( hipMemcpy(jobs[j].A, sym.data(), (size_t) nn * nn * sizeof(double), hipMemcpyHostToDevice) );
   }
   HS_HIP( hipMemcpy(djobs.p, jobs.data(), (size_t) count * sizeof(hs_sxm_job), hipMemcpyHostToDevice) );
   HS_HIP( hipMemcpy(dact.p, act.data(), (size_t) count * sizeof(int), hipMemcpyHostToDevice) );
   const hs_sxm_job* dj = reinterpret_cast<const hs_sxm_job*>(djobs.p);
   const int* da = reinterpret_cast<const int*>(dact.p);
   HS_CALL( hs_ecl_clear(0, count, dj) );
   HS_CALL( hs_syevx_many_cols(0, count, nmax, cap, dj, da) );
   HS_CALL( hs_syevx_many_below(0, count, nmax, bound, maxk, dj, da) );
   HS_HIP( hipDeviceSynchronize() );
   std::vector<double> h;
   long long voff = 0;
   for (int j = 0; j < count; ++j)
   {
      const long long ol = HS_SYEVX_OUT(n[j]);
      h.resize((size_t) ol);
      HS_HIP( hipMemcpy(h.data(), dev.p + outo[j], (size_t) (maxk > 0 ? ol : HS_SYEVX_OUT_VEC) * sizeof(double), hipMemcpyDeviceToHost) );
      const int k = maxk > 0 ? (int) h[0] : 0;
      if ( k < 0 || k > maxk )
         return HIPSDP_ERR_NUMERIC;
      cnt[j] = k;
      memcpy(lam + (size_t) j * maxk, h.data() + HS_SYEVX_OUT_LAM, (size_t) k * sizeof(double));
      if ( V != NULL )
         memcpy(V + voff, h.data() + HS_SYEVX_OUT_VEC, (size_t) k * n[j] * sizeof(double));
      voff += (long long) maxk * n[j];
   }
   return HIPSDP_OK;
}

extern "C" int hipsdp_tridiag_unit(int device, int n, const double* A, double* d, double* e, double* Vrefl, double* tau)
{
   HS_CALL( pick_device(device) );
   if ( n < 2 || n > HS_SYEVX_MAXN || A == NULL || d == NULL || e == NULL || Vrefl == NULL || tau == NULL )
      return HIPSDP_ERR_ARG;
   DevBuf din, dws;
   HS_CALL( din.alloc((long long) n * n) ); HS_CALL( dws.alloc((long long) hs_syevx_ws(n)) );
   HS_CALL( din.up(A, (long long) n * n) );
   HS_CALL( hs_syevx_tridiag_dev(0, n, din.p, dws.p) );
   HS_HIP( hipDeviceSynchronize() );
   double* pd; double* pe; double* pr; double* pt;
   hs_syevx_tridiag_view(n, dws.p, &pd, &pe, &pr, &pt);
   HS_HIP( hipMemcpy(d, pd, (size_t) n * sizeof(double), hipMemcpyDeviceToHost) );
   HS_HIP( hipMemcpy(e, pe, (size_t) n * sizeof(double), hipMemcpyDeviceToHost) );
   HS_HIP( hipMemcpy(tau, pt, (size_t) (n - 1) * sizeof(double), hipMemcpyDeviceToHost) );
   tau[n - 1] = 0.0;
   HS_HIP( hipMemcpy(Vrefl, pr, (size_t) n * n * sizeof(double), hipMemcpyDeviceToHost) );
   return HIPSDP_OK;
}

extern "C" int hipsdp_tvec_unit(int device, int n, const double* d, const double* e, double* lam, double* Z)
{
   HS_CALL( pick_device(device) );
   if ( n < 2 || n > HS_SYEVX_MAXN || d == NULL || e == NULL || lam == NULL || Z == NULL )
      return HIPSDP_ERR_ARG;
   DevBuf dws, dout;
   HS_CALL( dws.alloc((long long) hs_syevr_ws(n)) ); HS_CALL( dout.alloc(HS_SYEVR_OUT(n)) );
   double* pd; double* pe; double* pr; double* pt;
   hs_syevx_tridiag_view(n, dws.p, &pd, &pe, &pr, &pt);
   HS_HIP( hipMemset(pe, 0, (size_t) n * sizeof(double)) );
   HS_HIP( hipMemcpy(pd, d, (size_t) n * sizeof(double), hipMemcpyHostToDevice) );
   HS_HIP( hipMemcpy(pe, e, (size_t) (n - 1) * sizeof(double), hipMemcpyHostToDevice) );
   HS_CALL( hs_syevr_tvec_dev(0, n, 1, dout.p, dws.p) );
   HS_HIP( hipDeviceSynchronize() );
   HS_HIP( hipMemcpy(lam, dout.p, (size_t) n * sizeof(double), hipMemcpyDeviceToHost) );
   HS_HIP( hipMemcpy(Z, hs_syevr_tvec_view(n, dws.p), (size_t) n * n * sizeof(double), hipMemcpyDeviceToHost) );
   return HIPSDP_OK;
}

/* the batched full decomposition of hipsdp_psd_project_many_large on dense host matrices (hs_ppl_syevr_many_host, csrc/psd_large.hip) */
extern "C" int hipsdp_syevr_many_unit(int device, int count, const int* n, const double* A, int cap, double* lam, double* V)
{
   HS_CALL( pick_device(device) );
   return hs_ppl_syevr_many_host(device, count, n, A, cap, lam, V);
}

/* the device structure of a block kept as nonzeros, copied to the host as it stands (tests/test_gpu_sparse_master.py compares the
 * structure hipsdp_master_gather builds on the device with the one hs_sp_build makes from the node's triplets) */
extern "C" int hipsdp_sparse_dump_unit(hipsdp_solver* solver, int block, long long* counts, int* voff, int* vrow, int* vcol, double* vval,
   int* poff, int* prow, int* pcol, int* pvar, double* pval, int* foff, int* frow, int* fcol, double* fval, int* soff, int* srow, int* sent)
{
   const hs_sparse* sp = NULL;
   if ( solver == NULL || counts == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( hs_solver_sparse_block(solver, block, &sp) );
   if ( sp == NULL )
      return HIPSDP_ERR_ARG;
   counts[0] = sp->n; counts[1] = sp->m; counts[2] = sp->nnz; counts[3] = sp->npos; counts[4] = sp->nfull; counts[5] = sp->nslots;
   const size_t m1 = (size_t) sp->m + 1, nz = (size_t) sp->nnz, np = (size_t) sp->npos, nf = (size_t) sp->nfull, ns = (size_t) sp->nslots;
   struct { void* dst; const void* src; size_t bytes; } cp[] = {
      {voff, sp->voff, m1 * sizeof(int)}, {vrow, sp->vrow, nz * sizeof(int)}, {vcol, sp->vcol, nz * sizeof(int)}, {vval, sp->vval, nz * sizeof(double)},
      {poff, sp->poff, (np + 1) * sizeof(int)}, {prow, sp->prow, np * sizeof(int)}, {pcol, sp->pcol, np * sizeof(int)},
      {pvar, sp->pvar, nz * sizeof(int)}, {pval, sp->pval, nz * sizeof(double)},
      {foff, sp->foff, m1 * sizeof(int)}, {frow, sp->frow, nf * sizeof(int)}, {fcol, sp->fcol, nf * sizeof(int)}, {fval, sp->fval, nf * sizeof(double)},
      {soff, sp->soff, m1 * sizeof(int)}, {srow, sp->srow, ns * sizeof(int)}, {sent, sp->sent, (ns + 1) * sizeof(int)}};
   for (auto& c : cp)
      if ( c.dst != NULL && c.bytes > 0 )
         HS_HIP( hipMemcpy(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost) );
   return HIPSDP_OK;
}

/* k_cm_form_z alone on a loaded solver (hs_check_many_form_z, csrc/cut_calls.hip: the head of a chunk of hipsdp_check_y_many with every
 * matrix laid out as a plain n x n array), and the size of its groups */
extern "C" int hipsdp_form_z_many_unit(hipsdp_solver* solver, int count, const double* Y, double* Z, int* served, int* launches)
{
   return hs_check_many_form_z(solver, count, Y, Z, served, launches);
}

extern "C" int hipsdp_check_many_group(void)
{
   return HS_CM_G;
}

/* the coefficient launches of hipsdp_rounding_frame alone on host data of one block (hs_rf_coefs_host, csrc/rounding.hip): the kernels and
 * the routing rule of the call */
extern "C" int hipsdp_rounding_coefs_unit(int device, int n, int m, int form, const double* V, const double* A, long long nnz, const int* var,
   const int* row, const int* col, const double* val, double* out, int* route, int* slices)
{
   return hs_rf_coefs_host(device, n, m, form, V, A, nnz, var, row, col, val, out, route, slices);
}

/* the fan-out of hipsdp_solve_objectives alone (hs_objs_fanout, csrc/kernels.hip): the sources in device memory as the engine holds them
 * (the objectives in rows of m rounded up to even), the lanes filled with the guard word, one launch, the lanes back */
extern "C" int hipsdp_objs_fanout_unit(int device, int count, int m, int q, int nblk, const int* ns, const double* B, const double* b_own,
   int have_start, const double* y, const double* x, const double* z, const double* XZ, int gap, double guard, long long* lane_len,
   long long* offs, double* lanes, int* launches)
{
   if ( count < 1 || m < 0 || q < 0 || nblk < 0 || nblk > HS_S1_MAXBLK || (nblk > 0 && ns == NULL) || gap < 0 || (gap & 1) || lane_len == NULL
      || offs == NULL || (have_start != 0 && have_start != 1) )
      return HIPSDP_ERR_ARG;
   for (int k = 0; k < nblk; ++k)
      if ( ns[k] < 1 )
         return HIPSDP_ERR_ARG;
   const long long len = hs_objs_lane_layout(m, q, nblk, ns, gap, offs);
   *lane_len = len;
   if ( launches != NULL ) *launches = 0;
   if ( lanes == NULL )
      return HIPSDP_OK;
   if ( (m > 0 && (B == NULL || b_own == NULL)) || (have_start && ((m > 0 && y == NULL) || (q > 0 && (x == NULL || z == NULL)) || (nblk > 0 && XZ == NULL))) )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long mp = (m + 1) & ~1LL, qp = (q + 1) & ~1LL;
   /* the sources, each at an even offset: B (count rows of mp), b_own, y, x, z, X_0, Z_0, ... */
   std::vector<long long> so;
   long long tot = 0;
   auto put = [&](long long n) { so.push_back(tot); tot += (n + 1) & ~1LL; };
   put((long long) count * mp); put(m); put(m); put(q); put(q);
   for (int k = 0; k < nblk; ++k) { put((long long) ns[k] * ns[k]); put((long long) ns[k] * ns[k]); }
   std::vector<double> hs((size_t) tot + 2, 0.0);
   for (int j = 0; j < count; ++j)
      for (int i = 0; i < m; ++i)
         hs[(size_t) (so[0] + j * mp + i)] = B[(size_t) j * m + i];
   for (int i = 0; i < m; ++i) hs[(size_t) (so[1] + i)] = b_own[i];
   if ( have_start )
   {
      for (int i = 0; i < m; ++i) hs[(size_t) (so[2] + i)] = y[i];
      for (int i = 0; i < q; ++i) { hs[(size_t) (so[3] + i)] = x[i]; hs[(size_t) (so[4] + i)] = z[i]; }
      const double* p = XZ;
      for (int k = 0; k < 2 * nblk; ++k)
      {
         const long long n2 = (long long) ns[k / 2] * ns[k / 2];
         for (long long e = 0; e < n2; ++e) hs[(size_t) (so[5 + k] + e)] = p[e];
         p += n2;
      }
   }
   (void) qp;
   const long long nl = (long long) count + 1;
   DevBuf dS, dL;
   HS_CALL( dS.alloc(tot + 2) ); HS_CALL( dL.alloc(nl * len) );
   HS_CALL( dS.up(hs.data(), tot) );
   {
      std::vector<double> fill((size_t) (nl * len), guard);
      HS_CALL( dL.up(fill.data(), nl * len) );
   }
   hs_fan_plan plan;
   memset(&plan, 0, sizeof(plan));
   auto seg = [&](const double* own, const double* src, long long stride, long long dst, long long n) {
      if ( n <= 0 ) return;
      hs_fan_seg& S = plan.seg[plan.nseg++];
      S.src0 = own; S.src = src; S.stride = stride; S.dst = dst; S.len = n;
   };
   seg(dS.p + so[1], dS.p + so[0], mp, offs[0], m);
   if ( have_start )
   {
      seg(dS.p + so[2], dS.p + so[2], 0, offs[1], m);
      seg(dS.p + so[3], dS.p + so[3], 0, offs[2], q);
      seg(dS.p + so[4], dS.p + so[4], 0, offs[3], q);
      for (int k = 0; k < 2 * nblk; ++k)
         seg(dS.p + so[5 + k], dS.p + so[5 + k], 0, offs[4 + k], (long long) ns[k / 2] * ns[k / 2]);
   }
   if ( plan.nseg > 0 )
   {
      HS_CALL( hs_objs_fanout(0, &plan, dL.p, len, (int) nl) );
      if ( launches != NULL ) *launches = 1;
   }
   HS_HIP( hipDeviceSynchronize() );
   return dL.down(lanes, nl * len);
}

/* ---- test entries of the small-problem passes and of their recorded forms inside the single-workgroup batch kernel (kernels.hip: the
 * RB_* records of k_red_batch).  recorded = 0: the engine function with no batch open, the kernel gets its own launch; 1: the same call
 * between hs_red_batch_hold(0) and hs_red_batch_release().  *pending: records waiting just before the release - 0 when the call declined
 * (or recorded = 0).  Outputs start as NaN on the device, so that what an operation does not write shows. */
namespace {
struct RecScope
{
   int recorded;
   explicit RecScope(int r) : recorded(r) { hs_red_batch_reset(); if ( recorded ) hs_red_batch_hold(0); }
   int close(int rc, int* pending)
   {
      if ( pending != NULL ) *pending = hs_red_batch_pending();
      if ( recorded && rc == HS_OK ) rc = hs_red_batch_release();
      if ( hipDeviceSynchronize() != hipSuccess && rc == HS_OK ) rc = HS_ERR_HIP;
      hs_red_batch_reset();
      return rc;
   }
};
bool flag01(int v) { return v == 0 || v == 1; }
}

/* hs_dir_block_small: out = s1 Zinv - X - sym((c X R + E) Zinv), n x n each, E may be NULL.  n > HS_SMALL_N: the engine's HS_ERR_ARG */
extern "C" int hipsdp_small_dir_block_unit(int device, int n, double c, double s1, const double* X, const double* R, const double* E,
   const double* Zinv, int recorded, double* out, int* pending)
{
   if ( n < 1 || n > 4096 || !flag01(recorded) || X == NULL || R == NULL || Zinv == NULL || out == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n2 = (long long) n * n;
   DevBuf dX, dR, dE, dZ, dO;
   HS_CALL( dX.alloc(n2) ); HS_CALL( dR.alloc(n2) ); HS_CALL( dE.alloc(n2) ); HS_CALL( dZ.alloc(n2) ); HS_CALL( dO.alloc(n2) );
   HS_CALL( nan_fill(dO, n2) );
   HS_CALL( dX.up(X, n2) ); HS_CALL( dR.up(R, n2) ); HS_CALL( dZ.up(Zinv, n2) );
   if ( E != NULL ) HS_CALL( dE.up(E, n2) );
   RecScope sc(recorded);
   int rc = hs_dir_block_small(0, n, c, dX.p, dR.p, E != NULL ? dE.p : NULL, dZ.p, s1, dO.p);
   HS_CALL( sc.close(rc, pending) );
   return dO.down(out, n2);
}

/* hs_lp_rows_small: t_r = Dext[r, :] . v (Dext q x m1); mode 0: out1 = t - z; mode 1: out1 = t + eta rd, out2 = sigmu / z - x -
 * (x out1 + elp) / z (elp may be NULL); out1[q], out2[q] (mode 0 leaves out2 alone) */
extern "C" int hipsdp_small_lp_rows_unit(int device, int q, int m1, const double* Dext, const double* v, int mode, double eta, double sigmu,
   const double* x, const double* z, const double* rd, const double* elp, int recorded, double* out1, double* out2, int* pending)
{
   if ( q < 1 || m1 < 1 || !flag01(mode) || !flag01(recorded) || Dext == NULL || v == NULL || x == NULL || z == NULL || rd == NULL
         || out1 == NULL || out2 == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long qm = (long long) q * m1;
   DevBuf dD, dv, dx, dz, dr, de, d1, d2;
   HS_CALL( dD.alloc(qm) ); HS_CALL( dv.alloc(m1) ); HS_CALL( dx.alloc(q) ); HS_CALL( dz.alloc(q) ); HS_CALL( dr.alloc(q) );
   HS_CALL( de.alloc(q) ); HS_CALL( d1.alloc(q) ); HS_CALL( d2.alloc(q) );
   HS_CALL( nan_fill(d1, q) ); HS_CALL( nan_fill(d2, q) );
   HS_CALL( dD.up(Dext, qm) ); HS_CALL( dv.up(v, m1) ); HS_CALL( dx.up(x, q) ); HS_CALL( dz.up(z, q) ); HS_CALL( dr.up(rd, q) );
   if ( elp != NULL ) HS_CALL( de.up(elp, q) );
   RecScope sc(recorded);
   int rc = hs_lp_rows_small(0, q, m1, dD.p, dv.p, mode, eta, sigmu, dx.p, dz.p, dr.p, elp != NULL ? de.p : NULL, d1.p, d2.p);
   HS_CALL( sc.close(rc, pending) );
   HS_CALL( d1.down(out1, q) );
   return d2.down(out2, q);
}

/* hs_apply_A_small: out[i] = sum_k <A_k[i], V_k> + sum_r Dext[r][i] vlp[r], i < m1, over nblk blocks of n2[k] entries (A: the blocks one
 * behind the other, block k as m1 x n2[k]; V likewise) and q LP rows (Dext q x m1; q = 0: not read); epi 1: vout[i - 1] = out[i] - scal
 * vin[i - 1], epi 2: vout[i - 1] = vin[i - 1] scal - out[i], i >= 1 (epi 0 leaves vout alone); out[m1], vin, vout[m1 - 1] */
extern "C" int hipsdp_small_apply_A_unit(int device, int m1, int nblk, const int* n2, const double* A, const double* V, int q,
   const double* Dext, const double* vlp, int epi, double scal, const double* vin, int recorded, double* out, double* vout, int* pending)
{
   if ( m1 < 1 || nblk < 1 || nblk > HS_AS_MAXBLK || n2 == NULL || A == NULL || V == NULL || q < 0 || (q > 0 && (Dext == NULL || vlp == NULL))
         || epi < 0 || epi > 2 || (m1 > 1 && (vin == NULL || vout == NULL)) || !flag01(recorded) || out == NULL )
      return HIPSDP_ERR_ARG;
   long long tot = 0;
   for (int k = 0; k < nblk; ++k)
   {
      if ( n2[k] < 1 )
         return HIPSDP_ERR_ARG;
      tot += n2[k];
   }
   HS_CALL( pick_device(device) );
   DevBuf dA, dV, dD, dl, dO, di, dvo;
   HS_CALL( dA.alloc(tot * m1) ); HS_CALL( dV.alloc(tot) ); HS_CALL( dD.alloc((long long) q * m1) ); HS_CALL( dl.alloc(q) );
   HS_CALL( dO.alloc(m1) ); HS_CALL( di.alloc(m1 - 1) ); HS_CALL( dvo.alloc(m1 - 1) );
   HS_CALL( nan_fill(dO, m1) ); HS_CALL( nan_fill(dvo, m1 - 1) );
   HS_CALL( dA.up(A, tot * m1) ); HS_CALL( dV.up(V, tot) ); HS_CALL( dD.up(Dext, (long long) q * m1) ); HS_CALL( dl.up(vlp, q) );
   HS_CALL( di.up(vin, m1 - 1) );
   hs_as_args B;
   memset(&B, 0, sizeof(B));
   B.nblk = nblk;
   long long off = 0;
   for (int k = 0; k < nblk; ++k)
   {
      B.n2[k] = n2[k]; B.A[k] = dA.p + off * m1; B.V[k] = dV.p + off;
      off += n2[k];
   }
   RecScope sc(recorded);
   int rc = hs_apply_A_small(0, m1, &B, q, dD.p, dl.p, dO.p, epi, scal, di.p, dvo.p);
   HS_CALL( sc.close(rc, pending) );
   HS_CALL( dO.down(out, m1) );
   return dvo.down(vout, m1 - 1);
}

/* the element-wise kernels of the small path in one call, each one line of arithmetic: in[6][n] = x, z, r, elp, a, b; par = sigmu, eta,
 * alpha, s0, s1.  hs_lp_dir: o_lp = sigmu / z - x - (eta x r + elp) / z (use_elp = 0: without elp); hs_vec_mul: o_mul = a .* b;
 * hs_make_ext: o_ext[n + 1] = [s0; s1 a]; hs_axpy3: ys += alpha xs on three vectors of nn[0], nn[1], nn[2] entries (>= 0), one behind
 * the other in xs and ys (ys read and written) */
extern "C" int hipsdp_small_elementwise_unit(int device, int n, const int* nn, const double* par, int use_elp, const double* in,
   const double* xs, int recorded, double* o_lp, double* o_mul, double* o_ext, double* ys, int* pending)
{
   if ( n < 1 || nn == NULL || nn[0] < 0 || nn[1] < 0 || nn[2] < 0 || par == NULL || !flag01(use_elp) || in == NULL || xs == NULL
         || !flag01(recorded) || o_lp == NULL || o_mul == NULL || o_ext == NULL || ys == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long n3 = (long long) nn[0] + nn[1] + nn[2];
   DevBuf dI, dX, dY, dL, dM, dE;
   HS_CALL( dI.alloc(6LL * n) ); HS_CALL( dX.alloc(n3) ); HS_CALL( dY.alloc(n3) ); HS_CALL( dL.alloc(n) ); HS_CALL( dM.alloc(n) );
   HS_CALL( dE.alloc(n + 1) );
   HS_CALL( nan_fill(dL, n) ); HS_CALL( nan_fill(dM, n) ); HS_CALL( nan_fill(dE, n + 1) );
   HS_CALL( dI.up(in, 6LL * n) ); HS_CALL( dX.up(xs, n3) ); HS_CALL( dY.up(ys, n3) );
   const double* x = dI.p; const double* z = dI.p + n; const double* r = dI.p + 2LL * n; const double* elp = dI.p + 3LL * n;
   const double* a = dI.p + 4LL * n; const double* b = dI.p + 5LL * n;
   RecScope sc(recorded);
   int rc = hs_lp_dir(0, n, par[0], par[1], x, z, r, use_elp ? elp : NULL, dL.p);
   if ( rc == HS_OK ) rc = hs_vec_mul(0, n, a, b, dM.p);
   if ( rc == HS_OK ) rc = hs_make_ext(0, n, par[3], par[4], a, dE.p);
   if ( rc == HS_OK ) rc = hs_axpy3(0, par[2], nn[0], dX.p, dY.p, nn[1], dX.p + nn[0], dY.p + nn[0], nn[2], dX.p + nn[0] + nn[1],
         dY.p + nn[0] + nn[1]);
   HS_CALL( sc.close(rc, pending) );
   HS_CALL( dL.down(o_lp, n) ); HS_CALL( dM.down(o_mul, n) ); HS_CALL( dE.down(o_ext, n + 1) );
   return dY.down(ys, n3);
}

/* hs_gemv_t with a free row pitch: out[e] = sum_i coef[i] A[i lda + e] + sa add[e], A: R rows of lda >= E doubles (the last one E).
 * add_mode 0: no additive term; 1: add[E], an array of its own; 2: the output itself, which starts as add[E] (as ipm.hip calls it:
 * hs_gemv_t(..., 1.0, out, out)) */
extern "C" int hipsdp_small_gemv_t_unit(int device, int R, long long E, long long lda, const double* A, const double* coef, double sa,
   int add_mode, const double* add, int recorded, double* out, int* pending)
{
   if ( R < 1 || E < 1 || lda < E || A == NULL || coef == NULL || add_mode < 0 || add_mode > 2 || (add_mode > 0 && add == NULL)
         || !flag01(recorded) || out == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long na = span(R, (int) E, lda);
   DevBuf dA, dc, dadd, dO;
   HS_CALL( dA.alloc(na) ); HS_CALL( dc.alloc(R) ); HS_CALL( dadd.alloc(E) ); HS_CALL( dO.alloc(E) );
   HS_CALL( nan_fill(dO, E) );
   HS_CALL( dA.up(A, na) ); HS_CALL( dc.up(coef, R) );
   if ( add_mode == 1 ) HS_CALL( dadd.up(add, E) );
   if ( add_mode == 2 ) HS_CALL( dO.up(add, E) );
   RecScope sc(recorded);
   int rc = hs_gemv_t(0, R, E, dA.p, lda, dc.p, sa, add_mode == 0 ? NULL : (add_mode == 1 ? dadd.p : dO.p), dO.p);
   HS_CALL( sc.close(rc, pending) );
   return dO.down(out, E);
}

/* `count` <= 8 reductions of one kind (0 hs_dot <a, b>, 1 hs_absmax max |a|, 2 hs_ratio_min min over b < 0 of -a / b, 3 hs_lp_s0
 * sum (a / b) c^2), reduction j over len[j] >= 1 entries - the operands of the reductions one behind the other in a, b, c - into
 * out[slot[j]] (slot[j] < nslots <= 32), accumulate[j] = 1: combined with what the slot holds.  Every slot is first set to preset[.] by
 * hs_fill_scalar.  recorded = 1: fills and reductions inside ONE hs_red_batch_begin / hs_red_batch_end (the fills are records too:
 * *pending counts them, and more than the batch holds are launched on the way); 0: no batch, every call a launch of its own */
extern "C" int hipsdp_reductions_unit(int device, int kind, int count, const int* len, const int* slot, const int* accumulate,
   const double* a, const double* b, const double* c, int nslots, const double* preset, int recorded, double* out, int* pending)
{
   if ( kind < 0 || kind > 3 || count < 1 || count > 8 || len == NULL || slot == NULL || accumulate == NULL || a == NULL || b == NULL
         || c == NULL || nslots < 1 || nslots > 32 || preset == NULL || !flag01(recorded) || out == NULL )
      return HIPSDP_ERR_ARG;
   long long tot = 0;
   for (int j = 0; j < count; ++j)
   {
      if ( len[j] < 1 || slot[j] < 0 || slot[j] >= nslots || !flag01(accumulate[j]) )
         return HIPSDP_ERR_ARG;
      tot += len[j];
   }
   HS_CALL( pick_device(device) );
   DevBuf dA, dB, dC, dO, dW;
   HS_CALL( dA.alloc(tot) ); HS_CALL( dB.alloc(tot) ); HS_CALL( dC.alloc(tot) ); HS_CALL( dO.alloc(nslots) );
   HS_CALL( dW.alloc(HS_RED_WS_DOUBLES) );
   HS_CALL( nan_fill(dO, nslots) ); HS_CALL( nan_fill(dW, HS_RED_WS_DOUBLES) );
   HS_CALL( dA.up(a, tot) ); HS_CALL( dB.up(b, tot) ); HS_CALL( dC.up(c, tot) );
   hs_red_batch_reset();
   if ( recorded )
      hs_red_batch_begin(0);
   int rc = HS_OK;
   for (int k = 0; k < nslots && rc == HS_OK; ++k)
      rc = hs_fill_scalar(0, dO.p + k, preset[k]);
   long long off = 0;
   for (int j = 0; j < count && rc == HS_OK; ++j)
   {
      double* o = dO.p + slot[j];
      switch ( kind )
      {
      case 0:  rc = hs_dot(0, len[j], dA.p + off, dB.p + off, o, accumulate[j], dW.p); break;
      case 1:  rc = hs_absmax(0, len[j], dA.p + off, o, accumulate[j], dW.p); break;
      case 2:  rc = hs_ratio_min(0, len[j], dA.p + off, dB.p + off, o, accumulate[j], dW.p); break;
      default: rc = hs_lp_s0(0, len[j], dA.p + off, dB.p + off, dC.p + off, o, accumulate[j], dW.p); break;
      }
      off += len[j];
   }
   if ( pending != NULL ) *pending = hs_red_batch_pending();
   if ( recorded && rc == HS_OK ) rc = hs_red_batch_end();
   if ( hipDeviceSynchronize() != hipSuccess && rc == HS_OK ) rc = HS_ERR_HIP;
   hs_red_batch_reset();
   HS_CALL( rc );
   return dO.down(out, nslots);
}

/* the two small solves with the factor of M, m <= 64.  M (m x m, symmetric positive definite) is factored on the device as the engine
 * does it (hs_potrf_psd with diag0 = diag(M) and a mask: L and inv(L) as 64 x 64); *fail: the factorization flag.
 * form 0: hs_red_batch_solve inside a batch on nrhs right-hand sides, ld >= m apart: rhs[nrhs x ld] in place (entries m .. ld - 1 of a
 *         row are not touched); *pending: records before the batch's end.  u2, wt are not used.
 * form 1: k_solve2_small through hs_solve2_small: rhs[2 m] comes in as [g ; b] (g travels as row 0 of an Mx: Mx[0][1 + i] = g[i]) and
 *         goes out as the two solutions; u2[m], wt[m + 1].  nrhs, ld are not used, *pending = 0.
 * The switch HIPSDP_SMALL_SOLVE is read by the call, as the engine reads it */
extern "C" int hipsdp_small_solve_unit(int device, int m, const double* M, int form, int nrhs, long long ld, double* rhs, double* u2,
   double* wt, int* pending, int* fail)
{
   if ( m < 1 || m > 64 || M == NULL || !flag01(form) || rhs == NULL || (form == 0 && (nrhs < 1 || nrhs > 8 || ld < m))
         || (form == 1 && (u2 == NULL || wt == NULL)) )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long m2 = (long long) m * m;
   const long long nr = form == 0 ? nrhs * ld : 2LL * m;
   DevBuf dL, dD, dG, dR, dMx, db, dU, dW;
   int* dint = NULL;
   HS_CALL( dL.alloc(m2) ); HS_CALL( dD.alloc(hs_potrf_dinv_len(m)) ); HS_CALL( dG.alloc(m) ); HS_CALL( dR.alloc(nr) );
   HS_CALL( dMx.alloc(m + 1) ); HS_CALL( db.alloc(m) ); HS_CALL( dU.alloc(m) ); HS_CALL( dW.alloc(m + 1) );
   HS_CALL( nan_fill(dU, m) ); HS_CALL( nan_fill(dW, m + 1) );
   std::vector<double> dg(m), mx0(m + 1, 0.0);
   for (int i = 0; i < m; ++i) dg[i] = M[(long long) i * m + i];
   HS_CALL( dL.up(M, m2) ); HS_CALL( dG.up(dg.data(), m) );
   if ( form == 0 )
      HS_CALL( dR.up(rhs, nr) );
   else
   {
      for (int i = 0; i < m; ++i) mx0[1 + i] = rhs[i];
      HS_CALL( dMx.up(mx0.data(), m + 1) ); HS_CALL( db.up(rhs + m, m) ); HS_CALL( nan_fill(dR, nr) );
   }
   HS_HIP( hipMemset(dD.p, 0, (size_t) hs_potrf_dinv_len(m) * sizeof(double)) );
   HS_HIP( hipMalloc((void**) &dint, (size_t) (m + 1) * sizeof(int)) );
   int rc = hipMemset(dint, 0, (size_t) (m + 1) * sizeof(int)) == hipSuccess ? HS_OK : HS_ERR_HIP;
   int pend = 0;
   hs_red_batch_reset();
   if ( rc == HS_OK ) rc = hs_potrf_psd(0, m, dL.p, dD.p, dint, dG.p, dint + 1, 0);
   if ( rc == HS_OK && form == 0 )
   {
      hs_red_batch_begin(0);
      if ( hs_red_batch_solve(0, m, dD.p, dL.p, nrhs, dR.p, ld) != 1 ) rc = HS_ERR_ARG;
      pend = hs_red_batch_pending();
      if ( rc == HS_OK ) rc = hs_red_batch_end();
   }
   else if ( rc == HS_OK )
      rc = hs_solve2_small(0, m, dMx.p, db.p, dD.p, dL.p, dR.p, dU.p, dW.p, hs_small_solve_by_substitution());
   if ( hipDeviceSynchronize() != hipSuccess && rc == HS_OK ) rc = HS_ERR_HIP;
   hs_red_batch_reset();
   int hflag = 0;
   if ( rc == HS_OK && hipMemcpy(&hflag, dint, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess ) rc = HS_ERR_HIP;
   (void) hipFree(dint);
   HS_CALL( rc );
   if ( pending != NULL ) *pending = pend;
   if ( fail != NULL ) *fail = hflag;
   HS_CALL( dR.down(rhs, nr) );
   if ( form == 1 )
   {
      HS_CALL( dU.down(u2, m) ); HS_CALL( dW.down(wt, m + 1) );
   }
   return HIPSDP_OK;
}

/* three linear combinations of the rows of A (R rows of lda >= E doubles): out[v][e] = sum_i c[v][i] A[i lda + e], c[3][R], out[3][E].
 * fused = 1: hs_gemv_t3, and when it does not take the shape (odd E or lda) the three hs_gemv_t calls the engine then makes;
 * fused = 0: three hs_gemv_t calls.  *took = 1 when the fused kernel ran */
extern "C" int hipsdp_gemv_t3_unit(int device, int R, long long E, long long lda, const double* A, const double* c, int fused, double* out,
   int* took)
{
   if ( R < 1 || E < 1 || lda < E || A == NULL || c == NULL || !flag01(fused) || out == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long na = span(R, (int) E, lda), Ep = E + (E & 1);
   DevBuf dA, dc, dO;
   HS_CALL( dA.alloc(na) ); HS_CALL( dc.alloc(3LL * R) ); HS_CALL( dO.alloc(3 * Ep) );
   HS_CALL( nan_fill(dO, 3 * Ep) );
   HS_CALL( dA.up(A, na) ); HS_CALL( dc.up(c, 3LL * R) );
   hs_red_batch_reset();
   int t = 0, rc = HS_OK;
   if ( fused )
   {
      t = hs_gemv_t3(0, R, E, dA.p, lda, dc.p, dc.p + R, dc.p + 2LL * R, dO.p, dO.p + Ep, dO.p + 2 * Ep);
      if ( t < 0 ) { rc = -t; t = 0; }
   }
   if ( t == 0 )
      for (int v = 0; v < 3 && rc == HS_OK; ++v)
         rc = hs_gemv_t(0, R, E, dA.p, lda, dc.p + (long long) v * R, 0.0, NULL, dO.p + v * Ep);
   if ( hipDeviceSynchronize() != hipSuccess && rc == HS_OK ) rc = HS_ERR_HIP;
   HS_CALL( rc );
   if ( took != NULL ) *took = t;
   for (int v = 0; v < 3; ++v)
      HS_HIP( hipMemcpy(out + v * E, dO.p + v * Ep, (size_t) E * sizeof(double), hipMemcpyDeviceToHost) );
   return HIPSDP_OK;
}

/* hs_gemv_n (the pass A): out[v][i] = sum_e A[i lda + e] V[v][e], i < R, v < nv <= 4; A: R rows of lda >= E doubles, V[nv][E].  The
 * device copies of the vectors start voff >= 0 doubles behind a 16-byte aligned address (an odd voff takes the two-at-a-time loads
 * away); wsdoubles >= 0: the workspace the call is given for the split form.  info[0] = slices a row is cut into (the launcher's rule,
 * recomputed here from the same inputs; 1: one workgroup per row), info[1] = 1 when the launcher takes the two-at-a-time kernel */
extern "C" int hipsdp_pass_a_unit(int device, int R, long long E, long long lda, const double* A, int nv, const double* V, int voff,
   long long wsdoubles, double* out, int* info)
{
   if ( R < 1 || E < 1 || lda < E || A == NULL || nv < 1 || nv > 4 || V == NULL || voff < 0 || voff > 64 || wsdoubles < 0 || out == NULL )
      return HIPSDP_ERR_ARG;
   HS_CALL( pick_device(device) );
   const long long na = span(R, (int) E, lda), Ep = E + (E & 1);
   DevBuf dA, dV, dO, dW;
   HS_CALL( dA.alloc(na) ); HS_CALL( dV.alloc(nv * Ep + voff) ); HS_CALL( dO.alloc((long long) nv * R) ); HS_CALL( dW.alloc(wsdoubles) );
   HS_CALL( nan_fill(dO, (long long) nv * R) ); HS_CALL( nan_fill(dW, wsdoubles) );
   HS_CALL( dA.up(A, na) );
   const double* vp[4];
   for (int v = 0; v < nv; ++v)
   {
      HS_HIP( hipMemcpy(dV.p + voff + v * Ep, V + v * E, (size_t) E * sizeof(double), hipMemcpyHostToDevice) );
      vp[v] = dV.p + voff + v * Ep;
   }
   if ( info != NULL )
   {
      /* gemv_n_launch of kernels.hip */
      const bool vec = (lda & 1) == 0 && (voff & 1) == 0;
      long long nsplit = 1;
      if ( R < 512 && E >= 16384 )
      {
         nsplit = (1024 + R - 1) / R;
         if ( nsplit > E / 8192 ) nsplit = E / 8192;
         if ( nsplit < 1 ) nsplit = 1;
         if ( nsplit * nv * R > wsdoubles ) nsplit = 1;
      }
      info[0] = (int) nsplit; info[1] = vec ? 1 : 0;
   }
   hs_red_batch_reset();
   int rc = hs_gemv_n(0, R, E, dA.p, lda, nv, vp, dO.p, R, dW.p, wsdoubles);
   if ( hipDeviceSynchronize() != hipSuccess && rc == HS_OK ) rc = HS_ERR_HIP;
   HS_CALL( rc );
   return dO.down(out, (long long) nv * R);
}

/* k_r1_minors's scans (hs_r1_minors_unit, csrc/rank1.hip) on `count` host matrices, matrix k of n[k] rows (1 .. 512), one behind the
 * other in Z: minorev[k], minorind[2 k], minordet[k], detind[2 k] as hipsdp_rank1_check_many returns them for one (candidate, block) */
extern "C" int hipsdp_rank1_minors_unit(int device, int count, const int* n, const double* Z, double feastol, double* minorev, int* minorind,
   double* minordet, int* detind)
{
   if ( count < 1 || n == NULL || Z == NULL || !(feastol >= 0.0) || minorev == NULL || minorind == NULL || minordet == NULL || detind == NULL )
      return HIPSDP_ERR_ARG;
   std::vector<long long> off((size_t) count + 1, 0);
   int nmax = 0;
   for (int k = 0; k < count; ++k)
   {
      if ( n[k] < 1 || n[k] > HS_SYEVX_MAXN )
         return HIPSDP_ERR_ARG;
      off[k + 1] = off[k] + (long long) n[k] * n[k];
      nmax = std::max(nmax, n[k]);
   }
   HS_CALL( pick_device(device) );
   DevBuf dZ, dn, doff, dout, dind;
   HS_CALL( dZ.alloc(off[count]) ); HS_CALL( dn.alloc(((long long) count + 1) / 2) ); HS_CALL( doff.alloc(count) );
   HS_CALL( dout.alloc(2LL * count) ); HS_CALL( dind.alloc(2LL * count) );
   HS_CALL( dZ.up(Z, off[count]) );
   HS_HIP( hipMemcpy(dn.p, n, (size_t) count * sizeof(int), hipMemcpyHostToDevice) );
   HS_HIP( hipMemcpy(doff.p, off.data(), (size_t) count * sizeof(long long), hipMemcpyHostToDevice) );
   HS_CALL( hs_r1_minors_unit(0, count, nmax, reinterpret_cast<const int*>(dn.p), reinterpret_cast<const long long*>(doff.p), dZ.p, feastol, dout.p,
         reinterpret_cast<int*>(dind.p)) );
   HS_HIP( hipDeviceSynchronize() );
   std::vector<double> o(2 * (size_t) count);
   std::vector<int> ind(4 * (size_t) count);
   HS_CALL( dout.down(o.data(), 2LL * count) );
   HS_HIP( hipMemcpy(ind.data(), dind.p, ind.size() * sizeof(int), hipMemcpyDeviceToHost) );
   for (int k = 0; k < count; ++k)
   {
      minorev[k] = o[2 * (size_t) k]; minordet[k] = o[2 * (size_t) k + 1];
      minorind[2 * k] = ind[4 * (size_t) k]; minorind[2 * k + 1] = ind[4 * (size_t) k + 1];
      detind[2 * k] = ind[4 * (size_t) k + 2]; detind[2 * k + 1] = ind[4 * (size_t) k + 3];
   }
   return HIPSDP_OK;
}

/* the three-index values kernels of hipsdp_rank1_check_many on `count` host matrices (n[k] rows, 1 .. 512, one behind the other in Z):
 * hs_lsel_many_small up to 64 rows, hs_lsel_many_mid up to 128, above that hs_ecl_clear, hs_syevx_many_cols and hs_syevx_many_index; then
 * hs_r1_result.  Every matrix is a block of its own with one candidate.  lam[3 k ..]: eigenvalues 1, n - 1, n of matrix k. */
extern "C" int hipsdp_lsel_many_unit(int device, int count, const int* n, const double* Z, double* lam)
{
   if ( count < 1 || count > 65535 || n == NULL || Z == NULL || lam == NULL )
      return HIPSDP_ERR_ARG;
   std::vector<long long> off((size_t) count + 1, 0);
   long long ws_len = 0;
   for (int k = 0; k < count; ++k)
   {
      if ( n[k] < 1 || n[k] > HS_SYEVX_MAXN )
         return HIPSDP_ERR_ARG;
      off[k + 1] = off[k] + (long long) n[k] * n[k];
   }
   /* the tables in the order of the classes */
   std::vector<int> order;
   int cnt[3] = {0, 0, 0}, top[3] = {0, 0, 0};
   for (int cls = 0; cls < 3; ++cls)
      for (int k = 0; k < count; ++k)
         if ( (n[k] <= 64 ? 0 : (n[k] <= HS_SC_MAXN ? 1 : 2)) == cls )
         {
            order.push_back(k);
            ++cnt[cls];
            top[cls] = std::max(top[cls], n[k]);
            if ( cls == 2 )
               ws_len += (((long long) hs_syevx_ws(n[k]) + 1) & ~1LL) + HS_SXM_OUT(n[k]);
         }
   HS_CALL( pick_device(device) );
   const long long jobw = (long long) (sizeof(hs_ec_job) / sizeof(double)), blkw = (long long) (sizeof(hs_cm_blk) / sizeof(double)),
      sxw = (long long) (sizeof(hs_sxm_job) / sizeof(double));
   DevBuf dZ, dws, dlam, djobs, dblks, dsx, dact, dres;
   HS_CALL( dZ.alloc(off[count]) ); HS_CALL( dws.alloc(ws_len) ); HS_CALL( dlam.alloc(4LL * count) );
   HS_CALL( djobs.alloc(jobw * count) ); HS_CALL( dblks.alloc(blkw * count) ); HS_CALL( dsx.alloc(sxw * cnt[2]) );
   HS_CALL( dact.alloc(((long long) cnt[2] + 1) / 2) ); HS_CALL( dres.alloc((long long) HS_R1_RESW * count) );
   HS_CALL( dZ.up(Z, off[count]) );
   std::vector<hs_ec_job> jobs((size_t) count);
   std::vector<hs_cm_blk> blks((size_t) count);
   std::vector<hs_sxm_job> sx((size_t) cnt[2]);
   std::vector<int> act((size_t) cnt[2], HS_SXM_ACTIVE);
   memset(jobs.data(), 0, jobs.size() * sizeof(hs_ec_job));
   long long wpos = 0;
   for (int t = 0; t < count; ++t)
   {
      const int k = order[t], nk = n[k];
      jobs[t].n = nk; jobs[t].blk = t;
      blks[t].Z = dZ.p + off[k]; blks[t].zstride = 0;
      blks[t].lam = dlam.p + 4LL * t; blks[t].lstride = 0;
      if ( nk <= HS_SC_MAXN )
         continue;
      const int j = t - cnt[0] - cnt[1];
      double* ws = dws.p + wpos;
      double* out = ws + (((long long) hs_syevx_ws(nk) + 1) & ~1LL);
      wpos += (((long long) hs_syevx_ws(nk) + 1) & ~1LL) + HS_SXM_OUT(nk);
      HS_CALL( hs_syevx_many_job(nk, ws, out, &sx[j]) );
      HS_HIP( hipMemcpy(sx[j].A, dZ.p + off[k], (size_t) nk * nk * sizeof(double), hipMemcpyDeviceToDevice) );
      blks[t].lam = out + HS_SYEVX_OUT_LAM;
   }
   HS_HIP( hipMemcpy(djobs.p, jobs.data(), jobs.size() * sizeof(hs_ec_job), hipMemcpyHostToDevice) );
   HS_HIP( hipMemcpy(dblks.p, blks.data(), blks.size() * sizeof(hs_cm_blk), hipMemcpyHostToDevice) );
   const hs_ec_job* dj = reinterpret_cast<const hs_ec_job*>(djobs.p);
   const hs_cm_blk* db = reinterpret_cast<const hs_cm_blk*>(dblks.p);
   if ( cnt[0] > 0 )
      HS_CALL( hs_lsel_many_small(0, cnt[0], 1, top[0], dj, db) );
   if ( cnt[1] > 0 )
   {
      const int cus = hs_device_cus();
      HS_CALL( hs_lsel_many_mid(0, cnt[1], 1, top[1], cus > 0 ? cus : 256, dj + cnt[0], db + cnt[0]) );
   }
   if ( cnt[2] > 0 )
   {
      HS_HIP( hipMemcpy(dsx.p, sx.data(), sx.size() * sizeof(hs_sxm_job), hipMemcpyHostToDevice) );
      HS_HIP( hipMemcpy(dact.p, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice) );
      const hs_sxm_job* ds = reinterpret_cast<const hs_sxm_job*>(dsx.p);
      const int* da = reinterpret_cast<const int*>(dact.p);
      HS_CALL( hs_ecl_clear(0, cnt[2], ds) );
      HS_CALL( hs_syevx_many_cols(0, cnt[2], top[2], hs_syevx_many_cap(cnt[2]), ds, da) );
      HS_CALL( hs_syevx_many_index(0, cnt[2], top[2], ds, da) );
   }
   HS_CALL( hs_r1_result(0, count, 1, dj, db, dres.p) );
   HS_HIP( hipDeviceSynchronize() );
   std::vector<double> res((size_t) HS_R1_RESW * count);
   HS_CALL( dres.down(res.data(), (long long) res.size()) );
   for (int t = 0; t < count; ++t)
      for (int i = 0; i < 3; ++i)
         lam[3 * (size_t) order[t] + i] = res[(size_t) HS_R1_RESW * t + i];
   return HIPSDP_OK;
}
