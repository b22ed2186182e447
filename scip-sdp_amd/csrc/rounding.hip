/* rounding.hip - the coefficient table of the primal rounding problem for ALL eigenvectors of every block (hipsdp_rounding_frame; host
 * side: cut_calls.hip).
 *
 * The reference's warm start with relax/warmstartproject = 4 (solvePrimalRoundingProblem, relax_sdp.c:1551-2640) decomposes the start
 * matrix X* of every block and needs, for EVERY eigenvector v_j of a block (all n of them) and every matrix of the block,
 *    obj[j] = v_j^T A_0 v_j (:1906-1923)      val[j][i] = v_j^T A_i v_j (:1926-1947)
 * - n (m + 1) n (n + 1) / 2 multiply-adds per block.  ec_sweep (hs_ec_sweep.h) serves 8 vectors per pass over A_i; for n vectors that is
 * n / 8 passes.  Over the storage index p of a matrix the table is a GEMM:
 *    C[j][i] = sum_p P[j][p] A_i[p],    P[j][p] = w_p V[j][r_p] V[j][c_p],   w = 1 on the diagonal of a packed triangle, 2 off it
 * whose operand P is formed from V while it is staged.
 *
 *    k_rf_gather        (32, blocks)   eigenvalues and vectors from the decomposition's output into the solver's frame; for a block of
 *                                      the scalar route the transposed copy VT[r][j] as well
 *    k_rf_coefs_mc      (tiles x slices, blocks)  blocks of more than 64 rows held as packed triangles or dense rows.  Tile = 64 vectors
 *                                      x 64 matrices (row 0 = the constant matrix), four wavefronts of 16 vectors x 64 matrices each, K =
 *                                      the storage index in ascending order in panels of 16 through LDS: the A panel is read as runs of
 *                                      16 consecutive entries of each matrix row (128 bytes), the P panel is formed from V (L2: 2 MB at
 *                                      512 rows) with consecutive lanes on consecutive p, so that V[j][c_p] is read in runs and V[j][r_p]
 *                                      is one address per row of the triangle; v_mfma_f64_16x16x4_f64 with the fragment layout of
 *                                      k_ppl_recombine (psd_large.hip).  A block with few tiles is cut into slices of K (hs_rf_slice_rule,
 *                                      a function of (n, m) alone); slice s writes its own partial table.
 *    k_rf_coefs_scalar  ((m + 1) ceil(n / 64) / 4, blocks)  blocks of at most 64 rows and blocks kept as nonzeros (the constant matrix of
 *                                      those is the dense row 0): thread j owns v_j for matrix i, sums over the entries of A_i in storage
 *                                      order, reads V through VT so that a wavefront reads whole lines; no reduction across threads
 *    k_rf_store         (32, blocks)   eigenvalues, obj and coef - the slices added in slice order - and the vectors into the result
 *
 * HAZARD RULE: no atomic operation, no flag; inside a launch no workgroup reads what another writes (the coefficient
 * launches read V / VT of the launch before and write part, the store launch reads part); every sum has a fixed order.  The bits of a
 * block depend on its own V and matrices alone. */
#include "hs_kernels.h"
#include "hs_round_plan.h"
#include <cstring>
#include <vector>

#define RF_NT 256
#define RF_T  HS_RF_TILE
#define RF_K  HS_RF_TK
#define RF_LD 80              /* pitch of a panel row in LDS (PL_LD of psd_large.hip) */
#define RF_GG 32              /* workgroups per block of the gather and store launches */

static_assert(RF_T == 64 && RF_K == 16 && RF_NT == 256, "the staging maps of k_rf_coefs_mc");

typedef double rf_v4 __attribute__((ext_vector_type(4)));

namespace {

__global__ void __launch_bounds__(RF_NT) k_rf_gather(const hs_rf_job* __restrict__ jobs)
{
   const hs_rf_job J = jobs[blockIdx.y];
   const int n = J.n;
   const long long n2 = (long long) n * n, stride = (long long) gridDim.x * RF_NT, first = (long long) blockIdx.x * RF_NT + threadIdx.x;
   for (long long e = first; e < n; e += stride)
      J.lam[e] = J.lam_src[e];
   for (long long e = first; e < n2; e += stride)
   {
      const double v = J.V_src[e];
      J.V[e] = v;
      if ( J.VT != NULL )
      {
         const int j = (int) (e / n), r = (int) (e - (long long) j * n);
         J.VT[(long long) r * n + j] = v;
      }
   }
}

/* v_j^T A_i v_j over the entries of A_i in storage order; vt = VT + j */
__device__ __forceinline__ double rf_scalar_sum(const hs_ec_job& E, int i, int n, const double* __restrict__ vt)
{
   double acc = 0.0;
   if ( E.form == HS_EC_PACKED )
   {
      const double* __restrict__ a = E.A + (long long) i * E.ld;
      long long p = 0;
      for (int r = 0; r < n; ++r)
      {
         const double vr = vt[(long long) r * n];
         for (int c = 0; c <= r; ++c, ++p)
            acc += hs_rf_weight(r, c) * a[p] * vr * vt[(long long) c * n];
      }
   }
   else if ( E.form == HS_EC_SPARSE && i > 0 )
   {
      for (int e = E.sp.voff[i - 1]; e < E.sp.voff[i]; ++e)
      {
         const int r = E.sp.vrow[e], c = E.sp.vcol[e];
         acc += hs_rf_weight(r, c) * E.sp.vval[e] * vt[(long long) r * n] * vt[(long long) c * n];
      }
   }
   else
   {
      /* dense rows; the constant matrix of a block kept as nonzeros is its dense row 0 */
      const double* __restrict__ a = E.A + (long long) i * E.ld;
      for (int r = 0; r < n; ++r)
      {
         const double vr = vt[(long long) r * n];
         for (int c = 0; c < n; ++c)
            acc += a[(long long) r * n + c] * vr * vt[(long long) c * n];
      }
   }
   return acc;
}

/* item = i jw + j, jw = n rounded up to 64: a wavefront has one matrix */
__global__ void __launch_bounds__(RF_NT) k_rf_coefs_scalar(int m, const hs_ec_job* __restrict__ ejobs, const hs_rf_job* __restrict__ jobs)
{
   const hs_rf_job J = jobs[blockIdx.y];
   if ( J.route != 0 )
      return;
   const int n = J.n, jw = (n + 63) & ~63;
   const long long item = (long long) blockIdx.x * RF_NT + threadIdx.x;
   if ( item >= ((long long) m + 1) * jw )
      return;
   const int i = (int) (item / jw), j = (int) (item - (long long) i * jw);
   if ( j >= n )
      return;
   const hs_ec_job E = ejobs[blockIdx.y];
   J.part[(long long) j * (m + 1) + i] = rf_scalar_sum(E, i, n, J.VT + j);
}

/* Tile (tj, ti) of slice s of block blockIdx.y.  Wavefront w owns the vectors 16 w .. 16 w + 15 of the tile and its 64 matrices: four
 * accumulators of v_mfma_f64_16x16x4_f64 (lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and D[(l >> 4) + 4 r][l & 15], r = 0 .. 3).
 * Staging: thread t forms P for the entry p0 + (t & 15) and the vectors (t >> 4) + 16 u, u = 0 .. 3 (one decode per panel), and loads
 * the entries p0 + 4 (t & 3) .. + 3 of matrix t >> 2. */
template <bool PACKED>
__device__ __forceinline__ void rf_tile(const hs_ec_job& E, const hs_rf_job& J, int m, int tj, int ti, int s, double (*sP)[RF_LD],
   double (*sA)[RF_LD])
{
   const int n = J.n, m1 = m + 1, j0 = RF_T * tj, i0 = RF_T * ti;
   const long long pbeg = (long long) s * J.pps * RF_K;
   const long long pend = pbeg + J.pps * RF_K < J.klen ? pbeg + J.pps * RF_K : J.klen;
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
   const int pp = tid & 15, jj = tid >> 4, ii = tid >> 2, kq = 4 * (tid & 3);
   const bool ain = i0 + ii < m1;
   const double* __restrict__ arow = E.A + (long long) (ain ? i0 + ii : 0) * E.ld;
   const double* __restrict__ V = J.V;
   rf_v4 acc[4];
#pragma unroll
   for (int c = 0; c < 4; ++c)
      acc[c] = (rf_v4) {0.0, 0.0, 0.0, 0.0};
   for (long long p0 = pbeg; p0 < pend; p0 += RF_K)
   {
      {
         const long long p = p0 + pp;
         const bool pin = p < pend;
         int r = 0, c = 0;
         double w = 1.0;
         if ( pin )
         {
            if ( PACKED )
            {
               hs_rf_decode(p, &r, &c);
               w = hs_rf_weight(r, c);
            }
            else
            {
               r = (int) (p / n);
               c = (int) (p - (long long) r * n);
            }
         }
#pragma unroll
         for (int u = 0; u < 4; ++u)
         {
            const int j = j0 + jj + 16 * u;
            double v = 0.0;
            if ( pin && j < n )
               v = w * V[(long long) j * n + r] * V[(long long) j * n + c];
            sP[pp][jj + 16 * u] = v;
         }
      }
#pragma unroll
      for (int t = 0; t < 4; ++t)
      {
         const long long p = p0 + kq + t;
         sA[kq + t][ii] = ain && p < pend ? arow[p] : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < RF_K / 4; ++q)
      {
         const double a = sP[4 * q + lk][16 * wave + lr];
#pragma unroll
         for (int c = 0; c < 4; ++c)
            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sA[4 * q + lk][16 * c + lr], acc[c], 0, 0, 0);
      }
      __syncthreads();
   }
   double* __restrict__ part = J.part + (long long) s * n * m1;
#pragma unroll
   for (int r = 0; r < 4; ++r)
   {
      const int j = j0 + 16 * wave + lk + 4 * r;
#pragma unroll
      for (int c = 0; c < 4; ++c)
      {
         const int i = i0 + 16 * c + lr;
         if ( j < n && i < m1 )
            part[(long long) j * m1 + i] = acc[c][r];
      }
   }
}

/* blockIdx.x = (s ntj + tj) nti + ti */
__global__ void __launch_bounds__(RF_NT) k_rf_coefs_mc(int m, const hs_ec_job* __restrict__ ejobs, const hs_rf_job* __restrict__ jobs)
{
   __shared__ double sP[RF_K][RF_LD], sA[RF_K][RF_LD];
   const hs_rf_job J = jobs[blockIdx.y];
   if ( J.route != 1 )
      return;
   const int ntj = (J.n + RF_T - 1) / RF_T, nti = (m + 1 + RF_T - 1) / RF_T;
   if ( (long long) blockIdx.x >= (long long) J.slices * ntj * nti )
      return;
   const int ti = (int) (blockIdx.x % nti), rest = (int) (blockIdx.x / nti), tj = rest % ntj, s = rest / ntj;
   const hs_ec_job E = ejobs[blockIdx.y];
   if ( E.form == HS_EC_PACKED )
      rf_tile<true>(E, J, m, tj, ti, s, sP, sA);
   else
      rf_tile<false>(E, J, m, tj, ti, s, sP, sA);
}

__global__ void __launch_bounds__(RF_NT) k_rf_store(int m, const hs_rf_job* __restrict__ jobs, double* __restrict__ eig, double* __restrict__ obj,
   double* __restrict__ coef, double* __restrict__ vec)
{
   const hs_rf_job J = jobs[blockIdx.y];
   const int n = J.n, m1 = m + 1;
   const long long tab = (long long) n * m1, n2 = (long long) n * n;
   const long long stride = (long long) gridDim.x * RF_NT, first = (long long) blockIdx.x * RF_NT + threadIdx.x;
   for (long long e = first; e < n; e += stride)
      eig[J.row0 + e] = J.lam_src[e];
   for (long long e = first; e < tab; e += stride)
   {
      const long long j = e / m1;
      const int i = (int) (e - j * m1);
      double t = J.part[e];
      for (int s = 1; s < J.slices; ++s)
         t += J.part[s * tab + e];
      if ( i == 0 )
         obj[J.row0 + j] = t;
      else
         coef[(J.row0 + j) * m + (i - 1)] = t;
   }
   if ( vec != NULL )
      for (long long e = first; e < n2; e += stride)
         vec[J.vec0 + e] = J.V_src[e];
}

}

int hs_rf_gather(hipStream_t st, int count, const hs_rf_job* jobs)
{
   if ( count < 1 || count > 65535 || jobs == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_rf_gather, dim3(RF_GG, (unsigned) count), dim3(RF_NT), 0, st, jobs);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_rf_coefs_scalar(hipStream_t st, int count, int nmax, int m, const hs_ec_job* ejobs, const hs_rf_job* jobs)
{
   if ( count < 1 || count > 65535 || nmax < 1 || nmax > HS_RF_MAXN || m < 0 || ejobs == NULL || jobs == NULL )
      return HS_ERR_ARG;
   const long long items = ((long long) m + 1) * ((nmax + 63) & ~63);
   hipLaunchKernelGGL(k_rf_coefs_scalar, dim3((unsigned) ((items + RF_NT - 1) / RF_NT), (unsigned) count), dim3(RF_NT), 0, st, m, ejobs, jobs);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_rf_coefs_mc(hipStream_t st, int count, long long tiles, int m, const hs_ec_job* ejobs, const hs_rf_job* jobs)
{
   if ( count < 1 || count > 65535 || tiles < 1 || tiles > 0x7fffffffLL || m < 0 || ejobs == NULL || jobs == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_rf_coefs_mc, dim3((unsigned) tiles, (unsigned) count), dim3(RF_NT), 0, st, m, ejobs, jobs);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_rf_store(hipStream_t st, int count, int m, const hs_rf_job* jobs, double* eig, double* obj, double* coef, double* vec)
{
   if ( count < 1 || count > 65535 || m < 0 || jobs == NULL || eig == NULL || obj == NULL || coef == NULL )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_rf_store, dim3(RF_GG, (unsigned) count), dim3(RF_NT), 0, st, m, jobs, eig, obj, coef, vec);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_rf_coefs_host(int device, int n, int m, int form, const double* V, const double* A, long long nnz, const int* var, const int* row,
   const int* col, const double* val, double* out, int* route, int* slices)
{
   if ( n < 1 || n > HS_RF_MAXN || m < 0 || (form != HS_EC_DENSE && form != HS_EC_PACKED && form != HS_EC_SPARSE) || V == NULL || A == NULL
      || out == NULL || nnz < 0 || (form == HS_EC_SPARSE && nnz > 0 && (var == NULL || row == NULL || col == NULL || val == NULL)) )
      return HS_ERR_ARG;
   std::vector<int> voff((size_t) m + 1, 0);
   if ( form == HS_EC_SPARSE )
      for (long long e = 0; e < nnz; ++e)
      {
         if ( var[e] < 1 || var[e] > m || row[e] < 0 || row[e] >= n || col[e] < 0 || col[e] > row[e] || (e > 0 && var[e] < var[e - 1]) )
            return HS_ERR_ARG;
         ++voff[var[e]];
      }
   for (int i = 0; i < m; ++i)
      voff[i + 1] += voff[i];
   HS_HIP( hipSetDevice(device) );
   const long long n2 = (long long) n * n, m1 = (long long) m + 1;
   const long long ld = form == HS_EC_PACKED ? hs_rf_klen(n, 1) : n2, alen = form == HS_EC_SPARSE ? n2 : m1 * ld;
   hs_rf_job J;
   memset(&J, 0, sizeof(J));
   J.n = n;
   J.route = hs_rf_route(n, form == HS_EC_SPARSE);
   J.klen = hs_rf_klen(n, form == HS_EC_PACKED);
   const hs_rf_slices S = hs_rf_slice_rule(n, m, J.klen);
   J.slices = J.route ? S.slices : 1;
   J.pps = J.route ? S.pps : 0;
   if ( route != NULL ) *route = J.route;
   if ( slices != NULL ) *slices = J.slices;
   const long long tab = n * m1;
   /* one allocation: V source | lam source | frame lam | frame V | VT | part | summed table + eig + obj | A | nonzero values; ints behind */
   const long long o_vs = 0, o_ls = o_vs + n2, o_l = o_ls + n, o_v = o_l + n, o_vt = o_v + n2, o_part = o_vt + n2, o_res = o_part + J.slices * tab;
   const long long o_a = o_res + tab + 2 * n, o_val = o_a + alen, o_end = o_val + (form == HS_EC_SPARSE ? nnz : 0);
   double* d = NULL;
   int* di = NULL;
   char* dt = NULL;
   int rc = HS_OK;
   std::vector<double> res((size_t) (tab + 2 * n));
   do
   {
      hipError_t e = hipMalloc((void**) &d, (size_t) o_end * sizeof(double));
      if ( e == hipSuccess ) e = hipMalloc((void**) &di, (size_t) (m1 + 2 * nnz + 1) * sizeof(int));
      if ( e == hipSuccess ) e = hipMalloc((void**) &dt, sizeof(hs_rf_job) + sizeof(hs_ec_job));
      if ( e == hipSuccess ) e = hipMemset(d, 0, (size_t) o_end * sizeof(double));
      if ( e == hipSuccess ) e = hipMemcpy(d + o_vs, V, (size_t) n2 * sizeof(double), hipMemcpyHostToDevice);
      if ( e == hipSuccess ) e = hipMemcpy(d + o_a, A, (size_t) alen * sizeof(double), hipMemcpyHostToDevice);
      hs_ec_job E;
      memset(&E, 0, sizeof(E));
      E.n = n; E.form = form; E.ld = ld; E.A = d + o_a;
      if ( form == HS_EC_SPARSE )
      {
         E.sp.nnz = nnz;
         E.sp.voff = di; E.sp.vrow = di + m1; E.sp.vcol = di + m1 + nnz; E.sp.vval = d + o_val;
         if ( e == hipSuccess ) e = hipMemcpy(di, voff.data(), (size_t) m1 * sizeof(int), hipMemcpyHostToDevice);
         if ( nnz > 0 )
         {
            if ( e == hipSuccess ) e = hipMemcpy(di + m1, row, (size_t) nnz * sizeof(int), hipMemcpyHostToDevice);
            if ( e == hipSuccess ) e = hipMemcpy(di + m1 + nnz, col, (size_t) nnz * sizeof(int), hipMemcpyHostToDevice);
            if ( e == hipSuccess ) e = hipMemcpy(d + o_val, val, (size_t) nnz * sizeof(double), hipMemcpyHostToDevice);
         }
      }
      J.lam_src = d + o_ls; J.V_src = d + o_vs; J.lam = d + o_l; J.V = d + o_v;
      J.VT = J.route == 0 ? d + o_vt : NULL;
      J.part = d + o_part;
      J.row0 = 0; J.vec0 = 0;
      if ( e == hipSuccess ) e = hipMemcpy(dt, &J, sizeof(J), hipMemcpyHostToDevice);
      if ( e == hipSuccess ) e = hipMemcpy(dt + sizeof(J), &E, sizeof(E), hipMemcpyHostToDevice);
      if ( e != hipSuccess ) { hs_record_hip_error(e, "hs_rf_coefs_host", __FILE__, __LINE__); rc = HS_ERR_HIP; break; }
      const hs_rf_job* dj = reinterpret_cast<const hs_rf_job*>(dt);
      const hs_ec_job* de = reinterpret_cast<const hs_ec_job*>(dt + sizeof(J));
      double* r = d + o_res;
      if ( (rc = hs_rf_gather(NULL, 1, dj)) != HS_OK ) break;
      if ( (rc = hs_rf_coefs_scalar(NULL, 1, n, m, de, dj)) != HS_OK ) break;
      if ( (rc = hs_rf_coefs_mc(NULL, 1, hs_rf_tiles(n, m, J.slices), m, de, dj)) != HS_OK ) break;
      /* eig [n] | obj [n] | coef [n m] */
      if ( (rc = hs_rf_store(NULL, 1, m, dj, r, r + n, r + 2 * n, NULL)) != HS_OK ) break;
      e = hipMemcpy(res.data(), r, res.size() * sizeof(double), hipMemcpyDeviceToHost);
      if ( e != hipSuccess ) { hs_record_hip_error(e, "hs_rf_coefs_host (result)", __FILE__, __LINE__); rc = HS_ERR_HIP; }
   } while ( false );
   if ( d != NULL ) (void) hipFree(d);
   if ( di != NULL ) (void) hipFree(di);
   if ( dt != NULL ) (void) hipFree(dt);
   if ( rc != HS_OK )
      return rc;
   for (long long j = 0; j < n; ++j)
   {
      out[j * m1] = res[(size_t) (n + j)];
      for (int i = 0; i < m; ++i)
         out[j * m1 + 1 + i] = res[(size_t) (2 * n + j * m + i)];
   }
   return HS_OK;
}
