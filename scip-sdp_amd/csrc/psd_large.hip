/* psd_large.hip - the PSD projections of all blocks of 129 .. 512 rows of a node (or of many nodes) in one call:
 * hipsdp_psd_project_many_large, the partner of hipsdp_psd_project_many (psd_many.hip) for the jobs that call hands, one after the
 * other, to the single-call chain (psd.hip: thirteen pool allocations, a block-Jacobi decomposition, a GEMM and a synchronisation
 * per job).  Here the decomposition goes through the tridiagonal form and every launch holds all jobs of a chunk:
 *
 *    upload            job tables + all triplets, packed into the thread's pinned staging, one asynchronous copy
 *    k_ppl_expand      (32, jobs): workgroup g of a job zeroes the rows g, g + 32, .. of the job's matrix and of its reflector array,
 *                      barrier, then scatters the triplets that fall into ITS rows (both triangles are filled)
 *    hs_syevx_many_cols (syevx.hip, unchanged)  nmax - 1 launches: the tridiagonal forms
 *    hs_syevr_many_tvec (syevr.hip)             5 + 6 ceil(nmax / 32) launches: all eigenvalues, all eigenvectors of T
 *    hs_syevr_many_back (syevr.hip)             1 launch: the back-transformation of all vectors of all jobs
 *    k_ppl_recombine   (upper-triangle tiles of 64 x 64, jobs): panels of 16 columns of the two operands go through LDS, the clamped
 *                      eigenvalues are applied as the second one is staged, the sum over k runs in ascending order on
 *                      v_mfma_f64_16x16x4_f64:
 *                      mode 0  R[i][j] = sum_c V[i][c] lam'_c V[j][c]     mode 1  R[i][j] = sum_k lam'_k V[k][i] V[k][j]
 *                      the same tile code with the two strides of V exchanged.  Stores the tile (entries with j >= i), per row of
 *                      the tile the number of kept entries (ballot), and the tile's total.
 *    k_ppl_write       (jobs, 16 rows): own prefix over the counts of the launch before (rows of the job, totals of the jobs before
 *                      it), then the kept entries at the job's offset of the packed result, row-major, by ballot-ordered
 *                      compaction per 64 columns (k_pp_write of psd_many.hip).  A job over its cap takes no room.
 *    read-back         totals and the packed triplets: one device->host copy, one synchronisation, then one memcpy per job
 *
 * Launches of a chunk: hs_ppl_launches(nmax) = nmax + 8 + 6 ceil(nmax / 32), whatever the number of jobs (hs_psd_large_plan.h).
 * Hazard rule: inside a launch no workgroup reads what another workgroup writes; the kernel boundary is the only
 * synchronisation between workgroups; every sum runs in a fixed order.  A job's numbers depend on its own data alone: same bits
 * whatever the batch, the chunking, the position and the calling thread. */
#include "hs_kernels.h"
#include "hs_psd_large_plan.h"
#include "hs_chunks.h"
#include "hs_cut_stats.h"
#include "../../include/hipsdp.h"
#include <cstring>

namespace {

#define PL_NT 256
#define PL_T  HS_PPL_TILE     /* rows and columns of an output tile: four wavefronts of 16 rows x 64 columns */
#define PL_K  16              /* columns of a panel */
#define PL_LD 80              /* pitch of a panel row in LDS: 16 doubles off a multiple of 64, so the four k of a fragment hit different banks */
#define PL_EG 32              /* workgroups per job of the expand launch */

typedef double pl_v4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(PL_NT) k_ppl_expand(const hs_ppl_job* __restrict__ jobs, const int* __restrict__ row, const int* __restrict__ col,
   const double* __restrict__ val)
{
   const hs_ppl_job J = jobs[blockIdx.y];
   const int n = J.n, g = blockIdx.x, G = gridDim.x;
   for (int i = g; i < n; i += G)
      for (int c = threadIdx.x; c < n; c += PL_NT)
      {
         J.A[(size_t) i * n + c] = 0.0;
         J.R[(size_t) i * n + c] = 0.0;
      }
   __syncthreads();                 /* (orders the workgroup's own global stores: the scatter lands on the zeroed rows) */
   for (int e = threadIdx.x; e < J.nnz; e += PL_NT)
   {
      const int r = row[J.trip + e], c = col[J.trip + e];
      const double v = val[J.trip + e];
      if ( r % G == g )
         J.A[(size_t) r * n + c] = v;
      if ( c % G == g )
         J.A[(size_t) c * n + r] = v;
   }
}

/* s[kk][xx] = operand entry (x0 + xx, k0 + kk), zero beyond n.  mode 1: entry (x, k) = V[k n + x], consecutive threads walk x;
 * mode 0: V[x n + k], consecutive threads walk k - either way a wavefront reads whole lines.  SCALE: times the clamped eigenvalue k. */
template <bool SCALE>
__device__ __forceinline__ void ppl_panel(double (*s)[PL_LD], const hs_ppl_job& J, int x0, int k0, int mode, double eps)
{
   const int n = J.n;
   for (int idx = threadIdx.x; idx < PL_K * PL_T; idx += PL_NT)
   {
      const int kk = mode == 1 ? idx / PL_T : idx % PL_K;
      const int xx = mode == 1 ? idx % PL_T : idx / PL_K;
      const int x = x0 + xx, k = k0 + kk;
      double v = 0.0;
      if ( x < n && k < n )
      {
         v = mode == 1 ? J.V[(size_t) k * n + x] : J.V[(size_t) x * n + k];
         if ( SCALE )
         {
            const double l = J.lam[k];
            v *= (l - J.minev < -eps) ? J.minev : l;
         }
      }
      s[kk][xx] = v;
   }
}

/* Tile (ti, tj), ti <= tj, of job blockIdx.y.  Wavefront w owns the rows 16 w .. 16 w + 15 of the tile and its 64 columns: four
 * accumulators of v_mfma_f64_16x16x4_f64 (lane l holds A[l & 15][l >> 4], B[l >> 4][l & 15] and D[(l >> 4) + 4 r][l & 15], r = 0 .. 3). */
__global__ void __launch_bounds__(PL_NT) k_ppl_recombine(const hs_ppl_job* __restrict__ jobs, double eps, int mode)
{
   __shared__ double sA[PL_K][PL_LD], sB[PL_K][PL_LD];
   __shared__ int swt[PL_NT / 64];
   const hs_ppl_job J = jobs[blockIdx.y];
   const int n = J.n, ntc = J.ntc;
   int ti = 0, rem = blockIdx.x;
   if ( rem >= ntc * (ntc + 1) / 2 )
      return;
   while ( rem >= ntc - ti )
   {
      rem -= ntc - ti;
      ++ti;
   }
   const int tj = ti + rem, i0 = PL_T * ti, j0 = PL_T * tj;
   const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
   pl_v4 acc[4];
#pragma unroll
   for (int c = 0; c < 4; ++c)
      acc[c] = (pl_v4) {0.0, 0.0, 0.0, 0.0};
   for (int k0 = 0; k0 < n; k0 += PL_K)
   {
      ppl_panel<false>(sA, J, i0, k0, mode, eps);
      ppl_panel<true>(sB, J, j0, k0, mode, eps);
      __syncthreads();
#pragma unroll
      for (int q = 0; q < PL_K / 4; ++q)
      {
         const double a = sA[4 * q + lk][16 * wave + lr];
#pragma unroll
         for (int c = 0; c < 4; ++c)
            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[4 * q + lk][16 * c + lr], acc[c], 0, 0, 0);
      }
      __syncthreads();
   }
   int wtot = 0;
#pragma unroll
   for (int r = 0; r < 4; ++r)
   {
      const int i = i0 + 16 * wave + lk + 4 * r;
      int rowc = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c)
      {
         const int j = j0 + 16 * c + lr;
         const double v = acc[c][r];
         const bool in = i < n && j < n && j >= i;
         if ( in )
            J.A[(size_t) i * n + j] = v;
         const unsigned long long mask = __ballot(in && fabs(v) > eps);
         rowc += __popcll((mask >> (16 * lk)) & 0xffffULL);         /* the 16 lanes that hold row i */
         wtot += __popcll(mask);
      }
      if ( lr == 0 && i < n )
         J.cnt[i * ntc + tj] = rowc;
   }
   if ( lane == 0 )
      swt[wave] = wtot;
   __syncthreads();
   if ( tid == 0 )
      J.cnt[n * ntc + ti * ntc + tj] = swt[0] + swt[1] + swt[2] + swt[3];
}

/* entries the projection of a job keeps: the totals of its upper-triangle tiles, in a fixed order */
__device__ __forceinline__ int ppl_total(const hs_ppl_job& J)
{
   const int* __restrict__ t = J.cnt + J.n * J.ntc;
   int s = 0;
   for (int ti = 0; ti < J.ntc; ++ti)
      for (int tj = ti; tj < J.ntc; ++tj)
         s += t[ti * J.ntc + tj];
   return s;
}

/* workgroup (job, y) writes the rows 16 y .. 16 y + 15 of the job: wavefront w the rows 16 y + w + 4 k.  The job's offset in the
 * packed result = sum of the totals of the jobs before it (a job that does not fit its cap takes no room and writes nothing). */
__global__ void __launch_bounds__(PL_NT) k_ppl_write(const hs_ppl_job* __restrict__ jobs, double eps, long long outlen, int* __restrict__ tot,
   int* __restrict__ orow, int* __restrict__ ocol, double* __restrict__ oval)
{
   __shared__ long long sh[PL_NT / 64];
   __shared__ int srow[HIPSDP_PSD_LARGE_MAXN];
   const hs_ppl_job J = jobs[blockIdx.x];
   const int n = J.n, ntc = J.ntc, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   if ( (int) blockIdx.y * 16 >= n )
      return;
   const int total = ppl_total(J);
   if ( blockIdx.y == 0 && tid == 0 )
      tot[blockIdx.x] = total;
   if ( total > J.cap )
      return;
   for (int r = tid; r < n; r += PL_NT)
   {
      int s = 0;
      for (int q = r / PL_T; q < ntc; ++q)
         s += J.cnt[r * ntc + q];
      srow[r] = s;
   }
   long long before = 0;
   for (int b = tid; b < (int) blockIdx.x; b += PL_NT)
   {
      const int t = ppl_total(jobs[b]);
      before += t <= jobs[b].cap ? t : 0;
   }
   for (int off = 32; off > 0; off >>= 1)
      before += __shfl_down(before, off, 64);
   if ( lane == 0 )
      sh[wave] = before;
   __syncthreads();
   const long long base = sh[0] + sh[1] + sh[2] + sh[3];
   for (int k = 0; k < 4; ++k)
   {
      const int r = (int) blockIdx.y * 16 + wave + 4 * k;
      if ( r >= n )
         break;
      int part = 0;
      for (int rr = lane; rr < r; rr += 64)
         part += srow[rr];
      for (int off = 32; off > 0; off >>= 1)
         part += __shfl_xor(part, off, 64);
      long long pos = base + part;
      for (int c0 = r; c0 < n; c0 += 64)
      {
         const int c = c0 + lane;
         const double v = c < n ? J.A[(size_t) r * n + c] : 0.0;
         const bool keep = c < n && fabs(v) > eps;
         const unsigned long long mask = __ballot(keep);
         const long long at = pos + __popcll(mask & ((1ULL << lane) - 1ULL));
         if ( keep && at < outlen )
         {
            orow[at] = r;
            ocol[at] = c;
            oval[at] = v;
         }
         pos += __popcll(mask);
      }
   }
}

/* per host thread: a stream, the pinned staging of the upload, the device block (upload mirror, slabs, counts, result) and the
 * pinned mirror of the result.  All three grow only; the destructor returns them when the thread ends. */
struct ppl_ctx
{
   int device;
   hipStream_t stream;
   char* hup; size_t hup_bytes;
   char* dwork; size_t dwork_bytes;
   char* hout; size_t out_bytes;
   ppl_ctx() : device(-1), stream(NULL), hup(NULL), hup_bytes(0), dwork(NULL), dwork_bytes(0), hout(NULL), out_bytes(0) {}
   void release()
   {
      if ( device >= 0 )
         (void) hipSetDevice(device);
      if ( stream != NULL )
      {
         (void) hipStreamSynchronize(stream);
         (void) hipStreamDestroy(stream);
      }
      if ( hup != NULL ) (void) hipHostFree(hup);
      if ( hout != NULL ) (void) hipHostFree(hout);
      if ( dwork != NULL ) (void) hipFree(dwork);
      device = -1; stream = NULL; hup = dwork = hout = NULL; hup_bytes = dwork_bytes = out_bytes = 0;
   }
   ~ppl_ctx() { release(); }
};
thread_local ppl_ctx g_ppl;

int ppl_context(int device, ppl_ctx** out)
{
   if ( g_ppl.device != device || g_ppl.stream == NULL )
   {
      g_ppl.release();
      HS_HIP( hipSetDevice(device) );
      HS_HIP( hipStreamCreateWithFlags(&g_ppl.stream, hipStreamNonBlocking) );
      g_ppl.device = device;
   }
   *out = &g_ppl;
   return HS_OK;
}

/* the three buffers hold at least the given sizes afterwards (the stream is idle between chunks: nothing still uses the old ones) */
int ppl_grow(ppl_ctx* c, size_t up, size_t work, size_t out)
{
   if ( up > c->hup_bytes )
   {
      if ( c->hup != NULL ) (void) hipHostFree(c->hup);
      c->hup = NULL; c->hup_bytes = 0;
      up += up / 2;
      HS_HIP( hipHostMalloc((void**) &c->hup, up, hipHostMallocDefault) );
      c->hup_bytes = up;
   }
   if ( work > c->dwork_bytes )
   {
      if ( c->dwork != NULL ) (void) hipFree(c->dwork);
      c->dwork = NULL; c->dwork_bytes = 0;
      work += work / 4;
      HS_HIP( hipMalloc((void**) &c->dwork, work) );
      c->dwork_bytes = work;
   }
   if ( out > c->out_bytes )
   {
      if ( c->hout != NULL ) (void) hipHostFree(c->hout);
      c->hout = NULL; c->out_bytes = 0;
      out += out / 2;
      HS_HIP( hipHostMalloc((void**) &c->hout, out, hipHostMallocDefault) );
      c->out_bytes = out;
   }
   return HS_OK;
}

size_t ppl_up16(size_t b) { return (b + 15) & ~(size_t) 15; }
size_t ppl_up256(size_t b) { return (b + 255) & ~(size_t) 255; }

CutStats g_stats;

long long ppl_ws_len(int n) { return (long long) hs_syevr_ws(n); }
long long ppl_out_len(int n) { return HS_SYEVR_OUT(n); }

/* one chunk of served jobs; *overflow: some job did not fit its cap */
int ppl_run_chunk(int device, hipsdp_psd_job* jobs, const std::vector<hs_ppl_item>& items, const hs_ppl_chunk& C, double epsilon, int mode,
   bool* overflow)
{
   const size_t nb = (size_t) (C.end - C.first);
   ppl_ctx* c = NULL;
   HS_CALL( ppl_context(device, &c) );
   /* upload: [hs_ppl_job table | hs_sxm_job table | hs_srm_job table | act | values | rows | columns] */
   const size_t u_tab = 0, u_sx = ppl_up16(u_tab + nb * sizeof(hs_ppl_job)), u_sr = ppl_up16(u_sx + nb * sizeof(hs_sxm_job));
   const size_t u_act = ppl_up16(u_sr + nb * sizeof(hs_srm_job)), u_val = ppl_up16(u_act + nb * sizeof(int));
   const size_t u_row = ppl_up16(u_val + (size_t) C.trips * sizeof(double)), u_col = ppl_up16(u_row + (size_t) C.trips * sizeof(int));
   const size_t up_bytes = ppl_up16(u_col + (size_t) C.trips * sizeof(int));
   /* device block: [upload mirror | decomposition workspaces | eigenpairs | counts | result: totals, values, rows, columns] */
   const size_t w_ws = ppl_up256(up_bytes), w_out = ppl_up256(w_ws + (size_t) C.ws_len * sizeof(double));
   const size_t w_cnt = ppl_up256(w_out + (size_t) C.out_len * sizeof(double)), w_res = ppl_up256(w_cnt + (size_t) C.cnt_len * sizeof(int));
   const size_t o_val = ppl_up16(nb * sizeof(int)), o_row = o_val + (size_t) C.res_len * sizeof(double);
   const size_t o_col = ppl_up16(o_row + (size_t) C.res_len * sizeof(int)), res_bytes = ppl_up16(o_col + (size_t) C.res_len * sizeof(int));
   HS_CALL( ppl_grow(c, up_bytes, w_res + res_bytes, res_bytes) );
   hs_ppl_job* tab = reinterpret_cast<hs_ppl_job*>(c->hup + u_tab);
   hs_sxm_job* sx = reinterpret_cast<hs_sxm_job*>(c->hup + u_sx);
   hs_srm_job* sr = reinterpret_cast<hs_srm_job*>(c->hup + u_sr);
   int* act = reinterpret_cast<int*>(c->hup + u_act);
   double* uval = reinterpret_cast<double*>(c->hup + u_val);
   int* urow = reinterpret_cast<int*>(c->hup + u_row);
   int* ucol = reinterpret_cast<int*>(c->hup + u_col);
   double* dws = reinterpret_cast<double*>(c->dwork + w_ws);
   double* dout = reinterpret_cast<double*>(c->dwork + w_out);
   int* dcnt = reinterpret_cast<int*>(c->dwork + w_cnt);
   char* dres = c->dwork + w_res;
   for (size_t k = 0; k < nb; ++k)
   {
      const hs_ppl_item& it = items[(size_t) C.first + k];
      const hipsdp_psd_job& J = jobs[it.job];
      HS_CALL( hs_syevx_many_job(it.n, dws + it.ws_off, dout + it.out_off, &sx[k]) );       /* (its selection output is not used) */
      HS_CALL( hs_syevr_many_job(it.n, dws + it.ws_off, dout + it.out_off, &sr[k]) );
      act[k] = HS_SXM_ACTIVE;
      hs_ppl_job& T = tab[k];
      memset(&T, 0, sizeof(T));
      T.n = it.n; T.nnz = it.nnz; T.cap = it.cap; T.ntc = it.ntc; T.trip = it.trip;
      T.A = sx[k].A; T.R = sx[k].R; T.lam = dout + it.out_off; T.V = dout + it.out_off + HS_SYEVR_OUT_VEC(it.n);
      T.minev = J.minev; T.cnt = dcnt + it.cnt_off;
      if ( it.nnz > 0 )
      {
         memcpy(uval + it.trip, J.val, (size_t) it.nnz * sizeof(double));
         memcpy(urow + it.trip, J.row, (size_t) it.nnz * sizeof(int));
         memcpy(ucol + it.trip, J.col, (size_t) it.nnz * sizeof(int));
      }
   }
   hipStream_t st = c->stream;
   const hs_ppl_job* dtab = reinterpret_cast<const hs_ppl_job*>(c->dwork + u_tab);
   const hs_sxm_job* dsx = reinterpret_cast<const hs_sxm_job*>(c->dwork + u_sx);
   const hs_srm_job* dsr = reinterpret_cast<const hs_srm_job*>(c->dwork + u_sr);
   const int* dact = reinterpret_cast<const int*>(c->dwork + u_act);
   int launches = 0;
   int rc = HS_OK;
   do
   {
      hipError_t e = hipMemcpyAsync(c->dwork, c->hup, up_bytes, hipMemcpyHostToDevice, st);
      if ( e != hipSuccess ) { hs_record_hip_error(e, "hipMemcpyAsync(psd_project_many_large)", __FILE__, __LINE__); rc = HS_ERR_HIP; break; }
      if ( (rc = hs_ppl_expand(st, (int) nb, dtab, reinterpret_cast<const int*>(c->dwork + u_row),
               reinterpret_cast<const int*>(c->dwork + u_col), reinterpret_cast<const double*>(c->dwork + u_val))) != HS_OK )
         break;
      ++launches;
      if ( (rc = hs_syevx_many_cols(st, (int) nb, C.nmax, hs_syevx_many_cap((int) nb), dsx, dact)) != HS_OK )
         break;
      launches += C.nmax - 1;
      if ( (rc = hs_syevr_many_tvec(st, (int) nb, C.nmax, dsr)) != HS_OK )
         break;
      launches += 5 + 6 * ((C.nmax + 31) / 32);
      if ( (rc = hs_syevr_many_back(st, (int) nb, C.nmax, dsr)) != HS_OK )
         break;
      ++launches;
      if ( (rc = hs_ppl_recombine(st, (int) nb, C.nmax, dtab, epsilon, mode)) != HS_OK )
         break;
      ++launches;
      if ( (rc = hs_ppl_write(st, (int) nb, C.nmax, dtab, epsilon, C.res_len, reinterpret_cast<int*>(dres), reinterpret_cast<int*>(dres + o_row),
               reinterpret_cast<int*>(dres + o_col), reinterpret_cast<double*>(dres + o_val))) != HS_OK )
         break;
      ++launches;
      e = hipGetLastError();
      if ( e != hipSuccess ) { hs_record_hip_error(e, "kernel launch (psd_project_many_large)", __FILE__, __LINE__); rc = HS_ERR_HIP; break; }
      e = hipMemcpyAsync(c->hout, dres, res_bytes, hipMemcpyDeviceToHost, st);
      if ( e != hipSuccess ) { hs_record_hip_error(e, "hipMemcpyAsync(psd_project_many_large, result)", __FILE__, __LINE__); rc = HS_ERR_HIP; }
   } while ( false );
   g_stats.launches += launches;
   const hipError_t es = hipStreamSynchronize(st);
   ++g_stats.readbacks;
   if ( rc == HS_OK && es != hipSuccess )
   {
      hs_record_hip_error(es, "hipStreamSynchronize(psd_project_many_large)", __FILE__, __LINE__);
      rc = HS_ERR_HIP;
   }
   if ( rc != HS_OK )
      return rc;
   const int* htot = reinterpret_cast<const int*>(c->hout);
   const double* oval = reinterpret_cast<const double*>(c->hout + o_val);
   const int* orow = reinterpret_cast<const int*>(c->hout + o_row);
   const int* ocol = reinterpret_cast<const int*>(c->hout + o_col);
   long long pos = 0;
   for (size_t k = 0; k < nb; ++k)
   {
      hipsdp_psd_job& J = jobs[items[(size_t) C.first + k].job];
      const int t = htot[k];
      J.nnz_out = t;
      if ( t > J.cap )
      {
         *overflow = true;
         continue;
      }
      if ( t < 0 || pos + t > C.res_len )
         return HS_ERR_NUMERIC;
      if ( t > 0 )
      {
         memcpy(J.valout, oval + pos, (size_t) t * sizeof(double));
         memcpy(J.rowout, orow + pos, (size_t) t * sizeof(int));
         memcpy(J.colout, ocol + pos, (size_t) t * sizeof(int));
      }
      pos += t;
   }
   return HS_OK;
}

}

/* the three launches over a job table in device memory, for this file and for hipsdp_rounding_frame / hipsdp_rounding_recombine
 * (cut_calls.hip): the expand launch writes X where the column launches read it, the recombination and the write run on jobs that point
 * at a solver's rounding frame (minev = -infinity: no eigenvalue is raised); nmax: the largest n of the table */
int hs_ppl_expand(hipStream_t st, int count, const hs_ppl_job* djobs, const int* row, const int* col, const double* val)
{
   hipLaunchKernelGGL(k_ppl_expand, dim3(PL_EG, (unsigned) count), dim3(PL_NT), 0, st, djobs, row, col, val);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_ppl_recombine(hipStream_t st, int count, int nmax, const hs_ppl_job* djobs, double eps, int mode)
{
   if ( nmax < 1 || nmax > HIPSDP_PSD_LARGE_MAXN )
      return HS_ERR_ARG;
   const int ntc = (nmax + PL_T - 1) / PL_T;
   hipLaunchKernelGGL(k_ppl_recombine, dim3((unsigned) (ntc * (ntc + 1) / 2), (unsigned) count), dim3(PL_NT), 0, st, djobs, eps, mode);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_ppl_write(hipStream_t st, int count, int nmax, const hs_ppl_job* djobs, double eps, long long outlen, int* tot, int* orow, int* ocol,
   double* oval)
{
   hipLaunchKernelGGL(k_ppl_write, dim3((unsigned) count, (unsigned) ((nmax + 15) / 16)), dim3(PL_NT), 0, st, djobs, eps, outlen, tot, orow,
      ocol, oval);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

/* the batched decomposition alone on `count` dense host matrices of mixed sizes (129 .. 512 rows each), for the unit entry
 * hipsdp_syevr_many_unit (units.hip): the matrices into the heads of their workspaces, reflector arrays cleared, the column launches
 * with `cap` workgroups per matrix at most, stages 2 to 4; lam and V per matrix one after the other */
int hs_ppl_syevr_many_host(int device, int count, const int* n, const double* A, int cap, double* lam, double* V)
{
   if ( count < 1 || count > HIPSDP_PSD_MANY_MAXJOBS || n == NULL || A == NULL || cap < 1 || cap > 128 || lam == NULL || V == NULL )
      return HS_ERR_ARG;
   int nmax = 0;
   long long ws_len = 0, out_len = 0;
   for (int j = 0; j < count; ++j)
   {
      if ( n[j] < HIPSDP_PSD_LARGE_MINN || n[j] > HIPSDP_PSD_LARGE_MAXN )
         return HS_ERR_ARG;
      nmax = n[j] > nmax ? n[j] : nmax;
      ws_len += (ppl_ws_len(n[j]) + 31) & ~31LL;
      out_len += (ppl_out_len(n[j]) + 31) & ~31LL;
   }
   ppl_ctx* c = NULL;
   HS_CALL( ppl_context(device, &c) );
   const size_t nb = (size_t) count;
   const size_t u_sx = 0, u_sr = ppl_up16(u_sx + nb * sizeof(hs_sxm_job)), u_act = ppl_up16(u_sr + nb * sizeof(hs_srm_job));
   const size_t up_bytes = ppl_up16(u_act + nb * sizeof(int));
   const size_t w_ws = ppl_up256(up_bytes), w_out = ppl_up256(w_ws + (size_t) ws_len * sizeof(double));
   const size_t work = w_out + (size_t) out_len * sizeof(double);
   HS_CALL( ppl_grow(c, up_bytes, work, (size_t) out_len * sizeof(double)) );
   hs_sxm_job* sx = reinterpret_cast<hs_sxm_job*>(c->hup + u_sx);
   hs_srm_job* sr = reinterpret_cast<hs_srm_job*>(c->hup + u_sr);
   int* act = reinterpret_cast<int*>(c->hup + u_act);
   double* dws = reinterpret_cast<double*>(c->dwork + w_ws);
   double* dout = reinterpret_cast<double*>(c->dwork + w_out);
   std::vector<long long> oo(nb);
   long long wo = 0, ooff = 0;
   for (size_t k = 0; k < nb; ++k)
   {
      HS_CALL( hs_syevx_many_job(n[k], dws + wo, dout + ooff, &sx[k]) );
      HS_CALL( hs_syevr_many_job(n[k], dws + wo, dout + ooff, &sr[k]) );
      act[k] = HS_SXM_ACTIVE;
      oo[k] = ooff;
      wo += (ppl_ws_len(n[k]) + 31) & ~31LL;
      ooff += (ppl_out_len(n[k]) + 31) & ~31LL;
   }
   hipStream_t st = c->stream;
   HS_HIP( hipMemcpyAsync(c->dwork, c->hup, up_bytes, hipMemcpyHostToDevice, st) );
   HS_HIP( hipStreamSynchronize(st) );
   /* the matrices: the symmetric matrix the single-matrix path builds from the triangle at [c n + i], i >= c; reflector arrays zero */
   std::vector<double> sym;
   const double* in = A;
   for (size_t k = 0; k < nb; ++k)
   {
      const int nn = n[k];
      sym.resize((size_t) nn * nn);
      for (int i = 0; i < nn; ++i)
         for (int cc = 0; cc < nn; ++cc)
            sym[(size_t) i * nn + cc] = (cc <= i) ? in[(size_t) cc * nn + i] : in[(size_t) i * nn + cc];
      HS_HIP( hipMemcpy(sx[k].A, sym.data(), (size_t) nn * nn * sizeof(double), hipMemcpyHostToDevice) );
      HS_HIP( hipMemset(sx[k].R, 0, (size_t) nn * nn * sizeof(double)) );
      in += (size_t) nn * nn;
   }
   HS_HIP( hipDeviceSynchronize() );
   const hs_sxm_job* dsx = reinterpret_cast<const hs_sxm_job*>(c->dwork + u_sx);
   const hs_srm_job* dsr = reinterpret_cast<const hs_srm_job*>(c->dwork + u_sr);
   HS_CALL( hs_syevx_many_cols(st, count, nmax, cap, dsx, reinterpret_cast<const int*>(c->dwork + u_act)) );
   HS_CALL( hs_syevr_many_tvec(st, count, nmax, dsr) );
   HS_CALL( hs_syevr_many_back(st, count, nmax, dsr) );
   HS_HIP( hipMemcpyAsync(c->hout, dout, (size_t) out_len * sizeof(double), hipMemcpyDeviceToHost, st) );
   HS_HIP( hipStreamSynchronize(st) );
   const double* ho = reinterpret_cast<const double*>(c->hout);
   for (size_t k = 0; k < nb; ++k)
   {
      const int nn = n[k];
      memcpy(lam, ho + oo[k], (size_t) nn * sizeof(double));
      memcpy(V, ho + oo[k] + HS_SYEVR_OUT_VEC(nn), (size_t) nn * nn * sizeof(double));
      lam += nn;
      V += (size_t) nn * nn;
   }
   return HS_OK;
}

extern "C" int hipsdp_psd_project_many_large(int device, int count, hipsdp_psd_job* jobs, double epsilon, int mode)
{
   const hs_ppl_rules rules = {ppl_ws_len, ppl_out_len};
   if ( device < 0 )
      return HIPSDP_ERR_ARG;
   HS_CALL( hs_ppl_check(count, jobs, mode) );
   if ( count == 0 )
      return HIPSDP_OK;
   int nd = 0;
   if ( hipGetDeviceCount(&nd) != hipSuccess || nd <= 0 )
      return HIPSDP_ERR_NODEVICE;
   if ( device >= nd )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(device) );
   ++g_stats.calls;
   std::vector<hs_ppl_item> items;
   HS_CALL( hs_ppl_items(count, jobs, &rules, &items) );
   /* a job this call does not serve: nnz_out = -1, nothing written (the convention of hipsdp_eigencuts_all_large) */
   for (int j = 0; j < count; ++j)
      if ( jobs[j].n < HIPSDP_PSD_LARGE_MINN || jobs[j].n > HIPSDP_PSD_LARGE_MAXN )
         jobs[j].nnz_out = -1;
   const int mib = hs_chunk_env("HIPSDP_PSD_LARGE_CHUNK");             /* MiB of workspace per chunk (read at every call) */
   const long long budget = (mib > 0 ? mib : 512LL) * 1024 * 1024;
   bool overflow = false;
   for (int start = 0; start < (int) items.size(); )
   {
      hs_ppl_chunk C;
      HS_CALL( hs_ppl_chunk_make(&items, start, budget, &rules, &C) );
      HS_CALL( ppl_run_chunk(device, jobs, items, C, epsilon, mode, &overflow) );
      start = C.end;
   }
   return overflow ? HIPSDP_ERR_ARG : HIPSDP_OK;
}

extern "C" int hipsdp_psd_project_many_large_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_stats.get(calls, launches, readbacks);
}
