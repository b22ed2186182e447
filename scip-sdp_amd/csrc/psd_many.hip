/* psd_many.hip - the PSD projections of all blocks of a node (or of many nodes) in one call: hipsdp_psd_project_many.
 *
 * The warm-start producer of the reference projects one block at a time (relax_sdp.c:2680-2774 for Z, :3405-3445 for X) and
 * hipsdp_psd_project (psd.hip) mirrors that: per block thirteen pool allocations, a memset, an expand launch, a one-workgroup
 * decomposition with two copies, a clamp, a GEMM, three launches for the sparsification and a synchronisation.  A block of 10-128
 * rows is work for one compute unit, so - as for the separation round (eigcuts.hip) - all jobs go into the same few launches:
 *
 *    upload          job table + all triplets, packed into the thread's pinned staging, one asynchronous copy
 *    k_pp_expand     one workgroup per job: zero the n x n slab, barrier, scatter the triplets into both triangles
 *    hs_syev_small_many (eigi.hip, unchanged)   at most three launches: the decompositions hs_syev_small_dev gives the single call
 *    k_pp_recombine  one workgroup per job: V into LDS (odd pitch), clamped eigenvalues on the fly, the upper triangle of
 *                    mode 0  R[i][j] = sum_c V[i][c] lam'_c V[j][c]     mode 1  R[i][j] = sum_k lam'_k V[k][i] V[k][j]
 *                    in ascending index order by fma; counts the kept entries per row, scans the rows, stores the job's total
 *    k_pp_write      (job, 16 rows): own prefix over the job totals, then the kept entries at the job's offset of the packed result,
 *                    row-major, by ballot-ordered compaction per 64 columns (as k_write_rows of psd.hip)
 *    read-back       totals and packed triplets sit in pinned, device-mapped memory: one synchronisation
 *
 * Hazard rule: inside a launch no workgroup reads what another workgroup writes.  The zeroing and the scatter of a
 * slab belong to the same workgroup; every workgroup of k_pp_write recomputes the prefix over the totals of the launch before.
 * A job's numbers depend on its own data alone (its slab, its workgroup, sums in a fixed order): same bits whatever the batch. */
#include "hs_kernels.h"
#include "hs_psd_plan.h"
#include "../../include/hipsdp.h"
#include <atomic>
#include <cstring>

namespace {

#define PP_NT 256

__global__ void __launch_bounds__(PP_NT) k_pp_expand(const hs_pp_job* __restrict__ jobs, const int* __restrict__ row, const int* __restrict__ col,
   const double* __restrict__ val)
{
   const hs_pp_job J = jobs[blockIdx.x];
   const int n2 = J.n * J.n;
   for (int e = threadIdx.x; e < n2; e += PP_NT)
      J.A[e] = 0.0;
   __syncthreads();                 /* (orders the workgroup's own global stores: the scatter lands on the zeroed slab) */
   for (int e = threadIdx.x; e < J.nnz; e += PP_NT)
   {
      const int r = row[J.trip + e], c = col[J.trip + e];
      const double v = val[J.trip + e];
      J.A[r * J.n + c] = v;
      J.A[c * J.n + r] = v;
   }
}

/* dynamic LDS of k_pp_recombine for a job of n rows: V with pitch n | 1, the clamped eigenvalues, two counts per row */
static size_t pp_lds(int n)
{
   return ((size_t) n * (n | 1) + n) * sizeof(double) + (size_t) 2 * n * sizeof(int);
}

/* Lane = column j, a wavefront item = 4 rows x 64 columns.  mode 0 reads V[j][c] (lane stride = the odd pitch: conflict-free) and
 * V[i][c] (one address: broadcast); mode 1 reads V[k][j] (consecutive lanes, consecutive words) and V[k][i] (broadcast). */
__global__ void __launch_bounds__(PP_NT) k_pp_recombine(const hs_pp_job* __restrict__ jobs, double eps, int mode, int* __restrict__ tot)
{
   extern __shared__ __attribute__((aligned(16))) char pp_smem[];
   const hs_pp_job J = jobs[blockIdx.x];
   const int n = J.n, ld = n | 1, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   double* sV = reinterpret_cast<double*>(pp_smem);
   double* sl = sV + n * ld;
   int* scnt = reinterpret_cast<int*>(sl + n);              /* [2 i + q]: kept entries of row i in the columns 64 q .. 64 q + 63 */
   for (int e = tid; e < n * n; e += PP_NT)
   {
      const int k = e / n;
      sV[k * ld + (e - k * n)] = J.V[e];
   }
   for (int k = tid; k < n; k += PP_NT)
   {
      const double l = J.lam[k];
      sl[k] = (l - J.minev < -eps) ? J.minev : l;
      scnt[2 * k] = 0; scnt[2 * k + 1] = 0;
   }
   __syncthreads();
   const int nq = (n + 63) >> 6, ng = (n + 3) >> 2;
   for (int item = wave; item < ng * nq; item += PP_NT / 64)
   {
      const int g = item / nq, q = item - g * nq, i0 = 4 * g;
      if ( 64 * q + 63 < i0 )
         continue;                                          /* the 64 columns lie left of the diagonal */
      const int j = 64 * q + lane, jj = j < n ? j : n - 1;
      int ii[4];
      for (int k = 0; k < 4; ++k)
         ii[k] = i0 + k < n ? i0 + k : n - 1;
      double acc[4] = {0.0, 0.0, 0.0, 0.0};
      if ( mode == 0 )
      {
         for (int c = 0; c < n; ++c)
         {
            const double s = sV[jj * ld + c] * sl[c];
            for (int k = 0; k < 4; ++k)
               acc[k] = fma(sV[ii[k] * ld + c], s, acc[k]);
         }
      }
      else
      {
         for (int c = 0; c < n; ++c)
         {
            const double s = sl[c] * sV[c * ld + jj];
            for (int k = 0; k < 4; ++k)
               acc[k] = fma(sV[c * ld + ii[k]], s, acc[k]);
         }
      }
      for (int k = 0; k < 4; ++k)
      {
         const int i = i0 + k;
         const bool in = i < n && j < n && j >= i;
         if ( in )
            J.A[i * n + j] = acc[k];
         const unsigned long long mask = __ballot(in && fabs(acc[k]) > eps);
         if ( lane == 0 && i < n )
            scnt[2 * i + q] = __popcll(mask);
      }
   }
   __syncthreads();
   if ( wave == 0 )
   {
      /* lane t owns the rows 2 t and 2 t + 1 (n <= 128) */
      const int r0 = 2 * lane, r1 = 2 * lane + 1;
      const int c0 = r0 < n ? scnt[2 * r0] + scnt[2 * r0 + 1] : 0;
      const int c1 = r1 < n ? scnt[2 * r1] + scnt[2 * r1 + 1] : 0;
      int incl = c0 + c1;
      for (int off = 1; off < 64; off <<= 1)
      {
         const int v = __shfl_up(incl, off, 64);
         if ( lane >= off )
            incl += v;
      }
      const int excl = incl - c0 - c1;
      if ( r0 < n ) J.rowoff[r0] = excl;
      if ( r1 < n ) J.rowoff[r1] = excl + c0;
      if ( lane == 63 )
      {
         J.rowoff[n] = incl;
         tot[blockIdx.x] = incl;
      }
   }
}

/* workgroup (job, y) writes the rows 16 y .. 16 y + 15 of the job: wavefront w the rows 16 y + w + 4 k.  The job's offset in the
 * packed result = sum of the totals of the jobs before it (a job that does not fit its cap takes no room and writes nothing). */
__global__ void __launch_bounds__(PP_NT) k_pp_write(const hs_pp_job* __restrict__ jobs, const int* __restrict__ tot, double eps, long long outlen,
   int* __restrict__ htot, int* __restrict__ orow, int* __restrict__ ocol, double* __restrict__ oval)
{
   __shared__ long long sh[PP_NT / 64];
   const hs_pp_job J = jobs[blockIdx.x];
   const int n = J.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
   if ( (int) blockIdx.y * 16 >= n )
      return;
   const int total = tot[blockIdx.x];
   if ( blockIdx.y == 0 && tid == 0 )
      htot[blockIdx.x] = total;
   if ( total > J.cap )
      return;
   long long before = 0;
   for (int b = tid; b < (int) blockIdx.x; b += PP_NT)
   {
      const int t = tot[b];
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
      long long pos = base + J.rowoff[r];
      for (int c0 = r; c0 < n; c0 += 64)
      {
         const int c = c0 + lane;
         const double v = c < n ? J.A[r * n + c] : 0.0;
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

/* per host thread: a stream, the pinned staging of the upload, the device block (upload mirror, slabs, offsets, totals) and the
 * pinned, device-mapped result.  All three grow only; the destructor returns them when the thread ends. */
struct pp_ctx
{
   int device;
   hipStream_t stream;
   char* hup; size_t hup_bytes;
   char* dwork; size_t dwork_bytes;
   char* hout; char* dout; size_t out_bytes;
   pp_ctx() : device(-1), stream(NULL), hup(NULL), hup_bytes(0), dwork(NULL), dwork_bytes(0), hout(NULL), dout(NULL), out_bytes(0) {}
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
      device = -1; stream = NULL; hup = dwork = hout = dout = NULL; hup_bytes = dwork_bytes = out_bytes = 0;
   }
   ~pp_ctx() { release(); }
};
thread_local pp_ctx g_pp;

int pp_context(int device, pp_ctx** out)
{
   if ( g_pp.device != device || g_pp.stream == NULL )
   {
      g_pp.release();
      HS_HIP( hipSetDevice(device) );
      HS_HIP( hipStreamCreateWithFlags(&g_pp.stream, hipStreamNonBlocking) );
      g_pp.device = device;
   }
   *out = &g_pp;
   return HS_OK;
}

/* the three buffers hold at least the given sizes afterwards (the stream is idle between calls: nothing still uses the old ones) */
int pp_grow(pp_ctx* c, size_t up, size_t work, size_t out)
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
      work += work / 2;
      HS_HIP( hipMalloc((void**) &c->dwork, work) );
      c->dwork_bytes = work;
   }
   if ( out > c->out_bytes )
   {
      if ( c->hout != NULL ) (void) hipHostFree(c->hout);
      c->hout = c->dout = NULL; c->out_bytes = 0;
      out += out / 2;
      HS_HIP( hipHostMalloc((void**) &c->hout, out, hipHostMallocMapped) );
      c->out_bytes = out;
      HS_HIP( hipHostGetDevicePointer((void**) &c->dout, c->hout, 0) );
   }
   return HS_OK;
}

size_t pp_up16(size_t b) { return (b + 15) & ~(size_t) 15; }

std::atomic<long long> g_calls(0), g_launches(0), g_readbacks(0);

/* the batched jobs of a plan; *overflow: some job did not fit its cap */
int pp_run_batched(int device, hipsdp_psd_job* jobs, const hs_pp_plan& P, double epsilon, int mode, bool* overflow)
{
   const size_t nb = P.items.size();
   pp_ctx* c = NULL;
   HS_CALL( pp_context(device, &c) );
   /* upload: [hs_pp_job table | hs_eig_job table | values | rows | columns] */
   const size_t u_tab = 0, u_eig = pp_up16(u_tab + nb * sizeof(hs_pp_job)), u_val = pp_up16(u_eig + nb * sizeof(hs_eig_job));
   const size_t u_row = pp_up16(u_val + (size_t) P.trips * sizeof(double)), u_col = pp_up16(u_row + (size_t) P.trips * sizeof(int));
   const size_t up_bytes = pp_up16(u_col + (size_t) P.trips * sizeof(int));
   /* device block: [upload mirror | matrix slabs | decomposition slabs | row offsets | totals] */
   const size_t w_a = (up_bytes + 255) & ~(size_t) 255, w_ws = w_a + (size_t) P.a_len * sizeof(double);
   const size_t w_off = w_ws + (size_t) P.ws_len * sizeof(double), w_tot = pp_up16(w_off + (size_t) P.row_len * sizeof(int));
   const size_t work_bytes = w_tot + nb * sizeof(int);
   /* result: [values | rows | columns | totals] */
   const size_t o_row = (size_t) P.out_len * sizeof(double), o_col = pp_up16(o_row + (size_t) P.out_len * sizeof(int));
   const size_t o_tot = pp_up16(o_col + (size_t) P.out_len * sizeof(int)), out_bytes = o_tot + nb * sizeof(int);
   HS_CALL( pp_grow(c, up_bytes, work_bytes, out_bytes) );
   hs_pp_job* tab = reinterpret_cast<hs_pp_job*>(c->hup + u_tab);
   hs_eig_job* eig = reinterpret_cast<hs_eig_job*>(c->hup + u_eig);
   double* uval = reinterpret_cast<double*>(c->hup + u_val);
   int* urow = reinterpret_cast<int*>(c->hup + u_row);
   int* ucol = reinterpret_cast<int*>(c->hup + u_col);
   double* dA = reinterpret_cast<double*>(c->dwork + w_a);
   double* dws = reinterpret_cast<double*>(c->dwork + w_ws);
   int* doff = reinterpret_cast<int*>(c->dwork + w_off);
   int* dtot = reinterpret_cast<int*>(c->dwork + w_tot);
   for (size_t k = 0; k < nb; ++k)
   {
      const hs_pp_item& it = P.items[k];
      const hipsdp_psd_job& J = jobs[it.job];
      hs_pp_job& T = tab[k];
      memset(&T, 0, sizeof(T));
      T.n = it.n; T.nnz = it.nnz; T.cap = it.cap; T.trip = it.trip;
      T.A = dA + it.a_off; T.lam = dws + it.ws_off; T.V = dws + it.ws_off + hs_syev_many_vecpos(it.n); T.minev = J.minev;
      T.rowoff = doff + it.row_off;
      memset(&eig[k], 0, sizeof(hs_eig_job));
      eig[k].n = it.n; eig[k].in = dA + it.a_off; eig[k].ws = dws + it.ws_off;
      if ( it.nnz > 0 )
      {
         memcpy(uval + it.trip, J.val, (size_t) it.nnz * sizeof(double));
         memcpy(urow + it.trip, J.row, (size_t) it.nnz * sizeof(int));
         memcpy(ucol + it.trip, J.col, (size_t) it.nnz * sizeof(int));
      }
   }
   hipStream_t st = c->stream;
   const hs_pp_job* dtab = reinterpret_cast<const hs_pp_job*>(c->dwork + u_tab);
   int launches = 0;
   int rc = HS_OK;
   do
   {
      hipError_t e = hipMemcpyAsync(c->dwork, c->hup, up_bytes, hipMemcpyHostToDevice, st);
      if ( e != hipSuccess ) { hs_record_hip_error(e, "hipMemcpyAsync(psd_project_many)", __FILE__, __LINE__); rc = HS_ERR_HIP; break; }
      if ( (rc = hs_pp_expand(st, (int) nb, dtab, reinterpret_cast<const int*>(c->dwork + u_row),
               reinterpret_cast<const int*>(c->dwork + u_col), reinterpret_cast<const double*>(c->dwork + u_val))) != HS_OK )
         break;
      ++launches;
      if ( (rc = hs_syev_small_many(st, (int) nb, eig, reinterpret_cast<const hs_eig_job*>(c->dwork + u_eig), &launches)) != HS_OK )
         break;
      if ( (rc = hs_pp_recombine(st, (int) nb, P.nmax, dtab, epsilon, mode, dtot)) != HS_OK )
         break;
      ++launches;
      if ( (rc = hs_pp_write(st, (int) nb, P.nmax, dtab, dtot, epsilon, P.out_len, reinterpret_cast<int*>(c->dout + o_tot),
               reinterpret_cast<int*>(c->dout + o_row), reinterpret_cast<int*>(c->dout + o_col), reinterpret_cast<double*>(c->dout))) != HS_OK )
         break;
      ++launches;
      e = hipGetLastError();
      if ( e != hipSuccess ) { hs_record_hip_error(e, "kernel launch (psd_project_many)", __FILE__, __LINE__); rc = HS_ERR_HIP; }
   } while ( false );
   g_launches += launches;
   const hipError_t es = hipStreamSynchronize(st);
   ++g_readbacks;
   if ( rc == HS_OK && es != hipSuccess )
   {
      hs_record_hip_error(es, "hipStreamSynchronize(psd_project_many)", __FILE__, __LINE__);
      rc = HS_ERR_HIP;
   }
   if ( rc != HS_OK )
      return rc;
   const int* htot = reinterpret_cast<const int*>(c->hout + o_tot);
   const double* oval = reinterpret_cast<const double*>(c->hout);
   const int* orow = reinterpret_cast<const int*>(c->hout + o_row);
   const int* ocol = reinterpret_cast<const int*>(c->hout + o_col);
   long long pos = 0;
   for (size_t k = 0; k < nb; ++k)
   {
      hipsdp_psd_job& J = jobs[P.items[k].job];
      const int t = htot[k];
      J.nnz_out = t;
      if ( t > J.cap )
      {
         *overflow = true;
         continue;
      }
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

int pp_class(int n) { return hs_syev_many_class(n); }
long long pp_scratch(int n) { return hs_syev_small_scratch(n); }

}

/* the three launches over a job table in device memory, for this file and for the recombinations of hipsdp_rounding_recombine
 * (cut_calls.hip), whose jobs point at a solver's rounding frame; nmax: the largest n of the table */
int hs_pp_expand(hipStream_t st, int count, const hs_pp_job* djobs, const int* row, const int* col, const double* val)
{
   hipLaunchKernelGGL(k_pp_expand, dim3((unsigned) count), dim3(PP_NT), 0, st, djobs, row, col, val);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_pp_recombine(hipStream_t st, int count, int nmax, const hs_pp_job* djobs, double eps, int mode, int* dtot)
{
   if ( nmax < 1 || nmax > HS_PP_MAXN )
      return HS_ERR_ARG;
   static hs_attr_mask attr_done;
   HS_CALL( hs_func_max_lds(reinterpret_cast<const void*>(&k_pp_recombine), (int) pp_lds(HS_PP_MAXN), &attr_done) );
   hipLaunchKernelGGL(k_pp_recombine, dim3((unsigned) count), dim3(PP_NT), pp_lds(nmax), st, djobs, eps, mode, dtot);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_pp_write(hipStream_t st, int count, int nmax, const hs_pp_job* djobs, const int* dtot, double eps, long long outlen, int* htot,
   int* orow, int* ocol, double* oval)
{
   hipLaunchKernelGGL(k_pp_write, dim3((unsigned) count, (unsigned) ((nmax + 15) / 16)), dim3(PP_NT), 0, st, djobs, dtot, eps, outlen, htot,
      orow, ocol, oval);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

extern "C" int hipsdp_psd_project_many(int device, int count, hipsdp_psd_job* jobs, double epsilon, int mode)
{
   const hs_pp_rules rules = {pp_class, pp_scratch};
   hs_pp_plan P;
   if ( device < 0 )
      return HIPSDP_ERR_ARG;
   HS_CALL( hs_pp_plan_make(count, jobs, mode, &rules, &P) );
   if ( count == 0 )
      return HIPSDP_OK;
   int nd = 0;
   if ( hipGetDeviceCount(&nd) != hipSuccess || nd <= 0 )
      return HIPSDP_ERR_NODEVICE;
   if ( device >= nd )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(device) );
   ++g_calls;
   bool overflow = false;
   if ( !P.items.empty() )
      HS_CALL( pp_run_batched(device, jobs, P, epsilon, mode, &overflow) );
   for (size_t k = 0; k < P.big.size(); ++k)
   {
      hipsdp_psd_job& J = jobs[P.big[k]];
      J.nnz_out = 0;
      const int rc = hs_psd_project_one(device, J.n, J.nnz, J.row, J.col, J.val, J.minev, epsilon, mode, J.cap, &J.nnz_out, J.rowout,
         J.colout, J.valout);
      ++g_readbacks;
      if ( rc == HIPSDP_ERR_ARG && J.nnz_out > J.cap )
         overflow = true;
      else if ( rc != HIPSDP_OK )
         return rc;
   }
   return overflow ? HIPSDP_ERR_ARG : HIPSDP_OK;
}

extern "C" int hipsdp_psd_project_many_stats(long long* calls, long long* launches, long long* readbacks)
{
   if ( calls != NULL ) *calls = g_calls.load();
   if ( launches != NULL ) *launches = g_launches.load();
   if ( readbacks != NULL ) *readbacks = g_readbacks.load();
   return HIPSDP_OK;
}
