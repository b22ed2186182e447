/* onevar_large.hip - the host side of hipsdp_onevar_bounds_large: the one-variable SDPs of blocks of 129 .. 512 rows.
 *
 * The jobs are those of hipsdp_onevar_bounds_all (onevar.hip): M_i(mu) = Z_b(u) + (mu - u_i) A_i, the semismooth Newton method of
 * SCIPsolveOneVarSDPDense per job.  Above 128 rows the eigenpair of a job is the tridiagonal path of syevx.hip - one launch per column -,
 * so the loop of a job cannot stay inside one launch.  The JOBS go into the launches instead: the call runs as ROUNDS, round r is
 * evaluation r of every job that is still active, and every launch of a round is batched over the jobs:
 *     form M (k_onevar_large_form, eigi.hip) | nmax - 1 column launches (k_syevx_col_many) | values | vector of T | back-transformation
 *     (hs_syevx_many_select) | decide (k_onevar_large_decide: g, the branch of ov_decide, the next point or the result) | count
 * = nmax + 5 launches, whatever the number of jobs and blocks; then ONE int comes back, the number of jobs that go on.  In front of
 * the rounds k_ec_form_z forms Z_b(u) of the blocks with a NEWTON or TWOPOINT job (none: left out).  With R rounds (the most
 * tridiagonalisations a job needed) a chunk issues  z + R (nmax + 5)  launches, z = 1 with Z(u) and 0 without, and R + 1 read-backs
 * (the last one carries the result rows).
 *
 * A job needs hs_syevx_ws(n) + HS_SXM_OUT(n) doubles (4.7 MB at 512 rows) in the solver's grow-only cut workspace, so the jobs are
 * ordered by descending n and run in CHUNKS of at most 512 MiB of such workspace (HIPSDP_ONEVAR_LARGE_CHUNK in the environment: a job
 * count instead; hs_chunks.h), one chunk after the other on the solver's stream; the layout of a chunk: hs_ovl_layout, hs_cut_plan.h.  A chunk is a
 * call of its own in everything but the entry: its blocks, their Z(u), its rounds, its read-backs.  The bits of a job depend on
 * nothing but the job: every entry of M has one writer, no sum crosses workgroups, and the number of workgroups per job (fewer when
 * there are many jobs) only decides who owns which rows.
 *
 * DECLINED (an infinite bound) is decided here, before anything is read: such a job never reaches the device.
 * The solver is seen through hs_solver_dims, hs_solver_block_n, hs_solver_cut_enter_large and hs_solver_cut_blocks (hs_kernels.h). */
#include "hs_common.h"
#include "hs_kernels.h"
#include "hs_chunks.h"
#include "hs_cut_stats.h"
#include "../../include/hipsdp.h"
#include <algorithm>
#include <cstring>
#include <vector>

static CutStats g_ovl;

static_assert(sizeof(hs_sxm_job) == 6 * sizeof(double), "hs_ovl_layout: jobw");
#define OVL_JOBW 6
#define OVL_BUDGET (512LL * 1024 * 1024 / (long long) sizeof(double))     /* doubles of job workspace per chunk */

extern "C" int hipsdp_onevar_bounds_large_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_ovl.get(calls, launches, readbacks);
}

long long hs_onevar_large_job_len(int n)
{
   return (((long long) hs_syevx_ws(n) + 1) & ~1LL) + HS_SXM_OUT(n);
}

void hs_onevar_large_plan(int m, int count, const hs_ovl_row* rows, long long z_len, hs_ovl_layout* L, std::vector<long long>* ws,
   std::vector<long long>* out)
{
   std::vector<long long> wl((size_t) count), ol((size_t) count);
   for (int k = 0; k < count; ++k)
   {
      wl[k] = (long long) hs_syevx_ws(rows[k].n);
      ol[k] = HS_SXM_OUT(rows[k].n);
   }
   ws->assign((size_t) count, 0);
   out->assign((size_t) count, 0);
   hs_ovl_layout_make(m, count, HS_OVA_TAB, OVL_JOBW, HS_OV_RES, HS_OVL_STATE, z_len, wl.data(), ol.data(), ws->data(), out->data(), L);
}

int hs_onevar_large_chunk(hipStream_t st, const hs_ovl_chunk* c, const hs_ovl_layout& L, const std::vector<long long>& ws,
   const std::vector<long long>& out, long long* launches, long long* readbacks, int* rounds)
{
   const int count = c->count;
   if ( count < 1 || c->rows == NULL || c->dblocks == NULL || c->dev == NULL || c->pin == NULL || c->maxevals < 1
      || (int) ws.size() != count || (int) out.size() != count || (c->nz > 0 && c->u == NULL) )
      return HS_ERR_ARG;
   double* pin = c->pin;
   double* dev = c->dev;
   if ( c->m > 0 && c->u != NULL )
      memcpy(pin + L.u, c->u, (size_t) c->m * sizeof(double));
   hs_sxm_job* hjobs = reinterpret_cast<hs_sxm_job*>(pin + L.jobs);
   int* hact = reinterpret_cast<int*>(pin + L.act);
   int nmax = 0, both = 0;
   for (int k = 0; k < count; ++k)
   {
      const hs_ovl_row& r = c->rows[k];
      double* t = pin + L.tab + (long long) k * HS_OVA_TAB;
      t[0] = (double) r.var; t[1] = (double) r.kind; t[2] = r.lb; t[3] = r.ub; t[4] = r.shift;
      t[5] = (double) r.entry; t[6] = (double) k; t[7] = 0.0;
      HS_CALL( hs_syevx_many_job(r.n, dev + ws[k], dev + out[k], &hjobs[k]) );
      hact[k] = HS_SXM_ACTIVE | (r.kind == HIPSDP_ONEVAR_NEWTON ? HS_SXM_VEC : 0) | (r.kind == HS_OV_KIND_EXTREMES ? HS_SXM_BOTH : 0);
      both |= r.kind == HS_OV_KIND_EXTREMES ? 1 : 0;
      nmax = r.n > nmax ? r.n : nmax;
   }
   int* hnact = reinterpret_cast<int*>(pin + L.nactive);
   hnact[0] = 0; hnact[1] = 0;
   HS_HIP( hipMemcpyAsync(dev, pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );
   if ( c->nz > 0 )
   {
      HS_CALL( hs_ec_form_z(st, c->nz, c->nzmax, c->m, c->dblocks, dev + L.u) );
      *launches += 1;
   }
   const int cap = c->cap > 0 ? (c->cap < 128 ? c->cap : 128) : hs_syevx_many_cap(count);
   hs_ovl_par P;
   memset(&P, 0, sizeof(P));
   P.count = count; P.maxevals = c->maxevals; P.grid = cap < 64 ? cap : 64;
   P.feastol = c->feastol; P.infinity = c->infinity;
   P.blocks = c->dblocks; P.tab = dev + L.tab;
   P.jobs = reinterpret_cast<const hs_sxm_job*>(dev + L.jobs);
   P.act = reinterpret_cast<int*>(dev + L.act);
   P.nactive = reinterpret_cast<int*>(dev + L.nactive);
   P.state = dev + L.state; P.res = dev + L.res;
   int r = 0;
   for (;;)
   {
      P.round = r;
      HS_CALL( hs_onevar_large_form(st, &P) );
      HS_CALL( hs_syevx_many_cols(st, count, nmax, cap, P.jobs, P.act) );
      HS_CALL( hs_syevx_many_select(st, count, nmax, both, P.jobs, P.act) );
      HS_CALL( hs_onevar_large_decide(st, &P) );
      *launches += nmax + 5;
      ++r;
      /* the last round a job can take brings the result rows with its count */
      const bool last = r >= c->maxevals;
      if ( last )
         HS_HIP( hipMemcpyAsync(pin + L.nactive, dev + L.nactive, (size_t) (2 + L.len.res_len) * sizeof(double), hipMemcpyDeviceToHost, st) );
      else
         HS_HIP( hipMemcpyAsync(pin + L.nactive, dev + L.nactive, sizeof(int), hipMemcpyDeviceToHost, st) );
      HS_HIP( hipStreamSynchronize(st) );
      *readbacks += 1;
      if ( hnact[0] < 0 || hnact[0] > count || (last && hnact[0] != 0) )
         return HS_ERR_NUMERIC;
      if ( last )
      {
         *rounds = r;
         return HS_OK;
      }
      if ( hnact[0] == 0 )
         break;
   }
   HS_HIP( hipMemcpyAsync(pin + L.res, dev + L.res, (size_t) L.len.res_len * sizeof(double), hipMemcpyDeviceToHost, st) );
   HS_HIP( hipStreamSynchronize(st) );
   *readbacks += 1;
   *rounds = r;
   return HS_OK;
}

extern "C" int hipsdp_onevar_bounds_large(hipsdp_solver* s, const double* u, int count, const int* blocks, const int* vars, const int* kind,
   const double* lb, const double* ub, const hipsdp_onevar_opts* opts, int* status, double* optval, double* lmin, double* grad, int* evals)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || u == NULL || lb == NULL || ub == NULL || opts == NULL || status == NULL || optval == NULL
      || count < 0 || !(opts->feastol >= 0.0) || (blocks == NULL) != (vars == NULL)
      || (blocks == NULL && (long long) count != (long long) nb * m) )
      return HIPSDP_ERR_ARG;
   for (int j = 0; j < count; ++j)
   {
      if ( blocks != NULL && (blocks[j] < 0 || blocks[j] >= nb || vars[j] < 0 || vars[j] >= m) )
         return HIPSDP_ERR_ARG;
      if ( kind != NULL && kind[j] != HIPSDP_ONEVAR_NEWTON && kind[j] != HIPSDP_ONEVAR_TWOPOINT && kind[j] != HIPSDP_ONEVAR_EXTREMES )
         return HIPSDP_ERR_ARG;
   }
   if ( count == 0 )
      return HIPSDP_OK;
   for (int j = 0; j < count; ++j)
      status[j] = -1;

   /* the blocks this call serves: whole matrices on this device, 129 .. 512 rows (none for a solver with a communicator or sharded
    * matrices) */
   std::vector<int> ids;
   HS_CALL( hs_solver_cut_enter_large(s, HIPSDP_ONEVAR_LARGE_MAXN, &ids) );
   std::vector<char> served((size_t) nb, 0);
   for (size_t k = 0; k < ids.size(); ++k)
      served[ids[k]] = hs_solver_block_n(s, ids[k]) > HIPSDP_ONEVAR_MAXN ? 1 : 0;
   auto block_of = [&](int j) { return blocks != NULL ? blocks[j] : j / m; };
   auto kind_of = [&](int j) { return kind != NULL ? kind[j] : HIPSDP_ONEVAR_NEWTON; };
   std::vector<int> list;                            /* the caller's indices of the jobs that reach the device */
   bool any = false;
   for (int j = 0; j < count; ++j)
   {
      if ( !served[block_of(j)] )
         continue;
      any = true;
      if ( hs_onevar_large_declined(kind_of(j), lb[j], ub[j], opts->infinity) )
      {
         status[j] = HIPSDP_ONEVAR_DECLINED;
         optval[j] = 0.0;
         if ( lmin != NULL ) lmin[j] = 0.0;
         if ( grad != NULL ) grad[j] = 0.0;
         if ( evals != NULL ) evals[j] = 0;
         continue;
      }
      list.push_back(j);
   }
   if ( !any )
      return HIPSDP_OK;
   std::stable_sort(list.begin(), list.end(), [&](int a, int c) { return hs_solver_block_n(s, block_of(a)) > hs_solver_block_n(s, block_of(c)); });
   const int total = (int) list.size();
   std::vector<long long> job_len((size_t) total);
   for (int k = 0; k < total; ++k)
      job_len[k] = hs_onevar_large_job_len(hs_solver_block_n(s, block_of(list[k])));
   const int maxevals = opts->maxevals > 0 ? opts->maxevals : 100;

   /* one chunk: jobs start .. end - 1 of the list */
   auto chunk = [&](int start, int end) -> int
   {
      const int cnt = end - start;
      /* the chunk's blocks, those with a NEWTON or TWOPOINT job first: k_ec_form_z runs over that head alone */
      std::vector<int> use((size_t) nb, -1), entry((size_t) nb, -1), tids;
      for (int k = start; k < end; ++k)
      {
         const int b = block_of(list[k]), needz = kind_of(list[k]) != HIPSDP_ONEVAR_EXTREMES ? 1 : 0;
         use[b] = use[b] > needz ? use[b] : needz;
      }
      int nz = 0, nzmax = 0;
      long long zlen = 0;
      std::vector<long long> zoff;
      for (int pass = 1; pass >= 0; --pass)
         for (int b = 0; b < nb; ++b)
            if ( use[b] == pass )
            {
               const int n = hs_solver_block_n(s, b);
               entry[b] = (int) tids.size();
               tids.push_back(b);
               zoff.push_back(zlen);
               zlen += hs_cut_mat_len(n);
               if ( pass == 1 ) { ++nz; nzmax = n > nzmax ? n : nzmax; }
            }
      std::vector<hs_ovl_row> rows((size_t) cnt);
      for (int k = 0; k < cnt; ++k)
      {
         const int j = list[start + k], b = block_of(j), i = vars != NULL ? vars[j] : j % m;
         hs_ovl_row& r = rows[k];
         r.n = hs_solver_block_n(s, b); r.var = i; r.kind = kind_of(j); r.entry = entry[b];
         r.lb = lb[j]; r.ub = ub[j]; r.shift = u[i];
      }
      hs_ovl_layout L;
      std::vector<long long> wso, outo;
      hs_onevar_large_plan(m, cnt, rows.data(), zlen, &L, &wso, &outo);
      for (size_t k = 0; k < zoff.size(); ++k)
         zoff[k] += L.Z;
      hs_solver_cut_ws w;
      HS_CALL( hs_solver_cut_blocks(s, tids, zoff, L.len.dev_len, L.len.pin_len, &w) );
      hs_ovl_chunk c;
      memset(&c, 0, sizeof(c));
      c.m = m; c.count = cnt; c.nz = nz; c.nzmax = nzmax; c.cap = 0; c.maxevals = maxevals;
      c.feastol = opts->feastol; c.infinity = opts->infinity;
      c.u = u; c.rows = rows.data(); c.dblocks = w.djobs; c.dev = w.dev; c.pin = w.pin;
      int rounds = 0;
      long long launches = 0, readbacks = 0;
      const int rc = hs_onevar_large_chunk(w.stream, &c, L, wso, outo, &launches, &readbacks, &rounds);
      g_ovl.launches += launches; g_ovl.readbacks += readbacks;
      HS_CALL( rc );
      for (int k = 0; k < cnt; ++k)
      {
         const int j = list[start + k];
         const double* r = w.pin + L.res + (long long) k * HS_OV_RES;
         if ( !(r[0] >= 0.0 && r[0] <= (double) HIPSDP_ONEVAR_DONE) )
            return HIPSDP_ERR_NUMERIC;
         status[j] = (int) r[0];
         optval[j] = r[1];
         if ( lmin != NULL ) lmin[j] = r[2];
         if ( grad != NULL ) grad[j] = r[3];
         if ( evals != NULL ) evals[j] = (int) r[4];
      }
      return HIPSDP_OK;
   };
   HS_CALL( hs_chunks_run(job_len.data(), total, OVL_BUDGET, hs_chunk_env("HIPSDP_ONEVAR_LARGE_CHUNK"), chunk) );
   ++g_ovl.calls;
   return HIPSDP_OK;
}
