/* onevar.hip - the host side of hipsdp_onevar_bounds: all one-variable SDPs of a block in one call.
 *
 * Reference: tightenBounds (cons_sdp.c:1968-2201) and tightenMatrices (:1856-1961) build, per variable i of a block, the constant
 * matrix C_i = A_0 - sum_{k != i} ub_k A_k (:2072-2099) and hand  mu A_i - C_i  to SCIPsolveOneVarSDPDense (solveonevarsdp.c:370-533).
 * With Z(u) = sum_k u_k A_k - A_0 that matrix is  Z(u) + (mu - u_i) A_i:  ONE Z(u) serves every variable of the block (k_ec_form_z,
 * eigcuts.hip, with the block as the only job), and the loop over i never changes u, so the jobs are independent: one workgroup per
 * job runs the whole Newton loop (k_onevar_small / k_onevar_mid, eigi.hip).
 *
 * The call: argument checks (before the device is looked at), one buffer  u[m] | job table [count][HS_OV_TAB]  through the pinned
 * mirror of the cut workspace and ONE upload, TWO launches, ONE read-back of [count][HS_OV_RES].  Workspace (doubles, device):
 *     u[m] | table | result | Z (n^2) | slabs (hs_onevar_slab: 2 n^2 per job above 64 rows)
 * the pinned mirror holds the first three.
 *
 * The solver is seen through hs_solver_dims, hs_solver_block_n and hs_solver_cut_job (hs_kernels.h) alone: the last one hands out the
 * cut workspace with the block as its only job, no decomposition slab (wsoff = -1).  The counters are a CutStats, as those of the cut
 * calls (cut_calls.hip).
 *
 * hipsdp_onevar_bounds_all (below) is the same round over ALL blocks of the solver in one call: a job names its block, the table of
 * hs_ec_job is that of the blocks with jobs (hs_solver_cut_enter / hs_solver_cut_blocks), and the launches are k_ec_form_z over the
 * blocks that have a NEWTON or TWOPOINT job plus one launch per size class (hs_onevar_all, eigi.hip).  Its layout: hs_ova_layout,
 * hs_cut_plan.h. */
#include "hs_common.h"
#include "hs_kernels.h"
#include "hs_cut_stats.h"
#include "../../include/hipsdp.h"
#include <algorithm>
#include <cstring>
#include <vector>

static CutStats g_ov;
static CutStats g_ova;       /* hipsdp_onevar_bounds_all */

extern "C" int hipsdp_onevar_bounds_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_ov.get(calls, launches, readbacks);
}

extern "C" int hipsdp_onevar_bounds(hipsdp_solver* s, int block, const double* u, int count, const int* vars, const int* kind,
   const double* lb, const double* ub, const hipsdp_onevar_opts* opts, int* status, double* optval, double* lmin, double* grad, int* evals)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || block < 0 || block >= nb || u == NULL || lb == NULL || ub == NULL || opts == NULL || status == NULL
      || optval == NULL || count < 0 || !(opts->feastol >= 0.0) || (vars == NULL && count != m) )
      return HIPSDP_ERR_ARG;
   for (int j = 0; j < count; ++j)
   {
      if ( vars != NULL && (vars[j] < 0 || vars[j] >= m) )
         return HIPSDP_ERR_ARG;
      if ( kind != NULL && kind[j] != HIPSDP_ONEVAR_NEWTON && kind[j] != HIPSDP_ONEVAR_TWOPOINT )
         return HIPSDP_ERR_ARG;
   }
   if ( count == 0 )
      return HIPSDP_OK;
   const int n = hs_solver_block_n(s, block);
   for (int j = 0; j < count; ++j)
      status[j] = -1;
   if ( n > HIPSDP_ONEVAR_MAXN )
      return HIPSDP_OK;

   const long long tab = m, res = tab + (long long) count * HS_OV_TAB, zoff = res + (long long) count * HS_OV_RES;
   const long long slab = zoff + (long long) n * n;
   hs_solver_cut_ws w;
   int served = 0;
   HS_CALL( hs_solver_cut_job(s, block, slab + hs_onevar_slab(n, count), zoff, zoff, -1, &w, &served) );
   if ( !served )
      return HIPSDP_OK;
   if ( m > 0 )
      memcpy(w.pin, u, (size_t) m * sizeof(double));
   for (int j = 0; j < count; ++j)
   {
      double* t = w.pin + tab + (long long) j * HS_OV_TAB;
      const int i = vars != NULL ? vars[j] : j;
      t[0] = (double) i;
      t[1] = (double) (kind != NULL ? kind[j] : HIPSDP_ONEVAR_NEWTON);
      t[2] = lb[j]; t[3] = ub[j]; t[4] = u[i];
   }
   hipStream_t st = w.stream;
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) res * sizeof(double), hipMemcpyHostToDevice, st) );
   HS_CALL( hs_ec_form_z(st, 1, n, m, w.djobs, w.dev) );
   hs_ov_par P;
   memset(&P, 0, sizeof(P));
   P.n = n; P.count = count; P.maxevals = opts->maxevals > 0 ? opts->maxevals : 100;
   P.feastol = opts->feastol; P.infinity = opts->infinity;
   P.blk = w.djobs; P.tab = w.dev + tab; P.slab = w.dev + slab; P.res = w.dev + res;
   HS_CALL( hs_onevar_newton(st, &P) );
   HS_HIP( hipMemcpyAsync(w.pin + res, w.dev + res, (size_t) count * HS_OV_RES * sizeof(double), hipMemcpyDeviceToHost, st) );
   HS_HIP( hipStreamSynchronize(st) );
   g_ov.launches += 2;
   g_ov.readbacks += 1;
   for (int j = 0; j < count; ++j)
   {
      const double* r = w.pin + res + (long long) j * HS_OV_RES;
      if ( !(r[0] >= 0.0 && r[0] <= (double) HIPSDP_ONEVAR_GAVEUP) )
         return HIPSDP_ERR_NUMERIC;
      status[j] = (int) r[0];
      optval[j] = r[1];
      if ( lmin != NULL ) lmin[j] = r[2];
      if ( grad != NULL ) grad[j] = r[3];
      if ( evals != NULL ) evals[j] = (int) r[4];
   }
   ++g_ov.calls;
   return HIPSDP_OK;
}

extern "C" int hipsdp_onevar_bounds_all_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_ova.get(calls, launches, readbacks);
}

/* One round over the blocks of the solver.  The rows of the table stand in workgroup order: the jobs of at most 64 rows in the
 * caller's order, then those of 65 to 128 rows by descending n (the long chains start first; among equal n the caller's order), and a
 * row carries the caller's index of its job as its slot in the result, so the copy-out needs no permutation.  The table of hs_ec_job
 * holds the blocks with a NEWTON or TWOPOINT job first: k_ec_form_z runs over that head alone. */
extern "C" int hipsdp_onevar_bounds_all(hipsdp_solver* s, const double* u, int count, const int* blocks, const int* vars, const int* kind,
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

   /* the blocks the shared launches serve: whole matrices on this device, at most HIPSDP_ONEVAR_MAXN rows (none for a solver with a
    * communicator or sharded matrices) */
   std::vector<int> ids;
   HS_CALL( hs_solver_cut_enter(s, -1, &ids) );
   std::vector<int> use((size_t) nb, -1);             /* -1: not served; -2: served, no job; 0: EXTREMES jobs alone; 1: needs Z(u) */
   for (size_t k = 0; k < ids.size(); ++k)
      if ( hs_solver_block_n(s, ids[k]) <= HIPSDP_ONEVAR_MAXN )
         use[ids[k]] = -2;
   std::vector<int> small, mid;                       /* the caller's job indices per class */
   for (int j = 0; j < count; ++j)
   {
      const int b = blocks != NULL ? blocks[j] : j / m;
      if ( use[b] == -1 )
         continue;
      const int needz = kind == NULL || kind[j] != HIPSDP_ONEVAR_EXTREMES ? 1 : 0;
      use[b] = use[b] > needz ? use[b] : needz;
      (hs_solver_block_n(s, b) <= 64 ? small : mid).push_back(j);
   }
   if ( small.empty() && mid.empty() )
      return HIPSDP_OK;
   std::stable_sort(mid.begin(), mid.end(), [&](int a, int c) {
      return hs_solver_block_n(s, blocks != NULL ? blocks[a] : a / m) > hs_solver_block_n(s, blocks != NULL ? blocks[c] : c / m); });

   /* the table of blocks (those that need Z first) and where their Z lie */
   std::vector<int> tids, entry((size_t) nb, -1);
   int nz = 0, nzmax = 0, nsmall = 0, nmid = 0;
   for (int pass = 1; pass >= 0; --pass)
      for (int b = 0; b < nb; ++b)
         if ( use[b] == pass )
         {
            entry[b] = (int) tids.size();
            tids.push_back(b);
            const int n = hs_solver_block_n(s, b);
            if ( pass == 1 ) { ++nz; nzmax = n > nzmax ? n : nzmax; }
         }
   long long zlen = 0;
   std::vector<long long> zoff(tids.size());
   for (size_t k = 0; k < tids.size(); ++k)
   {
      zoff[k] = zlen;
      zlen += hs_cut_mat_len(hs_solver_block_n(s, tids[k]));
   }
   for (size_t k = 0; k < small.size(); ++k)
   {
      const int n = hs_solver_block_n(s, blocks != NULL ? blocks[small[k]] : small[k] / m);
      nsmall = n > nsmall ? n : nsmall;
   }
   if ( !mid.empty() )
      nmid = hs_solver_block_n(s, blocks != NULL ? blocks[mid[0]] : mid[0] / m);
   int grid = 0;
   if ( !mid.empty() )
   {
      const int cus = hs_device_cus();
      grid = cus > 0 && cus < (int) mid.size() ? cus : (int) mid.size();
   }
   hs_ova_layout L;
   hs_ova_layout_make(m, count, HS_OVA_TAB, HS_OV_RES, zlen, grid, nmid, &L);
   for (size_t k = 0; k < zoff.size(); ++k)
      zoff[k] += L.Z;
   hs_solver_cut_ws w;
   HS_CALL( hs_solver_cut_blocks(s, tids, zoff, L.len.dev_len, L.len.pin_len, &w) );

   if ( m > 0 )
      memcpy(w.pin + L.u, u, (size_t) m * sizeof(double));
   long long row = 0;
   for (int cls = 0; cls < 2; ++cls)
   {
      const std::vector<int>& list = cls == 0 ? small : mid;
      for (size_t k = 0; k < list.size(); ++k, ++row)
      {
         const int j = list[k], b = blocks != NULL ? blocks[j] : j / m, i = vars != NULL ? vars[j] : j % m;
         double* t = w.pin + L.tab + row * HS_OVA_TAB;
         t[0] = (double) i;
         t[1] = (double) (kind != NULL ? kind[j] : HIPSDP_ONEVAR_NEWTON);
         t[2] = lb[j]; t[3] = ub[j]; t[4] = u[i];
         t[5] = (double) entry[b]; t[6] = (double) j; t[7] = 0.0;
      }
   }
   /* (rows of jobs that are not served stay unused behind `row`: the upload carries the whole table, the launches its head) */
   for (long long k = row * HS_OVA_TAB; k < (long long) count * HS_OVA_TAB; ++k)
      w.pin[L.tab + k] = 0.0;
   hipStream_t st = w.stream;
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );
   HS_CALL( hs_ec_form_z(st, nz, nzmax, m, w.djobs, w.dev + L.u) );
   hs_ova_par P;
   memset(&P, 0, sizeof(P));
   P.maxevals = opts->maxevals > 0 ? opts->maxevals : 100;
   P.feastol = opts->feastol; P.infinity = opts->infinity;
   P.jobs = w.djobs; P.res = w.dev + L.res;
   P.count = (int) small.size(); P.grid = P.count; P.nmax = nsmall; P.tab = w.dev + L.tab;
   HS_CALL( hs_onevar_all(st, 0, &P) );
   P.count = (int) mid.size(); P.grid = grid; P.nmax = nmid; P.tab = w.dev + L.tab + (long long) small.size() * HS_OVA_TAB;
   P.slab = w.dev + L.slabs;
   HS_CALL( hs_onevar_all(st, 1, &P) );
   HS_HIP( hipMemcpyAsync(w.pin + L.len.res_off, w.dev + L.len.res_off, (size_t) L.len.res_len * sizeof(double), hipMemcpyDeviceToHost, st) );
   HS_HIP( hipStreamSynchronize(st) );
   g_ova.launches += (nz > 0 ? 1 : 0) + (small.empty() ? 0 : 1) + (mid.empty() ? 0 : 1);
   g_ova.readbacks += 1;
   for (int cls = 0; cls < 2; ++cls)
   {
      const std::vector<int>& list = cls == 0 ? small : mid;
      for (size_t k = 0; k < list.size(); ++k)
      {
         const int j = list[k];
         const double* r = w.pin + L.res + (long long) j * HS_OV_RES;
         if ( !(r[0] >= 0.0 && r[0] <= (double) HIPSDP_ONEVAR_DONE) )
            return HIPSDP_ERR_NUMERIC;
         status[j] = (int) r[0];
         optval[j] = r[1];
         if ( lmin != NULL ) lmin[j] = r[2];
         if ( grad != NULL ) grad[j] = r[3];
         if ( evals != NULL ) evals[j] = (int) r[4];
      }
   }
   ++g_ova.calls;
   return HIPSDP_OK;
}
