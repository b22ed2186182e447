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
 * calls (cut_calls.hip). */
#include "hs_common.h"
#include "hs_kernels.h"
#include "hs_cut_stats.h"
#include "../../include/hipsdp.h"
#include <cstring>

static CutStats g_ov;

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
