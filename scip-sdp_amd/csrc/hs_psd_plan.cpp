/* hs_psd_plan.cpp - see hs_psd_plan.h */
#include "hs_psd_plan.h"
#include <stddef.h>

static long long pp_round(long long len)
{
   return (len + HS_PP_ALIGN - 1) / HS_PP_ALIGN * HS_PP_ALIGN;
}

int hs_pp_plan_make(int count, const hipsdp_psd_job* jobs, int mode, const hs_pp_rules* rules, hs_pp_plan* plan)
{
   if ( plan == NULL || rules == NULL || rules->cls == NULL || rules->scratch == NULL )
      return HIPSDP_ERR_ARG;
   if ( count < 0 || count > HIPSDP_PSD_MANY_MAXJOBS || (count > 0 && jobs == NULL) || mode < 0 || mode > 1 )
      return HIPSDP_ERR_ARG;
   for (int j = 0; j < count; ++j)
   {
      const hipsdp_psd_job& J = jobs[j];
      if ( J.n < 1 || J.nnz < 0 || J.cap < 0 || (J.nnz > 0 && (J.row == NULL || J.col == NULL || J.val == NULL))
         || (J.cap > 0 && (J.rowout == NULL || J.colout == NULL || J.valout == NULL)) )
         return HIPSDP_ERR_ARG;
      for (int e = 0; e < J.nnz; ++e)
         if ( J.row[e] < 0 || J.row[e] >= J.n || J.col[e] < 0 || J.col[e] >= J.n )
            return HIPSDP_ERR_ARG;
   }
   plan->items.clear(); plan->big.clear();
   plan->trips = plan->a_len = plan->ws_len = plan->row_len = plan->out_len = 0;
   plan->nmax = 0;
   for (int j = 0; j < count; ++j)
      if ( jobs[j].n > HS_PP_MAXN )
         plan->big.push_back(j);
   for (int cls = 0; cls < 3; ++cls)
      for (int j = 0; j < count; ++j)
      {
         const hipsdp_psd_job& J = jobs[j];
         if ( J.n > HS_PP_MAXN || rules->cls(J.n) != cls )
            continue;
         hs_pp_item it;
         it.job = j; it.n = J.n; it.nnz = J.nnz; it.cap = J.cap;
         it.trip = plan->trips; it.a_off = plan->a_len; it.ws_off = plan->ws_len; it.row_off = plan->row_len;
         plan->trips += J.nnz;
         plan->a_len += pp_round((long long) J.n * J.n);
         plan->ws_len += pp_round(rules->scratch(J.n));
         plan->row_len += J.n + 1;
         const long long full = (long long) J.n * (J.n + 1) / 2;
         plan->out_len += J.cap < full ? J.cap : full;
         if ( J.n > plan->nmax )
            plan->nmax = J.n;
         plan->items.push_back(it);
      }
   return HIPSDP_OK;
}
