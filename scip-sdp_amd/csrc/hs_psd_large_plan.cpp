/* hs_psd_large_plan.cpp - see hs_psd_large_plan.h */
#include "hs_psd_large_plan.h"
#include "hs_chunks.h"
#include <stddef.h>
#include <algorithm>

static long long ppl_round(long long len)
{
   return (len + HS_PPL_ALIGN - 1) / HS_PPL_ALIGN * HS_PPL_ALIGN;
}

int hs_ppl_check(int count, const hipsdp_psd_job* jobs, int mode)
{
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
   return HIPSDP_OK;
}

int hs_ppl_items(int count, const hipsdp_psd_job* jobs, const hs_ppl_rules* rules, std::vector<hs_ppl_item>* items)
{
   if ( items == NULL || rules == NULL || rules->ws_len == NULL || rules->out_len == NULL || count < 0 || (count > 0 && jobs == NULL) )
      return HIPSDP_ERR_ARG;
   items->clear();
   for (int j = 0; j < count; ++j)
   {
      const hipsdp_psd_job& J = jobs[j];
      if ( J.n < HIPSDP_PSD_LARGE_MINN || J.n > HIPSDP_PSD_LARGE_MAXN )
         continue;
      hs_ppl_item it;
      it.job = j; it.n = J.n; it.nnz = J.nnz; it.cap = J.cap;
      it.ntc = (J.n + HS_PPL_TILE - 1) / HS_PPL_TILE;
      it.trip = it.ws_off = it.out_off = it.cnt_off = 0;
      const long long cnt = ppl_round((long long) J.n * it.ntc + (long long) it.ntc * it.ntc);
      const long long full = (long long) J.n * (J.n + 1) / 2;
      const long long res = J.cap < full ? J.cap : full;
      it.len = (ppl_round(rules->ws_len(J.n)) + ppl_round(rules->out_len(J.n))) * (long long) sizeof(double) + cnt * (long long) sizeof(int)
         + (long long) J.nnz * (long long) (sizeof(double) + 2 * sizeof(int)) + res * (long long) (sizeof(double) + 2 * sizeof(int));
      items->push_back(it);
   }
   std::stable_sort(items->begin(), items->end(), [](const hs_ppl_item& a, const hs_ppl_item& b) { return a.n > b.n; });
   return HIPSDP_OK;
}

int hs_ppl_chunk_make(std::vector<hs_ppl_item>* items, int start, long long budget, const hs_ppl_rules* rules, hs_ppl_chunk* chunk)
{
   if ( items == NULL || chunk == NULL || rules == NULL || rules->ws_len == NULL || rules->out_len == NULL || start < 0
      || start >= (int) items->size() )
      return HIPSDP_ERR_ARG;
   const int total = (int) items->size();
   std::vector<long long> len((size_t) total);
   for (int i = 0; i < total; ++i)
      len[(size_t) i] = (*items)[(size_t) i].len;
   const int k = hs_chunk_end(len.data(), total, start, budget, 0);
   chunk->first = start; chunk->end = k;
   chunk->nmax = 0;
   chunk->trips = chunk->ws_len = chunk->out_len = chunk->cnt_len = chunk->res_len = 0;
   for (int i = start; i < k; ++i)
   {
      hs_ppl_item& it = (*items)[(size_t) i];
      it.trip = chunk->trips; it.ws_off = chunk->ws_len; it.out_off = chunk->out_len; it.cnt_off = chunk->cnt_len;
      chunk->trips += it.nnz;
      chunk->ws_len += ppl_round(rules->ws_len(it.n));
      chunk->out_len += ppl_round(rules->out_len(it.n));
      chunk->cnt_len += ppl_round((long long) it.n * it.ntc + (long long) it.ntc * it.ntc);
      const long long full = (long long) it.n * (it.n + 1) / 2;
      chunk->res_len += it.cap < full ? it.cap : full;
      if ( it.n > chunk->nmax )
         chunk->nmax = it.n;
   }
   return HIPSDP_OK;
}

int hs_ppl_launches(int nmax)
{
   return nmax + 8 + 6 * ((nmax + 31) / 32);
}
