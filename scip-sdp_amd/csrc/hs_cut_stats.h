/* hs_cut_stats.h - calls served, and their launches and read-backs: the counters behind hipsdp_eigencuts_all_stats,
 * hipsdp_sparsecuts_all_stats, hipsdp_sparsecuts_stats, hipsdp_sparsecuts_ex_stats and the two _large ones (cut_calls.hip),
 * hipsdp_onevar_bounds_stats (onevar.hip), its _large partner (onevar_large.hip), hipsdp_psd_project_many_large_stats (psd_large.hip) */
#ifndef HS_CUT_STATS_H
#define HS_CUT_STATS_H

#include "../../include/hipsdp.h"
#include <atomic>

struct CutStats
{
   std::atomic<long long> calls{0}, launches{0}, readbacks{0};
   int get(long long* c, long long* l, long long* r) const
   {
      if ( c != NULL ) *c = calls.load();
      if ( l != NULL ) *l = launches.load();
      if ( r != NULL ) *r = readbacks.load();
      return HIPSDP_OK;
   }
};

#endif
