/* hs_cut_stats.h - calls served, and their launches and read-backs: the counters behind hipsdp_eigencuts_all_stats,
 * hipsdp_sparsecuts_all_stats, hipsdp_sparsecuts_stats, hipsdp_sparsecuts_ex_stats (cut_calls.hip) and hipsdp_onevar_bounds_stats
 * (onevar.hip) */
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
