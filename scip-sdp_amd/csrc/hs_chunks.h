/* hs_chunks.h - the chunks of the calls over all blocks (or jobs) of 129 .. 512 rows (onevar_large.hip, cut_calls.hip, psd_large.hip,
 * units.hip): their served list, ordered by descending n, is taken in chunks, one after the other on the call's stream.  Where a chunk
 * ends, the environment variable that overrides it and the loop over the chunks are written down here once.
 * Host only and header only: no HIP, so the check programs of tests/harness include it with the host compiler alone. */
#ifndef HS_CHUNKS_H
#define HS_CHUNKS_H

#include <stdlib.h>
#include <limits>

/* items start .. (return value - 1) form the next chunk: as many as fit into `budget` units of len[] (the workspace an item takes), at
 * least one, and at most maxjobs when maxjobs > 0 */
static inline int hs_chunk_end(const long long* len, int count, int start, long long budget, int maxjobs)
{
   long long used = 0;
   int k = start;
   while ( k < count )
   {
      if ( k > start && (used + len[k] > budget || (maxjobs > 0 && k - start >= maxjobs)) )
         break;
      used += len[k];
      ++k;
   }
   return k;
}

/* the positive integer in the environment variable `name`, else 0 (looked up at every call: a process may change it between calls) */
static inline int hs_chunk_env(const char* name)
{
   const char* env = getenv(name);
   const int v = env != NULL ? atoi(env) : 0;
   return v > 0 ? v : 0;
}

/* run(start, end) over the chunks of a list of `count` items, in order; returns the first status that is not 0 (HS_OK), else 0.
 * forced > 0: chunks of `forced` items and the budget does not bind (a count stands alone: items of equal n may differ in length) */
template <class Run>
static inline int hs_chunks_run(const long long* len, int count, long long budget, int forced, Run run)
{
   for (int start = 0; start < count; )
   {
      const int end = hs_chunk_end(len, count, start, forced > 0 ? std::numeric_limits<long long>::max() / 2 : budget, forced);
      const int rc = run(start, end);
      if ( rc != 0 )
         return rc;
      start = end;
   }
   return 0;
}

#endif
