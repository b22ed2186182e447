/* psd_large_plan_check.cpp - stand-alone check of the host-side planning of hipsdp_psd_project_many_large
 * (scip-sdp_amd/csrc/hs_psd_large_plan.cpp), meant to be compiled with the host compiler and -fsanitize=address,undefined
 * (tests/test_psd_project_many_large_cpu.py does that).  Every array a job points to is a heap block of exactly the stated length, so
 * a read past a triplet list is reported.  Prints "psd large plan check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_psd_large_plan.h"
#include "hs_chunks.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static long long ws_rule(int n) { return 6LL * n * n + 150LL * n + 8; }             /* (any positive lengths do) */
static long long out_rule(int n) { return (long long) n * n + ((n + 1) & ~1); }

#define CHECK(cond) do { if ( !(cond) ) { printf("psd large plan check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct JobSet
{
   std::vector<hipsdp_psd_job> jobs;
   std::vector<void*> blocks;
   ~JobSet() { for (size_t k = 0; k < blocks.size(); ++k) free(blocks[k]); }
   template<class T> T* arr(int len) { if ( len <= 0 ) return NULL; T* p = (T*) calloc((size_t) len, sizeof(T)); blocks.push_back(p); return p; }
   void add(int n, int nnz, int cap, unsigned* seed)
   {
      hipsdp_psd_job J;
      J.n = n; J.nnz = nnz; J.cap = cap; J.nnz_out = -7; J.minev = 1e-4;
      int* r = arr<int>(nnz); int* c = arr<int>(nnz); double* v = arr<double>(nnz);
      for (int e = 0; e < nnz; ++e)
      {
         *seed = *seed * 1664525u + 1013904223u; r[e] = (int) ((*seed >> 8) % (unsigned) n);
         *seed = *seed * 1664525u + 1013904223u; c[e] = (int) ((*seed >> 8) % (unsigned) n);
         v[e] = 1.0 + e;
      }
      J.row = r; J.col = c; J.val = v;
      J.rowout = arr<int>(cap); J.colout = arr<int>(cap); J.valout = arr<double>(cap);
      jobs.push_back(J);
   }
};

static long long up(long long len) { return (len + HS_PPL_ALIGN - 1) / HS_PPL_ALIGN * HS_PPL_ALIGN; }

/* items: every served job once, largest first and stable; the chunks cover them in order; inside a chunk the slabs do not overlap */
static int check_plan(const JobSet& S, std::vector<hs_ppl_item>& items, long long budget, int* nchunks)
{
   const hs_ppl_rules rules = {ws_rule, out_rule};
   const int count = (int) S.jobs.size();
   std::vector<int> seen((size_t) count, 0);
   int served = 0;
   for (int j = 0; j < count; ++j)
      served += (S.jobs[j].n >= HIPSDP_PSD_LARGE_MINN && S.jobs[j].n <= HIPSDP_PSD_LARGE_MAXN) ? 1 : 0;
   CHECK( (int) items.size() == served );
   for (size_t k = 0; k < items.size(); ++k)
   {
      const hs_ppl_item& it = items[k];
      CHECK( it.job >= 0 && it.job < count && ++seen[it.job] == 1 );
      const hipsdp_psd_job& J = S.jobs[it.job];
      CHECK( J.n >= HIPSDP_PSD_LARGE_MINN && J.n <= HIPSDP_PSD_LARGE_MAXN );
      CHECK( it.n == J.n && it.nnz == J.nnz && it.cap == J.cap && it.ntc == (J.n + HS_PPL_TILE - 1) / HS_PPL_TILE && it.len > 0 );
      CHECK( it.len >= (ws_rule(J.n) + out_rule(J.n)) * (long long) sizeof(double) );
      if ( k > 0 )
         CHECK( items[k - 1].n > it.n || (items[k - 1].n == it.n && items[k - 1].job < it.job) );
   }
   *nchunks = 0;
   std::vector<long long> lens;
   for (size_t k = 0; k < items.size(); ++k)
      lens.push_back(items[k].len);
   for (int start = 0; start < (int) items.size(); )
   {
      hs_ppl_chunk C;
      CHECK( hs_ppl_chunk_make(&items, start, budget, &rules, &C) == HIPSDP_OK );
      CHECK( C.first == start && C.end > start && C.end <= (int) items.size() );
      /* the chunk ends where the one chunk rule says (hs_chunks.h) */
      CHECK( C.end == hs_chunk_end(lens.data(), (int) lens.size(), start, budget, 0) );
      long long used = 0, trips = 0, res = 0;
      for (int i = C.first; i < C.end; ++i)
      {
         const hs_ppl_item& it = items[(size_t) i];
         used += it.len;
         CHECK( it.trip == trips );
         trips += it.nnz;
         CHECK( it.ws_off % HS_PPL_ALIGN == 0 && it.out_off % HS_PPL_ALIGN == 0 && it.cnt_off % HS_PPL_ALIGN == 0 );
         if ( i > C.first )
         {
            const hs_ppl_item& pr = items[(size_t) i - 1];
            CHECK( it.ws_off == pr.ws_off + up(ws_rule(pr.n)) && it.out_off == pr.out_off + up(out_rule(pr.n)) );
            CHECK( it.cnt_off == pr.cnt_off + up((long long) pr.n * pr.ntc + (long long) pr.ntc * pr.ntc) );
         }
         else
            CHECK( it.ws_off == 0 && it.out_off == 0 && it.cnt_off == 0 );
         const long long full = (long long) it.n * (it.n + 1) / 2;
         res += it.cap < full ? it.cap : full;
      }
      const hs_ppl_item& la = items[(size_t) C.end - 1];
      CHECK( C.nmax == items[(size_t) C.first].n && C.trips == trips && C.res_len == res );
      CHECK( C.ws_len == la.ws_off + up(ws_rule(la.n)) && C.out_len == la.out_off + up(out_rule(la.n)) );
      CHECK( C.cnt_len == la.cnt_off + up((long long) la.n * la.ntc + (long long) la.ntc * la.ntc) );
      /* the chunk fits the budget unless it is a single job, and the next job would not have fitted */
      CHECK( used <= budget || C.end == C.first + 1 );
      if ( C.end < (int) items.size() )
         CHECK( used + items[(size_t) C.end].len > budget );
      start = C.end;
      ++*nchunks;
   }
   return 0;
}

int main(void)
{
   const hs_ppl_rules rules = {ws_rule, out_rule};
   std::vector<hs_ppl_item> items;
   unsigned seed = 4321u;
   int nchunks = 0;
   /* the launch formula at the sizes the tests use */
   CHECK( hs_ppl_launches(129) == 129 + 8 + 6 * 5 && hs_ppl_launches(160) == 160 + 8 + 6 * 5 && hs_ppl_launches(200) == 200 + 8 + 6 * 7 );
   CHECK( hs_ppl_launches(257) == 257 + 8 + 6 * 9 && hs_ppl_launches(512) == 512 + 8 + 6 * 16 );
   /* nothing to do */
   CHECK( hs_ppl_check(0, NULL, 0) == HIPSDP_OK && hs_ppl_items(0, NULL, &rules, &items) == HIPSDP_OK && items.empty() );
   /* mixed sizes with turned-away jobs among them, empty jobs and short caps; one chunk, then chunks forced small */
   {
      static const int ns[] = {200, 1, 129, 64, 512, 128, 257, 513, 160, 129, 300, 200, 511, 130};
      JobSet S;
      for (size_t k = 0; k < sizeof(ns) / sizeof(ns[0]); ++k)
         S.add(ns[k], k % 5 == 0 ? 0 : 3 * ns[k], k % 4 == 1 ? 2 : ns[k] * (ns[k] + 1) / 2, &seed);
      for (int mode = 0; mode < 2; ++mode)
         CHECK( hs_ppl_check((int) S.jobs.size(), S.jobs.data(), mode) == HIPSDP_OK );
      CHECK( hs_ppl_items((int) S.jobs.size(), S.jobs.data(), &rules, &items) == HIPSDP_OK );
      CHECK( items.size() == 10 && items[0].n == 512 && items.back().n == 129 && items.back().job == 9 );
      if ( check_plan(S, items, 512LL << 20, &nchunks) != 0 ) return 1;
      CHECK( nchunks == 1 );
      if ( check_plan(S, items, 1LL << 20, &nchunks) != 0 ) return 1;
      CHECK( nchunks == 10 );                                   /* (no job fits beside another: one job per chunk, never none) */
      if ( check_plan(S, items, 24LL << 20, &nchunks) != 0 ) return 1;
      CHECK( nchunks > 1 && nchunks < 10 );
      hs_ppl_chunk C;
      CHECK( hs_ppl_chunk_make(&items, 10, 1LL << 20, &rules, &C) == HIPSDP_ERR_ARG && hs_ppl_chunk_make(&items, -1, 1LL << 20, &rules, &C) == HIPSDP_ERR_ARG );
      CHECK( hs_ppl_chunk_make(NULL, 0, 1LL << 20, &rules, &C) == HIPSDP_ERR_ARG && hs_ppl_chunk_make(&items, 0, 1LL << 20, NULL, &C) == HIPSDP_ERR_ARG );
      CHECK( hs_ppl_chunk_make(&items, 0, 1LL << 20, &rules, NULL) == HIPSDP_ERR_ARG );
   }
   /* only turned-away jobs */
   {
      JobSet S;
      S.add(1, 1, 1, &seed); S.add(128, 10, 20, &seed); S.add(513, 0, 0, &seed);
      CHECK( hs_ppl_check(3, S.jobs.data(), 1) == HIPSDP_OK && hs_ppl_items(3, S.jobs.data(), &rules, &items) == HIPSDP_OK && items.empty() );
   }
   /* the largest table the entry point admits, sizes around the lower limit; one job more is refused */
   {
      JobSet S;
      for (int k = 0; k < HIPSDP_PSD_MANY_MAXJOBS + 1; ++k)
      {
         seed = seed * 1664525u + 1013904223u;
         const int n = 120 + (int) ((seed >> 10) % 30u);
         S.add(n, (int) ((seed >> 20) % 40u), n, &seed);
      }
      CHECK( hs_ppl_check(HIPSDP_PSD_MANY_MAXJOBS + 1, S.jobs.data(), 0) == HIPSDP_ERR_ARG );
      S.jobs.pop_back();
      CHECK( hs_ppl_check(HIPSDP_PSD_MANY_MAXJOBS, S.jobs.data(), 0) == HIPSDP_OK );
      CHECK( hs_ppl_items(HIPSDP_PSD_MANY_MAXJOBS, S.jobs.data(), &rules, &items) == HIPSDP_OK );
      if ( check_plan(S, items, 512LL << 20, &nchunks) != 0 ) return 1;
      if ( check_plan(S, items, 64LL << 20, &nchunks) != 0 ) return 1;
      CHECK( nchunks > 1 );
   }
   /* every argument error */
   {
      JobSet S;
      S.add(5, 6, 15, &seed); S.add(130, 30, 78, &seed); S.add(200, 9, 100, &seed);
      hipsdp_psd_job* J = S.jobs.data();
      CHECK( hs_ppl_check(3, J, 0) == HIPSDP_OK );
      CHECK( hs_ppl_check(-1, J, 0) == HIPSDP_ERR_ARG );
      CHECK( hs_ppl_check(3, NULL, 0) == HIPSDP_ERR_ARG );
      CHECK( hs_ppl_check(3, J, 2) == HIPSDP_ERR_ARG && hs_ppl_check(3, J, -1) == HIPSDP_ERR_ARG );
      CHECK( hs_ppl_items(3, J, NULL, &items) == HIPSDP_ERR_ARG && hs_ppl_items(3, J, &rules, NULL) == HIPSDP_ERR_ARG );
      hipsdp_psd_job keep = J[1];
      J[1].n = 0;                      CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].nnz = -1;                   CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].cap = -1;                   CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].row = NULL;                 CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].col = NULL;                 CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].val = NULL;                 CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].rowout = NULL;              CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].colout = NULL;              CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].valout = NULL;              CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG ); J[1] = keep;
      const_cast<int*>(J[1].row)[29] = 130;
      CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG );
      const_cast<int*>(J[1].row)[29] = 0;
      const_cast<int*>(J[1].col)[0] = -1;
      CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG );
      const_cast<int*>(J[1].col)[0] = 0;
      /* a turned-away job is checked like any other */
      const_cast<int*>(J[0].row)[5] = 5;
      CHECK( hs_ppl_check(3, J, 0) == HIPSDP_ERR_ARG );
      const_cast<int*>(J[0].row)[5] = 0;
      /* NULL arrays are fine where the length is zero */
      J[0].nnz = 0; J[0].row = NULL; J[0].col = NULL; J[0].val = NULL; J[2].cap = 0; J[2].rowout = NULL; J[2].colout = NULL; J[2].valout = NULL;
      CHECK( hs_ppl_check(3, J, 1) == HIPSDP_OK && hs_ppl_items(3, J, &rules, &items) == HIPSDP_OK && items.size() == 2 );
      if ( check_plan(S, items, 512LL << 20, &nchunks) != 0 ) return 1;
   }
   printf("psd large plan check: ok\n");
   return 0;
}
