/* psd_plan_check.cpp - stand-alone check of the host-side planning of hipsdp_psd_project_many (scip-sdp_amd/csrc/hs_psd_plan.cpp),
 * meant to be compiled with the host compiler and -fsanitize=address,undefined (tests/test_psd_project_many_cpu.py does that).
 * Every array a job points to is a heap block of exactly the stated length, so a read past a triplet list is reported.
 * Prints "psd plan check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_psd_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int cls_rule(int n) { return n < 10 ? 0 : (n <= 64 ? 1 : 2); }
static long long scratch_rule(int n) { return n < 10 ? 64 * 64 + 64 + 16 : 66000 + 7 * n; }      /* (any positive lengths do) */

#define CHECK(cond) do { if ( !(cond) ) { printf("psd plan check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct JobSet
{
   std::vector<hipsdp_psd_job> jobs;
   std::vector<void*> blocks;
   ~JobSet() { for (size_t k = 0; k < blocks.size(); ++k) free(blocks[k]); }
   template<class T> T* arr(int len) { if ( len <= 0 ) return NULL; T* p = (T*) calloc((size_t) len, sizeof(T)); blocks.push_back(p); return p; }
   void add(int n, int nnz, int cap, unsigned* seed)
   {
      hipsdp_psd_job J;
      J.n = n; J.nnz = nnz; J.cap = cap; J.nnz_out = -1; J.minev = 1e-4;
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

static int check_plan(const JobSet& S, const hs_pp_plan& P)
{
   const int count = (int) S.jobs.size();
   std::vector<int> seen((size_t) count, 0);
   long long trips = 0, outlen = 0;
   int nmax = 0;
   for (size_t k = 0; k < P.items.size(); ++k)
   {
      const hs_pp_item& it = P.items[k];
      CHECK( it.job >= 0 && it.job < count );
      const hipsdp_psd_job& J = S.jobs[it.job];
      CHECK( ++seen[it.job] == 1 && J.n <= HS_PP_MAXN );
      CHECK( it.n == J.n && it.nnz == J.nnz && it.cap == J.cap );
      CHECK( it.trip == trips );
      trips += J.nnz;
      CHECK( it.a_off % HS_PP_ALIGN == 0 && it.ws_off % HS_PP_ALIGN == 0 );
      if ( k > 0 )
      {
         const hs_pp_item& pr = P.items[k - 1];
         CHECK( cls_rule(pr.n) < cls_rule(it.n) || (cls_rule(pr.n) == cls_rule(it.n) && pr.job < it.job) );   /* sorted, stable */
         CHECK( it.a_off >= pr.a_off + (long long) pr.n * pr.n && it.ws_off >= pr.ws_off + scratch_rule(pr.n) );
         CHECK( it.row_off == pr.row_off + pr.n + 1 );
      }
      else
         CHECK( it.a_off == 0 && it.ws_off == 0 && it.row_off == 0 );
      const long long full = (long long) J.n * (J.n + 1) / 2;
      outlen += J.cap < full ? J.cap : full;
      nmax = J.n > nmax ? J.n : nmax;
   }
   for (size_t k = 0; k < P.big.size(); ++k)
   {
      CHECK( P.big[k] >= 0 && P.big[k] < count && ++seen[P.big[k]] == 1 && S.jobs[P.big[k]].n > HS_PP_MAXN );
      CHECK( k == 0 || P.big[k - 1] < P.big[k] );
   }
   for (int j = 0; j < count; ++j)
      CHECK( seen[j] == 1 );
   CHECK( P.trips == trips && P.out_len == outlen && P.nmax == nmax );
   if ( !P.items.empty() )
   {
      const hs_pp_item& la = P.items.back();
      CHECK( P.a_len >= la.a_off + (long long) la.n * la.n && P.ws_len >= la.ws_off + scratch_rule(la.n) && P.row_len == la.row_off + la.n + 1 );
   }
   else
      CHECK( P.a_len == 0 && P.ws_len == 0 && P.row_len == 0 && P.trips == 0 );
   return 0;
}

int main(void)
{
   const hs_pp_rules rules = {cls_rule, scratch_rule};
   hs_pp_plan P;
   unsigned seed = 12345u;
   /* nothing to do */
   CHECK( hs_pp_plan_make(0, NULL, 0, &rules, &P) == HIPSDP_OK && P.items.empty() && P.big.empty() );
   /* the sizes where something changes, in an order that is not the launch order, with empty jobs and short caps among them */
   {
      static const int ns[] = {128, 1, 65, 9, 129, 10, 64, 2, 300, 17, 63, 127, 16, 33, 9, 10};
      JobSet S;
      for (size_t k = 0; k < sizeof(ns) / sizeof(ns[0]); ++k)
         S.add(ns[k], k % 5 == 0 ? 0 : ns[k] * (ns[k] + 1) / 2, k % 4 == 1 ? 2 : ns[k] * (ns[k] + 1) / 2, &seed);
      for (int mode = 0; mode < 2; ++mode)
      {
         CHECK( hs_pp_plan_make((int) S.jobs.size(), S.jobs.data(), mode, &rules, &P) == HIPSDP_OK );
         CHECK( P.big.size() == 2 && P.items.size() == S.jobs.size() - 2 );
         if ( check_plan(S, P) != 0 ) return 1;
      }
   }
   /* the largest table the entry point admits, random sizes; one job more is refused */
   {
      JobSet S;
      for (int k = 0; k < HIPSDP_PSD_MANY_MAXJOBS + 1; ++k)
      {
         seed = seed * 1664525u + 1013904223u;
         const int n = 1 + (int) ((seed >> 10) % 140u);
         S.add(n, (int) ((seed >> 20) % 40u), n, &seed);
      }
      CHECK( hs_pp_plan_make(HIPSDP_PSD_MANY_MAXJOBS + 1, S.jobs.data(), 0, &rules, &P) == HIPSDP_ERR_ARG );
      S.jobs.pop_back();
      CHECK( hs_pp_plan_make(HIPSDP_PSD_MANY_MAXJOBS, S.jobs.data(), 0, &rules, &P) == HIPSDP_OK );
      if ( check_plan(S, P) != 0 ) return 1;
   }
   /* every argument error */
   {
      JobSet S;
      S.add(5, 6, 15, &seed); S.add(12, 30, 78, &seed); S.add(70, 9, 100, &seed);
      hipsdp_psd_job* J = S.jobs.data();
      CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_OK );
      CHECK( hs_pp_plan_make(-1, J, 0, &rules, &P) == HIPSDP_ERR_ARG );
      CHECK( hs_pp_plan_make(3, NULL, 0, &rules, &P) == HIPSDP_ERR_ARG );
      CHECK( hs_pp_plan_make(3, J, 2, &rules, &P) == HIPSDP_ERR_ARG && hs_pp_plan_make(3, J, -1, &rules, &P) == HIPSDP_ERR_ARG );
      CHECK( hs_pp_plan_make(3, J, 0, NULL, &P) == HIPSDP_ERR_ARG && hs_pp_plan_make(3, J, 0, &rules, NULL) == HIPSDP_ERR_ARG );
      hipsdp_psd_job keep = J[1];
      J[1].n = 0;                      CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].nnz = -1;                   CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].cap = -1;                   CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].row = NULL;                 CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].col = NULL;                 CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].val = NULL;                 CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].rowout = NULL;              CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].colout = NULL;              CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].valout = NULL;              CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      J[1].n = 11;                     /* the triplets were drawn for 12 rows: index 11 appears among 30 draws with this seed or not - force one */
      const_cast<int*>(J[1].row)[29] = 11;
      CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG ); J[1] = keep;
      const_cast<int*>(J[1].col)[0] = -1;
      CHECK( hs_pp_plan_make(3, J, 0, &rules, &P) == HIPSDP_ERR_ARG );
      const_cast<int*>(J[1].col)[0] = 0;
      /* NULL arrays are fine where the length is zero */
      J[0].nnz = 0; J[0].row = NULL; J[0].col = NULL; J[0].val = NULL; J[2].cap = 0; J[2].rowout = NULL; J[2].colout = NULL; J[2].valout = NULL;
      CHECK( hs_pp_plan_make(3, J, 1, &rules, &P) == HIPSDP_OK );
      if ( check_plan(S, P) != 0 ) return 1;
   }
   printf("psd plan check: ok\n");
   return 0;
}
