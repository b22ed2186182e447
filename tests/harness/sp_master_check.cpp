/* sp_master_check.cpp - stand-alone check of the host side of a master block kept as triplets (scip-sdp_amd/csrc/hs_sp_master.cpp),
 * meant to be compiled with the host compiler and -fsanitize=address,undefined (tests/test_sparse_master_cpu.py does that).
 * The three orders hs_spm_finalize produces are compared with a plain restatement: a std::map per slot keyed by (row, col) that
 * later entries overwrite.  Every input array is a heap block of exactly the stated length, so a read past a list is reported.
 * Prints "sp master check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_sp_master.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>

#define CHECK(cond) do { if ( !(cond) ) { printf("sp master check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

struct Trip { std::vector<int> slot, row, col; std::vector<double> val;
   void add(int s, int r, int c, double v) { slot.push_back(s); row.push_back(r); col.push_back(c); val.push_back(v); } };

template<class T> static T* exact(const std::vector<T>& v)
{
   if ( v.empty() )
      return NULL;
   T* p = (T*) malloc(v.size() * sizeof(T));
   memcpy(p, v.data(), v.size() * sizeof(T));
   return p;
}

static int check_case(int N, int S, const Trip& t)
{
   const long long nnz = (long long) t.val.size();
   int* sl = exact(t.slot); int* ro = exact(t.row); int* co = exact(t.col); double* va = exact(t.val);
   hs_spm_final f;
   const int rc = hs_spm_finalize(N, S, nnz, sl, ro, co, va, &f);
   free(sl); free(ro); free(co); free(va);
   CHECK(rc == HIPSDP_OK);
   /* the restatement */
   typedef std::map<std::pair<int, int>, double> Mat;
   std::vector<Mat> low((size_t) S), full((size_t) S);
   for (long long e = 0; e < nnz; ++e)
   {
      const int r = t.row[e] >= t.col[e] ? t.row[e] : t.col[e], c = t.row[e] >= t.col[e] ? t.col[e] : t.row[e];
      low[(size_t) t.slot[e]][std::make_pair(r, c)] = t.val[e];
   }
   std::map<std::pair<int, int>, std::map<int, double> > pos;
   long long L = 0, F = 0, R = 0;
   for (int k = 0; k < S; ++k)
      for (Mat::const_iterator it = low[(size_t) k].begin(); it != low[(size_t) k].end(); ++it)
      {
         ++L;
         full[(size_t) k][it->first] = it->second;
         full[(size_t) k][std::make_pair(it->first.second, it->first.first)] = it->second;
         pos[it->first][k] = it->second;
      }
   CHECK(f.N == N && f.S == S && f.L == L && f.P == (long long) pos.size());
   CHECK((long long) f.loff.size() == S + 1 && (long long) f.foff.size() == S + 1 && (long long) f.poff.size() == f.P + 1);
   CHECK((long long) f.lrow.size() == L && (long long) f.lcol.size() == L && (long long) f.lval.size() == L);
   CHECK((long long) f.pslot.size() == L && (long long) f.pval.size() == L && (long long) f.prow.size() == f.P && (long long) f.pcol.size() == f.P);
   long long e = 0, g = 0;
   for (int k = 0; k < S; ++k)
   {
      CHECK(f.loff[(size_t) k] == e && f.foff[(size_t) k] == g);
      for (Mat::const_iterator it = low[(size_t) k].begin(); it != low[(size_t) k].end(); ++it, ++e)
         CHECK(f.lrow[(size_t) e] == it->first.first && f.lcol[(size_t) e] == it->first.second
            && memcmp(&f.lval[(size_t) e], &it->second, sizeof(double)) == 0);
      int lastrow = -1;
      for (Mat::const_iterator it = full[(size_t) k].begin(); it != full[(size_t) k].end(); ++it, ++g)
      {
         CHECK(g < (long long) f.frow.size());
         CHECK(f.frow[(size_t) g] == it->first.first && f.fcol[(size_t) g] == it->first.second
            && memcmp(&f.fval[(size_t) g], &it->second, sizeof(double)) == 0);
         if ( it->first.first != lastrow )
            ++R;
         lastrow = it->first.first;
      }
      F += (long long) full[(size_t) k].size();
   }
   CHECK(f.loff[(size_t) S] == L && f.foff[(size_t) S] == F && f.F == F && f.R == R);
   CHECK((long long) f.frow.size() == F && (long long) f.fcol.size() == F && (long long) f.fval.size() == F);
   long long p = 0, q = 0;
   for (std::map<std::pair<int, int>, std::map<int, double> >::const_iterator it = pos.begin(); it != pos.end(); ++it, ++p)
   {
      CHECK(f.poff[(size_t) p] == q && f.prow[(size_t) p] == it->first.first && f.pcol[(size_t) p] == it->first.second);
      for (std::map<int, double>::const_iterator jt = it->second.begin(); jt != it->second.end(); ++jt, ++q)
         CHECK(f.pslot[(size_t) q] == jt->first && memcmp(&f.pval[(size_t) q], &jt->second, sizeof(double)) == 0);
   }
   CHECK(f.poff[(size_t) f.P] == L && q == L);
   return 0;
}

static int check_maps(void)
{
   const int N = 7, S = 5;
   std::vector<int> inv((size_t) N, 99), svar((size_t) S, 99);
   int ordered = -1;
   {
      const int act[4] = {0, -1, 2, 4}, kept[4] = {1, 2, 4, 6};
      int* a = (int*) malloc(sizeof(act)); int* k = (int*) malloc(sizeof(kept));
      memcpy(a, act, sizeof(act)); memcpy(k, kept, sizeof(kept));
      CHECK(hs_spm_node_maps(N, S, 4, a, 4, k, inv.data(), svar.data(), &ordered) == HIPSDP_OK);
      free(a); free(k);
      const int winv[7] = {-1, 0, 1, -1, 2, -1, 3}, wsv[5] = {1, 0, 3, 0, 4};
      CHECK(memcmp(inv.data(), winv, sizeof(winv)) == 0 && memcmp(svar.data(), wsv, sizeof(wsv)) == 0 && ordered == 1);
   }
   {
      const int act[3] = {3, 1, 4}, kept[1] = {0};
      CHECK(hs_spm_node_maps(N, S, 3, act, 1, kept, inv.data(), svar.data(), &ordered) == HIPSDP_OK && ordered == 0);
      CHECK(svar[3] == 1 && svar[1] == 2 && svar[4] == 3 && svar[0] == 0 && svar[2] == 0 && inv[0] == 0 && inv[1] == -1);
   }
   {
      CHECK(hs_spm_node_maps(N, S, 0, NULL, 0, NULL, inv.data(), svar.data(), &ordered) == HIPSDP_OK && ordered == 1);
      for (int r = 0; r < N; ++r) CHECK(inv[(size_t) r] == -1);
      for (int k = 0; k < S; ++k) CHECK(svar[(size_t) k] == 0);
   }
   {
      const int twice[2] = {2, 2}, big[1] = {5}, low[1] = {-2}, kept[2] = {1, 3}, down[2] = {3, 1}, out[1] = {7};
      CHECK(hs_spm_node_maps(N, S, 2, twice, 2, kept, inv.data(), svar.data(), &ordered) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_node_maps(N, S, 1, big, 2, kept, inv.data(), svar.data(), &ordered) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_node_maps(N, S, 1, low, 2, kept, inv.data(), svar.data(), &ordered) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_node_maps(N, S, 0, NULL, 2, down, inv.data(), svar.data(), &ordered) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_node_maps(N, S, 0, NULL, 1, out, inv.data(), svar.data(), &ordered) == HIPSDP_ERR_ARG);
   }
   return 0;
}

int main(void)
{
   /* duplicates (the last one wins, also when one is given in the upper triangle), upper-triangle input, an empty slot in the middle
    * and at the end, a diagonal-only slot, one position shared by all non-empty slots */
   {
      Trip t;
      t.add(0, 3, 1, 1.0); t.add(0, 1, 3, 2.0); t.add(0, 3, 1, 3.0);          /* (3, 1) three times: 3.0 stays */
      t.add(0, 0, 4, 4.0);                                                   /* upper triangle: stored as (4, 0) */
      t.add(0, 2, 2, -0.0);                                                  /* a negative zero keeps its sign */
      t.add(2, 0, 0, 5.0); t.add(2, 1, 1, 6.0); t.add(2, 4, 4, 7.0);          /* diagonal only */
      t.add(3, 4, 0, 8.0); t.add(3, 4, 3, 9.0); t.add(3, 2, 1, 10.0);
      t.add(0, 4, 2, 11.0); t.add(2, 4, 2, 12.0); t.add(3, 2, 4, 13.0);       /* (4, 2) in every non-empty slot */
      t.add(2, 4, 2, 14.0);                                                  /* ... and replaced in one of them */
      if ( check_case(5, 5, t) != 0 ) return 1;
   }
   /* one position shared by ALL slots (and nothing else), slots given in descending order */
   {
      Trip t;
      for (int k = 3; k >= 0; --k)
         t.add(k, 1, 2, 1.0 + k);
      if ( check_case(3, 4, t) != 0 ) return 1;
   }
   /* an empty block, with and without slots */
   {
      Trip t;
      if ( check_case(4, 3, t) != 0 ) return 1;
      if ( check_case(1, 0, t) != 0 ) return 1;
   }
   /* a dense slot beside sparse ones, entries in reverse order */
   {
      Trip t;
      for (int r = 11; r >= 0; --r)
         for (int c = 11; c >= 0; --c)
            if ( r >= c )
               t.add(1, (r + c) % 2 ? r : c, (r + c) % 2 ? c : r, 100.0 * r + c);
      t.add(0, 11, 11, 1.5); t.add(2, 0, 0, 2.5); t.add(2, 11, 0, 3.5);
      if ( check_case(12, 3, t) != 0 ) return 1;
   }
   /* pseudo-random with many collisions */
   {
      Trip t;
      unsigned seed = 12345u;
      for (int e = 0; e < 600; ++e)
      {
         seed = seed * 1664525u + 1013904223u; const int s = (int) ((seed >> 8) % 9u);
         seed = seed * 1664525u + 1013904223u; const int r = (int) ((seed >> 8) % 6u);
         seed = seed * 1664525u + 1013904223u; const int c = (int) ((seed >> 8) % 6u);
         t.add(s == 4 ? 5 : s, r, c, 0.25 * e);                              /* slot 4 stays empty */
      }
      if ( check_case(6, 9, t) != 0 ) return 1;
   }
   /* indices outside the block are refused, by the check of an upload and by the sort */
   {
      const int s1[1] = {0}, r1[1] = {2}, c1[1] = {0};
      const double v1[1] = {1.0};
      hs_spm_final f;
      CHECK(hs_spm_check(2, 1, 1, s1, 0, r1, c1) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_check(3, 1, 1, s1, 0, r1, c1) == HIPSDP_OK);
      CHECK(hs_spm_check(3, 1, 1, NULL, 1, r1, c1) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_check(3, 1, 1, NULL, 0, r1, c1) == HIPSDP_OK);
      CHECK(hs_spm_check(3, 0, 1, s1, 0, r1, c1) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_finalize(2, 1, 1, s1, r1, c1, v1, &f) == HIPSDP_ERR_ARG);
      CHECK(hs_spm_finalize(3, 1, 1, s1, r1, c1, v1, &f) == HIPSDP_OK && f.L == 1 && f.F == 2 && f.R == 2 && f.P == 1);
   }
   if ( check_maps() != 0 ) return 1;
   printf("sp master check: ok\n");
   return 0;
}
