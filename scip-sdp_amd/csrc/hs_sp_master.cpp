/* hs_sp_master.cpp - see hs_sp_master.h.  Runs once per master block (the first gather after its entries changed), never per node. */
#include "hs_sp_master.h"
#include <algorithm>
#include <numeric>
#include <climits>

int hs_spm_check(int N, int S, long long nnz, const int* slot, int oneslot, const int* row, const int* col)
{
   if ( N < 1 || S < 0 || nnz < 0 || (nnz > 0 && (row == NULL || col == NULL)) )
      return HIPSDP_ERR_ARG;
   if ( slot == NULL && nnz > 0 && (oneslot < 0 || oneslot >= S) )
      return HIPSDP_ERR_ARG;
   for (long long e = 0; e < nnz; ++e)
      if ( (slot != NULL && (slot[e] < 0 || slot[e] >= S)) || row[e] < 0 || row[e] >= N || col[e] < 0 || col[e] >= N )
         return HIPSDP_ERR_ARG;
   return HIPSDP_OK;
}

int hs_spm_finalize(int N, int S, long long nnz, const int* slot, const int* row, const int* col, const double* val, hs_spm_final* out)
{
   if ( out == NULL || (nnz > 0 && (slot == NULL || val == NULL)) || hs_spm_check(N, S, nnz, slot, 0, row, col) != HIPSDP_OK )
      return HIPSDP_ERR_ARG;
   if ( nnz > INT_MAX / 2 )
      return HIPSDP_ERR_ARG;
   auto R = [&](long long e) { return row[e] >= col[e] ? row[e] : col[e]; };
   auto C = [&](long long e) { return row[e] >= col[e] ? col[e] : row[e]; };
   std::vector<long long> ord((size_t) nnz);
   std::iota(ord.begin(), ord.end(), 0LL);
   std::stable_sort(ord.begin(), ord.end(), [&](long long a, long long b) {
      if ( slot[a] != slot[b] ) return slot[a] < slot[b];
      if ( R(a) != R(b) ) return R(a) < R(b);
      return C(a) < C(b);
   });
   hs_spm_final& f = *out;
   f.N = N; f.S = S;
   f.loff.assign((size_t) S + 1, 0);
   f.lrow.clear(); f.lcol.clear(); f.lval.clear();
   std::vector<int> lslot;
   for (size_t k = 0; k < ord.size(); ++k)
   {
      const long long e = ord[k];
      if ( k + 1 < ord.size() )
      {
         const long long g = ord[k + 1];
         if ( slot[e] == slot[g] && R(e) == R(g) && C(e) == C(g) )
            continue;                                     /* the last of equal keys wins */
      }
      lslot.push_back(slot[e]); f.lrow.push_back(R(e)); f.lcol.push_back(C(e)); f.lval.push_back(val[e]);
      ++f.loff[(size_t) slot[e] + 1];
   }
   for (int k = 0; k < S; ++k)
      f.loff[(size_t) k + 1] += f.loff[(size_t) k];
   f.L = (long long) f.lrow.size();
   /* by position; inside a position by slot (the keys are distinct now) */
   std::vector<int> po((size_t) f.L);
   std::iota(po.begin(), po.end(), 0);
   std::stable_sort(po.begin(), po.end(), [&](int a, int b) {
      if ( f.lrow[a] != f.lrow[b] ) return f.lrow[a] < f.lrow[b];
      if ( f.lcol[a] != f.lcol[b] ) return f.lcol[a] < f.lcol[b];
      return lslot[a] < lslot[b];
   });
   f.poff.clear(); f.prow.clear(); f.pcol.clear();
   f.pslot.assign((size_t) f.L, 0); f.pval.assign((size_t) f.L, 0.0);
   for (long long k = 0; k < f.L; ++k)
   {
      const int e = po[(size_t) k];
      if ( k == 0 || f.lrow[e] != f.lrow[po[(size_t) k - 1]] || f.lcol[e] != f.lcol[po[(size_t) k - 1]] )
      {
         f.poff.push_back((int) k);
         f.prow.push_back(f.lrow[e]);
         f.pcol.push_back(f.lcol[e]);
      }
      f.pslot[(size_t) k] = lslot[e];
      f.pval[(size_t) k] = f.lval[e];
   }
   f.P = (long long) f.prow.size();
   f.poff.push_back((int) f.L);
   /* both triangles per slot, row-major */
   long long F = 0;
   for (long long e = 0; e < f.L; ++e)
      F += f.lrow[e] != f.lcol[e] ? 2 : 1;
   if ( F > INT_MAX - 1 )
      return HIPSDP_ERR_ARG;
   f.foff.assign((size_t) S + 1, 0);
   f.frow.clear(); f.fcol.clear(); f.fval.clear();
   f.frow.reserve((size_t) F); f.fcol.reserve((size_t) F); f.fval.reserve((size_t) F);
   f.R = 0;
   std::vector<std::pair<std::pair<int, int>, double> > ent;
   for (int k = 0; k < S; ++k)
   {
      ent.clear();
      for (int e = f.loff[(size_t) k]; e < f.loff[(size_t) k + 1]; ++e)
      {
         ent.push_back(std::make_pair(std::make_pair(f.lrow[e], f.lcol[e]), f.lval[e]));
         if ( f.lrow[e] != f.lcol[e] )
            ent.push_back(std::make_pair(std::make_pair(f.lcol[e], f.lrow[e]), f.lval[e]));
      }
      std::sort(ent.begin(), ent.end(), [](const std::pair<std::pair<int, int>, double>& a, const std::pair<std::pair<int, int>, double>& b) {
         return a.first < b.first; });
      for (size_t t = 0; t < ent.size(); ++t)
      {
         if ( t == 0 || ent[t].first.first != ent[t - 1].first.first )
            ++f.R;
         f.frow.push_back(ent[t].first.first); f.fcol.push_back(ent[t].first.second); f.fval.push_back(ent[t].second);
      }
      f.foff[(size_t) k + 1] = (int) f.frow.size();
   }
   f.F = (long long) f.frow.size();
   return HIPSDP_OK;
}

int hs_spm_node_maps(int N, int S, int nactive, const int* act, int nkept, const int* kept, int* inv, int* svar, int* ordered)
{
   if ( N < 1 || S < 0 || nactive < 0 || nkept < 0 || nkept > N || (nactive > 0 && act == NULL) || (nkept > 0 && kept == NULL)
      || inv == NULL || (S > 0 && svar == NULL) || ordered == NULL )
      return HIPSDP_ERR_ARG;
   for (int r = 0; r < N; ++r)
      inv[r] = -1;
   for (int k = 0; k < S; ++k)
      svar[k] = 0;
   for (int r = 0; r < nkept; ++r)
   {
      if ( kept[r] < 0 || kept[r] >= N || (r > 0 && kept[r] <= kept[r - 1]) )
         return HIPSDP_ERR_ARG;
      inv[kept[r]] = r;
   }
   int last = -1;
   *ordered = 1;
   for (int a = 0; a < nactive; ++a)
   {
      if ( act[a] < -1 || act[a] >= S )
         return HIPSDP_ERR_ARG;
      if ( act[a] < 0 )
         continue;
      if ( svar[act[a]] != 0 )
         return HIPSDP_ERR_ARG;
      svar[act[a]] = a + 1;
      if ( act[a] < last )
         *ordered = 0;
      last = act[a];
   }
   return HIPSDP_OK;
}
