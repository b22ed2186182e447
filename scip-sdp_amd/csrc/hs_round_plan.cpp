/* hs_round_plan.cpp - see hs_round_plan.h */
#include "hs_round_plan.h"
#include <algorithm>

static long long even(long long len) { return (len + 1) & ~1LL; }
static long long ints(long long count) { return even((count + 1) / 2); }          /* doubles that hold `count` ints */

hs_rf_block hs_rf_block_make(int n, int m, int route, int slices, const hs_rf_rules* rules)
{
   hs_rf_block B;
   long long at = 0;
   B.mat = B.ws = B.out = 0;
   if ( n <= HS_RF_SMALLN )
   {
      B.mat = 0;
      B.ws = hs_cut_mat_len(n);
      B.out = B.ws;                                /* (eigenvalues and vectors lie inside the slab) */
      at = B.ws + even(rules->small_scratch(n));
   }
   else
   {
      B.ws = B.mat = 0;                            /* (the matrix is the head of the workspace) */
      B.out = even(rules->large_ws(n));
      at = B.out + even(rules->large_out(n));
   }
   B.VT = at;
   at += route == 0 ? hs_cut_mat_len(n) : 0;
   B.part = at;
   at += even((long long) slices * n * ((long long) m + 1));
   B.len = at;
   return B;
}

void hs_rf_items(int nb, int m, const int* ns, const int* ok, const int* form, const int* xnnz, int with_vecs, const hs_rf_rules* rules,
   std::vector<hs_rf_item>* items)
{
   items->clear();
   for (int b = 0; b < nb; ++b)
   {
      if ( ns[b] < 1 || ns[b] > HS_RF_MAXN || !ok[b] )
         continue;
      hs_rf_item it;
      it.blk = b; it.n = ns[b];
      it.nonzeros = form[b] == 2 ? 1 : 0;
      it.route = hs_rf_route(it.n, it.nonzeros);
      it.klen = hs_rf_klen(it.n, form[b] == 1);
      const hs_rf_slices S = hs_rf_slice_rule(it.n, m, it.klen);
      it.slices = it.route ? S.slices : 1;
      it.pps = it.route ? S.pps : 0;
      it.nnz = xnnz != NULL ? xnnz[b] : 0;
      /* its block, its rows of the result, its triplets (a value and two ints each), its rows of the tables */
      it.len = hs_rf_block_make(it.n, m, it.route, it.slices, rules).len + (long long) it.n * (2 + (long long) m)
         + (with_vecs ? (long long) it.n * it.n : 0) + 2 * it.nnz + 64;
      items->push_back(it);
   }
   std::stable_sort(items->begin(), items->end(), [](const hs_rf_item& a, const hs_rf_item& b) { return a.n > b.n; });
}

long long hs_rf2_item_len(int n, int cap)
{
   const long long full = (long long) n * (n + 1) / 2, res = cap < full ? cap : full;
   const long long tc = (n + HS_RF_TILE - 1) / HS_RF_TILE;
   return (long long) n + hs_cut_mat_len(n) + ints((long long) n * tc + tc * tc + n + 2) + 2 * res + 32;
}

void hs_rf_layout_make(int m, int cnt, int nsmall, int nlarge, long long trips, long long rows, long long vec_len, const hs_rf_widths* w,
   long long blocks_len, hs_rf_layout* L)
{
   L->rf = 0;
   L->pp = even((long long) cnt * w->rf);
   L->eig = L->pp + even((long long) nsmall * w->pp);
   L->ppl = L->eig + even((long long) nsmall * w->eig);
   L->sx = L->ppl + even((long long) nlarge * w->ppl);
   L->sr = L->sx + even((long long) nlarge * w->sx);
   L->act = L->sr + even((long long) nlarge * w->sr);
   L->val = L->act + ints(nlarge);
   L->row = L->val + even(trips);
   L->col = L->row + ints(trips);
   L->r_eig = L->col + ints(trips);
   L->r_obj = L->r_eig + rows;
   L->r_coef = L->r_obj + rows;
   L->r_vec = L->r_coef + rows * m;
   L->blocks = even(L->r_vec + vec_len);
   L->len.upload_len = L->r_eig;
   L->len.res_off = L->r_eig; L->len.res_len = L->blocks - L->r_eig;
   L->len.pin_len = L->blocks; L->len.dev_len = L->blocks + blocks_len;
}

void hs_rf2_layout_make(int nsmall, int nlarge, long long rows, long long cap_small, long long cap_large, const hs_rf_widths* w,
   long long ints_len, long long mats_len, hs_rf2_layout* L)
{
   L->lam = 0;
   L->pp = even(rows);
   L->ppl = L->pp + even((long long) nsmall * w->pp);
   L->t_small = L->ppl + even((long long) nlarge * w->ppl);
   L->t_large = L->t_small + ints(nsmall);
   L->v_small = L->t_large + ints(nlarge);
   L->r_small = L->v_small + even(cap_small);
   L->c_small = L->r_small + ints(cap_small);
   L->v_large = L->c_small + ints(cap_small);
   L->r_large = L->v_large + even(cap_large);
   L->c_large = L->r_large + ints(cap_large);
   L->tot = L->c_large + ints(cap_large);
   L->ints = L->tot + ints(nsmall);
   L->mats = L->ints + ints(ints_len);
   L->len.upload_len = L->t_small;
   L->len.res_off = L->t_small; L->len.res_len = L->tot - L->t_small;
   L->len.pin_len = L->tot; L->len.dev_len = L->mats + mats_len;
}
