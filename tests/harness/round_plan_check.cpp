/* round_plan_check.cpp - TEST INFRASTRUCTURE.  A stand-alone host program over csrc/hs_round_plan.h / .cpp and csrc/hs_chunks.h (built and
 * run by tests/harness/host_check.py with the host compiler and -fsanitize=address,undefined):
 *    the packed decode p -> (r, c), exhaustively for n = 1 .. 512
 *    the launch-count formulas of both stages against the sums they stand for
 *    the K-slice rule: a function of (n, m) and the storage length alone, slices that cover the storage index exactly once
 *    the chunk plan: every served block in exactly one chunk, descending n, workspace within the limit; the layouts do not overlap */
#include "hs_round_plan.h"
#include "hs_chunks.h"
#include <stdio.h>
#include <stdlib.h>

#define CHECK(c) do { if ( !(c) ) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } } while ( 0 )

static long long scratch(int n) { return n < 33 ? 1200 : 16 + 3LL * 128 * 128; }
static long long lws(int n) { return 2LL * n * n + 40LL * n; }
static long long lout(int n) { return (((long long) n + 1) & ~1LL) + (long long) n * n; }

int main(void)
{
   /* decode: every p of every n up to 512 (the positions of n are a prefix of those of 512, so one pass is exhaustive for all n) */
   {
      long long p = 0;
      for (int r = 0; r < HS_RF_MAXN; ++r)
         for (int c = 0; c <= r; ++c, ++p)
         {
            int rr = -1, cc = -1;
            hs_rf_decode(p, &rr, &cc);
            CHECK( rr == r && cc == c );
            CHECK( hs_rf_weight(rr, cc) == (r == c ? 1.0 : 2.0) );
         }
      CHECK( p == hs_rf_klen(HS_RF_MAXN, 1) && p == 512LL * 513 / 2 );
      for (int n = 1; n <= HS_RF_MAXN; ++n)
      {
         int rr, cc;
         hs_rf_decode(hs_rf_klen(n, 1) - 1, &rr, &cc);
         CHECK( rr == n - 1 && cc == n - 1 && hs_rf_klen(n, 0) == (long long) n * n );
      }
   }
   /* launches */
   for (int nmax = 0; nmax <= HS_RF_MAXN; nmax = nmax == 0 ? 129 : nmax + 1)
      for (int small = 0; small < 2; ++small)
      {
         long long want = 0;
         if ( small ) want += 1 + 3;
         if ( nmax > 0 ) want += 1 + (nmax - 1) + 5 + 6 * ((nmax + 31) / 32) + 1;
         if ( small || nmax > 0 ) want += 4;
         CHECK( hs_rf_launches(small, nmax) == want );
         CHECK( hs_rf2_launches(small, nmax > 0) == 2 * small + (nmax > 0 ? 2 : 0) );
      }
   CHECK( hs_rf_launches(1, 0) == 8 && hs_rf_launches(0, 130) == 130 + 6 + 30 + 4 && hs_rf_launches(1, 512) == 4 + 512 + 6 + 96 + 4 );
   /* the slice rule */
   {
      const int ms[] = {0, 1, 3, 5, 20, 63, 64, 70, 1000, 5000};
      int split_seen = 0;
      for (int n = 1; n <= HS_RF_MAXN; ++n)
         for (int packed = 0; packed < 2; ++packed)
            for (int m : ms)
            {
               const long long klen = hs_rf_klen(n, packed);
               const hs_rf_slices S = hs_rf_slice_rule(n, m, klen), T = hs_rf_slice_rule(n, m, klen);
               CHECK( S.slices == T.slices && S.pps == T.pps && S.panels == T.panels );
               CHECK( S.slices >= 1 && S.slices <= HS_RF_MAXSL && S.panels == (klen + HS_RF_TK - 1) / HS_RF_TK );
               long long covered = 0, next = 0;
               for (int s = 0; s < S.slices; ++s)
               {
                  const long long beg = (long long) s * S.pps * HS_RF_TK;
                  long long end = beg + S.pps * HS_RF_TK;
                  if ( end > klen ) end = klen;
                  CHECK( beg == next && end > beg );
                  covered += end - beg;
                  next = end;
               }
               CHECK( covered == klen && next == klen );
               CHECK( S.slices == 1 || S.pps >= HS_RF_MINPAN );
               split_seen += S.slices > 1;
            }
      CHECK( split_seen > 0 );
      CHECK( hs_rf_slice_rule(130, 1, hs_rf_klen(130, 1)).slices > 1 );               /* the K-split shape of the GPU tests */
      CHECK( hs_rf_slice_rule(512, 20, hs_rf_klen(512, 1)).slices == HS_RF_MAXSL );
      CHECK( hs_rf_route(64, 0) == 0 && hs_rf_route(65, 0) == 1 && hs_rf_route(65, 1) == 0 && hs_rf_route(512, 1) == 0 );
   }
   /* items, chunks, layouts */
   {
      const hs_rf_rules rules = {scratch, lws, lout};
      const hs_rf_widths W = {13, 8, 3, 9, 6, 7};
      const int ns[] = {12, 600, 130, 64, 65, 512, 1, 129, 300, 128, 17, 512, 40};
      const int nb = (int) (sizeof(ns) / sizeof(ns[0]));
      int ok[nb], form[nb], xnnz[nb];
      for (int b = 0; b < nb; ++b)
      {
         ok[b] = b != 4;
         form[b] = b % 3;
         xnnz[b] = ns[b] <= HS_RF_MAXN ? ns[b] * ns[b] : 5;
      }
      for (int m : {1, 20, 1000})
      {
         std::vector<hs_rf_item> items;
         hs_rf_items(nb, m, ns, ok, form, xnnz, 1, &rules, &items);
         CHECK( (int) items.size() == nb - 2 );
         std::vector<int> seen((size_t) nb, 0);
         std::vector<long long> len(items.size());
         for (size_t k = 0; k < items.size(); ++k)
         {
            const hs_rf_item& it = items[k];
            CHECK( it.blk >= 0 && it.blk < nb && it.n == ns[it.blk] && ok[it.blk] && it.n <= HS_RF_MAXN );
            CHECK( k == 0 || items[k - 1].n > it.n || (items[k - 1].n == it.n && items[k - 1].blk < it.blk) );
            CHECK( it.route == hs_rf_route(it.n, form[it.blk] == 2) && it.klen == hs_rf_klen(it.n, form[it.blk] == 1) );
            CHECK( it.slices == (it.route ? hs_rf_slice_rule(it.n, m, it.klen).slices : 1) );
            const hs_rf_block B = hs_rf_block_make(it.n, m, it.route, it.slices, &rules);
            CHECK( B.len <= it.len && B.VT <= B.part && B.part + (long long) it.slices * it.n * (m + 1) <= B.len );
            CHECK( (B.mat & 1) == 0 && (B.ws & 1) == 0 && (B.out & 1) == 0 && (B.VT & 1) == 0 && (B.part & 1) == 0 && (B.len & 1) == 0 );
            CHECK( it.n > HS_RF_SMALLN ? B.out >= lws(it.n) && B.VT >= B.out + lout(it.n) : B.ws >= (long long) it.n * it.n && B.VT >= B.ws + scratch(it.n) );
            len[k] = it.len;
         }
         for (long long budget : {1LL, 3000000LL, 64LL * 1024 * 1024})
            for (int forced : {0, 1, 3})
            {
               std::fill(seen.begin(), seen.end(), 0);
               int last_n = HS_RF_MAXN + 1, chunks = 0;
               const int rc = hs_chunks_run(len.data(), (int) items.size(), budget, forced, [&](int start, int end)
                  {
                     long long used = 0, trips = 0, rows = 0, vec = 0, blocks = 0;
                     int nlarge = 0;
                     if ( end <= start ) return 1;
                     for (int k = start; k < end; ++k)
                     {
                        const hs_rf_item& it = items[(size_t) k];
                        if ( it.n > last_n ) return 2;
                        last_n = it.n;
                        ++seen[(size_t) it.blk];
                        used += it.len; trips += it.nnz; rows += it.n; vec += (long long) it.n * it.n;
                        blocks += hs_rf_block_make(it.n, m, it.route, it.slices, &rules).len;
                        nlarge += it.n > HS_RF_SMALLN;
                     }
                     if ( forced > 0 ? end - start > forced : (end - start > 1 && used > budget) ) return 3;
                     hs_rf_layout L;
                     hs_rf_layout_make(m, end - start, end - start - nlarge, nlarge, trips, rows, vec, &W, blocks, &L);
                     const long long o[] = {L.rf, L.pp, L.eig, L.ppl, L.sx, L.sr, L.act, L.val, L.row, L.col, L.r_eig, L.r_obj, L.r_coef,
                        L.r_vec, L.blocks, L.len.dev_len};
                     for (int q = 0; q + 1 < 16; ++q)
                        if ( o[q] > o[q + 1] ) return 4;
                     if ( L.r_vec + vec > L.blocks || L.len.dev_len - L.blocks != blocks || L.len.upload_len != L.r_eig
                        || L.len.res_off != L.r_eig || L.len.res_off + L.len.res_len != L.blocks || L.len.pin_len != L.blocks )
                        return 5;
                     /* what the chunk limit counts covers what the layout takes */
                     if ( L.len.dev_len > used ) return 6;
                     ++chunks;
                     return 0;
                  });
               CHECK( rc == 0 );
               for (int b = 0; b < nb; ++b)
                  CHECK( seen[(size_t) b] == (ok[b] && ns[b] <= HS_RF_MAXN ? 1 : 0) );
               CHECK( chunks >= 1 && (forced != 1 || chunks == (int) items.size()) );
            }
      }
      /* stage 2 */
      hs_rf2_layout L2;
      hs_rf2_layout_make(3, 2, 1000, 500, 70000, &W, 4000, 300000, &L2);
      const long long o2[] = {L2.lam, L2.pp, L2.ppl, L2.t_small, L2.t_large, L2.v_small, L2.r_small, L2.c_small, L2.v_large, L2.r_large,
         L2.c_large, L2.tot, L2.ints, L2.mats, L2.len.dev_len};
      for (int q = 0; q + 1 < 15; ++q)
         CHECK( o2[q] <= o2[q + 1] && (o2[q] & 1) == 0 );
      CHECK( L2.pp >= 1000 && L2.r_small - L2.v_small >= 500 && L2.c_small - L2.r_small >= 250 && L2.r_large - L2.v_large >= 70000 );
      CHECK( L2.len.upload_len == L2.t_small && L2.len.res_off == L2.t_small && L2.len.res_off + L2.len.res_len == L2.tot );
      CHECK( L2.len.dev_len - L2.mats == 300000 && L2.mats - L2.ints >= 2000 );
      CHECK( hs_rf2_item_len(512, 512 * 513 / 2) >= 512 + 512LL * 512 + 2LL * 512 * 513 / 2 );
   }
   printf("round plan check: ok\n");
   return 0;
}
