/* cut_plan_rounds_check.cpp - stand-alone check of the workspace layout of the sparse-cut rounds (hs_scr_layout, hs_scr_block of
 * scip-sdp_amd/csrc/hs_cut_plan.h/.cpp), meant to be compiled with the host compiler and -fsanitize=address,undefined
 * (tests/test_sparsecuts_variants_cpu.py does that), in the manner of cut_plan_check.cpp.
 * Over a grid of shapes: the head of the layout IS the layout of hipsdp_sparsecuts_all (same offsets, same upload, same read-back), the
 * per-block pieces behind `state` are carved as the driver of csrc/ipm.hip carves them - ascending, disjoint, every start even, the
 * state struct inside its slot, the last piece ending at dev_len - and every piece is written through on a heap block of exactly
 * dev_len doubles, so a piece that leaves the workspace is reported.
 * Prints "cut plan rounds check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_cut_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do { if ( !(cond) ) { printf("cut plan rounds check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static long long scratch_rule(int n) { return n < 10 ? 4177 : 65559 + (n & 1); }         /* (any positive lengths do; one of them odd) */

static int check(int nb, int m, int maxcuts, const std::vector<int>& rows, const std::vector<int>& sizes)
{
   long long vec_len = 0, slab = 0, state_len = 0;
   int smax = 1;
   for (int b = 0; b < nb; ++b)
   {
      const int ns = sizes[b] <= rows[b] ? sizes[b] : 1;
      vec_len += (long long) maxcuts * rows[b];
      slab += hs_cut_mat_len(rows[b]) + scratch_rule(rows[b]);
      state_len += hs_scr_block_make(rows[b], ns, scratch_rule(ns)).len;
      if ( sizes[b] <= rows[b] && sizes[b] > smax )
         smax = sizes[b];
   }
   hs_scr_layout L;
   hs_sc_layout S;
   hs_scr_layout_make(nb, m, maxcuts, smax, vec_len, slab, state_len, &L);
   hs_sc_layout_make(nb, m, maxcuts, smax, vec_len, slab, &S);
   CHECK( L.sc.y == S.y && L.sc.sizes == S.sizes && L.sc.slabs == S.slabs && L.sc.r.lmin == S.r.lmin && L.sc.r.vec == S.r.vec );
   CHECK( L.sc.r.ints == S.r.ints && L.sc.r.sup == S.r.sup && L.sc.r.smax == smax );
   CHECK( L.len.res_off == S.len.res_off && L.len.res_len == S.len.res_len && L.len.upload_len == S.len.upload_len );
   CHECK( L.len.pin_len == S.len.pin_len );
   CHECK( L.state >= S.len.dev_len && L.state % 2 == 0 && L.len.dev_len == L.state + state_len );
   double* buf = (double*) malloc((size_t) L.len.dev_len * sizeof(double));
   CHECK( buf != NULL );
   long long cur = L.state;
   for (int b = 0; b < nb; ++b)
   {
      const int n = rows[b], ns = sizes[b] <= n ? sizes[b] : 1;
      const hs_scr_block B = hs_scr_block_make(n, ns, scratch_rule(ns));
      CHECK( B.st == 0 && B.v0 >= (long long) ((sizeof(hs_scr_state) + 7) / 8) && B.ZS >= B.v0 + n && B.wsS >= B.ZS + (long long) ns * ns );
      CHECK( B.len >= B.wsS + scratch_rule(ns) );
      CHECK( (cur + B.v0) % 2 == 0 && (cur + B.ZS) % 2 == 0 && (cur + B.wsS) % 2 == 0 && (cur + B.len) % 2 == 0 );
      hs_scr_state* st = reinterpret_cast<hs_scr_state*>(buf + cur + B.st);
      st->maxeig = 1.0; st->nc = 2; st->iters = 3; st->flags = 4; st->done = 5;
      for (int i = 0; i < n; ++i) buf[cur + B.v0 + i] = 6.0;
      for (int i = 0; i < ns * ns; ++i) buf[cur + B.ZS + i] = 7.0;
      for (long long i = 0; i < scratch_rule(ns); ++i) buf[cur + B.wsS + i] = 8.0;
      CHECK( st->maxeig == 1.0 && st->nc == 2 && st->iters == 3 && st->flags == 4 && st->done == 5 );
      for (int i = 0; i < n; ++i) CHECK( buf[cur + B.v0 + i] == 6.0 );
      for (int i = 0; i < ns * ns; ++i) CHECK( buf[cur + B.ZS + i] == 7.0 );
      cur += B.len;
   }
   CHECK( cur == L.len.dev_len );
   free(buf);
   return 0;
}

int main(void)
{
   static const int NB[] = {1, 2, 3, 7}, M[] = {0, 1, 2, 5}, MC[] = {0, 1, 5}, ROWS[] = {1, 2, 3, 9, 10, 127, 128}, SZ[] = {1, 2, 4, 10, 128, 1000};
   long long shapes = 0;
   for (int inb = 0; inb < 4; ++inb) for (int im = 0; im < 4; ++im) for (int imc = 0; imc < 3; ++imc) for (int draw = 0; draw < 7; ++draw)
   {
      const int nb = NB[inb];
      std::vector<int> rows((size_t) nb), sizes((size_t) nb);
      for (int b = 0; b < nb; ++b)
      {
         rows[b] = ROWS[(b + draw) % 7];
         sizes[b] = SZ[(b + 2 * draw) % 6];
      }
      if ( check(nb, M[im], MC[imc], rows, sizes) != 0 ) return 1;
      ++shapes;
   }
   /* the state of a block fits the doubles set aside for it */
   CHECK( sizeof(hs_scr_state) <= HS_SCR_STATE_LEN * sizeof(double) );
   printf("cut plan rounds check: ok (%lld shapes)\n", shapes);
   return 0;
}
