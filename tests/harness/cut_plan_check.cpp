/* cut_plan_check.cpp - stand-alone check of the workspace layouts of the cut calls (scip-sdp_amd/csrc/hs_cut_plan.cpp), meant to be
 * compiled with the host compiler and -fsanitize=address,undefined (tests/test_cut_plan_cpu.py does that).
 * Over a grid of shapes every layout is taken apart into its segments, which must come in the documented order, pairwise disjoint and
 * aligned to their element type, with the read-back window around the result arrays and nothing else; the views are then written
 * through, element by element, on heap blocks of exactly the stated lengths, so an array that leaves its buffer is reported.  For a few
 * shapes per form the offsets are compared with literal numbers: the values of the expressions the entry points of csrc/ipm.hip
 * carried before the layouts were written down here (one deliberate difference, see scl_literals).
 * Prints "cut plan check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_cut_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do { if ( !(cond) ) { printf("cut plan check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static long long scratch_rule(int n) { return 1000 + 7 * n; }           /* (any positive lengths do) */
static long long syevx_ws_rule(int n)                                    /* hs_syevx_ws of csrc/syevx.hip */
{
   const long long n2 = ((long long) n * n + 1) & ~1LL, nl = ((long long) n + 1) & ~1LL;
   return 2 * n2 + 5 * nl + 4 * 32 * nl;
}
static long long syevx_out_rule(int n) { return 40 + 32LL * n; }          /* HS_SYEVX_OUT(n); HS_SYEVX_OUT_VEC is 40 */

/* a segment in bytes from the start of the workspace */
struct Seg { const char* name; long long off, len; int align; bool result; };
static Seg dbl(const char* name, long long off, long long count, bool result) { Seg s = {name, 8 * off, 8 * count, 8, result}; return s; }
static Seg ints(const char* name, long long off, long long count, bool result) { Seg s = {name, 8 * off, 4 * count, 4, result}; return s; }

/* the segments in the order given: ascending, disjoint, aligned; the read-back window holds the result segments and no other; the
 * pinned buffer holds the upload and the read-back, the device buffer everything */
static int check_segments(const std::vector<Seg>& segs, const hs_cut_lens& len)
{
   const long long r0 = 8 * len.res_off, r1 = 8 * (len.res_off + len.res_len);
   CHECK( len.res_off >= 0 && len.res_len >= 0 && len.upload_len >= 0 );
   for (size_t k = 0; k < segs.size(); ++k)
   {
      const Seg& s = segs[k];
      CHECK( s.off >= 0 && s.len >= 0 && s.off % s.align == 0 );
      if ( k > 0 )
         CHECK( segs[k - 1].off + segs[k - 1].len <= s.off );
      if ( s.result )
         CHECK( r0 <= s.off && s.off + s.len <= r1 );
      else
         CHECK( s.off + s.len <= r0 || r1 <= s.off );
      CHECK( s.off + s.len <= 8 * len.dev_len );
   }
   CHECK( len.pin_len >= len.upload_len && len.pin_len >= len.res_off + len.res_len );
   CHECK( len.upload_len <= len.res_off );                    /* the upload does not reach into the results */
   return 0;
}

/* the view of the result arrays on a heap block that ends where the layout says the last of them ends: every element is written */
static int check_view(const hs_cut_res& r, long long m, int maxcuts, long long vec_len, long long buf_len, bool with_sup)
{
   double* buf = (double*) malloc((size_t) (buf_len > 0 ? buf_len : 1) * sizeof(double));
   CHECK( buf != NULL );
   const hs_sc_out o = hs_cut_view(r, buf);
   const long long slots = (long long) r.nb * maxcuts;
   CHECK( o.lmin == buf + r.lmin && o.eig == buf + r.eig && o.lhs == buf + r.lhs && o.coef == buf + r.coef && o.vec == buf + r.vec );
   CHECK( o.smax == r.smax && o.pad == 0 );
   for (long long k = 0; k < r.nb; ++k) o.lmin[k] = 1.0;
   for (long long k = 0; k < slots; ++k) { o.eig[k] = 2.0; o.lhs[k] = 3.0; }
   for (long long k = 0; k < slots * m; ++k) o.coef[k] = 4.0;
   for (long long k = 0; k < vec_len; ++k) o.vec[k] = 5.0;
   if ( r.ints >= 0 )
   {
      CHECK( (void*) o.ncuts == (void*) (buf + r.ints) && o.iters == o.ncuts + r.nb && o.flags == o.iters + r.nb );
      CHECK( (void*) o.sup == (void*) (buf + r.sup) );
      for (long long k = 0; k < r.nb; ++k) { o.ncuts[k] = 6; o.iters[k] = 7; o.flags[k] = 8; }
      if ( with_sup )
         for (long long k = 0; k < slots * r.smax; ++k) o.sup[k] = 9;
   }
   else
      CHECK( o.ncuts == NULL && o.iters == NULL && o.flags == NULL && o.sup == NULL );
   /* nothing wrote over anything else */
   for (long long k = 0; k < r.nb; ++k) CHECK( o.lmin[k] == 1.0 );
   for (long long k = 0; k < slots; ++k) CHECK( o.eig[k] == 2.0 && o.lhs[k] == 3.0 );
   for (long long k = 0; k < slots * m; ++k) CHECK( o.coef[k] == 4.0 );
   for (long long k = 0; k < vec_len; ++k) CHECK( o.vec[k] == 5.0 );
   if ( r.ints >= 0 )
      for (long long k = 0; k < r.nb; ++k) CHECK( o.ncuts[k] == 6 && o.iters[k] == 7 && o.flags[k] == 8 );
   free(buf);
   return 0;
}

static int check_ec(int nb, int m, int maxcuts, long long vec_len, long long slab_len)
{
   hs_ec_layout L;
   hs_ec_layout_make(nb, m, maxcuts, vec_len, slab_len, &L);
   const long long slots = (long long) nb * maxcuts;
   std::vector<Seg> segs;
   segs.push_back(dbl("y", L.y, m, false));
   segs.push_back(dbl("ncuts", L.ncuts, nb, true));
   segs.push_back(dbl("lmin", L.r.lmin, nb, true));
   segs.push_back(dbl("eig", L.r.eig, slots, true));
   segs.push_back(dbl("lhs", L.r.lhs, slots, true));
   segs.push_back(dbl("coef", L.r.coef, slots * m, true));
   segs.push_back(dbl("vec", L.r.vec, vec_len, true));
   segs.push_back(dbl("slabs", L.slabs, slab_len, false));
   if ( check_segments(segs, L.len) != 0 ) return 1;
   CHECK( L.y == 0 && L.len.upload_len == m && L.r.ints == -1 && L.r.sup == -1 && L.r.nb == nb );
   CHECK( L.len.res_off == L.ncuts && L.len.res_off + L.len.res_len == L.slabs && L.len.dev_len == L.slabs + slab_len );
   /* the device view up to the slabs, the pinned view in a block of pin_len */
   if ( check_view(L.r, m, maxcuts, vec_len, L.slabs, false) != 0 ) return 1;
   if ( check_view(L.r, m, maxcuts, vec_len, L.len.pin_len, false) != 0 ) return 1;
   return 0;
}

static int check_sc(int nb, int m, int maxcuts, int smax, long long vec_len, long long slab_len)
{
   hs_sc_layout L;
   hs_sc_layout_make(nb, m, maxcuts, smax, vec_len, slab_len, &L);
   const long long slots = (long long) nb * maxcuts;
   std::vector<Seg> segs;
   segs.push_back(dbl("y", L.y, m, false));
   segs.push_back(ints("sizes", L.sizes, nb, false));
   segs.push_back(dbl("lmin", L.r.lmin, nb, true));
   segs.push_back(dbl("eig", L.r.eig, slots, true));
   segs.push_back(dbl("lhs", L.r.lhs, slots, true));
   segs.push_back(dbl("coef", L.r.coef, slots * m, true));
   segs.push_back(dbl("vec", L.r.vec, vec_len, true));
   segs.push_back(ints("ncuts, iters, flags", L.r.ints, 3LL * nb, true));
   segs.push_back(ints("sup", L.r.sup, slots * smax, false));
   segs.push_back(dbl("slabs", L.slabs, slab_len, false));
   if ( check_segments(segs, L.len) != 0 ) return 1;
   CHECK( L.y == 0 && L.r.nb == nb && L.r.smax == smax );
   CHECK( 8 * L.len.upload_len >= 8 * L.sizes + 4LL * nb );            /* y and the sizes go up in one copy */
   CHECK( L.len.res_off == L.r.lmin && L.len.res_off + L.len.res_len == L.r.sup && L.len.dev_len == L.slabs + slab_len );
   if ( check_view(L.r, m, maxcuts, vec_len, L.slabs, true) != 0 ) return 1;
   if ( check_view(L.r, m, maxcuts, vec_len, L.len.pin_len, false) != 0 ) return 1;
   return 0;
}

static int check_scl(int n, int m, int maxcuts, int smax, long long ws_len, long long out_len, long long out_vec)
{
   hs_scl_layout L;
   hs_scl_layout_make(n, m, maxcuts, smax, ws_len, out_len, out_vec, &L);
   const long long vec_len = (long long) maxcuts * n;
   std::vector<Seg> segs;
   segs.push_back(dbl("y", L.y, m, false));
   segs.push_back(dbl("lmin", L.r.lmin, 1, true));
   segs.push_back(dbl("eig", L.r.eig, maxcuts, true));
   segs.push_back(dbl("lhs", L.r.lhs, maxcuts, true));
   segs.push_back(dbl("coef", L.r.coef, (long long) maxcuts * m, true));
   segs.push_back(dbl("vec", L.r.vec, vec_len, true));
   segs.push_back(ints("ncuts, iters, flags", L.r.ints, 3, true));
   segs.push_back(ints("sup", L.r.sup, (long long) maxcuts * smax, false));
   segs.push_back(dbl("Z", L.Z, (long long) n * n, false));
   segs.push_back(dbl("ws", L.ws, ws_len, false));
   segs.push_back(dbl("o1", L.o1, out_len, false));
   segs.push_back(dbl("o2", L.o2, out_vec, false));
   segs.push_back(dbl("MT", L.MT, (long long) n * n, false));
   if ( check_segments(segs, L.len) != 0 ) return 1;
   CHECK( L.y == 0 && L.len.upload_len == m && L.r.nb == 1 && L.r.smax == smax );
   CHECK( L.len.res_off == L.r.lmin && L.len.res_off + L.len.res_len == L.r.sup );
   CHECK( L.Z % 2 == 0 && L.MT % 2 == 0 );
   CHECK( L.len.pin_len >= L.len.res_off + out_vec );                   /* maxcuts = 0 reads the head of o1 back to the results' place */
   CHECK( L.len.dev_len >= L.MT + (long long) n * n );
   if ( check_view(L.r, m, maxcuts, vec_len, L.Z, true) != 0 ) return 1;
   if ( check_view(L.r, m, maxcuts, vec_len, L.len.pin_len, false) != 0 ) return 1;
   return 0;
}

/* the offsets as literal numbers: the values of the expressions of hipsdp_eigencuts_all before this file existed */
static int ec_literals(void)
{
   hs_ec_layout L;
   hs_ec_layout_make(3, 5, 2, 262, 20307, &L);                      /* blocks of 1, 2, 128 rows; m + 2 odd */
   CHECK( L.ncuts == 6 && L.r.lmin == 9 && L.r.eig == 12 && L.r.lhs == 18 && L.r.coef == 24 && L.r.vec == 54 && L.slabs == 316 );
   CHECK( L.len.res_off == 6 && L.len.res_len == 310 && L.len.upload_len == 5 && L.len.pin_len == 316 && L.len.dev_len == 20623 );
   hs_ec_layout_make(2, 2, 5, 655, 19311, &L);                      /* 3, 128 rows; m + 2 even */
   CHECK( L.ncuts == 4 && L.r.lmin == 6 && L.r.eig == 8 && L.r.lhs == 18 && L.r.coef == 28 && L.r.vec == 48 && L.slabs == 703 );
   CHECK( L.len.res_off == 4 && L.len.res_len == 699 && L.len.upload_len == 2 && L.len.pin_len == 703 && L.len.dev_len == 20014 );
   hs_ec_layout_make(7, 0, 1, 140, 24396, &L);                      /* 1, 2, 3, 128, 1, 2, 3 rows; no variables */
   CHECK( L.ncuts == 2 && L.r.lmin == 9 && L.r.eig == 16 && L.r.lhs == 23 && L.r.coef == 30 && L.r.vec == 30 && L.slabs == 170 );
   CHECK( L.len.res_off == 2 && L.len.res_len == 168 && L.len.upload_len == 0 && L.len.pin_len == 170 && L.len.dev_len == 24566 );
   CHECK( hs_cut_mat_len(1) == 2 && hs_cut_mat_len(2) == 4 && hs_cut_mat_len(3) == 10 && hs_cut_mat_len(128) == 16384 );
   return 0;
}

/* ... of hipsdp_sparsecuts_all and of sparsecuts_small (the last shape: block 1 of 2, 3, 128, 1 rows alone).  nb, 3 nb and
 * slots * smax are odd in the first shape and even in the second; m + 2 is odd in the first and even in the second */
static int sc_literals(void)
{
   hs_sc_layout L;
   hs_sc_layout_make(3, 5, 1, 1, 131, 20307, &L);
   CHECK( L.sizes == 6 && L.r.lmin == 8 && L.r.eig == 11 && L.r.lhs == 14 && L.r.coef == 17 && L.r.vec == 32 && L.r.ints == 163 );
   CHECK( L.r.sup == 168 && L.slabs == 170 && L.len.res_off == 8 && L.len.res_len == 160 && L.len.upload_len == 8 );
   CHECK( L.len.pin_len == 168 && L.len.dev_len == 20477 );
   hs_sc_layout_make(2, 2, 5, 2, 655, 19311, &L);
   CHECK( L.sizes == 4 && L.r.lmin == 5 && L.r.eig == 7 && L.r.lhs == 17 && L.r.coef == 27 && L.r.vec == 47 && L.r.ints == 702 );
   CHECK( L.r.sup == 705 && L.slabs == 715 && L.len.res_off == 5 && L.len.res_len == 700 && L.len.upload_len == 5 );
   CHECK( L.len.pin_len == 705 && L.len.dev_len == 20026 );
   hs_sc_layout_make(7, 1, 2, 128, 280, 24396, &L);
   CHECK( L.sizes == 2 && L.r.lmin == 6 && L.r.eig == 13 && L.r.lhs == 27 && L.r.coef == 41 && L.r.vec == 55 && L.r.ints == 335 );
   CHECK( L.r.sup == 346 && L.slabs == 1242 && L.len.res_off == 6 && L.len.res_len == 340 && L.len.upload_len == 6 );
   CHECK( L.len.pin_len == 346 && L.len.dev_len == 25638 );
   hs_sc_layout_make(4, 3, 5, 3, 15, 1031, &L);
   CHECK( L.sizes == 4 && L.r.lmin == 6 && L.r.eig == 10 && L.r.lhs == 30 && L.r.coef == 50 && L.r.vec == 110 && L.r.ints == 125 );
   CHECK( L.r.sup == 131 && L.slabs == 161 && L.len.res_off == 6 && L.len.res_len == 125 && L.len.upload_len == 6 );
   CHECK( L.len.pin_len == 131 && L.len.dev_len == 1192 );
   return 0;
}

/* ... of sparsecuts_large.  Up to the supports the numbers are those of the earlier expressions.  Behind them the earlier code put Z
 * at sup + (maxcuts smax + 1) / 2, an ODD offset whenever that length is odd (25 in the first shape, 1 in the second); the layout
 * rounds the supports up to an even length, so there Z and everything behind it lie ONE double further (`pad`), and Z and MT are even
 * for every shape.  In the last two shapes (lengths 130 and 0) nothing moved.  The third shape passes odd stand-ins for the two
 * lengths of syevx.hip, which are even for every real n, to reach the odd side of their roundings. */
static int scl_literals(void)
{
   hs_scl_layout L;
   long long pad = 1;
   hs_scl_layout_make(129, 5, 5, 10, 50574, 4168, 40, &L);
   CHECK( L.r.lmin == 6 && L.r.eig == 7 && L.r.lhs == 12 && L.r.coef == 17 && L.r.vec == 42 && L.r.ints == 687 && L.r.sup == 690 );
   CHECK( L.len.res_off == 6 && L.len.res_len == 684 && L.len.upload_len == 5 && L.len.pin_len == 690 );
   CHECK( L.Z == 715 + pad && L.ws == 17357 + pad && L.o1 == 67931 + pad && L.o2 == 72099 + pad && L.MT == 72139 + pad );
   CHECK( L.len.dev_len == 88781 + pad );
   hs_scl_layout_make(512, 2, 1, 1, 592384, 16424, 40, &L);
   CHECK( L.r.lmin == 4 && L.r.eig == 5 && L.r.lhs == 6 && L.r.coef == 7 && L.r.vec == 9 && L.r.ints == 521 && L.r.sup == 524 );
   CHECK( L.len.res_off == 4 && L.len.res_len == 520 && L.len.upload_len == 2 && L.len.pin_len == 524 );
   CHECK( L.Z == 525 + pad && L.ws == 262669 + pad && L.o1 == 855053 + pad && L.o2 == 871477 + pad && L.MT == 871517 + pad );
   CHECK( L.len.dev_len == 1133661 + pad );
   pad = 0;
   hs_scl_layout_make(130, 0, 2, 130, 70001, 4201, 40, &L);
   CHECK( L.r.lmin == 2 && L.r.eig == 3 && L.r.lhs == 5 && L.r.coef == 7 && L.r.vec == 7 && L.r.ints == 267 && L.r.sup == 270 );
   CHECK( L.len.res_off == 2 && L.len.res_len == 268 && L.len.upload_len == 0 && L.len.pin_len == 270 );
   CHECK( L.Z == 400 + pad && L.ws == 17300 + pad && L.o1 == 87302 + pad && L.o2 == 91504 + pad && L.MT == 91544 + pad );
   CHECK( L.len.dev_len == 108444 + pad );
   hs_scl_layout_make(511, 1, 0, 1, 590340, 16392, 40, &L);
   CHECK( L.r.lmin == 2 && L.r.eig == 3 && L.r.lhs == 3 && L.r.coef == 3 && L.r.vec == 3 && L.r.ints == 3 && L.r.sup == 6 );
   CHECK( L.len.res_off == 2 && L.len.res_len == 4 && L.len.upload_len == 1 && L.len.pin_len == 42 );
   CHECK( L.Z == 6 + pad && L.ws == 261128 + pad && L.o1 == 851468 + pad && L.o2 == 867860 + pad && L.MT == 867900 + pad );
   CHECK( L.len.dev_len == 1129022 + pad );
   return 0;
}

int main(void)
{
   static const int NB[] = {1, 2, 3, 7}, M[] = {0, 1, 2, 5}, MC[] = {0, 1, 2, 5}, ROWS[] = {1, 2, 3, 128}, NL[] = {129, 130, 511, 512};
   long long shapes = 0;
   for (int inb = 0; inb < 4; ++inb) for (int im = 0; im < 4; ++im) for (int imc = 0; imc < 4; ++imc) for (int draw = 0; draw < 4; ++draw)
   {
      const int nb = NB[inb], m = M[im], maxcuts = MC[imc];
      /* the blocks' rows: the four sizes in turn, from a different one per draw */
      std::vector<int> rows((size_t) nb);
      long long sum = 0, slab = 0;
      int nmax = 0;
      for (int b = 0; b < nb; ++b)
      {
         rows[b] = ROWS[(b + draw) % 4];
         sum += rows[b];
         slab += hs_cut_mat_len(rows[b]) + scratch_rule(rows[b]);
         nmax = rows[b] > nmax ? rows[b] : nmax;
      }
      if ( check_ec(nb, m, maxcuts, maxcuts * sum, slab) != 0 ) return 1;
      const int smaxes[3] = {1, 2, nmax};
      for (int is = 0; is < 3; ++is)
      {
         /* all blocks served (hipsdp_sparsecuts_all) */
         if ( check_sc(nb, m, maxcuts, smaxes[is], maxcuts * sum, slab) != 0 ) return 1;
         /* one block served and no other has vectors (hipsdp_sparsecuts): the first and the last */
         for (int only = 0; only < nb; only += (nb > 1 ? nb - 1 : 1))
         {
            const int n = rows[only], smax = smaxes[is] <= n ? smaxes[is] : n;
            if ( check_sc(nb, m, maxcuts, smax, (long long) maxcuts * n, hs_cut_mat_len(n) + scratch_rule(n)) != 0 ) return 1;
         }
         ++shapes;
      }
   }
   for (int in = 0; in < 4; ++in) for (int im = 0; im < 4; ++im) for (int imc = 0; imc < 4; ++imc)
   {
      const int n = NL[in], smaxes[3] = {1, 2, n};
      for (int is = 0; is < 3; ++is)
      {
         if ( check_scl(n, M[im], MC[imc], smaxes[is], syevx_ws_rule(n), syevx_out_rule(n), 40) != 0 ) return 1;
         ++shapes;
      }
   }
   /* odd stand-ins for the two lengths handed in (even for every real n) */
   if ( check_scl(129, 1, 1, 1, 70001, 4201, 40) != 0 || check_scl(512, 5, 5, 2, 70001, 4202, 40) != 0 ) return 1;
   if ( ec_literals() != 0 || sc_literals() != 0 || scl_literals() != 0 ) return 1;
   printf("cut plan check: ok (%lld shapes)\n", shapes);
   return 0;
}
