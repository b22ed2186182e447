/* cut_plan_large_check.cpp - stand-alone check of the chunk layout of hipsdp_sparsecuts_all_large (hs_sclr_layout_make,
 * hs_sclr_block_make, hs_sclr_launches: scip-sdp_amd/csrc/hs_cut_plan.h/.cpp) and of its chunks (hs_chunk_end), meant to be compiled
 * with the host compiler and -fsanitize=address,undefined (tests/test_sparsecuts_all_large_cpu.py does that).
 *     y[m] | sizes[nb] (int) | tridiagonal jobs | block table | Z_S jobs | act (int) | res | sup | per block: state | v0 | Z | MT | Z_S |
 *     its slab | workspace of the tridiagonal form | selection output
 * Over m = 0, 1, 6, 25, nb = 1 .. 6 blocks of which a subset of mixed rows is served, maxcuts = 0, 1, 5, with and without Z_S: the parts
 * must come in that order, pairwise disjoint, every one at an even offset (the matrices too), the upload everything in front of the
 * result, the pinned mirror ending behind the result's ints and in front of the supports; every part is then written through on heap
 * blocks of exactly the pinned and the device length.  The chunks of mixed n must cover the list without gaps, stay within the
 * budget unless a chunk is one block, and respect the block cap.  The launch formula is compared with literal numbers.
 * Prints "cut plan large check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_cut_plan.h"
#include "hs_chunks.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do { if ( !(cond) ) { printf("cut plan large check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static const int JOBW = 6, XJOBW = 7, SJOBW = 3;       /* sizeof(hs_sxm_job), sizeof(hs_sclr_job), sizeof(hs_eig_job) in doubles */

/* stand-ins for hs_syevx_ws(n), HS_SXM_OUT(n) and hs_syev_small_scratch(ns): lengths of the same order, odd ones among them */
static long long ws_len(int n) { const long long n2 = ((long long) n * n + 1) & ~1LL, nl = ((long long) n + 1) & ~1LL; return 2 * n2 + 5 * nl + 4 * 32 * nl - (n % 3 == 0); }
static long long out_len(int n) { return 80 + (((long long) n + 1) & ~1LL); }
static long long scratch_len(int ns) { return (long long) ns * ns + 3LL * ns + 129; }

static int check(int m, int nb, const std::vector<int>& rows, const std::vector<int>& zs, int maxcuts, int smax)
{
   const int count = (int) rows.size();
   std::vector<hs_sclr_block> B((size_t) count);
   std::vector<long long> start((size_t) count);
   long long blocks_len = 0, vec_len = 0;
   for (int j = 0; j < count; ++j)
   {
      const int n = rows[j], ns = zs[j];
      const hs_sclr_block b = hs_sclr_block_make(n, ns, scratch_len(ns), ws_len(n), out_len(n));
      CHECK( b.st == 0 && b.v0 >= HS_SCR_STATE_LEN && b.Z >= b.v0 + n && b.MT >= b.Z + (long long) n * n && b.ZS >= b.MT + (long long) n * n );
      CHECK( b.wsS >= b.ZS + (long long) ns * ns && b.ws >= b.wsS + (ns > 0 ? scratch_len(ns) : 0) && b.out >= b.ws + ws_len(n) );
      CHECK( b.len >= b.out + out_len(n) );
      CHECK( b.v0 % 2 == 0 && b.Z % 2 == 0 && b.MT % 2 == 0 && b.ZS % 2 == 0 && b.wsS % 2 == 0 && b.ws % 2 == 0 && b.out % 2 == 0 && b.len % 2 == 0 );
      CHECK( (size_t) HS_SCR_STATE_LEN * sizeof(double) >= sizeof(hs_scr_state) );
      B[j] = b;
      start[j] = blocks_len;
      blocks_len += b.len;
      vec_len += (long long) maxcuts * n;
   }
   hs_sclr_layout L;
   hs_sclr_layout_make(nb, m, maxcuts, smax, vec_len, count, JOBW, XJOBW, SJOBW, blocks_len, &L);
   const long long slots = (long long) nb * maxcuts;
   CHECK( L.y == 0 && L.sizes >= m && (L.jobs - L.sizes) * 2 >= nb && L.xjobs >= L.jobs + (long long) count * JOBW );
   CHECK( L.sjobs >= L.xjobs + (long long) count * XJOBW && L.act >= L.sjobs + (long long) count * SJOBW );
   CHECK( (L.len.res_off - L.act) * 2 >= count );
   CHECK( L.sizes % 2 == 0 && L.jobs % 2 == 0 && L.xjobs % 2 == 0 && L.sjobs % 2 == 0 && L.act % 2 == 0 && L.len.res_off % 2 == 0 && L.blocks % 2 == 0 );
   CHECK( L.r.lmin == L.len.res_off && L.r.eig == L.r.lmin + nb && L.r.lhs == L.r.eig + slots && L.r.coef == L.r.lhs + slots );
   CHECK( L.r.vec == L.r.coef + slots * m && L.r.ints == L.r.vec + vec_len && (L.r.sup - L.r.ints) * 2 >= 3LL * nb );
   CHECK( (L.blocks - L.r.sup) * 2 >= slots * smax && L.r.nb == nb && L.r.smax == smax );
   /* one upload in front of the result; the mirror ends behind the result's ints, in front of the supports */
   CHECK( L.len.upload_len == L.len.res_off && L.len.res_len == L.r.sup - L.len.res_off && L.len.pin_len == L.r.sup );
   CHECK( L.len.pin_len <= L.blocks && L.len.dev_len == L.blocks + blocks_len );

   double* pin = (double*) malloc((size_t) L.len.pin_len * sizeof(double));
   CHECK( pin != NULL );
   for (long long k = 0; k < m; ++k) pin[L.y + k] = 1.0;
   int* sizes = (int*) (pin + L.sizes);
   for (int k = 0; k < nb; ++k) sizes[k] = 2;
   for (long long k = 0; k < (long long) count * JOBW; ++k) pin[L.jobs + k] = 3.0;
   for (long long k = 0; k < (long long) count * XJOBW; ++k) pin[L.xjobs + k] = 4.0;
   for (long long k = 0; k < (long long) count * SJOBW; ++k) pin[L.sjobs + k] = 5.0;
   int* act = (int*) (pin + L.act);
   for (int k = 0; k < count; ++k) act[k] = 6;
   hs_sc_out h = hs_cut_view(L.r, pin);
   for (int k = 0; k < nb; ++k) { h.lmin[k] = 7.0; h.ncuts[k] = 8; h.iters[k] = 9; h.flags[k] = 10; }
   for (long long k = 0; k < slots; ++k) { h.eig[k] = 11.0; h.lhs[k] = 12.0; }
   for (long long k = 0; k < slots * m; ++k) h.coef[k] = 13.0;
   for (long long k = 0; k < vec_len; ++k) h.vec[k] = 14.0;
   for (long long k = 0; k < m; ++k) CHECK( pin[L.y + k] == 1.0 );
   for (int k = 0; k < nb; ++k) CHECK( sizes[k] == 2 );
   for (long long k = 0; k < (long long) count * JOBW; ++k) CHECK( pin[L.jobs + k] == 3.0 );
   for (long long k = 0; k < (long long) count * XJOBW; ++k) CHECK( pin[L.xjobs + k] == 4.0 );
   for (long long k = 0; k < (long long) count * SJOBW; ++k) CHECK( pin[L.sjobs + k] == 5.0 );
   for (int k = 0; k < count; ++k) CHECK( act[k] == 6 );
   for (int k = 0; k < nb; ++k) CHECK( h.lmin[k] == 7.0 && h.ncuts[k] == 8 && h.iters[k] == 9 && h.flags[k] == 10 );
   for (long long k = 0; k < slots; ++k) CHECK( h.eig[k] == 11.0 && h.lhs[k] == 12.0 );
   for (long long k = 0; k < slots * m; ++k) CHECK( h.coef[k] == 13.0 );
   for (long long k = 0; k < vec_len; ++k) CHECK( h.vec[k] == 14.0 );
   free(pin);

   if ( L.len.dev_len <= 8000000 )
   {
      double* dev = (double*) malloc((size_t) L.len.dev_len * sizeof(double));
      CHECK( dev != NULL );
      hs_sc_out o = hs_cut_view(L.r, dev);
      for (long long k = 0; k < slots * smax; ++k) o.sup[k] = 15;
      for (int j = 0; j < count; ++j)
      {
         double* base = dev + L.blocks + start[j];
         const int n = rows[j], ns = zs[j];
         hs_scr_state* S = (hs_scr_state*) (base + B[j].st);
         S->maxeig = 20.0 + j; S->nc = j; S->iters = j; S->flags = j; S->done = j;
         for (int k = 0; k < n; ++k) base[B[j].v0 + k] = 21.0 + j;
         for (long long k = 0; k < (long long) n * n; ++k) { base[B[j].Z + k] = 22.0 + j; base[B[j].MT + k] = 23.0 + j; }
         for (long long k = 0; k < (long long) ns * ns; ++k) base[B[j].ZS + k] = 24.0 + j;
         for (long long k = 0; k < (ns > 0 ? scratch_len(ns) : 0); ++k) base[B[j].wsS + k] = 25.0 + j;
         for (long long k = 0; k < ws_len(n); ++k) base[B[j].ws + k] = 26.0 + j;
         for (long long k = 0; k < out_len(n); ++k) base[B[j].out + k] = 27.0 + j;
      }
      for (long long k = 0; k < slots * smax; ++k) CHECK( o.sup[k] == 15 );
      for (int j = 0; j < count; ++j)
      {
         const double* base = dev + L.blocks + start[j];
         const int n = rows[j], ns = zs[j];
         const hs_scr_state* S = (const hs_scr_state*) (base + B[j].st);
         CHECK( S->maxeig == 20.0 + j && S->nc == j && S->iters == j && S->flags == j && S->done == j );
         for (int k = 0; k < n; ++k) CHECK( base[B[j].v0 + k] == 21.0 + j );
         for (long long k = 0; k < (long long) n * n; ++k) CHECK( base[B[j].Z + k] == 22.0 + j && base[B[j].MT + k] == 23.0 + j );
         for (long long k = 0; k < (long long) ns * ns; ++k) CHECK( base[B[j].ZS + k] == 24.0 + j );
         for (long long k = 0; k < (ns > 0 ? scratch_len(ns) : 0); ++k) CHECK( base[B[j].wsS + k] == 25.0 + j );
         for (long long k = 0; k < ws_len(n); ++k) CHECK( base[B[j].ws + k] == 26.0 + j );
         for (long long k = 0; k < out_len(n); ++k) CHECK( base[B[j].out + k] == 27.0 + j );
      }
      free(dev);
   }
   return 0;
}

static long long block_len(int n, int ns) { return hs_sclr_block_make(n, ns, scratch_len(ns), ws_len(n), out_len(n)).len; }

static int chunks(void)
{
   const long long budget = 512LL * 1024 * 1024 / 8;
   /* a block of 512 rows takes about 9 MB: 4.24 n^2 doubles */
   const long long big = block_len(512, 0);
   CHECK( big * 8 > 8800000 && big * 8 < 9200000 );
   /* mixed n, descending: 100 blocks of 512, 257, 200 and 129 rows, 670 MB of workspace: two chunks */
   std::vector<long long> len;
   for (int k = 0; k < 100; ++k)
      len.push_back(block_len(k < 70 ? 512 : (k < 80 ? 257 : (k < 90 ? 200 : 129)), 24 + k % 5));
   int start = 0, n = 0;
   while ( start < 100 )
   {
      const int end = hs_chunk_end(len.data(), 100, start, budget, 0);
      long long used = 0;
      for (int k = start; k < end; ++k) used += len[k];
      CHECK( end > start && end <= 100 && (used <= budget || end == start + 1) );
      CHECK( end == 100 || used + len[end] > budget );          /* (as many as fit) */
      start = end;
      ++n;
   }
   CHECK( n == 2 );
   /* a block count instead: one per chunk, three per chunk */
   const long long nolimit = 1LL << 60;                        /* (what the call passes with a block count) */
   for (int k = 0; k < 100; ++k) CHECK( hs_chunk_end(len.data(), 100, k, nolimit, 1) == k + 1 );
   CHECK( hs_chunk_end(len.data(), 100, 0, nolimit, 3) == 3 && hs_chunk_end(len.data(), 100, 99, nolimit, 3) == 100 );
   CHECK( hs_chunk_end(len.data(), 100, 69, nolimit, 3) == 72 );
   CHECK( hs_chunk_end(len.data(), 100, 5, 1, 0) == 6 && hs_chunk_end(len.data(), 0, 0, budget, 0) == 0 );
   return 0;
}

static int launches(void)
{
   /* variant 0: nmax + 6 (nmax + 5 without cuts), whatever maxcuts is */
   CHECK( hs_sclr_launches(0, 5, 200) == 206 && hs_sclr_launches(0, 1, 200) == 206 && hs_sclr_launches(0, 0, 200) == 205 );
   CHECK( hs_sclr_launches(0, 5, 129) == 135 && hs_sclr_launches(0, 5, 512) == 518 );
   /* 1 + (nmax + 3) + maxcuts (1 + 4 s + d (nmax + 3)) + 1 + [maxcuts > 0] */
   CHECK( hs_sclr_launches(1, 5, 200) == 231 && hs_sclr_launches(2, 5, 200) == 1226 && hs_sclr_launches(4, 5, 200) == 1226 );
   CHECK( hs_sclr_launches(6, 5, 200) == 1226 && hs_sclr_launches(7, 5, 200) == 1246 && hs_sclr_launches(3, 5, 200) == 1246 );
   CHECK( hs_sclr_launches(7, 1, 129) == 1 + 132 + (1 + 4 + 132) + 1 + 1 && hs_sclr_launches(7, 0, 129) == 134 );
   for (unsigned v = 1; v < 8; ++v)
      for (int mc = 0; mc <= 6; ++mc)
         for (int n = 129; n <= 512; n += 127)
         {
            const int s = (v & 1) ? 1 : 0, d = (v & 6) ? 1 : 0;
            CHECK( hs_sclr_launches(v, mc, n) == 1 + (n + 3) + (long long) mc * (1 + 4 * s + d * (n + 3)) + 1 + (mc > 0 ? 1 : 0) );
         }
   return 0;
}

static int literals(void)
{
   const hs_sclr_block b = hs_sclr_block_make(5, 3, 7, 11, 4);
   CHECK( b.st == 0 && b.v0 == 4 && b.Z == 10 && b.MT == 36 && b.ZS == 62 && b.wsS == 72 && b.ws == 80 && b.out == 92 && b.len == 96 );
   const hs_sclr_block c = hs_sclr_block_make(5, 0, 0, 11, 4);
   CHECK( c.ZS == 62 && c.wsS == 62 && c.ws == 62 && c.out == 74 && c.len == 78 );
   hs_sclr_layout L;
   hs_sclr_layout_make(3, 5, 2, 4, 20, 2, JOBW, XJOBW, SJOBW, b.len + c.len, &L);
   CHECK( L.y == 0 && L.sizes == 6 && L.jobs == 8 && L.xjobs == 20 && L.sjobs == 34 && L.act == 40 && L.len.res_off == 42 );
   CHECK( L.r.lmin == 42 && L.r.eig == 45 && L.r.lhs == 51 && L.r.coef == 57 && L.r.vec == 87 && L.r.ints == 107 && L.r.sup == 112 );
   CHECK( L.blocks == 124 && L.len.dev_len == 124 + 96 + 78 && L.len.pin_len == 112 && L.len.upload_len == 42 && L.len.res_len == 70 );
   return 0;
}

int main(void)
{
   static const int ROWS[] = {129, 130, 200, 257, 511, 512, 150}, MS[] = {0, 1, 6, 25}, MC[] = {0, 1, 5};
   long long shapes = 0;
   for (int nb = 1; nb <= 6; ++nb) for (int im = 0; im < 4; ++im) for (int ic = 0; ic < 3; ++ic) for (int draw = 0; draw < 7; ++draw)
   {
      const int count = 1 + (nb + draw) % nb;
      std::vector<int> rows((size_t) count), zs((size_t) count);
      int smax = 1;
      for (int k = 0; k < count; ++k)
      {
         rows[k] = ROWS[(k + draw) % 7];
         zs[k] = draw % 2 ? 0 : (k % 2 ? 128 : 3 + k);
         const int size = draw % 2 ? 5 + 100 * k : zs[k];
         smax = size > smax ? size : smax;
      }
      if ( check(MS[im], nb, rows, zs, MC[ic], smax) != 0 ) return 1;
      ++shapes;
   }
   if ( chunks() != 0 || launches() != 0 || literals() != 0 ) return 1;
   printf("cut plan large check: ok (%lld shapes)\n", shapes);
   return 0;
}
