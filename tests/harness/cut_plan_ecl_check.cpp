/* cut_plan_ecl_check.cpp - stand-alone check of the chunk layout of hipsdp_eigencuts_all_large (hs_ecl_layout_make, hs_ecl_block_make,
 * hs_ecl_launches: scip-sdp_amd/csrc/hs_cut_plan.h/.cpp) and of its chunks (hs_chunk_end), meant to be compiled with the host
 * compiler and -fsanitize=address,undefined (tests/test_eigencuts_all_large_cpu.py does that).
 *     y[m] | tridiagonal jobs | vecoff (long long) | act (int) | res (lmin, eig, lhs, coef, vec, ints) | per block: workspace of the
 *     tridiagonal form | selection output
 * Over m = 0, 1, 6, 25, nb = 1 .. 6 blocks of which a subset of mixed rows is served, maxcuts = 0, 1, 5, 32: the parts must come in that
 * order, pairwise disjoint, every one at an even offset (16 bytes), the upload everything in front of the result, the one read-back the
 * result alone, the pinned mirror ending behind the result's ints; every part is then written through on heap blocks of exactly the
 * pinned and the device length.  The chunks of mixed n must cover the list without gaps, stay within the 512 MiB budget unless a chunk
 * is one block, and respect the block count of the environment override.  Offsets of one small case and the launch formula are
 * compared with literal numbers.
 * Prints "cut plan ecl check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_cut_plan.h"
#include "hs_chunks.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do { if ( !(cond) ) { printf("cut plan ecl check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static const int JOBW = 6;       /* sizeof(hs_sxm_job) in doubles */

/* stand-ins for hs_syevx_ws(n) and HS_SXB_OUT(n): the lengths themselves, and odd ones among them */
static long long ws_len(int n) { const long long n2 = ((long long) n * n + 1) & ~1LL, nl = ((long long) n + 1) & ~1LL; return 2 * n2 + 5 * nl + 4 * 32 * nl - (n % 3 == 0); }
static long long out_len(int n) { return 80 + 32LL * n - (n % 5 == 0); }

static int check(int m, int nb, const std::vector<int>& rows, int maxcuts)
{
   const int count = (int) rows.size();
   std::vector<hs_ecl_block> B((size_t) count);
   std::vector<long long> start((size_t) count);
   long long blocks_len = 0, vec_len = 0;
   for (int j = 0; j < count; ++j)
   {
      const int n = rows[j];
      const hs_ecl_block b = hs_ecl_block_make(ws_len(n), out_len(n));
      CHECK( b.ws == 0 && b.out >= b.ws + ws_len(n) && b.len >= b.out + out_len(n) );
      CHECK( b.out % 2 == 0 && b.len % 2 == 0 );
      B[j] = b;
      start[j] = blocks_len;
      blocks_len += b.len;
      vec_len += (long long) maxcuts * n;
   }
   hs_ecl_layout L;
   hs_ecl_layout_make(nb, m, maxcuts, vec_len, count, JOBW, blocks_len, &L);
   const long long slots = (long long) nb * maxcuts;
   CHECK( L.y == 0 && L.jobs >= m && L.vecoff >= L.jobs + (long long) count * JOBW && L.act >= L.vecoff + count );
   CHECK( (L.len.res_off - L.act) * 2 >= count );
   CHECK( L.jobs % 2 == 0 && L.vecoff % 2 == 0 && L.act % 2 == 0 && L.len.res_off % 2 == 0 && L.r.ints % 2 == 0 && L.blocks % 2 == 0 );
   CHECK( L.r.lmin == L.len.res_off && L.r.eig == L.r.lmin + nb && L.r.lhs == L.r.eig + slots && L.r.coef == L.r.lhs + slots );
   CHECK( L.r.vec == L.r.coef + slots * m && L.r.ints >= L.r.vec + vec_len && (L.r.sup - L.r.ints) * 2 >= 3LL * nb );
   CHECK( L.r.nb == nb && L.r.smax == 0 && L.blocks == L.r.sup );
   /* one upload in front of the result; one read-back: the result; the mirror ends behind the result's ints */
   CHECK( L.len.upload_len == L.len.res_off && L.len.res_len == L.r.sup - L.len.res_off && L.len.pin_len == L.r.sup );
   CHECK( L.len.pin_len <= L.blocks && L.len.dev_len == L.blocks + blocks_len );

   double* pin = (double*) malloc((size_t) (L.len.pin_len > 0 ? L.len.pin_len : 1) * sizeof(double));
   CHECK( pin != NULL );
   for (long long k = 0; k < m; ++k) pin[L.y + k] = 1.0;
   for (long long k = 0; k < (long long) count * JOBW; ++k) pin[L.jobs + k] = 3.0;
   long long* vo = (long long*) (pin + L.vecoff);
   for (int k = 0; k < count; ++k) vo[k] = 4 + k;
   int* act = (int*) (pin + L.act);
   for (int k = 0; k < count; ++k) act[k] = 6;
   hs_sc_out h = hs_cut_view(L.r, pin);
   for (int k = 0; k < nb; ++k) { h.lmin[k] = 7.0; h.ncuts[k] = 8; h.iters[k] = 9; h.flags[k] = 10; }
   for (long long k = 0; k < slots; ++k) { h.eig[k] = 11.0; h.lhs[k] = 12.0; }
   for (long long k = 0; k < slots * m; ++k) h.coef[k] = 13.0;
   for (long long k = 0; k < vec_len; ++k) h.vec[k] = 14.0;
   for (long long k = 0; k < m; ++k) CHECK( pin[L.y + k] == 1.0 );
   for (long long k = 0; k < (long long) count * JOBW; ++k) CHECK( pin[L.jobs + k] == 3.0 );
   for (int k = 0; k < count; ++k) CHECK( vo[k] == 4 + k && act[k] == 6 );
   for (int k = 0; k < nb; ++k) CHECK( h.lmin[k] == 7.0 && h.ncuts[k] == 8 && h.iters[k] == 9 && h.flags[k] == 10 );
   for (long long k = 0; k < slots; ++k) CHECK( h.eig[k] == 11.0 && h.lhs[k] == 12.0 );
   for (long long k = 0; k < slots * m; ++k) CHECK( h.coef[k] == 13.0 );
   for (long long k = 0; k < vec_len; ++k) CHECK( h.vec[k] == 14.0 );
   /* the last int of the result is the last thing of the mirror */
   CHECK( (double*) (h.flags + nb) <= pin + L.len.pin_len );
   free(pin);

   if ( L.len.dev_len <= 8000000 )
   {
      double* dev = (double*) malloc((size_t) L.len.dev_len * sizeof(double));
      CHECK( dev != NULL );
      for (int j = 0; j < count; ++j)
      {
         double* base = dev + L.blocks + start[j];
         const int n = rows[j];
         for (long long k = 0; k < ws_len(n); ++k) base[B[j].ws + k] = 26.0 + j;
         for (long long k = 0; k < out_len(n); ++k) base[B[j].out + k] = 27.0 + j;
      }
      for (int j = 0; j < count; ++j)
      {
         const double* base = dev + L.blocks + start[j];
         const int n = rows[j];
         for (long long k = 0; k < ws_len(n); ++k) CHECK( base[B[j].ws + k] == 26.0 + j );
         for (long long k = 0; k < out_len(n); ++k) CHECK( base[B[j].out + k] == 27.0 + j );
      }
      free(dev);
   }
   return 0;
}

static long long block_len(int n) { return hs_ecl_block_make(ws_len(n), out_len(n)).len; }

static int chunks(void)
{
   const long long budget = 512LL * 1024 * 1024 / 8;
   /* a block of 512 rows takes about 4.9 MB: 2 n^2 + 165 n doubles */
   const long long big = block_len(512);
   CHECK( big * 8 > 4800000 && big * 8 < 4950000 );
   /* mixed n, descending: 200 blocks of 512, 257, 200 and 129 rows, 780 MB of workspace: two chunks */
   std::vector<long long> len;
   for (int k = 0; k < 200; ++k)
      len.push_back(block_len(k < 150 ? 512 : (k < 170 ? 257 : (k < 185 ? 200 : 129))));
   int start = 0, n = 0;
   while ( start < 200 )
   {
      const int end = hs_chunk_end(len.data(), 200, start, budget, 0);
      long long used = 0;
      for (int k = start; k < end; ++k) used += len[k];
      CHECK( end > start && end <= 200 && (used <= budget || end == start + 1) );
      CHECK( end == 200 || used + len[end] > budget );          /* (as many as fit) */
      start = end;
      ++n;
   }
   CHECK( n == 2 );
   /* the environment override, a block count instead: one per chunk, three per chunk */
   const long long nolimit = 1LL << 60;                        /* (what the call passes with a block count) */
   for (int k = 0; k < 200; ++k) CHECK( hs_chunk_end(len.data(), 200, k, nolimit, 1) == k + 1 );
   CHECK( hs_chunk_end(len.data(), 200, 0, nolimit, 3) == 3 && hs_chunk_end(len.data(), 200, 199, nolimit, 3) == 200 );
   CHECK( hs_chunk_end(len.data(), 200, 149, nolimit, 3) == 152 );
   CHECK( hs_chunk_end(len.data(), 200, 5, 1, 0) == 6 && hs_chunk_end(len.data(), 0, 0, budget, 0) == 0 );
   return 0;
}

static int launches(void)
{
   /* 2 + (nmax - 1) + 1 + 2 [maxcuts > 0] + 1 */
   CHECK( hs_ecl_launches(5, 200) == 205 && hs_ecl_launches(1, 200) == 205 && hs_ecl_launches(32, 200) == 205 && hs_ecl_launches(0, 200) == 203 );
   CHECK( hs_ecl_launches(5, 129) == 134 && hs_ecl_launches(0, 129) == 132 && hs_ecl_launches(5, 512) == 517 && hs_ecl_launches(0, 512) == 515 );
   for (int mc = 0; mc <= 32; ++mc)
      for (int n = 129; n <= 512; ++n)
      {
         CHECK( hs_ecl_launches(mc, n) == n + 3 + (mc > 0 ? 2 : 0) );
         CHECK( hs_ecl_launches(mc, n) <= n + 6 );             /* (the budget the call was given) */
      }
   return 0;
}

static int literals(void)
{
   const hs_ecl_block b = hs_ecl_block_make(11, 5);
   CHECK( b.ws == 0 && b.out == 12 && b.len == 18 );
   const hs_ecl_block c = hs_ecl_block_make(8, 4);
   CHECK( c.out == 8 && c.len == 12 );
   hs_ecl_layout L;
   /* 3 blocks, m = 5, maxcuts 2, 20 doubles of vectors, 2 served */
   hs_ecl_layout_make(3, 5, 2, 20, 2, JOBW, b.len + c.len, &L);
   CHECK( L.y == 0 && L.jobs == 6 && L.vecoff == 18 && L.act == 20 && L.len.res_off == 22 );
   CHECK( L.r.lmin == 22 && L.r.eig == 25 && L.r.lhs == 31 && L.r.coef == 37 && L.r.vec == 67 && L.r.ints == 88 && L.r.sup == 94 );
   CHECK( L.blocks == 94 && L.len.dev_len == 94 + 18 + 12 && L.len.pin_len == 94 && L.len.upload_len == 22 && L.len.res_len == 72 );
   /* maxcuts = 0: lmin and the ints alone */
   hs_ecl_layout_make(3, 5, 0, 0, 2, JOBW, b.len + c.len, &L);
   CHECK( L.r.lmin == 22 && L.r.eig == 25 && L.r.vec == 25 && L.r.ints == 26 && L.r.sup == 32 && L.len.res_len == 10 );
   return 0;
}

int main(void)
{
   static const int ROWS[] = {129, 130, 200, 257, 511, 512, 150}, MS[] = {0, 1, 6, 25}, MC[] = {0, 1, 5, 32};
   long long shapes = 0;
   for (int nb = 1; nb <= 6; ++nb) for (int im = 0; im < 4; ++im) for (int ic = 0; ic < 4; ++ic) for (int draw = 0; draw < 7; ++draw)
   {
      const int count = 1 + (nb + draw) % nb;
      std::vector<int> rows((size_t) count);
      for (int k = 0; k < count; ++k)
         rows[k] = ROWS[(k + draw) % 7];
      if ( check(MS[im], nb, rows, MC[ic]) != 0 ) return 1;
      ++shapes;
   }
   if ( chunks() != 0 || launches() != 0 || literals() != 0 ) return 1;
   printf("cut plan ecl check: ok (%lld shapes)\n", shapes);
   return 0;
}
