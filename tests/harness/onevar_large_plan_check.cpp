/* onevar_large_plan_check.cpp - stand-alone check of the chunk layout and the chunk splitter of hipsdp_onevar_bounds_large
 * (hs_ovl_layout_make: scip-sdp_amd/csrc/hs_cut_plan.cpp; hs_chunk_end, hs_chunks_run: csrc/hs_chunks.h), meant to be compiled with the host compiler and
 * -fsanitize=address,undefined (tests/test_onevar_large_cpu.py does that).
 *     u[m] | table | job table | act (int) | nactive | result | state | Z of the chunk's blocks | per job: workspace, output
 * Over m = 0, 1, 6, 7, count = 1 .. 9 jobs of mixed rows the parts must come in that order, pairwise disjoint, each at an even offset,
 * the upload in front of the result, the pinned mirror behind it and in front of the state; every part is then written through on heap
 * blocks of exactly the pinned and the device length.  The splitter must cover a list without gaps, keep a chunk within its budget
 * unless it is one job, and respect the job cap.  A few shapes are compared with literal numbers.
 * Prints "onevar large plan check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_cut_plan.h"
#include "hs_chunks.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do { if ( !(cond) ) { printf("onevar large plan check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static const int TABW = 8, JOBW = 6, RESW = 6, STATEW = 10;      /* HS_OVA_TAB, sizeof(hs_sxm_job) / 8, HS_OV_RES, HS_OVL_STATE */

/* stand-ins for hs_syevx_ws(n) and HS_SXM_OUT(n) of csrc/syevx.hip / hs_kernels.h: the same formulas */
static long long ws_len(int n) { const long long n2 = ((long long) n * n + 1) & ~1LL, nl = ((long long) n + 1) & ~1LL; return 2 * n2 + 5 * nl + 4 * 32 * nl; }
static long long out_len(int n) { return 80 + (((long long) n + 1) & ~1LL); }

static int check(int m, const std::vector<int>& rows, long long zlen)
{
   const int count = (int) rows.size();
   std::vector<long long> wl((size_t) count), ol((size_t) count), ws((size_t) count, -1), out((size_t) count, -1);
   for (int k = 0; k < count; ++k)
   {
      wl[k] = ws_len(rows[k]) - (k % 2);            /* (odd lengths too: the layout rounds them up) */
      ol[k] = out_len(rows[k]) - (k % 3 == 0 ? 1 : 0);
   }
   hs_ovl_layout L;
   hs_ovl_layout_make(m, count, TABW, JOBW, RESW, STATEW, zlen, wl.data(), ol.data(), ws.data(), out.data(), &L);
   CHECK( L.u == 0 && L.tab >= m && L.jobs >= L.tab + (long long) count * TABW && L.act >= L.jobs + (long long) count * JOBW );
   CHECK( (L.nactive - L.act) * 2 >= count && L.res == L.nactive + 2 && L.state >= L.res + (long long) count * RESW );
   CHECK( L.Z >= L.state + (long long) count * STATEW && L.slabs >= L.Z + zlen );
   CHECK( L.tab % 2 == 0 && L.jobs % 2 == 0 && L.act % 2 == 0 && L.nactive % 2 == 0 && L.res % 2 == 0 && L.state % 2 == 0 && L.Z % 2 == 0
      && L.slabs % 2 == 0 );
   long long at = L.slabs;
   for (int k = 0; k < count; ++k)
   {
      CHECK( ws[k] == at && ws[k] % 2 == 0 && out[k] >= ws[k] + wl[k] && out[k] % 2 == 0 );
      at = out[k] + ol[k];
      at += at & 1;
   }
   CHECK( L.len.dev_len == at );
   CHECK( L.len.upload_len == L.res && L.len.res_off == L.res && L.len.res_len == (long long) count * RESW );
   CHECK( L.len.pin_len == L.res + L.len.res_len && L.len.pin_len <= L.state && L.len.dev_len >= L.len.pin_len );

   double* pin = (double*) malloc((size_t) L.len.pin_len * sizeof(double));
   CHECK( pin != NULL );
   for (long long k = 0; k < m; ++k) pin[L.u + k] = 1.0;
   for (long long k = 0; k < (long long) count * TABW; ++k) pin[L.tab + k] = 2.0;
   for (long long k = 0; k < (long long) count * JOBW; ++k) pin[L.jobs + k] = 3.0;
   int* act = (int*) (pin + L.act);
   for (int k = 0; k < count; ++k) act[k] = 4;
   int* nact = (int*) (pin + L.nactive);
   nact[0] = 5; nact[1] = 5;
   for (long long k = 0; k < L.len.res_len; ++k) pin[L.res + k] = 6.0;
   for (long long k = 0; k < m; ++k) CHECK( pin[L.u + k] == 1.0 );
   for (long long k = 0; k < (long long) count * TABW; ++k) CHECK( pin[L.tab + k] == 2.0 );
   for (long long k = 0; k < (long long) count * JOBW; ++k) CHECK( pin[L.jobs + k] == 3.0 );
   for (int k = 0; k < count; ++k) CHECK( act[k] == 4 );
   CHECK( nact[0] == 5 && nact[1] == 5 );
   for (long long k = 0; k < L.len.res_len; ++k) CHECK( pin[L.res + k] == 6.0 );
   free(pin);

   if ( L.len.dev_len <= 8000000 )
   {
      double* dev = (double*) malloc((size_t) L.len.dev_len * sizeof(double));
      CHECK( dev != NULL );
      for (long long k = 0; k < L.Z; ++k) dev[k] = 0.0;
      for (long long k = 0; k < (long long) count * STATEW; ++k) dev[L.state + k] = 7.0;
      for (long long k = 0; k < zlen; ++k) dev[L.Z + k] = 8.0;
      for (int j = 0; j < count; ++j)
      {
         for (long long k = 0; k < wl[j]; ++k) dev[ws[j] + k] = 10.0 + j;
         for (long long k = 0; k < ol[j]; ++k) dev[out[j] + k] = 100.0 + j;
      }
      for (long long k = 0; k < (long long) count * STATEW; ++k) CHECK( dev[L.state + k] == 7.0 );
      for (long long k = 0; k < zlen; ++k) CHECK( dev[L.Z + k] == 8.0 );
      for (int j = 0; j < count; ++j)
      {
         for (long long k = 0; k < wl[j]; ++k) CHECK( dev[ws[j] + k] == 10.0 + j );
         for (long long k = 0; k < ol[j]; ++k) CHECK( dev[out[j] + k] == 100.0 + j );
      }
      free(dev);
   }
   return 0;
}

static int chunks(void)
{
   /* 64 jobs of 512 rows with the default budget of 512 MiB: 4.7 MB each, so one chunk holds 113 of them - all 64 */
   std::vector<long long> len(64, ws_len(512) + out_len(512));
   const long long budget = 512LL * 1024 * 1024 / 8;
   CHECK( hs_chunk_end(len.data(), 64, 0, budget, 0) == 64 );
   len.assign(300, ws_len(512) + out_len(512));
   const int per = (int) (budget / len[0]);
   CHECK( per == 113 );
   int start = 0, n = 0;
   while ( start < 300 )
   {
      const int end = hs_chunk_end(len.data(), 300, start, budget, 0);
      CHECK( end > start && end - start <= per && (end == 300 || end - start == per) );
      start = end;
      ++n;
   }
   CHECK( n == 3 );
   /* a job count: chunks of exactly two, the last one of what is left; a budget below one job still makes progress */
   CHECK( hs_chunk_end(len.data(), 7, 0, len[0] * 2, 2) == 2 && hs_chunk_end(len.data(), 7, 6, len[0] * 2, 2) == 7 );
   CHECK( hs_chunk_end(len.data(), 7, 3, 1, 0) == 4 );
   CHECK( hs_chunk_end(len.data(), 0, 0, budget, 0) == 0 );
   /* descending lengths: the budget counts the doubles of the jobs, not their number */
   long long mixed[5] = { 100, 60, 40, 30, 5 };
   CHECK( hs_chunk_end(mixed, 5, 0, 160, 0) == 2 && hs_chunk_end(mixed, 5, 2, 160, 0) == 5 );
   return 0;
}

/* what a job of n rows counts for in a chunk (hs_onevar_large_job_len, csrc/onevar_large.hip, from the stand-ins above) */
static long long job_len(int n) { return ((ws_len(n) + 1) & ~1LL) + out_len(n); }

/* the driver: a forced job count stands alone.  The call used to pass  job_len[start] * count  as the budget of such a chunk, which is
 * no bound only because the lengths do not increase along a list ordered by descending n - asserted here for every n the call serves -
 * so on such a list the driver's chunks are those of that budget */
static int driver(void)
{
   for (int n = 3; n <= 512; ++n)
      CHECK( job_len(n) >= job_len(n - 1) );
   static const int ROWS[] = {512, 512, 511, 257, 257, 257, 200, 130, 129, 129, 129};
   std::vector<long long> len;
   for (int k = 0; k < 11; ++k)
      len.push_back(job_len(ROWS[k]));
   for (int forced = 1; forced <= 12; ++forced)
   {
      int next = 0, bad = 0;
      CHECK( hs_chunks_run(len.data(), 11, 1, forced, [&](int start, int end)
         {
            bad += (start != next || end != (start + forced < 11 ? start + forced : 11)) ? 1 : 0;
            bad += end != hs_chunk_end(len.data(), 11, start, len[start] * forced, forced) ? 1 : 0;
            next = end;
            return 0;
         }) == 0 );
      CHECK( bad == 0 && next == 11 );
   }
   /* no forced count: the budget binds; the first status that is not 0 ends the walk and is returned */
   int calls = 0;
   CHECK( hs_chunks_run(len.data(), 11, len[0] * 2, 0, [&](int start, int end) { ++calls; return end - start == 2 && start == 0 ? 0 : 7; }) == 7 );
   CHECK( calls == 2 );
   CHECK( hs_chunks_run(len.data(), 0, 1, 0, [&](int, int) { ++calls; return 7; }) == 0 && calls == 2 );
   return 0;
}

static int literals(void)
{
   hs_ovl_layout L;
   long long wl[2] = { 11, 4 }, ol[2] = { 3, 2 }, ws[2], out[2];
   hs_ovl_layout_make(5, 2, TABW, JOBW, RESW, STATEW, 7, wl, ol, ws, out, &L);
   CHECK( L.u == 0 && L.tab == 6 && L.jobs == 22 && L.act == 34 && L.nactive == 36 && L.res == 38 && L.state == 50 && L.Z == 70 && L.slabs == 78 );
   CHECK( ws[0] == 78 && out[0] == 90 && ws[1] == 94 && out[1] == 98 && L.len.dev_len == 100 );
   CHECK( L.len.upload_len == 38 && L.len.res_off == 38 && L.len.res_len == 12 && L.len.pin_len == 50 );
   return 0;
}

int main(void)
{
   static const int ROWS[] = {2, 3, 64, 65, 128, 129, 257, 512, 130}, MS[] = {0, 1, 6, 7};
   long long shapes = 0;
   for (int count = 1; count <= 9; ++count) for (int im = 0; im < 4; ++im) for (int draw = 0; draw < 9; ++draw)
   {
      std::vector<int> rows((size_t) count);
      long long zlen = 0;
      for (int k = 0; k < count; ++k)
      {
         rows[k] = ROWS[(k + draw) % 9];
         if ( k % 2 == 0 ) zlen += hs_cut_mat_len(rows[k]);
      }
      if ( check(MS[im], rows, zlen) != 0 ) return 1;
      ++shapes;
   }
   if ( chunks() != 0 || driver() != 0 || literals() != 0 ) return 1;
   printf("onevar large plan check: ok (%lld shapes)\n", shapes);
   return 0;
}
