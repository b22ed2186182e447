/* onevar_plan_check.cpp - stand-alone check of the workspace layout of hipsdp_onevar_bounds_all (hs_ova_layout,
 * scip-sdp_amd/csrc/hs_cut_plan.cpp), meant to be compiled with the host compiler and -fsanitize=address,undefined
 * (tests/test_onevar_all_cpu.py does that).
 *     u[m] | table [count][tabw] | result [count][resw] | Z of every block with jobs | slabs of the 65-128 class
 * Over nb = 1 .. 5 blocks (rows drawn from both size classes), count = 0, 1, 1000 jobs and a grid cap of 1 and 256 for the 65-128
 * class the segments must come in that order, pairwise disjoint, matrices at even offsets, the read-back window around the result
 * alone, the pinned length over upload and read-back; table and result are then written through on heap blocks of exactly the pinned
 * length, every Z and every workgroup's slab on a block of exactly the device length.  A few shapes are compared with literal numbers.
 * Prints "onevar plan check: ok" and returns 0, or says what failed and returns 1. */
#include "hs_cut_plan.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CHECK(cond) do { if ( !(cond) ) { printf("onevar plan check FAILED at line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static const int TABW = 8, RESW = 6;           /* HS_OVA_TAB, HS_OV_RES of csrc/hs_kernels.h */

static int check(int m, int count, const std::vector<int>& rows, int cap)
{
   long long zlen = 0;
   int nmid = 0, jobs_mid = 0;
   for (size_t b = 0; b < rows.size(); ++b)
   {
      zlen += hs_cut_mat_len(rows[b]);
      if ( rows[b] > 64 )
      {
         nmid = rows[b] > nmid ? rows[b] : nmid;
         ++jobs_mid;
      }
   }
   /* the jobs go round the blocks: those of the 65-128 class are count * jobs_mid / nb, the grid at most the cap */
   const long long midjobs = (long long) count * jobs_mid / (long long) rows.size();
   const int grid = (int) (midjobs < cap ? midjobs : cap);
   hs_ova_layout L;
   hs_ova_layout_make(m, count, TABW, RESW, zlen, grid, grid > 0 ? nmid : 0, &L);
   const long long tab_len = (long long) count * TABW, res_len = (long long) count * RESW;
   const long long slab_one = grid > 0 ? 2LL * nmid * nmid : 0;
   /* order and disjointness */
   CHECK( L.u == 0 && L.tab >= m && L.res == L.tab + tab_len && L.Z >= L.res + res_len && L.slabs >= L.Z + zlen );
   CHECK( L.len.dev_len == L.slabs + grid * slab_one );
   /* matrices start at even offsets */
   CHECK( L.tab % 2 == 0 && L.Z % 2 == 0 && L.slabs % 2 == 0 && slab_one % 2 == 0 );
   long long z = L.Z;
   for (size_t b = 0; b < rows.size(); ++b)
   {
      CHECK( z % 2 == 0 && z + (long long) rows[b] * rows[b] <= L.slabs );
      z += hs_cut_mat_len(rows[b]);
   }
   /* the read-back is the result and nothing else; the upload is u and the table and does not reach into it; the pinned mirror
    * holds both */
   CHECK( L.len.res_off == L.res && L.len.res_len == res_len && L.len.upload_len == L.res );
   CHECK( L.len.upload_len >= L.tab + tab_len && L.len.upload_len <= L.len.res_off );
   CHECK( L.len.pin_len >= L.len.upload_len && L.len.pin_len >= L.len.res_off + L.len.res_len && L.len.pin_len <= L.Z );
   CHECK( L.len.dev_len >= L.len.pin_len );

   /* written through: the pinned mirror ... */
   double* pin = (double*) malloc((size_t) (L.len.pin_len > 0 ? L.len.pin_len : 1) * sizeof(double));
   CHECK( pin != NULL );
   for (long long k = 0; k < m; ++k) pin[L.u + k] = 1.0;
   for (long long k = 0; k < tab_len; ++k) pin[L.tab + k] = 2.0;
   for (long long k = 0; k < res_len; ++k) pin[L.res + k] = 3.0;
   for (long long k = 0; k < m; ++k) CHECK( pin[L.u + k] == 1.0 );
   for (long long k = 0; k < tab_len; ++k) CHECK( pin[L.tab + k] == 2.0 );
   for (long long k = 0; k < res_len; ++k) CHECK( pin[L.res + k] == 3.0 );
   free(pin);
   /* ... and the device side: every Z with its own rows, every workgroup's slab */
   if ( L.len.dev_len <= 40000000 )
   {
      double* dev = (double*) malloc((size_t) (L.len.dev_len > 0 ? L.len.dev_len : 1) * sizeof(double));
      CHECK( dev != NULL );
      for (long long k = 0; k < L.len.pin_len; ++k) dev[k] = 0.0;
      z = L.Z;
      for (size_t b = 0; b < rows.size(); ++b)
      {
         for (long long k = 0; k < (long long) rows[b] * rows[b]; ++k) dev[z + k] = 4.0 + (double) b;
         z += hs_cut_mat_len(rows[b]);
      }
      for (int w = 0; w < grid; ++w)
         for (long long k = 0; k < slab_one; ++k) dev[L.slabs + w * slab_one + k] = 100.0 + w;
      z = L.Z;
      for (size_t b = 0; b < rows.size(); ++b)
      {
         for (long long k = 0; k < (long long) rows[b] * rows[b]; ++k) CHECK( dev[z + k] == 4.0 + (double) b );
         z += hs_cut_mat_len(rows[b]);
      }
      for (int w = 0; w < grid; ++w)
         CHECK( dev[L.slabs + w * slab_one] == 100.0 + w && dev[L.slabs + (w + 1) * slab_one - 1] == 100.0 + w );
      free(dev);
   }
   return 0;
}

/* the offsets as literal numbers */
static int literals(void)
{
   hs_ova_layout L;
   /* the five blocks of the tests (3, 17, 64, 65, 128 rows), six variables, 30 jobs, twelve of them on twelve workgroups */
   hs_ova_layout_make(6, 30, TABW, RESW, 10 + 290 + 4096 + 4226 + 16384, 12, 128, &L);
   CHECK( L.u == 0 && L.tab == 6 && L.res == 246 && L.Z == 426 && L.slabs == 25432 );
   CHECK( L.len.res_off == 246 && L.len.res_len == 180 && L.len.upload_len == 246 && L.len.pin_len == 426 );
   CHECK( L.len.dev_len == 25432 + 12LL * 2 * 128 * 128 );
   /* an odd number of variables and of result doubles; no job of the 65-128 class */
   hs_ova_layout_make(5, 3, TABW, 5, 10, 0, 0, &L);
   CHECK( L.tab == 6 && L.res == 30 && L.Z == 46 && L.slabs == 56 && L.len.dev_len == 56 && L.len.pin_len == 45 );
   /* a round of 100000 jobs on 256 compute units: the slabs are 64 MB whatever the count */
   hs_ova_layout_make(40, 100000, TABW, RESW, 16384, 256, 128, &L);
   CHECK( L.len.dev_len - L.slabs == 256LL * 2 * 128 * 128 && (L.len.dev_len - L.slabs) * 8 == 64LL * 1024 * 1024 );
   /* nothing at all */
   hs_ova_layout_make(0, 0, TABW, RESW, 0, 0, 0, &L);
   CHECK( L.tab == 0 && L.res == 0 && L.Z == 0 && L.slabs == 0 && L.len.dev_len == 0 && L.len.pin_len == 0 );
   return 0;
}

int main(void)
{
   static const int ROWS[] = {3, 17, 64, 65, 128, 1, 127, 66}, COUNT[] = {0, 1, 1000}, CAP[] = {1, 256}, MS[] = {0, 1, 6, 7};
   long long shapes = 0;
   for (int nb = 1; nb <= 5; ++nb) for (int ic = 0; ic < 3; ++ic) for (int ig = 0; ig < 2; ++ig) for (int im = 0; im < 4; ++im)
      for (int draw = 0; draw < 8; ++draw)
      {
         std::vector<int> rows((size_t) nb);
         for (int b = 0; b < nb; ++b)
            rows[b] = ROWS[(b + draw) % 8];
         if ( check(MS[im], COUNT[ic], rows, CAP[ig]) != 0 ) return 1;
         ++shapes;
      }
   if ( literals() != 0 ) return 1;
   printf("onevar plan check: ok (%lld shapes)\n", shapes);
   return 0;
}
