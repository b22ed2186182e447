/* hs_round_plan.h - host-side planning of hipsdp_rounding_frame / hipsdp_rounding_recombine (kernels: csrc/rounding.hip, host side:
 * csrc/cut_calls.hip), and the three rules the kernels and the host must agree on, written down once for both:
 *    hs_rf_weight      the weight of a stored entry (1 on the diagonal, 2 off it) in the packed and the nonzero form - the sweep of the
 *                      dense eigenvector cuts (hs_ec_sweep.h) takes it from here as well
 *    hs_rf_decode      the position (r, c), c <= r, of entry p of a packed lower triangle (p = r (r + 1) / 2 + c), exact for every p the
 *                      engine can hold
 *    hs_rf_slice_rule  in how many slices the matrix-core kernel cuts the storage index of a block - a function of (n, m) and the
 *                      storage length alone, never of the call's other blocks
 * Beside them: which kernel serves a block (hs_rf_route), the order and the chunks of the served blocks, the layouts of a chunk of
 * either stage in the solver's cut workspace (the conventions of hs_cut_plan.h: offsets in doubles, the pinned mirror holds the head,
 * one upload, one read-back) and the launch counts of a chunk.
 * Host only apart from the three inline rules: nothing here includes or calls HIP, so the file compiles with the host compiler alone
 * (tests/harness/round_plan_check.cpp runs it under the sanitizers). */
#ifndef HS_ROUND_PLAN_H
#define HS_ROUND_PLAN_H

#include "hs_cut_plan.h"
#include <math.h>
#include <vector>

#if defined(__HIP__)
#define HS_RF_HD static inline __host__ __device__
#else
#define HS_RF_HD static inline
#endif

#define HS_RF_MAXN   512     /* blocks of more rows are not served */
#define HS_RF_SMALLN 128     /* up to here the one-launch decompositions (eigi.hip), above the batched tridiagonal path */
#define HS_RF_MCN    64      /* blocks of MORE rows held as dense rows or packed triangles go to the matrix cores */
#define HS_RF_TILE   64      /* vectors x matrices of an output tile of the matrix-core kernel */
#define HS_RF_TK     16      /* storage entries of a panel */
#define HS_RF_WGS    512     /* workgroups a block's launch aims at when it has few tiles (two per compute unit of the target) */
#define HS_RF_MINPAN 64      /* panels a slice has at least */
#define HS_RF_MAXSL  64      /* slices at most */

HS_RF_HD double hs_rf_weight(int r, int c) { return r == c ? 1.0 : 2.0; }

HS_RF_HD void hs_rf_decode(long long p, int* r, int* c)
{
   int rr = (int) ((sqrt(8.0 * (double) p + 1.0) - 1.0) * 0.5);
   while ( (long long) rr * (rr + 1) / 2 > p ) --rr;
   while ( (long long) (rr + 1) * (rr + 2) / 2 <= p ) ++rr;
   *r = rr;
   *c = (int) (p - (long long) rr * (rr + 1) / 2);
}

/* entries of a stored matrix: the packed lower triangle or the dense rows */
HS_RF_HD long long hs_rf_klen(int n, int packed) { return packed ? (long long) n * (n + 1) / 2 : (long long) n * n; }

/* slice s of `slices` covers the panels [s pps, min((s + 1) pps, panels)), i.e. the entries [16 s pps, min(16 (s + 1) pps, klen)):
 * every entry once, no slice empty */
struct hs_rf_slices { int slices; long long panels, pps; };
HS_RF_HD hs_rf_slices hs_rf_slice_rule(int n, int m, long long klen)
{
   hs_rf_slices S;
   const long long tiles = (long long) ((n + HS_RF_TILE - 1) / HS_RF_TILE) * (((long long) m + 1 + HS_RF_TILE - 1) / HS_RF_TILE);
   S.panels = (klen + HS_RF_TK - 1) / HS_RF_TK;
   long long want = (HS_RF_WGS + tiles - 1) / tiles;
   const long long most = S.panels / HS_RF_MINPAN;
   if ( want > most ) want = most;
   if ( want > HS_RF_MAXSL ) want = HS_RF_MAXSL;
   if ( want < 1 ) want = 1;
   S.pps = (S.panels + want - 1) / want;
   if ( S.pps < 1 ) S.pps = 1;
   S.slices = (int) ((S.panels + S.pps - 1) / S.pps);
   if ( S.slices < 1 ) S.slices = 1;
   return S;
}

/* workgroups of the matrix-core launch a block of n rows in `slices` slices has: its tiles of vectors x matrices, per slice */
HS_RF_HD long long hs_rf_tiles(int n, int m, int slices)
{
   return (long long) slices * ((n + HS_RF_TILE - 1) / HS_RF_TILE) * (((long long) m + 1 + HS_RF_TILE - 1) / HS_RF_TILE);
}

/* 1: the matrix-core kernel serves the block, 0: the scalar one (at most HS_RF_MCN rows, or kept as nonzeros) */
HS_RF_HD int hs_rf_route(int n, int nonzeros) { return n > HS_RF_MCN && !nonzeros ? 1 : 0; }

/* the lengths of the batched decompositions the plan depends on, in doubles (csrc/eigi.hip: hs_syev_small_scratch; csrc/syevr.hip:
 * hs_syevr_ws, HS_SYEVR_OUT) */
struct hs_rf_rules { long long (*small_scratch)(int n); long long (*large_ws)(int n); long long (*large_out)(int n); };

/* a served block of a stage-1 chunk, as offsets from the block's start, every one even:
 *    up to 128 rows:  mat (n x n: the expanded X) | ws (the decomposition's slab: eigenvalues, vectors)
 *    above:           ws (workspace of the tridiagonal form; its head is the matrix X is expanded into) | out (eigenvalues, vectors)
 *    then             VT (n x n, scalar route alone) | part (slices x n x (m + 1) partial tables)
 * len: where the next block starts */
struct hs_rf_block { long long mat, ws, out, VT, part, len; };
hs_rf_block hs_rf_block_make(int n, int m, int route, int slices, const hs_rf_rules* rules);

/* a served block in the order of the chunks: descending n, the caller's order among equal sizes */
struct hs_rf_item { int blk, n, nonzeros, route, slices; long long klen, pps, nnz, len; };
/* ns[nb]: rows of every block; ok[nb] != 0: the block has its matrices on this device; form[nb]: 0 dense rows, 1 packed, 2 nonzeros;
 * xnnz[nb]: triplets of X_b (stage 1; NULL: none); with_vecs: the vectors are part of the read-back.  len: doubles of a chunk's workspace
 * the block takes in stage 1 */
void hs_rf_items(int nb, int m, const int* ns, const int* ok, const int* form, const int* xnnz, int with_vecs, const hs_rf_rules* rules,
   std::vector<hs_rf_item>* items);
/* what the block takes in a chunk of stage 2: lambda, the n x n result, the counts, its part of the packed result (cap entries at most) */
long long hs_rf2_item_len(int n, int cap);

/* widths of a row of the job tables in doubles (sizeof / 8 of hs_rf_job, hs_pp_job, hs_eig_job, hs_ppl_job, hs_sxm_job, hs_srm_job) */
struct hs_rf_widths { int rf, pp, eig, ppl, sx, sr; };

/* STAGE 1, one chunk of cnt served blocks, nsmall of at most 128 rows and nlarge above (the large ones first), rows = sum of their n:
 *    rf jobs | pp jobs [nsmall] | eig jobs [nsmall] | ppl jobs [nlarge] | sx jobs [nlarge] | sr jobs [nlarge] | act [nlarge] (int)
 *    | triplet values [trips] | rows [trips] (int) | columns [trips] (int)
 *    | res: eig [rows] | obj [rows] | coef [rows m] | vec [vec_len]
 *    | blocks (hs_rf_block, blocks_len doubles in all)
 * every part starts at an even offset.  ONE upload carries everything in front of res, ONE read-back takes res. */
struct hs_rf_layout { long long rf, pp, eig, ppl, sx, sr, act, val, row, col, r_eig, r_obj, r_coef, r_vec, blocks; hs_cut_lens len; };
void hs_rf_layout_make(int m, int cnt, int nsmall, int nlarge, long long trips, long long rows, long long vec_len, const hs_rf_widths* w,
   long long blocks_len, hs_rf_layout* L);

/* STAGE 2, one chunk: rows = sum of n, cap_small / cap_large = sum of min(cap, n (n + 1) / 2) over the blocks of either class
 *    lambda [rows] | pp jobs [nsmall] | ppl jobs [nlarge]
 *    | res: totals [nsmall] (int) | totals [nlarge] (int) | values, rows (int), columns (int) of the small class | the same of the large
 *    | tot [nsmall] (int: the recombination's own totals) | ints [ints_len] (row offsets / tile counts) | the n x n results (mats_len) */
struct hs_rf2_layout { long long lam, pp, ppl, t_small, t_large, v_small, r_small, c_small, v_large, r_large, c_large, tot, ints, mats; hs_cut_lens len; };
void hs_rf2_layout_make(int nsmall, int nlarge, long long rows, long long cap_small, long long cap_large, const hs_rf_widths* w,
   long long ints_len, long long mats_len, hs_rf2_layout* L);

/* kernel launches of one chunk of hipsdp_rounding_frame: a function of the classes present and of nmax_large, the chunk's largest block
 * above 128 rows (0: none), alone - up to 128 rows the expand launch and the 3 decomposition launches; above it the expand launch,
 * nmax - 1 columns, 5 + 6 ceil(nmax / 32) launches for the values and the vectors of the tridiagonal matrices and the
 * back-transformation; then the launch that moves the pairs into the frame, the two coefficient launches and the one that stores the result */
static inline long long hs_rf_launches(int any_small, int nmax_large)
{
   if ( !any_small && nmax_large <= 0 )
      return 0;
   return (any_small ? 4 : 0) + (nmax_large > 0 ? (long long) nmax_large + 6 + 6 * (((long long) nmax_large + 31) / 32) : 0) + 4;
}
/* of one chunk of hipsdp_rounding_recombine: the recombination and the packed write of either class */
static inline long long hs_rf2_launches(int any_small, int any_large) { return (any_small ? 2 : 0) + (any_large ? 2 : 0); }

#endif
