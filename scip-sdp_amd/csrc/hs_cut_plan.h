/* hs_cut_plan.h - where everything lies in the workspace of the cut calls of csrc/cut_calls.hip (hipsdp_eigencuts_all, hipsdp_sparsecuts_all,
 * hipsdp_sparsecuts): one layout per call form, written down once.  All offsets and lengths count doubles from the start of the device
 * workspace; the pinned host buffer mirrors its head (upload and read-back lie at the same offsets), so ONE view function gives the
 * pointers the launches take (applied to the device buffer) and the pointers the copy-out reads (applied to the pinned one).
 * Host only: nothing here includes or calls HIP, so the file compiles with the host compiler alone (tests/harness/cut_plan_check.cpp
 * runs it under the sanitizers). */
#ifndef HS_CUT_PLAN_H
#define HS_CUT_PLAN_H

#include <string.h>

/* where the kernels of sparsecuts.hip / sparsecuts_large.hip put their results, all indexed by the block's index (hs_ec_job.blk) or its
 * slots blk * maxcuts + c; sup: smax ints per slot, the ascending support of the cut (k_sc_tpower writes it, k_sc_coefs reads it) */
struct hs_sc_out { int *ncuts, *iters, *flags; double *lmin, *eig, *lhs, *coef, *vec; int* sup; int smax, pad; };

/* the result arrays of a call over nb blocks with slots = nb maxcuts, in this order:
 *    lmin[nb] | eig[slots] | lhs[slots] | coef[slots m] | vec[vec_len] | ints: ncuts[nb], iters[nb], flags[nb] | sup[slots smax] (int)
 * ints and sup are -1 in the form that has none (eigencuts-all: its counts are doubles in front of lmin) */
struct hs_cut_res { long long lmin, eig, lhs, coef, vec, ints, sup; int nb, smax; };

/* res_off, res_len: the one read-back (to the same offset of the pinned buffer); upload_len: doubles uploaded from offset 0 */
struct hs_cut_lens { long long res_off, res_len, upload_len, pin_len, dev_len; };

/* hipsdp_eigencuts_all:  y | ncuts[nb] (as doubles) | res | slabs (Z and decomposition workspace of every batched block) */
struct hs_ec_layout { long long y, ncuts; hs_cut_res r; long long slabs; hs_cut_lens len; };
/* hipsdp_sparsecuts_all, and hipsdp_sparsecuts up to 128 rows:  y | sizes[nb] (int) | res | sup | slabs */
struct hs_sc_layout { long long y, sizes; hs_cut_res r; long long slabs; hs_cut_lens len; };
/* hipsdp_sparsecuts above 128 rows (nb = 1):  y | res | sup | Z | workspace of the tridiagonal form | the two selection outputs | MT;
 * Z and MT start at even offsets */
struct hs_scl_layout { long long y; hs_cut_res r; long long Z, ws, o1, o2, MT; hs_cut_lens len; };

/* hipsdp_sparsecuts_all_ex / hipsdp_sparsecuts_ex with a switch set (csrc/sparsecuts_rounds.hip): the layout of hs_sc_layout, and
 * behind its slabs, from `state` on, per served block (hs_scr_block): its hs_scr_state | the start vector of round 0 | Z_S | the
 * slab of the decomposition of Z_S */
struct hs_scr_layout { hs_sc_layout sc; long long state; hs_cut_lens len; };

/* hipsdp_onevar_bounds_all (csrc/onevar.hip):  u[m] | table [count][tabw] | result [count][resw] | Z of every block with jobs | slabs of
 * the 65-128 class (mid_grid workgroups x 2 mid_nmax^2: bounded by the launch grid, whatever the job count).  table, Z and slabs start
 * at even offsets; the pinned mirror holds u, table and result */
struct hs_ova_layout { long long u, tab, res, Z, slabs; hs_cut_lens len; };

/* what a block's loop keeps in the workspace between the launches of two rounds, besides the deflated Z (in place in its slab) */
struct hs_scr_state { double maxeig; int nc, iters, flags, done; };
#define HS_SCR_STATE_LEN 4             /* doubles set aside for it */

/* an n x n matrix in the workspace: n^2 doubles rounded up to an even count */
static inline long long hs_cut_mat_len(int n) { return ((long long) n * n + 1) & ~1LL; }

/* what a served block of n rows has behind `state` (ns: rows of its Z_S, scratch: hs_syev_small_scratch(ns)), as offsets from the
 * block's start, every one even: st | v0[n] | ZS[ns^2] | wsS[scratch]; len: where the next block starts */
struct hs_scr_block { long long st, v0, ZS, wsS, len; };
static inline hs_scr_block hs_scr_block_make(int n, int ns, long long scratch)
{
   hs_scr_block B;
   B.st = 0;
   B.v0 = HS_SCR_STATE_LEN;
   B.ZS = B.v0 + (((long long) n + 1) & ~1LL);
   B.wsS = B.ZS + hs_cut_mat_len(ns);
   B.len = B.wsS + ((scratch + 1) & ~1LL);
   return B;
}

/* vec_len: doubles of all vectors (maxcuts * rows of the blocks that return vectors); slab_len: sum of hs_cut_mat_len(n) +
 * hs_syev_small_scratch(n) over the batched blocks */
void hs_ec_layout_make(int nb, int m, int maxcuts, long long vec_len, long long slab_len, hs_ec_layout* L);
void hs_sc_layout_make(int nb, int m, int maxcuts, int smax, long long vec_len, long long slab_len, hs_sc_layout* L);
/* state_len: sum of hs_scr_block_make(..).len over the served blocks; upload and read-back are those of hs_sc_layout */
void hs_scr_layout_make(int nb, int m, int maxcuts, int smax, long long vec_len, long long slab_len, long long state_len, hs_scr_layout* L);
/* ws_len = hs_syevx_ws(n), out_len = HS_SYEVX_OUT(n), out_vec = HS_SYEVX_OUT_VEC (csrc/syevx.hip), passed in as numbers */
void hs_scl_layout_make(int n, int m, int maxcuts, int smax, long long ws_len, long long out_len, long long out_vec, hs_scl_layout* L);

/* z_len: sum of hs_cut_mat_len(n) over the blocks with jobs; mid_grid = 0: no job of the 65-128 class */
void hs_ova_layout_make(int m, int count, int tabw, int resw, long long z_len, int mid_grid, int mid_nmax, hs_ova_layout* L);

/* hipsdp_onevar_bounds_large (csrc/onevar_large.hip), ONE CHUNK of `count` jobs:
 *    u[m] | table [count][tabw] | job table [count][jobw] | act[count] (int) | nactive (int, one double) | result [count][resw]
 *    | state [count][statew] | Z of the chunk's blocks | per job: workspace of the tridiagonal form, then its selection output
 * every part starts at an even offset.  Uploaded: everything in front of the result; read back after every round: nactive alone, at the
 * end the result; the pinned mirror ends behind the result.  ws[k] / out[k]: where job k's workspace and output start (the caller's
 * arrays of `count` entries); ws_len[k], out_len[k]: hs_syevx_ws(n_k), HS_SXM_OUT(n_k), passed in as numbers */
struct hs_ovl_layout { long long u, tab, jobs, act, nactive, res, state, Z, slabs; hs_cut_lens len; };
void hs_ovl_layout_make(int m, int count, int tabw, int jobw, int resw, int statew, long long z_len, const long long* ws_len,
   const long long* out_len, long long* ws, long long* out, hs_ovl_layout* L);

/* hipsdp_sparsecuts_all_large (csrc/sparsecuts_large_rounds.hip), ONE CHUNK of `count` served blocks of a solver with nb blocks:
 *    y[m] | sizes[nb] (int) | tridiagonal jobs [count][jobw] | block table [count][xjobw] | Z_S jobs [count][sjobw] | act[count] (int)
 *    | res (the arrays of hs_cut_res over nb blocks) | sup | per served block (hs_sclr_block): hs_scr_state | v0[n] | Z | MT | Z_S | the
 *    slab of its decomposition | workspace of the tridiagonal form | its selection output
 * every part starts at an even offset.  The tables stand IN FRONT of the result, so that ONE upload (everything before res) carries y,
 * sizes and the tables, and the pinned mirror ends behind the result's ints (sup and everything behind it is never mirrored). */
struct hs_sclr_layout { long long y, sizes, jobs, xjobs, sjobs, act; hs_cut_res r; long long blocks; hs_cut_lens len; };
/* a served block of n rows, as offsets from the block's start: ns: rows of its Z_S (0: none, the call runs without recomputesparseev),
 * scratch = hs_syev_small_scratch(ns), ws_len = hs_syevx_ws(n), out_len = HS_SXM_OUT(n), passed in as numbers; len: where the next
 * block starts */
struct hs_sclr_block { long long st, v0, Z, MT, ZS, wsS, ws, out, len; };
hs_sclr_block hs_sclr_block_make(int n, int ns, long long scratch, long long ws_len, long long out_len);
/* jobw, xjobw, sjobw: doubles of a row of the three tables; blocks_len: sum of hs_sclr_block_make(..).len over the chunk's blocks */
void hs_sclr_layout_make(int nb, int m, int maxcuts, int smax, long long vec_len, int count, int jobw, int xjobw, int sjobw,
   long long blocks_len, hs_sclr_layout* L);
/* kernel launches of one chunk of hipsdp_sparsecuts_all_large: a function of (variant, maxcuts, nmax) alone, nmax the chunk's largest
 * block - Z(y); stage, nmax - 1 columns and 3 selection launches; with a switch set maxcuts rounds of a TPower launch, with
 * recomputesparseev (s) 3 decomposition launches and the cut, with recomputeinitial or exacttrans (d) the nmax + 3 again; the last
 * TPower launch; the coefficients */
static inline long long hs_sclr_launches(unsigned variant, int maxcuts, int nmax)
{
   const int s = (variant & 1u) ? 1 : 0, d = (variant & 6u) ? 1 : 0;
   const long long rounds = variant != 0 ? maxcuts : 0;       /* (variant 0: the whole loop is the one TPower launch) */
   return 1 + ((long long) nmax + 3) + rounds * (1 + 4 * s + (long long) d * (nmax + 3)) + 1 + (maxcuts > 0 ? 1 : 0);
}

/* hipsdp_eigencuts_all_large (csrc/eigcuts_large.hip), ONE CHUNK of `count` served blocks of a solver with nb blocks:
 *    y[m] | tridiagonal jobs [count][jobw] | vecoff[count] (long long) | act[count] (int)
 *    | res (the arrays of hs_cut_res over nb blocks: lmin, eig, lhs, coef, vec, then the ints ncuts, iters, flags)
 *    | per served block (hs_ecl_block): workspace of the tridiagonal form (its head is the matrix Z(y) is formed into) | its selection
 *    output
 * every part starts at an even offset.  The tables stand in front of the result: ONE upload (everything before res) carries y and the
 * tables, ONE read-back takes res, and the pinned mirror ends behind the result's ints. */
struct hs_ecl_layout { long long y, jobs, vecoff, act; hs_cut_res r; long long blocks; hs_cut_lens len; };
/* a served block, as offsets from the block's start: ws_len = hs_syevx_ws(n), out_len = HS_SXB_OUT(n), passed in as numbers; len: where
 * the next block starts */
struct hs_ecl_block { long long ws, out, len; };
hs_ecl_block hs_ecl_block_make(long long ws_len, long long out_len);
/* jobw: doubles of a row of the job table; vec_len: maxcuts * rows of the chunk's blocks; blocks_len: sum of hs_ecl_block_make(..).len */
void hs_ecl_layout_make(int nb, int m, int maxcuts, long long vec_len, int count, int jobw, long long blocks_len, hs_ecl_layout* L);
/* kernel launches of one chunk of hipsdp_eigencuts_all_large: a function of (maxcuts > 0, nmax) alone, nmax the chunk's largest block -
 * Z(y) and the clearing of the reflector arrays; nmax - 1 columns; the values; with maxcuts > 0 the vectors of the tridiagonal
 * matrices and their back-transformation; the launch that stores counts, lmin and, with maxcuts > 0, the coefficients */
static inline long long hs_ecl_launches(int maxcuts, int nmax)
{
   return 2 + ((long long) nmax - 1) + 1 + (maxcuts > 0 ? 2 : 0) + 1;
}

/* hipsdp_check_y_many (csrc/check_many.hip), ONE CHUNK of cc candidates over nsv served blocks, nlarge of them of 129 .. 512 rows:
 *    Yg [groups][m][group] (groups = ceil(cc / group): the candidates' points, a group's values of one variable side by side)
 *    | block table [nsv][blkw] | tridiagonal jobs [cc nlarge][jobw] | act[cc nlarge] (int)
 *    | res: lmin [cc][nsv], then lpviol [cc]
 *    | lam [cc][nsv - nlarge][2] (eigenvalue and half width of every matrix of at most 128 rows)
 *    | blocks: per served block its cc matrices one behind the other (blocks_len doubles in all: the caller lays them out)
 * every part starts at an even offset.  ONE upload carries everything in front of res, ONE read-back takes res, and the pinned mirror ends
 * behind it. */
struct hs_cm_layout { long long Yg, blks, jobs, act, res, lam, blocks; hs_cut_lens len; };
void hs_cm_layout_make(int m, int cc, int group, int nsv, int nlarge, int blkw, int jobw, long long blocks_len, hs_cm_layout* L);
/* kernel launches of one chunk of hipsdp_check_y_many: a function of the size classes present (blocks of at most 64 rows, of 65 .. 128,
 * of 129 .. 512) and of nmax, the chunk's largest block above 128 rows, alone - Z of all blocks and candidates (with a served block);
 * one launch per class of at most 128 rows; for the third class the clearing of the reflector arrays, nmax - 1 columns and the 3 launches
 * of the selection; the launch that stores lmin and lpviol */
static inline long long hs_cm_launches(int any, int small, int mid, int nmax_large)
{
   return (any ? 1 : 0) + (small ? 1 : 0) + (mid ? 1 : 0) + (nmax_large > 0 ? (long long) nmax_large + 3 : 0) + 1;
}

/* hipsdp_rank1_check_many (csrc/rank1.hip), ONE CHUNK: the parts and the order of hs_cm_layout, with
 *    res: [cc][nsv][resw] (resw = 7: eigenvalues 1, n - 1, n | minorev | minordet | minorind, detind as four ints)
 *    lam: [cc][nsv - nlarge][4] (eigenvalue 1, its half width, eigenvalues n - 1 and n of every matrix of at most 128 rows)
 * ONE upload carries everything in front of res, ONE read-back takes res. */
void hs_r1_layout_make(int m, int cc, int group, int nsv, int nlarge, int blkw, int jobw, int resw, long long blocks_len, hs_cm_layout* L);
/* kernel launches of one chunk of hipsdp_rank1_check_many: a function of the size classes present and of nmax, the chunk's largest block
 * above 128 rows, alone - Z of all blocks and candidates and the minors launch (with a served block); one values launch per class of at
 * most 128 rows; for the third class the clearing of the reflector arrays, nmax - 1 columns and ONE values launch (no vector launches:
 * hs_cm_launches's nmax + 3 becomes nmax + 1); the launch that stores the eigenvalues */
static inline long long hs_r1_launches(int any, int small, int mid, int nmax_large)
{
   return (any ? 3 : 0) + (small ? 1 : 0) + (mid ? 1 : 0) + (nmax_large > 0 ? (long long) nmax_large + 1 : 0);
}

/* hipsdp_rank1_approx (csrc/rank1.hip), ONE CHUNK of cnt asked-for blocks, nsm of them of at most 128 rows, with vec_len = sum n and
 * rhs_len = sum n (n + 1) / 2 over the chunk:
 *    y[m] | result table [cnt][tabw] | decomposition jobs [nsm][ejobw] | tridiagonal jobs [cnt - nsm][jobw] | act[cnt - nsm] (int)
 *    | res: lmax[cnt] | vec[vec_len] | rhs[rhs_len]
 *    | blocks (blocks_len doubles: per block Z and its decomposition slab, or the workspace of the tridiagonal form and its output)
 * every part starts at an even offset.  ONE upload carries everything in front of res, ONE read-back takes res. */
struct hs_r1a_layout { long long y, tab, ejobs, jobs, act, lmax, vec, rhs, blocks; hs_cut_lens len; };
static inline void hs_r1a_layout_make(int m, int cnt, int nsm, int tabw, int ejobw, int jobw, long long vec_len, long long rhs_len,
   long long blocks_len, hs_r1a_layout* L)
{
   const long long nlg = cnt - nsm;
   L->y = 0;
   L->tab = ((long long) m + 1) & ~1LL;
   L->ejobs = L->tab + (((long long) cnt * tabw + 1) & ~1LL);
   L->jobs = L->ejobs + (((long long) nsm * ejobw + 1) & ~1LL);
   L->act = L->jobs + ((nlg * jobw + 1) & ~1LL);
   L->lmax = L->act + ((((nlg + 1) / 2) + 1) & ~1LL);
   L->vec = L->lmax + (((long long) cnt + 1) & ~1LL);
   L->rhs = L->vec + ((vec_len + 1) & ~1LL);
   L->blocks = L->rhs + ((rhs_len + 1) & ~1LL);
   L->len.res_off = L->lmax; L->len.res_len = L->blocks - L->lmax;
   L->len.upload_len = L->lmax; L->len.pin_len = L->blocks; L->len.dev_len = L->blocks + blocks_len;
}
/* kernel launches of one chunk of hipsdp_rank1_approx: a function of the classes present (blocks of at most 128 rows; of 129 .. 512) and
 * of nmax, the chunk's largest block above 128 rows, alone - Z(y); the three launches of the batched full decomposition; for the second
 * class the launch that negates Z and clears the reflector arrays, nmax - 1 columns and the 3 selection launches; the launch that stores
 * lmax, vec and rhs */
static inline long long hs_r1a_launches(int small, int nmax_large)
{
   return 1 + (small ? 3 : 0) + (nmax_large > 0 ? (long long) nmax_large + 3 : 0) + 1;
}

/* the result arrays as pointers into the buffer that starts at base: the device workspace or its pinned mirror */
static inline hs_sc_out hs_cut_view(const hs_cut_res& r, double* base)
{
   hs_sc_out o;
   memset(&o, 0, sizeof(o));
   o.lmin = base + r.lmin; o.eig = base + r.eig; o.lhs = base + r.lhs; o.coef = base + r.coef; o.vec = base + r.vec;
   if ( r.ints >= 0 )
   {
      o.ncuts = reinterpret_cast<int*>(base + r.ints);
      o.iters = o.ncuts + r.nb;
      o.flags = o.iters + r.nb;
      o.sup = reinterpret_cast<int*>(base + r.sup);
   }
   o.smax = r.smax;
   return o;
}

#endif
