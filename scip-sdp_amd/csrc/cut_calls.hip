/* cut_calls.hip - the host side of the calls that serve many blocks, many candidate points or one large block of a loaded solver in a
 * fixed number of launches.  Section by section:
 *   1. what all calls share: CutDst and the copy-out of a block's cuts, block_sums (prefix sums of f(n) over blocks), the tail
 *      chunk_readback (cut_readback: with the view of a cut layout), sxm_job (a matrix of 129 .. 512 rows on the tridiagonal path);
 *   2. the sparse cuts of blocks of at most 128 rows, hipsdp_sparsecuts_all and hipsdp_sparsecuts with their _ex forms (the reference's
 *      refinement switches): sc_begin / scx_rounds / sc_finish (sparsecuts.hip, sparsecuts_rounds.hip), and hipsdp_sparsecuts of one
 *      block of 129 .. 512 rows (sparsecuts_large.hip);
 *   3. the cuts of all blocks of 129 .. 512 rows, hipsdp_sparsecuts_all_large (sparsecuts_large_rounds.hip) and
 *      hipsdp_eigencuts_all_large (eigcuts_large.hip): large_served, the chunk frame large_begin / large_end, sclr_chunk, ecl_chunk;
 *   4. hipsdp_eigencuts_all (eigcuts.hip, the many-forms of the decompositions: eigi.hip) and the extern "C" entries of 2. and 3.;
 *   5. the calls over candidate points, hipsdp_check_y_many (check_many.hip) and, behind 6., hipsdp_rank1_check_many (rank1.hip): the
 *      entry cm_enter, cm_candidate_len, the head of a chunk cm_begin (the caller names the layout), the eigenvalue stage
 *      cm_eigenvalues, the chunks cm_chunk and r1_chunk, the unit entry hs_check_many_form_z;
 *   6. hipsdp_rounding_frame / hipsdp_rounding_recombine, the two device stages of the primal rounding problem: rf_chunk, rf2_chunk
 *      (rounding.hip, psd_many.hip, psd_large.hip; planning: hs_round_plan.h);
 *   7. hipsdp_rank1_approx: r1a_chunk (rank1.hip).
 * Every call is the same choreography: argument checks (before the device is looked at), a layout of the solver's cut workspace
 * (hs_cut_plan.h), ONE upload through its pinned mirror, the launches, ONE read-back of the result range, the copy-out to the caller's
 * arrays; a call that may outgrow the budget does this once per chunk (hs_chunks_run, hs_chunks.h).  A new call uses the shared pieces
 * instead of copying a neighbour: large_begin / large_end for cuts of blocks of 129 .. 512 rows; cm_enter, cm_begin and cm_eigenvalues
 * for candidate points; sxm_job, block_sums and chunk_readback everywhere.  The solver itself is seen through the hs_solver_* functions
 * of hs_kernels.h alone: they enter a call, grow the workspace and keep its job tables on the device (ipm.hip). */
#include "hs_common.h"
#include "hs_kernels.h"
#include "hs_cut_plan.h"
#include "hs_round_plan.h"
#include "hs_chunks.h"
#include "hs_cut_stats.h"
#include "../../include/hipsdp.h"
#include <algorithm>
#include <cstring>
#include <vector>

namespace {

/* hipsdp_eigencuts_all, hipsdp_sparsecuts_all, hipsdp_sparsecuts, the two _ex calls with a switch set, hipsdp_sparsecuts_all_large,
 * hipsdp_eigencuts_all_large, hipsdp_check_y_many */
CutStats g_ec, g_sc, g_sc1, g_scx, g_scl, g_ecl, g_cm;

/* the caller's arrays of a call, or of one block of it (all but ncuts may be NULL) */
struct CutDst
{
   int* ncuts; double *lmin, *eigvals, *coefs, *lhs, *vecs; int *iters, *flags;
   /* those of block b of a call over all blocks, its vectors from voff on */
   CutDst block(int b, int maxcuts, int m, long long voff) const
   {
      const size_t slot = (size_t) b * maxcuts;
      return CutDst{ncuts + b, lmin != NULL ? lmin + b : NULL, eigvals + slot, coefs + slot * m, lhs + slot, vecs != NULL ? vecs + voff : NULL,
         iters != NULL ? iters + b : NULL, flags != NULL ? flags + b : NULL};
   }
};

bool variant_ok(unsigned variant)
{
   return variant <= (HS_SCR_SPARSEEV | HS_SCR_INITIAL | HS_SCR_EXACTTRANS);
}

/* where the vectors of block b start in the result, [nb]: their total length - maxcuts vectors per block, or per block of `members`
 * alone when that is given */
std::vector<long long> cut_vecoff(const hipsdp_solver* s, int nb, int maxcuts, const std::vector<int>* members = NULL)
{
   std::vector<char> in((size_t) nb, members == NULL ? 1 : 0);
   if ( members != NULL )
      for (int b : *members)
         in[b] = 1;
   std::vector<long long> vecoff((size_t) nb + 1, 0);
   for (int b = 0; b < nb; ++b)
      vecoff[b + 1] = vecoff[b] + (in[b] ? (long long) maxcuts * hs_solver_block_n(s, b) : 0);
   return vecoff;
}

/* sum[j] = f(n_0) + .. + f(n_{j-1}), [count]: the total - n_j: the rows of block ids[j] of the solver, of block j with ids == NULL */
template <class F>
std::vector<long long> block_sums(const hipsdp_solver* s, int count, const int* ids, F f)
{
   std::vector<long long> sum((size_t) count + 1, 0);
   for (int j = 0; j < count; ++j)
      sum[j + 1] = sum[j] + f(hs_solver_block_n(s, ids != NULL ? ids[j] : j));
   return sum;
}
long long n_rows(int n) { return n; }
long long n_full(int n) { return (long long) n * n; }
long long n_tri(int n) { return (long long) n * (n + 1) / 2; }

/* Z and the decomposition workspace of every block of a round */
long long ec_slab_len(const hipsdp_solver* s, const std::vector<int>& ids)
{
   long long len = 0;
   for (int b : ids)
      len += hs_cut_mat_len(hs_solver_block_n(s, b)) + hs_syev_small_scratch(hs_solver_block_n(s, b));
   return len;
}

/* the k cuts of one block of n rows - first slot `slot`, vectors from `voff` on - from a host view to the caller's arrays (vecs may be NULL) */
void cut_copy_out(const hs_sc_out& h, size_t slot, long long voff, int k, int m, int n, double* eigvals, double* lhs, double* coefs,
   double* vecs)
{
   if ( k <= 0 )
      return;
   memcpy(eigvals, h.eig + slot, (size_t) k * sizeof(double));
   memcpy(lhs, h.lhs + slot, (size_t) k * sizeof(double));
   if ( m > 0 )
      memcpy(coefs, h.coef + slot * m, (size_t) k * m * sizeof(double));
   if ( vecs != NULL )
      memcpy(vecs, h.vec + voff, (size_t) k * n * sizeof(double));
}

/* block b (n rows, k cuts, vectors from voff on) of a read-back view to the caller's arrays of that block */
int cut_block_out(const hs_sc_out& h, int b, int k, int maxcuts, long long voff, int m, int n, const CutDst& d)
{
   if ( k < 0 || k > maxcuts )
      return HIPSDP_ERR_NUMERIC;
   *d.ncuts = k;
   if ( d.lmin != NULL ) *d.lmin = h.lmin[b];
   if ( d.iters != NULL ) *d.iters = h.iters[b];
   if ( d.flags != NULL ) *d.flags = h.flags[b];
   cut_copy_out(h, (size_t) b * maxcuts, voff, k, m, n, d.eigvals, d.lhs, d.coefs, d.vecs);
   return HIPSDP_OK;
}

/* the tail of every call and chunk: ONE read-back of the result range to the pinned mirror, the launches and the read-back booked */
int chunk_readback(const hs_solver_cut_ws& w, const hs_cut_lens& len, int launches, CutStats* stats)
{
   HS_HIP( hipMemcpyAsync(w.pin + len.res_off, w.dev + len.res_off, (size_t) len.res_len * sizeof(double), hipMemcpyDeviceToHost, w.stream) );
   HS_HIP( hipStreamSynchronize(w.stream) );
   stats->launches += launches;
   stats->readbacks += 1;
   return HS_OK;
}

/* the same where the result range holds the arrays of a cut layout; h: their pinned view */
int cut_readback(const hs_solver_cut_ws& w, const hs_cut_res& r, const hs_cut_lens& len, int launches, CutStats* stats, hs_sc_out* h)
{
   HS_CALL( chunk_readback(w, len, launches, stats) );
   *h = hs_cut_view(r, w.pin);
   return HS_OK;
}

/* The job of a matrix of n rows (129 .. 512) on the batched tridiagonal path and its act word: `make` (hs_syevx_many_job,
 * hs_syevx_many_below_job) fills J from the matrix's workspace and selection output.  The caller has Z formed into the head of the
 * workspace, so that is where the column launches must read their matrix (hs_sxm_job.A). */
int sxm_job(int (*make)(int, double*, double*, hs_sxm_job*), int n, double* ws, double* out, int act, hs_sxm_job* J, int* hact)
{
   HS_CALL( make(n, ws, out, J) );
   if ( J->A != ws )
      return HIPSDP_ERR_NUMERIC;
   *hact = act;
   return HS_OK;
}

void sc_par_from_opts(const hipsdp_sparsecut_opts* opts, hs_sc_par* par)
{
   par->tol = opts->tol; par->feastol = opts->feastol;
   par->convtol = opts->convtol > 0.0 ? opts->convtol : 1e-6;
   par->maxcuts = opts->maxcuts;
   par->maxit = opts->maxit > 0 ? opts->maxit : HIPSDP_SPARSECUTS_MAXIT;
}

/* hs_syev_small_many as THREE launches whatever classes the jobs fall into: a class without jobs gets an empty launch */
int scx_syev(hipStream_t st, int count, const hs_eig_job* hjobs, const hs_eig_job* djobs, int* launches)
{
   int mine = 0;
   HS_CALL( hs_syev_small_many(st, count, hjobs, djobs, &mine) );
   HS_CALL( hs_scr_pad(st, 3 - mine) );
   *launches += 3;
   return HS_OK;
}

/* the tables of the rounds over the blocks `ids`, whose Z_S have ns[j] rows and whose states start at `cur` in the workspace */
int scx_tables(hipsdp_solver* s, const std::vector<int>& ids, const std::vector<int>& ns, double* cur, hs_solver_cut_ws* w)
{
   const int nj = (int) ids.size();
   std::vector<hs_scr_job> xj((size_t) nj);
   std::vector<hs_eig_job> sj;
   for (int j = 0; j < nj; ++j)
   {
      hs_scr_job& X = xj[j];
      memset(&X, 0, sizeof(X));
      const hs_scr_block B = hs_scr_block_make(hs_solver_block_n(s, ids[j]), ns[j], hs_syev_small_scratch(ns[j]));
      X.st = reinterpret_cast<hs_scr_state*>(cur + B.st);
      X.v0 = cur + B.v0;
      X.ZS = cur + B.ZS;
      X.wsS = cur + B.wsS;
      X.vposS = hs_syev_many_vecpos(ns[j]);
      cur += B.len;
   }
   for (int cls = 0; cls < 3; ++cls)
      for (int j = 0; j < nj; ++j)
         if ( hs_syev_many_class(ns[j]) == cls )
         {
            hs_eig_job E;
            memset(&E, 0, sizeof(E));
            E.n = ns[j]; E.in = xj[j].ZS; E.ws = xj[j].wsS;
            sj.push_back(E);
         }
   return hs_solver_cut_rounds(s, xj, sj, w);
}

/* a round of sc_round between its two ends: the workspace, what the launches take, the launches so far */
struct ScRun
{
   hs_solver_cut_ws w;
   hs_cut_res r;                 /* the result arrays: on w.dev what the launches write (out), on w.pin what the copy-out reads */
   hs_cut_lens len;
   hs_sc_out out;
   hs_sc_par par;
   const int* dsizes;
   int nj, nmax, m, maxcuts, launches;
};

/* The head of a round over the served blocks `ids` (ordered by decomposition class; sizes[nb]: the target sparsity of every block of the
 * solver): the layout - with `rounds` that of the refinement rounds, whose two further tables are uploaded as well -, the job tables,
 * y | sizes  in the pinned mirror, the ONE upload, Z(y). */
int sc_begin(hipsdp_solver* s, int m, int nb, const std::vector<int>& ids, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts,
   const std::vector<long long>& vecoff, bool rounds, ScRun* R)
{
   const int maxcuts = opts->maxcuts, nj = (int) ids.size();
   /* the largest support a served block can have: the pitch of the support lists */
   int smax = 1;
   for (int b : ids)
      if ( sizes[b] <= hs_solver_block_n(s, b) && sizes[b] > smax )
         smax = sizes[b];
   hs_scr_layout L;
   std::vector<int> ns;
   if ( !rounds )
   {
      hs_sc_layout_make(nb, m, maxcuts, smax, vecoff[nb], ec_slab_len(s, ids), &L.sc);
      L.len = L.sc.len;
   }
   else
   {
      /* rows of the blocks' Z_S; a block whose size exceeds its rows gets no cut, its job is a matrix of one row */
      ns.resize((size_t) nj);
      long long state_len = 0;
      for (int j = 0; j < nj; ++j)
      {
         const int n = hs_solver_block_n(s, ids[j]);
         ns[j] = sizes[ids[j]] <= n ? sizes[ids[j]] : 1;
         state_len += hs_scr_block_make(n, ns[j], hs_syev_small_scratch(ns[j])).len;
      }
      hs_scr_layout_make(nb, m, maxcuts, smax, vecoff[nb], ec_slab_len(s, ids), state_len, &L);
   }
   HS_CALL( hs_solver_cut_prepare(s, ids, vecoff, L.sc.slabs, L.len, &R->nmax, &R->w) );
   if ( rounds )
      HS_CALL( scx_tables(s, ids, ns, R->w.dev + L.state, &R->w) );
   const hs_solver_cut_ws& w = R->w;
   R->r = L.sc.r; R->len = L.len;
   R->out = hs_cut_view(L.sc.r, w.dev);
   sc_par_from_opts(opts, &R->par);
   R->dsizes = reinterpret_cast<const int*>(w.dev + L.sc.sizes);
   R->nj = nj; R->m = m; R->maxcuts = maxcuts;
   if ( m > 0 )
      memcpy(w.pin + L.sc.y, y, (size_t) m * sizeof(double));
   memcpy(w.pin + L.sc.sizes, sizes, (size_t) nb * sizeof(int));
   HS_HIP( hipMemcpyAsync(w.dev + L.sc.y, w.pin + L.sc.y, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, w.stream) );
   HS_CALL( hs_ec_form_z(w.stream, nj, R->nmax, m, w.djobs, w.dev + L.sc.y) );
   R->launches = 1;
   return HS_OK;
}

/* the tail of a round: with maxcuts > 0 the coefficients, then the ONE read-back; h: its view in the pinned mirror */
int sc_finish(ScRun& R, CutStats* stats, hs_sc_out* h)
{
   const hs_solver_cut_ws& w = R.w;
   if ( R.maxcuts > 0 )
   {
      HS_CALL( hs_sc_coefs(w.stream, R.nj, R.m, R.maxcuts, w.djobs, R.dsizes, &R.out) );
      ++R.launches;
   }
   return cut_readback(w, R.r, R.len, R.launches, stats, h);
}

/* The launches of a round with a switch set (variant: HS_SCR_* bits, != 0) between sc_begin and sc_finish: the decompositions of Z(y),
 * then maxcuts + 1 rounds - a TPower run of every block; with HS_SCR_SPARSEEV the decompositions of the Z_S and the cut behind them,
 * without it the cut inside the TPower launch; with HS_SCR_INITIAL or HS_SCR_EXACTTRANS the decompositions of the deflated Z.  The
 * last round cannot produce a cut (a block that is still running has maxcuts of them), so it is its TPower launch alone.  With s = 1
 * for HS_SCR_SPARSEEV and d = 1 for one of the other two, a call takes 4 + maxcuts (1 + 4 s + 3 d) + 1 launches and one more for the
 * coefficients when maxcuts > 0, whatever the blocks are. */
int scx_rounds(ScRun& R, unsigned variant)
{
   const hs_solver_cut_ws& w = R.w;
   hipStream_t st = w.stream;
   HS_CALL( scx_syev(st, R.nj, w.ejobs, w.dejobs, &R.launches) );
   for (int round = 0; round <= R.maxcuts; ++round)
   {
      HS_CALL( hs_scr_tpower(st, R.nj, R.nmax, w.djobs, w.dxjobs, R.dsizes, &R.par, variant, round, &R.out) );
      ++R.launches;
      if ( round == R.maxcuts )
         break;
      if ( variant & HS_SCR_SPARSEEV )
      {
         HS_CALL( scx_syev(st, R.nj, w.sjobs, w.dsjobs, &R.launches) );
         HS_CALL( hs_scr_cut(st, R.nj, w.djobs, w.dxjobs, R.dsizes, &R.par, &R.out) );
         ++R.launches;
      }
      if ( variant & (HS_SCR_INITIAL | HS_SCR_EXACTTRANS) )
         HS_CALL( scx_syev(st, R.nj, w.ejobs, w.dejobs, &R.launches) );
   }
   return HS_OK;
}

/* The round of the served blocks `ids`: Z(y), the decompositions, TPower - with a switch set the rounds of scx_rounds in their place,
 * booked under g_scx instead of stats0 - and, with maxcuts > 0, the coefficients, all enqueued on the solver's stream and followed by
 * ONE read-back.  The result block is indexed by the block's number whatever `ids` holds, so a round over one block computes that
 * block's bits of the round over all. */
int sc_round(hipsdp_solver* s, int m, int nb, const std::vector<int>& ids, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts,
   unsigned variant, const std::vector<long long>& vecoff, CutStats* stats0, hs_sc_out* h)
{
   ScRun R;
   HS_CALL( sc_begin(s, m, nb, ids, y, sizes, opts, vecoff, variant != 0, &R) );
   if ( variant != 0 )
      HS_CALL( scx_rounds(R, variant) );
   else
   {
      HS_CALL( hs_syev_small_many(R.w.stream, R.nj, R.w.ejobs, R.w.dejobs, &R.launches) );
      HS_CALL( hs_sc_tpower(R.w.stream, R.nj, R.nmax, R.w.djobs, R.dsizes, &R.par, &R.out) );
      ++R.launches;
   }
   return sc_finish(R, variant == 0 ? stats0 : &g_scx, h);
}

/* the argument checks of the sparse-cut calls over all blocks: nothing is written, no device is looked at */
int sc_all_args(const hipsdp_solver* s, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts, const CutDst& d, int* m, int* nb)
{
   if ( !hs_solver_dims(s, m, nb) || y == NULL || sizes == NULL || opts == NULL || d.ncuts == NULL || opts->maxcuts < 0 )
      return HIPSDP_ERR_ARG;
   if ( opts->maxcuts > 0 && (d.eigvals == NULL || d.coefs == NULL || d.lhs == NULL) )
      return HIPSDP_ERR_ARG;
   for (int b = 0; b < *nb; ++b)
      if ( sizes[b] < 1 )
         return HIPSDP_ERR_ARG;
   return HIPSDP_OK;
}

/* hipsdp_sparsecuts_all (variant = 0) and hipsdp_sparsecuts_all_ex with a switch set */
int sparsecuts_all_impl(hipsdp_solver* s, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts, unsigned variant,
   const CutDst& d)
{
   int m = 0, nb = 0;
   HS_CALL( sc_all_args(s, y, sizes, opts, d, &m, &nb) );
   const int maxcuts = opts->maxcuts;
   for (int b = 0; b < nb; ++b)
      d.ncuts[b] = -1;
   std::vector<int> ids;
   HS_CALL( hs_solver_cut_enter(s, -1, &ids) );
   const std::vector<long long> vecoff = cut_vecoff(s, nb, maxcuts);
   if ( !ids.empty() )
   {
      hs_sc_out h;
      HS_CALL( sc_round(s, m, nb, ids, y, sizes, opts, variant, vecoff, &g_sc, &h) );
      for (int b : ids)
         HS_CALL( cut_block_out(h, b, h.ncuts[b], maxcuts, vecoff[b], m, hs_solver_block_n(s, b), d.block(b, maxcuts, m, vecoff[b])) );
   }
   ++(variant == 0 ? g_sc : g_scx).calls;
   return HIPSDP_OK;
}

/* a block of at most 128 rows: the round of hipsdp_sparsecuts_all with this block as the only job, the same bits */
int sparsecuts_small(hipsdp_solver* s, int m, int nb, int block, const double* y, int size, const hipsdp_sparsecut_opts* opts, unsigned variant,
   const CutDst& d, int* served)
{
   std::vector<int> ids;
   HS_CALL( hs_solver_cut_enter(s, block, &ids) );
   *served = !ids.empty();
   if ( !*served )
      return HIPSDP_OK;
   const int maxcuts = opts->maxcuts;
   const std::vector<long long> vecoff = cut_vecoff(s, nb, maxcuts, &ids);       /* only this block has vectors */
   std::vector<int> sizes((size_t) nb, 1);
   sizes[block] = size;
   hs_sc_out h;
   HS_CALL( sc_round(s, m, nb, ids, y, sizes.data(), opts, variant, vecoff, &g_sc1, &h) );
   return cut_block_out(h, block, h.ncuts[block], maxcuts, vecoff[block], m, hs_solver_block_n(s, block), d);
}

/* a block of 129 .. 512 rows: Z(y), ONE tridiagonalisation, (lmin, v0) and maxeig from it, TPower in one workgroup, coefficients -
 * n + 7 launches (n + 2 with maxcuts == 0) and one read-back.  The workspace is that of the calls above: it only grows. */
int sparsecuts_large(hipsdp_solver* s, int m, int block, const double* y, int size, const hipsdp_sparsecut_opts* opts, const CutDst& d,
   int* served)
{
   const int maxcuts = opts->maxcuts, n = hs_solver_block_n(s, block);
   hs_scl_layout L;
   hs_scl_layout_make(n, m, maxcuts, size <= n ? size : 1, (long long) hs_syevx_ws(n), HS_SYEVX_OUT(n), HS_SYEVX_OUT_VEC, &L);
   hs_solver_cut_ws w;
   HS_CALL( hs_solver_cut_job(s, block, L.len.dev_len, L.len.pin_len, L.Z, L.ws, &w, served) );
   if ( !*served )
      return HIPSDP_OK;
   hipStream_t st = w.stream;
   double *dy = w.dev + L.y, *dZ = w.dev + L.Z, *dws = w.dev + L.ws, *o1 = w.dev + L.o1, *o2 = w.dev + L.o2;
   const hs_sc_out out = hs_cut_view(L.r, w.dev);
   hs_sc_par par;
   sc_par_from_opts(opts, &par);
   int launches = 0;
   if ( m > 0 )
   {
      memcpy(w.pin + L.y, y, (size_t) m * sizeof(double));
      HS_HIP( hipMemcpyAsync(dy, w.pin + L.y, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );
   }
   HS_CALL( hs_ec_form_z(st, 1, n, m, w.djobs, dy) );
   ++launches;
   HS_CALL( hs_syevx_tridiag_dev(st, n, dZ, dws) );
   launches += n;
   if ( maxcuts == 0 )
   {
      /* no result block: the one read-back is the head of the request's output (its eigenvalue), to where the result would lie */
      double* hres = w.pin + L.len.res_off;
      HS_CALL( hs_syevx_select_dev(st, n, HS_SYEVX_INDEX | HS_SYEVX_NOVEC, 1, 1, 0.0, 0, o1, dws) );
      ++launches;
      HS_HIP( hipMemcpyAsync(hres, o1, (size_t) HS_SYEVX_OUT_VEC * sizeof(double), hipMemcpyDeviceToHost, st) );
      HS_HIP( hipStreamSynchronize(st) );
      g_sc1.launches += launches;
      g_sc1.readbacks += 1;
      *d.ncuts = 0;
      if ( d.lmin != NULL ) *d.lmin = hres[HS_SYEVX_OUT_LAM];
      if ( d.iters != NULL ) *d.iters = 0;
      if ( d.flags != NULL ) *d.flags = 0;
      return HIPSDP_OK;
   }
   HS_CALL( hs_syevx_select_dev(st, n, HS_SYEVX_INDEX, 1, 1, 0.0, 0, o1, dws) );
   HS_CALL( hs_syevx_select_dev(st, n, HS_SYEVX_INDEX | HS_SYEVX_NOVEC, n, n, 0.0, 0, o2, dws) );
   HS_CALL( hs_scl_tpower(st, n, size, dZ, o1 + HS_SYEVX_OUT_LAM, o2 + HS_SYEVX_OUT_LAM, o1 + HS_SYEVX_OUT_VEC, w.dev + L.MT, &par, &out) );
   HS_CALL( hs_scl_coefs(st, m, maxcuts, size, w.djobs, &out) );
   launches += 3 + 1 + 1 + 1;
   hs_sc_out h;
   HS_CALL( cut_readback(w, L.r, L.len, launches, &g_sc1, &h) );
   return cut_block_out(h, 0, h.ncuts[0], maxcuts, 0, m, n, d);
}

/* ---- hipsdp_sparsecuts_all_large: all blocks of 129 .. 512 rows per launch, switches included (kernels: sparsecuts_large_rounds.hip) ---- */
static_assert(sizeof(hs_sxm_job) == 6 * sizeof(double), "hs_sclr_layout: jobw");
static_assert(sizeof(hs_sclr_job) == 7 * sizeof(double), "hs_sclr_layout: xjobw");
static_assert(sizeof(hs_eig_job) == 3 * sizeof(double), "hs_sclr_layout: sjobw");
#define SCLR_JOBW 6
#define SCLR_XJOBW 7
#define SCLR_SJOBW 3
#define SCLR_BUDGET (512LL * 1024 * 1024 / (long long) sizeof(double))    /* doubles of block workspace per chunk */

/* what a served block of n rows takes of the chunk's workspace (ns: rows of its Z_S, 0 without recomputesparseev) */
hs_sclr_block sclr_block(int n, int ns)
{
   return hs_sclr_block_make(n, ns, ns > 0 ? hs_syev_small_scratch(ns) : 0, (long long) hs_syevx_ws(n), HS_SXM_OUT(n));
}

/* the blocks a _large cut call serves: whole matrices on this device (none for a solver with a communicator or sharded matrices) of
 * HS_SC_MAXN + 1 .. maxn rows that pass `keep`, by descending n, the caller's order among equal sizes */
template <class Keep>
int large_served(hipsdp_solver* s, int maxn, Keep keep, std::vector<int>* ids)
{
   std::vector<int> all;
   HS_CALL( hs_solver_cut_enter_large(s, maxn, &all) );
   ids->clear();
   for (int b : all)
      if ( hs_solver_block_n(s, b) > HS_SC_MAXN && keep(b) )
         ids->push_back(b);
   std::stable_sort(ids->begin(), ids->end(), [&](int a, int c) { return hs_solver_block_n(s, a) > hs_solver_block_n(s, c); });
   return HS_OK;
}

/* a chunk of a _large cut call between its two ends, as ScRun is a round's: the workspace, the chunk's own result (indexed by the
 * block's number, vectors of the chunk's blocks alone), where every block's part of the workspace starts, the launches so far */
struct LargeRun
{
   hs_solver_cut_ws w;
   hs_cut_res r;
   hs_cut_lens len;
   std::vector<long long> vecoff;      /* [nb + 1] */
   std::vector<long long> start;       /* [cnt]: doubles from the device workspace's start */
   int nmax, launches;
};

/* The head of the chunk over the served blocks `ids` (descending n) of a solver with nb blocks.  len_of(j): what block j takes of the
 * workspace; make(vec_len, blocks_len, L): the call's layout (hs_sclr_layout, hs_ecl_layout: y, r, blocks and len are read from it);
 * z_of(j): where Z(y) of block j goes inside its part.  Leaves the workspace with the solver's table of the blocks (w.djobs) and y in
 * the pinned mirror; the call's tables and the ONE upload of [0, upload_len) are the caller's. */
template <class Layout, class LenOf, class Make, class ZOf>
int large_begin(hipsdp_solver* s, int m, int nb, const std::vector<int>& ids, const double* y, int maxcuts, LenOf len_of, Make make, ZOf z_of,
   Layout* L, LargeRun* R)
{
   const int cnt = (int) ids.size();
   R->nmax = 0; R->launches = 0;
   R->vecoff = cut_vecoff(s, nb, maxcuts, &ids);
   R->start.resize((size_t) cnt);
   long long blocks_len = 0;
   for (int j = 0; j < cnt; ++j)
   {
      const int n = hs_solver_block_n(s, ids[j]);
      R->nmax = n > R->nmax ? n : R->nmax;
      R->start[j] = blocks_len;
      blocks_len += len_of(j);
   }
   make(R->vecoff[nb], blocks_len, L);
   std::vector<long long> zoff((size_t) cnt);
   for (int j = 0; j < cnt; ++j)
   {
      R->start[j] += L->blocks;
      zoff[j] = R->start[j] + z_of(j);
   }
   HS_CALL( hs_solver_cut_blocks(s, ids, zoff, L->len.dev_len, L->len.pin_len, &R->w) );
   R->r = L->r; R->len = L->len;
   if ( m > 0 )
      memcpy(R->w.pin + L->y, y, (size_t) m * sizeof(double));
   return HS_OK;
}

/* The tail of the chunk: ONE read-back, its launches booked under `stats`, every block of the chunk to the caller's arrays.  gvecoff:
 * where a block's vectors start in the caller's array. */
int large_end(const hipsdp_solver* s, const LargeRun& R, int m, const std::vector<int>& ids, int maxcuts, CutStats* stats, const CutDst& d,
   const std::vector<long long>& gvecoff)
{
   hs_sc_out h;
   HS_CALL( cut_readback(R.w, R.r, R.len, R.launches, stats, &h) );
   for (int b : ids)
      HS_CALL( cut_block_out(h, b, h.ncuts[b], maxcuts, R.vecoff[b], m, hs_solver_block_n(s, b), d.block(b, maxcuts, m, gvecoff[b])) );
   return HIPSDP_OK;
}

/* ONE CHUNK: the served blocks `ids` (descending n) of a solver with nb blocks - a call of its own in everything but the entry: its
 * layout of the workspace (hs_sclr_layout), ONE upload of  y | sizes | the three tables | act,  the launches - hs_sclr_launches(variant,
 * maxcuts, nmax) of them, whatever the blocks do -, ONE read-back, the copy-out.  gvecoff: where a block's vectors start in the caller's
 * array. */
int sclr_chunk(hipsdp_solver* s, int m, int nb, const std::vector<int>& ids, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts,
   unsigned variant, const CutDst& d, const std::vector<long long>& gvecoff)
{
   const int cnt = (int) ids.size(), maxcuts = opts->maxcuts;
   const bool sparseev = (variant & HS_SCR_SPARSEEV) != 0, deflated = (variant & (HS_SCR_INITIAL | HS_SCR_EXACTTRANS)) != 0;
   int smax = 1;
   std::vector<hs_sclr_block> B((size_t) cnt);
   std::vector<int> ns((size_t) cnt);
   for (int j = 0; j < cnt; ++j)
   {
      const int n = hs_solver_block_n(s, ids[j]), size = sizes[ids[j]];
      if ( size <= n && size > smax )
         smax = size;
      ns[j] = sparseev ? size : 0;
      B[j] = sclr_block(n, ns[j]);
   }
   hs_sclr_layout L;
   LargeRun R;
   HS_CALL( large_begin(s, m, nb, ids, y, maxcuts, [&](int j) { return B[j].len; },
         [&](long long vec_len, long long blocks_len, hs_sclr_layout* l)
         { hs_sclr_layout_make(nb, m, maxcuts, smax, vec_len, cnt, SCLR_JOBW, SCLR_XJOBW, SCLR_SJOBW, blocks_len, l); },
         [&](int j) { return B[j].Z; }, &L, &R) );
   const hs_solver_cut_ws& w = R.w;
   hipStream_t st = w.stream;
   const int nmax = R.nmax;
   int& launches = R.launches;
   /* sizes | tables | act  behind y in the pinned mirror */
   memcpy(w.pin + L.sizes, sizes, (size_t) nb * sizeof(int));
   hs_sxm_job* hsx = reinterpret_cast<hs_sxm_job*>(w.pin + L.jobs);
   hs_sclr_job* hx = reinterpret_cast<hs_sclr_job*>(w.pin + L.xjobs);
   int* hact = reinterpret_cast<int*>(w.pin + L.act);
   std::vector<hs_eig_job> sj;               /* the Z_S jobs by decomposition class: the host copy hs_syev_small_many wants */
   for (int j = 0; j < cnt; ++j)
   {
      double* base = w.dev + R.start[j];
      HS_CALL( hs_syevx_many_job(hs_solver_block_n(s, ids[j]), base + B[j].ws, base + B[j].out, &hsx[j]) );
      hs_sclr_job& X = hx[j];
      memset(&X, 0, sizeof(X));
      X.st = reinterpret_cast<hs_scr_state*>(base + B[j].st);
      X.v0 = base + B[j].v0;
      X.MT = base + B[j].MT;
      if ( ns[j] > 0 )
      {
         X.ZS = base + B[j].ZS;
         X.wsS = base + B[j].wsS;
         X.vposS = hs_syev_many_vecpos(ns[j]);
      }
      X.vecoff = R.vecoff[ids[j]];
      hact[j] = HS_SXM_ACTIVE | HS_SXM_VEC | HS_SXM_BOTH;
   }
   for (int cls = 0; cls < 3 && sparseev; ++cls)
      for (int j = 0; j < cnt; ++j)
         if ( hs_syev_many_class(ns[j]) == cls )
         {
            hs_eig_job E;
            memset(&E, 0, sizeof(E));
            E.n = ns[j]; E.in = hx[j].ZS; E.ws = hx[j].wsS;
            sj.push_back(E);
         }
   if ( !sj.empty() )
      memcpy(w.pin + L.sjobs, sj.data(), sj.size() * sizeof(hs_eig_job));
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );

   const hs_sxm_job* dsx = reinterpret_cast<const hs_sxm_job*>(w.dev + L.jobs);
   const hs_sclr_job* dx = reinterpret_cast<const hs_sclr_job*>(w.dev + L.xjobs);
   const hs_eig_job* dsj = reinterpret_cast<const hs_eig_job*>(w.dev + L.sjobs);
   int* dact = reinterpret_cast<int*>(w.dev + L.act);
   const int* dsizes = reinterpret_cast<const int*>(w.dev + L.sizes);
   const hs_sc_out out = hs_cut_view(L.r, w.dev);
   hs_sc_par par;
   sc_par_from_opts(opts, &par);
   const int cap = hs_syevx_many_cap(cnt);
   HS_CALL( hs_ec_form_z(st, cnt, nmax, m, w.djobs, w.dev + L.y) );
   ++launches;
   /* (lmin, v0) and maxeig of Z(y) of every block: stage, nmax - 1 column launches, 3 selection launches */
   HS_CALL( hs_sclr_stage(st, cnt, w.djobs, dsx, dx, dsizes, dact, sparseev ? 1 : 0) );
   HS_CALL( hs_syevx_many_cols(st, cnt, nmax, cap, dsx, dact) );
   HS_CALL( hs_syevx_many_select(st, cnt, nmax, 1, dsx, dact) );
   launches += nmax + 3;
   if ( variant == 0 )
   {
      HS_CALL( hs_sclr_tpower_all(st, cnt, m, w.djobs, dsx, dx, dsizes, &par, &out) );
      ++launches;
   }
   else
   {
      /* what the tridiagonalisations of the deflated Z have to give a block that goes on */
      const int act_on = HS_SXM_ACTIVE | ((variant & HS_SCR_INITIAL) ? HS_SXM_VEC : 0) | ((variant & HS_SCR_EXACTTRANS) ? HS_SXM_BOTH : 0);
      for (int round = 0; round <= maxcuts; ++round)
      {
         HS_CALL( hs_sclr_tpower(st, cnt, m, w.djobs, dsx, dx, dsizes, &par, variant, round, act_on, dact, &out) );
         ++launches;
         if ( round == maxcuts )             /* (a block that is still running has maxcuts cuts: this run cannot produce one) */
            break;
         if ( sparseev )
         {
            HS_CALL( scx_syev(st, cnt, sj.data(), dsj, &launches) );
            HS_CALL( hs_sclr_cut(st, cnt, m, w.djobs, dx, dsizes, &par, dact, &out) );
            ++launches;
         }
         if ( deflated )
         {
            HS_CALL( hs_sclr_stage(st, cnt, w.djobs, dsx, dx, dsizes, dact, 0) );
            HS_CALL( hs_syevx_many_cols(st, cnt, nmax, cap, dsx, dact) );
            HS_CALL( hs_syevx_many_select(st, cnt, nmax, (variant & HS_SCR_EXACTTRANS) ? 1 : 0, dsx, dact) );
            launches += nmax + 3;
         }
      }
   }
   if ( maxcuts > 0 )
   {
      HS_CALL( hs_sclr_coefs(st, cnt, m, maxcuts, w.djobs, dx, dsizes, &out) );
      ++launches;
   }
   return large_end(s, R, m, ids, maxcuts, &g_scl, d, gvecoff);
}

int sparsecuts_all_large_impl(hipsdp_solver* s, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts, unsigned variant,
   const CutDst& d)
{
   int m = 0, nb = 0;
   HS_CALL( sc_all_args(s, y, sizes, opts, d, &m, &nb) );
   const int maxcuts = opts->maxcuts;
   for (int b = 0; b < nb; ++b)
      d.ncuts[b] = -1;
   /* the blocks this call serves: 129 .. 512 rows, and with recomputesparseev a target size the decomposition of Z_S takes */
   const bool sparseev = (variant & HS_SCR_SPARSEEV) != 0;
   std::vector<int> ids;
   HS_CALL( large_served(s, HIPSDP_SPARSECUTS_MAXN, [&](int b) { return !(sparseev && sizes[b] > HS_SC_MAXN); }, &ids) );
   if ( ids.empty() )
      return HIPSDP_OK;
   const int total = (int) ids.size();
   std::vector<long long> job_len((size_t) total);
   for (int k = 0; k < total; ++k)
      job_len[k] = sclr_block(hs_solver_block_n(s, ids[k]), sparseev ? sizes[ids[k]] : 0).len;
   const std::vector<long long> gvecoff = cut_vecoff(s, nb, maxcuts);
   HS_CALL( hs_chunks_run(job_len.data(), total, SCLR_BUDGET, hs_chunk_env("HIPSDP_SPARSECUTS_LARGE_CHUNK"), [&](int start, int end)
      {
         const std::vector<int> chunk(ids.begin() + start, ids.begin() + end);
         return sclr_chunk(s, m, nb, chunk, y, sizes, opts, variant, d, gvecoff);
      }) );
   ++g_scl.calls;
   return HIPSDP_OK;
}

/* hipsdp_sparsecuts (variant = 0, booked under g_sc1) and hipsdp_sparsecuts_ex with a switch set: blocks of at most 128 rows */
int sparsecuts_impl(hipsdp_solver* s, int block, const double* y, int size, const hipsdp_sparsecut_opts* opts, unsigned variant, const CutDst& d)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || block < 0 || block >= nb || y == NULL || opts == NULL || d.ncuts == NULL || size < 1
      || opts->maxcuts < 0 )
      return HIPSDP_ERR_ARG;
   if ( opts->maxcuts > 0 && (d.eigvals == NULL || d.coefs == NULL || d.lhs == NULL) )
      return HIPSDP_ERR_ARG;
   const int n = hs_solver_block_n(s, block);
   *d.ncuts = -1;
   if ( n > (variant == 0 ? HIPSDP_SPARSECUTS_MAXN : HS_SC_MAXN) )
      return HIPSDP_OK;
   /* not served (nothing else done): a solver with a communicator or sharded matrices, a block without matrices on this device */
   int served = 0;
   if ( n <= HS_SC_MAXN )
      HS_CALL( sparsecuts_small(s, m, nb, block, y, size, opts, variant, d, &served) );
   else
      HS_CALL( sparsecuts_large(s, m, block, y, size, opts, d, &served) );
   if ( served )
      ++(variant == 0 ? g_sc1 : g_scx).calls;
   return HIPSDP_OK;
}

/* ---- hipsdp_eigencuts_all_large: the dense cuts of all blocks of 129 .. 512 rows per launch (kernels: eigcuts_large.hip, syevx.hip) ---- */
hs_ecl_block ecl_block(int n)
{
   return hs_ecl_block_make((long long) hs_syevx_ws(n), HS_SXB_OUT(n));
}

/* ONE CHUNK: the served blocks `ids` (descending n) of a solver with nb blocks - its layout of the workspace (hs_ecl_layout), ONE upload
 * of  y | the table | vecoff | act,  hs_ecl_launches(maxcuts, nmax) launches whatever the blocks and their counts are, ONE read-back, the
 * copy-out.  gvecoff: where a block's vectors start in the caller's array. */
int ecl_chunk(hipsdp_solver* s, int m, int nb, const std::vector<int>& ids, const double* y, double tol, int maxcuts, const CutDst& d,
   const std::vector<long long>& gvecoff)
{
   const int cnt = (int) ids.size();
   std::vector<hs_ecl_block> B((size_t) cnt);
   for (int j = 0; j < cnt; ++j)
      B[j] = ecl_block(hs_solver_block_n(s, ids[j]));
   /* Z(y) of a block goes where the column launches read their matrix: the head of the block's workspace (hs_sxm_job.A) */
   hs_ecl_layout L;
   LargeRun R;
   HS_CALL( large_begin(s, m, nb, ids, y, maxcuts, [&](int j) { return B[j].len; },
         [&](long long vec_len, long long blocks_len, hs_ecl_layout* l) { hs_ecl_layout_make(nb, m, maxcuts, vec_len, cnt, SCLR_JOBW, blocks_len, l); },
         [&](int j) { return B[j].ws; }, &L, &R) );
   const hs_solver_cut_ws& w = R.w;
   const int nmax = R.nmax;
   int& launches = R.launches;
   hipStream_t st = w.stream;
   hs_sxm_job* hsx = reinterpret_cast<hs_sxm_job*>(w.pin + L.jobs);
   long long* hvo = reinterpret_cast<long long*>(w.pin + L.vecoff);
   int* hact = reinterpret_cast<int*>(w.pin + L.act);
   for (int j = 0; j < cnt; ++j)
   {
      double* base = w.dev + R.start[j];
      HS_CALL( sxm_job(hs_syevx_many_below_job, hs_solver_block_n(s, ids[j]), base + B[j].ws, base + B[j].out, HS_SXM_ACTIVE, &hsx[j], &hact[j]) );
      hvo[j] = R.vecoff[ids[j]];
   }
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );

   const hs_sxm_job* dsx = reinterpret_cast<const hs_sxm_job*>(w.dev + L.jobs);
   const long long* dvo = reinterpret_cast<const long long*>(w.dev + L.vecoff);
   const int* dact = reinterpret_cast<const int*>(w.dev + L.act);
   const hs_sc_out out = hs_cut_view(L.r, w.dev);
   HS_CALL( hs_ec_form_z(st, cnt, nmax, m, w.djobs, w.dev + L.y) );
   HS_CALL( hs_ecl_clear(st, cnt, dsx) );
   launches += 2;
   HS_CALL( hs_syevx_many_cols(st, cnt, nmax, hs_syevx_many_cap(cnt), dsx, dact) );
   launches += nmax - 1;
   /* eigenvalue <= -tol, most negative first, at most maxcuts: the count of the selection is the number of cuts */
   HS_CALL( hs_syevx_many_below(st, cnt, nmax, -tol, maxcuts, dsx, dact) );
   launches += maxcuts > 0 ? 3 : 1;
   HS_CALL( hs_ecl_cuts(st, cnt, nmax, m, maxcuts, w.djobs, dsx, dvo, &out) );
   ++launches;
   return large_end(s, R, m, ids, maxcuts, &g_ecl, d, gvecoff);
}

int eigencuts_all_large_impl(hipsdp_solver* s, const double* y, double tol, int maxcuts, const CutDst& d)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || y == NULL || d.ncuts == NULL || maxcuts < 0 || maxcuts > HIPSDP_EIGENCUTS_LARGE_MAXCUTS )
      return HIPSDP_ERR_ARG;
   if ( maxcuts > 0 && (d.eigvals == NULL || d.coefs == NULL || d.lhs == NULL) )
      return HIPSDP_ERR_ARG;
   for (int b = 0; b < nb; ++b)
      d.ncuts[b] = -1;
   /* the blocks this call serves: 129 .. 512 rows */
   std::vector<int> ids;
   HS_CALL( large_served(s, HIPSDP_EIGENCUTS_LARGE_MAXN, [](int) { return true; }, &ids) );
   if ( ids.empty() )
      return HIPSDP_OK;
   const int total = (int) ids.size();
   std::vector<long long> job_len((size_t) total);
   for (int k = 0; k < total; ++k)
      job_len[k] = ecl_block(hs_solver_block_n(s, ids[k])).len;
   const std::vector<long long> gvecoff = cut_vecoff(s, nb, maxcuts);
   HS_CALL( hs_chunks_run(job_len.data(), total, SCLR_BUDGET, hs_chunk_env("HIPSDP_EIGENCUTS_LARGE_CHUNK"), [&](int start, int end)
      {
         const std::vector<int> chunk(ids.begin() + start, ids.begin() + end);
         return ecl_chunk(s, m, nb, chunk, y, tol, maxcuts, d, gvecoff);
      }) );
   ++g_ecl.calls;
   return HIPSDP_OK;
}

}

extern "C" int hipsdp_eigencuts_all_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_ec.get(calls, launches, readbacks);
}

extern "C" int hipsdp_sparsecuts_all_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_sc.get(calls, launches, readbacks);
}

extern "C" int hipsdp_sparsecuts_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_sc1.get(calls, launches, readbacks);
}

extern "C" int hipsdp_sparsecuts_ex_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_scx.get(calls, launches, readbacks);
}

extern "C" int hipsdp_sparsecuts_all_large_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_scl.get(calls, launches, readbacks);
}

extern "C" int hipsdp_eigencuts_all_large_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_ecl.get(calls, launches, readbacks);
}

extern "C" int hipsdp_eigencuts_all(hipsdp_solver* s, const double* y, double tol, int maxcuts, int* ncuts, double* lmin, double* eigvals,
   double* coefs, double* lhs, double* vecs)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || y == NULL || ncuts == NULL || maxcuts < 0 )
      return HIPSDP_ERR_ARG;
   if ( maxcuts > 0 && (eigvals == NULL || coefs == NULL || lhs == NULL) )
      return HIPSDP_ERR_ARG;
   for (int b = 0; b < nb; ++b)
      ncuts[b] = 0;
   std::vector<int> ids;
   HS_CALL( hs_solver_cut_enter(s, -1, &ids) );
   const CutDst dst = {ncuts, lmin, eigvals, coefs, lhs, vecs, NULL, NULL};
   const std::vector<long long> vecoff = cut_vecoff(s, nb, maxcuts);
   const int nj = (int) ids.size();
   std::vector<char> served((size_t) nb, 0);
   if ( nj > 0 )
   {
      hs_ec_layout L;
      hs_ec_layout_make(nb, m, maxcuts, vecoff[nb], ec_slab_len(s, ids), &L);
      int nmax = 0;
      hs_solver_cut_ws w;
      HS_CALL( hs_solver_cut_prepare(s, ids, vecoff, L.slabs, L.len, &nmax, &w) );
      hipStream_t st = w.stream;
      double* dy = w.dev + L.y;
      int launches = 0;
      if ( m > 0 )
      {
         memcpy(w.pin + L.y, y, (size_t) m * sizeof(double));
         HS_HIP( hipMemcpyAsync(dy, w.pin + L.y, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );
      }
      HS_CALL( hs_ec_form_z(st, nj, nmax, m, w.djobs, dy) );
      ++launches;
      HS_CALL( hs_syev_small_many(st, nj, w.ejobs, w.dejobs, &launches) );
      HS_CALL( hs_ec_cuts(st, nj, nmax, m, nb, maxcuts, tol, w.djobs, w.dev + L.len.res_off) );
      ++launches;
      hs_sc_out h;
      HS_CALL( cut_readback(w, L.r, L.len, launches, &g_ec, &h) );
      for (int b : ids)
      {
         const int k = (int) w.pin[L.ncuts + b], n = hs_solver_block_n(s, b);
         if ( k > n )
            return HIPSDP_ERR_NUMERIC;
         HS_CALL( cut_block_out(h, b, k, maxcuts, vecoff[b], m, n, dst.block(b, maxcuts, m, vecoff[b])) );
         served[b] = 1;
      }
   }
   /* every other block: the per-block path, inside the same call */
   for (int b = 0; b < nb; ++b)
   {
      if ( served[b] )
         continue;
      const CutDst d = dst.block(b, maxcuts, m, vecoff[b]);
      double l0 = 0.0;
      HS_CALL( hs_solver_eigencuts_block(s, b, y, tol, maxcuts, d.ncuts, maxcuts > 0 ? d.eigvals : NULL, maxcuts > 0 ? d.coefs : NULL,
            maxcuts > 0 ? d.lhs : NULL, d.vecs, &l0) );
      if ( d.lmin != NULL )
         *d.lmin = l0;
   }
   ++g_ec.calls;
   return HIPSDP_OK;
}

extern "C" int hipsdp_sparsecuts_all(hipsdp_solver* s, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts, int* ncuts,
   double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags)
{
   return sparsecuts_all_impl(s, y, sizes, opts, 0, CutDst{ncuts, lmin, eigvals, coefs, lhs, vecs, iters, flags});
}

extern "C" int hipsdp_sparsecuts_all_ex(hipsdp_solver* s, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts, unsigned variant,
   int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags)
{
   if ( !variant_ok(variant) )
      return HIPSDP_ERR_ARG;
   return sparsecuts_all_impl(s, y, sizes, opts, variant, CutDst{ncuts, lmin, eigvals, coefs, lhs, vecs, iters, flags});
}

extern "C" int hipsdp_sparsecuts(hipsdp_solver* s, int block, const double* y, int size, const hipsdp_sparsecut_opts* opts, int* ncuts,
   double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags)
{
   return sparsecuts_impl(s, block, y, size, opts, 0, CutDst{ncuts, lmin, eigvals, coefs, lhs, vecs, iters, flags});
}

extern "C" int hipsdp_sparsecuts_ex(hipsdp_solver* s, int block, const double* y, int size, const hipsdp_sparsecut_opts* opts, unsigned variant,
   int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags)
{
   if ( !variant_ok(variant) )
      return HIPSDP_ERR_ARG;
   return sparsecuts_impl(s, block, y, size, opts, variant, CutDst{ncuts, lmin, eigvals, coefs, lhs, vecs, iters, flags});
}

extern "C" int hipsdp_sparsecuts_all_large(hipsdp_solver* s, const double* y, const int* sizes, const hipsdp_sparsecut_opts* opts,
   unsigned variant, int* ncuts, double* lmin, double* eigvals, double* coefs, double* lhs, double* vecs, int* iters, int* flags)
{
   if ( !variant_ok(variant) )
      return HIPSDP_ERR_ARG;
   return sparsecuts_all_large_impl(s, y, sizes, opts, variant, CutDst{ncuts, lmin, eigvals, coefs, lhs, vecs, iters, flags});
}

extern "C" int hipsdp_eigencuts_all_large(hipsdp_solver* s, const double* y, double tol, int maxcuts, int* ncuts, double* lmin, double* eigvals,
   double* coefs, double* lhs, double* vecs)
{
   return eigencuts_all_large_impl(s, y, tol, maxcuts, CutDst{ncuts, lmin, eigvals, coefs, lhs, vecs, NULL, NULL});
}

namespace {

/* ---- hipsdp_check_y_many: the feasibility check of many candidate points (kernels: check_many.hip, eigi.hip, syevx.hip) ---------------- */
static_assert(sizeof(hs_cm_blk) == 4 * sizeof(double), "hs_cm_layout: blkw");
#define CM_BLKW 4

/* the blocks the call serves, in the order of its tables: at most 64 rows, 65 .. 128 rows, 129 .. 512 rows by descending n, the caller's
 * order inside a class and among equal sizes; nmax_*: the largest block of a class (0: none), nmax: of all */
struct CmBlocks
{
   std::vector<int> ids;
   int nsmall, nmid, nlarge, nmax_small, nmax_mid, nmax_large, nmax;
};

int cm_class(int n) { return n <= 64 ? 0 : (n <= HS_SC_MAXN ? 1 : 2); }

int cm_served(hipsdp_solver* s, CmBlocks* P)
{
   std::vector<int> all;
   HS_CALL( hs_solver_cut_enter_large(s, HS_SYEVX_MAXN, &all) );
   P->ids.clear();
   P->nsmall = P->nmid = P->nlarge = P->nmax_small = P->nmax_mid = P->nmax_large = 0;
   for (int cls = 0; cls < 3; ++cls)
      for (int b : all)
      {
         const int n = hs_solver_block_n(s, b);
         if ( cm_class(n) != cls )
            continue;
         P->ids.push_back(b);
         int& cnt = cls == 0 ? P->nsmall : (cls == 1 ? P->nmid : P->nlarge);
         int& top = cls == 0 ? P->nmax_small : (cls == 1 ? P->nmax_mid : P->nmax_large);
         ++cnt;
         top = n > top ? n : top;
      }
   std::stable_sort(P->ids.begin() + P->nsmall + P->nmid, P->ids.end(),
      [&](int a, int c) { return hs_solver_block_n(s, a) > hs_solver_block_n(s, c); });
   P->nmax = std::max(P->nmax_small, std::max(P->nmax_mid, P->nmax_large));
   return HS_OK;
}

/* what a matrix of n rows takes of a chunk's workspace: Z alone up to 128 rows, above that the workspace of the tridiagonal form (Z is
 * formed into its head) and the selection output */
hs_ecl_block cm_large_block(int n) { return hs_ecl_block_make((long long) hs_syevx_ws(n), HS_SXM_OUT(n)); }
long long cm_mat_len(int n) { return n <= HS_SC_MAXN ? hs_cut_mat_len(n) : cm_large_block(n).len; }

/* The entry of a call over candidate points, behind its argument checks: served[nb] (may be NULL) = -1, then 0 for the blocks P that
 * the call serves; q, Dext: the solver's LP rows.  *go = false: a communicator or sharded matrices - nothing is served, nothing to do. */
int cm_enter(hipsdp_solver* s, int nb, int* served, CmBlocks* P, int* q, const double** Dext, bool* go)
{
   if ( served != NULL )
      for (int b = 0; b < nb; ++b)
         served[b] = -1;
   *go = hs_solver_lp_rows(s, q, Dext) != 0;
   if ( !*go )
      return HIPSDP_OK;
   HS_CALL( cm_served(s, P) );
   if ( served != NULL )
      for (int b : P->ids)
         served[b] = 0;
   return HIPSDP_OK;
}

/* what a candidate takes of the workspace: its point, its matrices, its jobs, and per served block lamw doubles of eigenvalues and resw
 * doubles of the result */
long long cm_candidate_len(const hipsdp_solver* s, int m, const CmBlocks& P, int lamw, int resw)
{
   long long per = (long long) m + (long long) P.nlarge * (SCLR_JOBW + 1) + (long long) (lamw + resw) * P.ids.size();
   for (int b : P.ids)
      per += cm_mat_len(hs_solver_block_n(s, b));
   return per;
}

/* a chunk between its layout and its launches: the workspace with the solver's table of the served blocks (w.djobs), the layout, where
 * the matrices of every served block start */
struct CmRun
{
   hs_solver_cut_ws w;
   hs_cm_layout L;
   std::vector<long long> start;       /* [nsv]: doubles from the device workspace's start */
   int launches;
};

/* the layout of hipsdp_check_y_many, as cm_begin takes it */
void cm_layout(int m, int cc, int nsv, int nlarge, long long blocks_len, hs_cm_layout* L)
{ hs_cm_layout_make(m, cc, HS_CM_G, nsv, nlarge, CM_BLKW, SCLR_JOBW, blocks_len, L); }

/* The head of the chunk over the candidates Y[0 .. cc) (rows of m): the layout - make(m, cc, nsv, nlarge, blocks_len, L): the call's
 * (cm_layout, r1_layout), with lamw doubles per matrix of at most 128 rows in L.lam; with_eig = false: every block's matrices are plain
 * n x n arrays and nothing of the eigenvalue path is laid out (the unit entry) -, the workspace, Yg, the block table and, for the
 * blocks of 129 .. 512 rows, the jobs of the batched tridiagonal path in the pinned mirror, the ONE upload, Z of every (candidate, block). */
int cm_begin(hipsdp_solver* s, int m, const CmBlocks& P, int cc, const double* Y, bool with_eig, int lamw,
   void (*make)(int, int, int, int, long long, hs_cm_layout*), CmRun* R)
{
   const int nsv = (int) P.ids.size(), nlarge = with_eig ? P.nlarge : 0, nsm = nsv - nlarge;
   R->start.resize((size_t) nsv);
   R->launches = 0;
   long long blocks_len = 0;
   for (int k = 0; k < nsv; ++k)
   {
      const int n = hs_solver_block_n(s, P.ids[k]);
      R->start[k] = blocks_len;
      blocks_len += (long long) cc * (k < nsm ? hs_cut_mat_len(n) : cm_large_block(n).len);
   }
   hs_cm_layout& L = R->L;
   make(m, cc, nsv, nlarge, blocks_len, &L);
   HS_CALL( hs_solver_cut_blocks(s, P.ids, std::vector<long long>((size_t) nsv, 0), L.len.dev_len, L.len.pin_len, &R->w) );
   const hs_solver_cut_ws& w = R->w;
   /* Yg[g][i][k] = Y[g HS_CM_G + k][i], zeros behind the last candidate */
   double* yg = w.pin + L.Yg;
   memset(yg, 0, (size_t) (L.blks - L.Yg) * sizeof(double));
   for (int c = 0; c < cc; ++c)
   {
      double* dst = yg + (long long) (c / HS_CM_G) * m * HS_CM_G + c % HS_CM_G;
      const double* src = Y + (size_t) c * m;
      for (int i = 0; i < m; ++i)
         dst[(long long) i * HS_CM_G] = src[i];
   }
   hs_cm_blk* hb = reinterpret_cast<hs_cm_blk*>(w.pin + L.blks);
   hs_sxm_job* hsx = reinterpret_cast<hs_sxm_job*>(w.pin + L.jobs);
   int* hact = reinterpret_cast<int*>(w.pin + L.act);
   for (int k = 0; k < nsv; ++k)
   {
      const int n = hs_solver_block_n(s, P.ids[k]);
      double* base = w.dev + L.blocks + R->start[k];
      hs_cm_blk& B = hb[k];
      if ( k < nsm )
      {
         B.Z = base; B.zstride = hs_cut_mat_len(n);
         B.lam = w.dev + L.lam + (long long) lamw * cc * k; B.lstride = lamw;
         continue;
      }
      /* job (block k, candidate c) of the tridiagonal path: Z goes where the column launches read their matrix, the head of its workspace */
      const hs_ecl_block E = cm_large_block(n);
      for (int c = 0; c < cc; ++c)
      {
         const size_t j = (size_t) (k - nsm) * cc + c;
         double* jb = base + (long long) c * E.len;
         HS_CALL( sxm_job(hs_syevx_many_job, n, jb + E.ws, jb + E.out, HS_SXM_ACTIVE, &hsx[j], &hact[j]) );
      }
      B.Z = base + E.ws; B.zstride = E.len;
      B.lam = base + E.out + HS_SYEVX_OUT_LAM; B.lstride = E.len;
   }
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, w.stream) );
   if ( nsv > 0 )
   {
      HS_CALL( hs_cm_form_z(w.stream, nsv, P.nmax, m, cc, w.djobs, reinterpret_cast<const hs_cm_blk*>(w.dev + L.blks), w.dev + L.Yg) );
      ++R->launches;
   }
   return HS_OK;
}

/* The eigenvalue stage of a chunk of cc candidates, class by class: `small` and `mid` (hs_lmin_many_*, hs_lsel_many_*), one launch
 * each, for the blocks of at most 64 and of 65 .. 128 rows; for those of 129 .. 512 rows the clearing of the reflector arrays, the
 * nmax_large - 1 column launches and close(st, jobs, nmax_large, dsx, dact), which takes close_launches launches. */
template <class Close>
int cm_eigenvalues(const CmBlocks& P, int cc, int (*small)(hipStream_t, int, int, int, const hs_ec_job*, const hs_cm_blk*),
   int (*mid)(hipStream_t, int, int, int, int, const hs_ec_job*, const hs_cm_blk*), Close close, int close_launches, CmRun* R)
{
   const hs_solver_cut_ws& w = R->w;
   hipStream_t st = w.stream;
   const hs_cm_blk* db = reinterpret_cast<const hs_cm_blk*>(w.dev + R->L.blks);
   if ( P.nsmall > 0 )
   {
      HS_CALL( small(st, P.nsmall, cc, P.nmax_small, w.djobs, db) );
      ++R->launches;
   }
   if ( P.nmid > 0 )
   {
      const int cus = hs_device_cus();
      HS_CALL( mid(st, P.nmid, cc, P.nmax_mid, cus > 0 ? cus : 256, w.djobs + P.nsmall, db + P.nsmall) );
      ++R->launches;
   }
   if ( P.nlarge > 0 )
   {
      const int jobs = P.nlarge * cc;
      const hs_sxm_job* dsx = reinterpret_cast<const hs_sxm_job*>(w.dev + R->L.jobs);
      const int* dact = reinterpret_cast<const int*>(w.dev + R->L.act);
      HS_CALL( hs_ecl_clear(st, jobs, dsx) );
      HS_CALL( hs_syevx_many_cols(st, jobs, P.nmax_large, hs_syevx_many_cap(jobs), dsx, dact) );
      HS_CALL( close(st, jobs, P.nmax_large, dsx, dact) );
      R->launches += 1 + (P.nmax_large - 1) + close_launches;
   }
   return HS_OK;
}

/* ONE CHUNK: the candidates Y[0 .. cc) - a call of its own in everything but the entry: ONE upload, hs_cm_launches(..) launches whatever
 * cc and the number of blocks are, ONE read-back, the copy-out to lmin (rows of nb) and lpviol (may be NULL) of these candidates */
int cm_chunk(hipsdp_solver* s, int m, int nb, const CmBlocks& P, int q, const double* Dext, int cc, const double* Y, double* lmin, double* lpviol)
{
   CmRun R;
   HS_CALL( cm_begin(s, m, P, cc, Y, true, 2, cm_layout, &R) );
   const hs_solver_cut_ws& w = R.w;
   const hs_cm_layout& L = R.L;
   const int nsv = (int) P.ids.size();
   /* the third class closes with the selection of eigenvalue 1: 3 launches */
   HS_CALL( cm_eigenvalues(P, cc, hs_lmin_many_small, hs_lmin_many_mid, [](hipStream_t st, int jobs, int nmax, const hs_sxm_job* dsx, const int* dact)
      { return hs_syevx_many_select(st, jobs, nmax, 0, dsx, dact); }, 3, &R) );
   HS_CALL( hs_cm_result(w.stream, nsv, cc, m, q, Dext, reinterpret_cast<const hs_cm_blk*>(w.dev + L.blks), w.dev + L.Yg, w.dev + L.res) );
   ++R.launches;
   if ( R.launches != hs_cm_launches(nsv > 0, P.nsmall > 0, P.nmid > 0, P.nmax_large) )
      return HIPSDP_ERR_NUMERIC;
   HS_CALL( chunk_readback(w, L.len, R.launches, &g_cm) );
   const double* res = w.pin + L.res;
   for (int c = 0; c < cc; ++c)
   {
      for (int k = 0; k < nsv; ++k)
         lmin[(size_t) c * nb + P.ids[k]] = res[(size_t) c * nsv + k];
      if ( lpviol != NULL )
         lpviol[c] = res[(size_t) cc * nsv + c];
   }
   return HIPSDP_OK;
}

int check_y_many_impl(hipsdp_solver* s, int count, const double* Y, double* lmin, double* lpviol, int* served)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || count < 0 || (count > 0 && (Y == NULL || lmin == NULL)) )
      return HIPSDP_ERR_ARG;
   if ( count == 0 )
      return HIPSDP_OK;
   int q = 0;
   const double* Dext = NULL;
   CmBlocks P;
   bool go = false;
   HS_CALL( cm_enter(s, nb, served, &P, &q, &Dext, &go) );
   if ( !go )
      return HIPSDP_OK;
   if ( P.ids.empty() && q == 0 )
   {
      if ( lpviol != NULL )
         for (int j = 0; j < count; ++j)
            lpviol[j] = 0.0;
      return HIPSDP_OK;
   }
   /* per served block two doubles of eigenvalues and lmin in the candidate's row of the result, which ends with lpviol */
   const std::vector<long long> job_len((size_t) count, cm_candidate_len(s, m, P, 2, 1) + 1);
   HS_CALL( hs_chunks_run(job_len.data(), count, SCLR_BUDGET, hs_chunk_env("HIPSDP_CHECK_MANY_CHUNK"), [&](int start, int end)
      {
         return cm_chunk(s, m, nb, P, q, Dext, end - start, Y + (size_t) start * m, lmin + (size_t) start * nb,
            lpviol != NULL ? lpviol + start : NULL);
      }) );
   ++g_cm.calls;
   return HIPSDP_OK;
}

}

int hs_check_many_form_z(hipsdp_solver* s, int count, const double* Y, double* Zout, int* served, int* launches)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || count < 1 || Y == NULL || Zout == NULL || launches == NULL )
      return HIPSDP_ERR_ARG;
   *launches = 0;
   if ( served != NULL )
      for (int b = 0; b < nb; ++b)
         served[b] = -1;
   CmBlocks P;
   HS_CALL( cm_served(s, &P) );
   if ( P.ids.empty() )
      return HIPSDP_OK;
   CmRun R;
   HS_CALL( cm_begin(s, m, P, count, Y, false, 2, cm_layout, &R) );
   const std::vector<long long> off = block_sums(s, nb, NULL, n_full);
   for (size_t k = 0; k < P.ids.size(); ++k)
   {
      const int b = P.ids[k], n = hs_solver_block_n(s, b);
      const double* Z = R.w.dev + R.L.blocks + R.start[k];
      for (int c = 0; c < count; ++c)
         HS_HIP( hipMemcpyAsync(Zout + (size_t) c * off[nb] + off[b], Z + (long long) c * hs_cut_mat_len(n), (size_t) n * n * sizeof(double),
               hipMemcpyDeviceToHost, R.w.stream) );
      if ( served != NULL )
         served[b] = 0;
   }
   HS_HIP( hipStreamSynchronize(R.w.stream) );
   *launches = R.launches;
   return HIPSDP_OK;
}

extern "C" int hipsdp_check_y_many(hipsdp_solver* s, int count, const double* Y, double* lmin, double* lpviol, int* served)
{
   return check_y_many_impl(s, count, Y, lmin, lpviol, served);
}

extern "C" int hipsdp_check_y_many_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_cm.get(calls, launches, readbacks);
}

namespace {

/* ---- hipsdp_rounding_frame / hipsdp_rounding_recombine: the two device stages of the primal rounding problem (kernels: rounding.hip, the
 * expand, recombine and write launches of psd_many.hip / psd_large.hip, the batched decompositions of eigi.hip, syevx.hip, syevr.hip;
 * planning: hs_round_plan.h) ------------------------------------------------------------------------------------------------------------ */
CutStats g_rf;

static_assert(sizeof(hs_rf_job) % 8 == 0 && sizeof(hs_pp_job) % 8 == 0 && sizeof(hs_eig_job) % 8 == 0 && sizeof(hs_ppl_job) % 8 == 0
   && sizeof(hs_sxm_job) % 8 == 0 && sizeof(hs_srm_job) % 8 == 0, "hs_rf_layout: rows of the tables are whole doubles");
const hs_rf_widths RF_W = {(int) (sizeof(hs_rf_job) / 8), (int) (sizeof(hs_pp_job) / 8), (int) (sizeof(hs_eig_job) / 8),
   (int) (sizeof(hs_ppl_job) / 8), (int) (sizeof(hs_sxm_job) / 8), (int) (sizeof(hs_srm_job) / 8)};

long long rf_small_scratch(int n) { return hs_syev_small_scratch(n); }
long long rf_large_ws(int n) { return (long long) hs_syevr_ws(n); }
long long rf_large_out(int n) { return HS_SYEVR_OUT(n); }
const hs_rf_rules RF_RULES = {rf_small_scratch, rf_large_ws, rf_large_out};

/* how many of the items [start, end) of a chunk, which descend in n, are above HS_RF_SMALLN rows: the leading ones */
template <class Item>
int rf_count_large(const std::vector<Item>& items, int start, int end)
{
   int nlarge = 0;
   while ( start + nlarge < end && items[(size_t) start + nlarge].n > HS_RF_SMALLN )
      ++nlarge;
   return nlarge;
}

/* the caller's arrays of hipsdp_rounding_frame */
struct RfArgs
{
   const int* xnnz; const int* const* xrow; const int* const* xcol; const double* const* xval;
   double *eigvals, *obj, *coefs, *vecs;
};

/* ONE CHUNK of stage 1: the served blocks items[start .. end), largest first - ONE upload (tables and triplets), hs_rf_launches(..)
 * launches whatever the number of blocks, ONE read-back, the copy-out */
int rf_chunk(hipsdp_solver* s, int m, const std::vector<hs_rf_item>& items, int start, int end, const RfArgs& a, const hs_round_frame& F,
   const std::vector<long long>& off, const std::vector<long long>& voff)
{
   const int cnt = end - start, nb = (int) off.size() - 1, nlarge = rf_count_large(items, start, end), nsmall = cnt - nlarge;
   std::vector<int> ids((size_t) cnt);
   std::vector<hs_rf_block> blk((size_t) cnt);
   std::vector<long long> at((size_t) cnt), row0((size_t) cnt), vec0((size_t) cnt), trip0((size_t) cnt);
   long long blocks_len = 0, rows = 0, vec_len = 0, trips = 0, tiles = 1;
   int nmax = 0;
   for (int k = 0; k < cnt; ++k)
   {
      const hs_rf_item& it = items[(size_t) start + k];
      ids[k] = it.blk;
      blk[k] = hs_rf_block_make(it.n, m, it.route, it.slices, &RF_RULES);
      at[k] = blocks_len; row0[k] = rows; vec0[k] = vec_len; trip0[k] = trips;
      blocks_len += blk[k].len;
      rows += it.n;
      vec_len += a.vecs != NULL ? (long long) it.n * it.n : 0;
      trips += it.nnz;
      nmax = it.n > nmax ? it.n : nmax;
      if ( it.route )
         tiles = std::max(tiles, hs_rf_tiles(it.n, m, it.slices));
   }
   hs_rf_layout L;
   hs_rf_layout_make(m, cnt, nsmall, nlarge, trips, rows, vec_len, &RF_W, blocks_len, &L);
   hs_solver_cut_ws w;
   HS_CALL( hs_solver_cut_blocks(s, ids, std::vector<long long>((size_t) cnt, 0), L.len.dev_len, L.len.pin_len, &w) );
   hs_rf_job* hrf = reinterpret_cast<hs_rf_job*>(w.pin + L.rf);
   hs_pp_job* hpp = reinterpret_cast<hs_pp_job*>(w.pin + L.pp);
   hs_eig_job* heig = reinterpret_cast<hs_eig_job*>(w.pin + L.eig);
   hs_ppl_job* hppl = reinterpret_cast<hs_ppl_job*>(w.pin + L.ppl);
   hs_sxm_job* hsx = reinterpret_cast<hs_sxm_job*>(w.pin + L.sx);
   hs_srm_job* hsr = reinterpret_cast<hs_srm_job*>(w.pin + L.sr);
   int* hact = reinterpret_cast<int*>(w.pin + L.act);
   double* hval = w.pin + L.val;
   int* hrow = reinterpret_cast<int*>(w.pin + L.row);
   int* hcol = reinterpret_cast<int*>(w.pin + L.col);
   const long long N = off[nb];
   for (int k = 0; k < cnt; ++k)
   {
      const hs_rf_item& it = items[(size_t) start + k];
      const int n = it.n, b = it.blk;
      double* base = w.dev + L.blocks + at[k];
      hs_rf_job& J = hrf[k];
      memset(&J, 0, sizeof(J));
      J.n = n; J.route = it.route; J.slices = it.slices; J.pps = it.pps; J.klen = it.klen;
      J.lam = F.dev + off[b]; J.V = F.dev + N + voff[b];
      J.VT = it.route == 0 ? base + blk[k].VT : NULL;
      J.part = base + blk[k].part;
      J.row0 = row0[k]; J.vec0 = vec0[k];
      if ( k < nlarge )
      {
         /* (the selection output of the first is not used) */
         HS_CALL( sxm_job(hs_syevx_many_job, n, base + blk[k].ws, base + blk[k].out, HS_SXM_ACTIVE, &hsx[k], &hact[k]) );
         HS_CALL( hs_syevr_many_job(n, base + blk[k].ws, base + blk[k].out, &hsr[k]) );
         hs_ppl_job& T = hppl[k];
         memset(&T, 0, sizeof(T));
         T.n = n; T.nnz = (int) it.nnz; T.ntc = (n + HS_RF_TILE - 1) / HS_RF_TILE; T.trip = trip0[k];
         T.A = hsx[k].A; T.R = hsx[k].R;
         J.lam_src = base + blk[k].out; J.V_src = base + blk[k].out + HS_SYEVR_OUT_VEC(n);
      }
      else
      {
         /* the decompositions want their table ordered by class: the small blocks of the chunk, which descend in n, backwards */
         const int t = cnt - 1 - k;
         hs_pp_job& T = hpp[t];
         memset(&T, 0, sizeof(T));
         T.n = n; T.nnz = (int) it.nnz; T.trip = trip0[k]; T.A = base + blk[k].mat;
         memset(&heig[t], 0, sizeof(hs_eig_job));
         heig[t].n = n; heig[t].in = base + blk[k].mat; heig[t].ws = base + blk[k].ws;
         J.lam_src = base + blk[k].ws; J.V_src = base + blk[k].ws + hs_syev_many_vecpos(n);
      }
      if ( it.nnz > 0 )
      {
         memcpy(hval + trip0[k], a.xval[b], (size_t) it.nnz * sizeof(double));
         memcpy(hrow + trip0[k], a.xrow[b], (size_t) it.nnz * sizeof(int));
         memcpy(hcol + trip0[k], a.xcol[b], (size_t) it.nnz * sizeof(int));
      }
   }
   hipStream_t st = w.stream;
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );
   const hs_rf_job* drf = reinterpret_cast<const hs_rf_job*>(w.dev + L.rf);
   const int* drow = reinterpret_cast<const int*>(w.dev + L.row);
   const int* dcol = reinterpret_cast<const int*>(w.dev + L.col);
   int launches = 0;
   if ( nsmall > 0 )
   {
      HS_CALL( hs_pp_expand(st, nsmall, reinterpret_cast<const hs_pp_job*>(w.dev + L.pp), drow, dcol, w.dev + L.val) );
      ++launches;
      HS_CALL( scx_syev(st, nsmall, heig, reinterpret_cast<const hs_eig_job*>(w.dev + L.eig), &launches) );
   }
   if ( nlarge > 0 )
   {
      const int nml = items[(size_t) start].n;
      const hs_sxm_job* dsx = reinterpret_cast<const hs_sxm_job*>(w.dev + L.sx);
      const hs_srm_job* dsr = reinterpret_cast<const hs_srm_job*>(w.dev + L.sr);
      HS_CALL( hs_ppl_expand(st, nlarge, reinterpret_cast<const hs_ppl_job*>(w.dev + L.ppl), drow, dcol, w.dev + L.val) );
      HS_CALL( hs_syevx_many_cols(st, nlarge, nml, hs_syevx_many_cap(nlarge), dsx, reinterpret_cast<const int*>(w.dev + L.act)) );
      HS_CALL( hs_syevr_many_tvec(st, nlarge, nml, dsr) );
      HS_CALL( hs_syevr_many_back(st, nlarge, nml, dsr) );
      launches += 1 + (nml - 1) + 5 + 6 * ((nml + 31) / 32) + 1;
   }
   HS_CALL( hs_rf_gather(st, cnt, drf) );
   HS_CALL( hs_rf_coefs_scalar(st, cnt, nmax, m, w.djobs, drf) );
   HS_CALL( hs_rf_coefs_mc(st, cnt, tiles, m, w.djobs, drf) );
   HS_CALL( hs_rf_store(st, cnt, m, drf, w.dev + L.r_eig, w.dev + L.r_obj, w.dev + L.r_coef, a.vecs != NULL ? w.dev + L.r_vec : NULL) );
   launches += 4;
   if ( launches != hs_rf_launches(nsmall > 0, nlarge > 0 ? items[(size_t) start].n : 0) )
      return HIPSDP_ERR_NUMERIC;
   HS_CALL( chunk_readback(w, L.len, launches, &g_rf) );
   for (int k = 0; k < cnt; ++k)
   {
      const hs_rf_item& it = items[(size_t) start + k];
      const size_t n = (size_t) it.n, o = (size_t) off[it.blk];
      memcpy(a.eigvals + o, w.pin + L.r_eig + row0[k], n * sizeof(double));
      memcpy(a.obj + o, w.pin + L.r_obj + row0[k], n * sizeof(double));
      if ( m > 0 )
         memcpy(a.coefs + o * m, w.pin + L.r_coef + row0[k] * m, n * m * sizeof(double));
      if ( a.vecs != NULL )
         memcpy(a.vecs + voff[it.blk], w.pin + L.r_vec + vec0[k], n * n * sizeof(double));
   }
   return HIPSDP_OK;
}

int rounding_frame_impl(hipsdp_solver* s, const RfArgs& a, int* served)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || a.xnnz == NULL || a.eigvals == NULL || a.obj == NULL || a.coefs == NULL )
      return HIPSDP_ERR_ARG;
   for (int b = 0; b < nb; ++b)
   {
      const int n = hs_solver_block_n(s, b);
      if ( a.xnnz[b] < 0 )
         return HIPSDP_ERR_ARG;
      if ( a.xnnz[b] == 0 )
         continue;
      if ( a.xrow == NULL || a.xcol == NULL || a.xval == NULL || a.xrow[b] == NULL || a.xcol[b] == NULL || a.xval[b] == NULL )
         return HIPSDP_ERR_ARG;
      for (int e = 0; e < a.xnnz[b]; ++e)
         if ( a.xrow[b][e] < 0 || a.xrow[b][e] >= n || a.xcol[b][e] < 0 || a.xcol[b][e] >= n )
            return HIPSDP_ERR_ARG;
   }
   hs_round_frame* F = NULL;
   HS_CALL( hs_solver_round_frame(s, 0, &F) );
   F->valid = 0;
   F->served.assign((size_t) nb, -1);
   if ( served != NULL )
      for (int b = 0; b < nb; ++b)
         served[b] = -1;
   std::vector<int> all;
   HS_CALL( hs_solver_cut_enter_large(s, HS_RF_MAXN, &all) );
   std::vector<int> ns((size_t) nb), ok((size_t) nb, 0), form((size_t) nb, 0);
   for (int b = 0; b < nb; ++b)
      ns[b] = hs_solver_block_n(s, b);
   for (int b : all)
   {
      ok[b] = 1;
      form[b] = hs_solver_block_form(s, b);
   }
   std::vector<hs_rf_item> items;
   hs_rf_items(nb, m, ns.data(), ok.data(), form.data(), a.xnnz, a.vecs != NULL, &RF_RULES, &items);
   if ( items.empty() )
   {
      F->valid = 1;                    /* (a frame that holds no block: stage 2 serves none) */
      return HIPSDP_OK;
   }
   /* where a block's eigenvalues and its vectors start in the frame and in the caller's arrays */
   const std::vector<long long> off = block_sums(s, nb, NULL, n_rows), voff = block_sums(s, nb, NULL, n_full);
   HS_CALL( hs_solver_round_frame(s, off[nb] + voff[nb], &F) );
   std::vector<long long> len(items.size());
   for (size_t k = 0; k < items.size(); ++k)
      len[k] = items[k].len;
   HS_CALL( hs_chunks_run(len.data(), (int) items.size(), SCLR_BUDGET, hs_chunk_env("HIPSDP_ROUNDING_CHUNK"), [&](int start, int end)
      { return rf_chunk(s, m, items, start, end, a, *F, off, voff); }) );
   for (const hs_rf_item& it : items)
   {
      F->served[it.blk] = 0;
      if ( served != NULL )
         served[it.blk] = 0;
   }
   F->valid = 1;
   ++g_rf.calls;
   return HIPSDP_OK;
}

/* a served block of stage 2 in the order of its chunks */
struct Rf2Item { int blk, n, cap; };

/* ONE CHUNK of stage 2: ONE upload (lambda and the two job tables), hs_rf2_launches(..) launches, ONE read-back, the copy-out */
int rf2_chunk(hipsdp_solver* s, const std::vector<Rf2Item>& items, int start, int end, const double* lambda, double epsilon, int mode,
   hipsdp_rounding_out* out, const hs_round_frame& F, const std::vector<long long>& off, const std::vector<long long>& voff, bool* overflow)
{
   const int cnt = end - start, nb = (int) off.size() - 1, nlarge = rf_count_large(items, start, end), nsmall = cnt - nlarge;
   std::vector<long long> row0((size_t) cnt), int0((size_t) cnt), mat0((size_t) cnt);
   long long rows = 0, cap_small = 0, cap_large = 0, ints_len = 0, mats_len = 0;
   int nmax_small = 0;
   for (int k = 0; k < cnt; ++k)
   {
      const Rf2Item& it = items[(size_t) start + k];
      const long long full = (long long) it.n * (it.n + 1) / 2, res = it.cap < full ? it.cap : full;
      const long long tc = (it.n + HS_RF_TILE - 1) / HS_RF_TILE;
      row0[k] = rows; int0[k] = ints_len; mat0[k] = mats_len;
      rows += it.n;
      mats_len += hs_cut_mat_len(it.n);
      if ( k < nlarge )
      {
         cap_large += res;
         ints_len += (it.n * tc + tc * tc + 1) & ~1LL;
      }
      else
      {
         cap_small += res;
         ints_len += ((long long) it.n + 2) & ~1LL;
         nmax_small = it.n > nmax_small ? it.n : nmax_small;
      }
   }
   hs_rf2_layout L;
   hs_rf2_layout_make(nsmall, nlarge, rows, cap_small, cap_large, &RF_W, ints_len, mats_len, &L);
   hs_solver_cut_ws w;
   HS_CALL( hs_solver_cut_plain(s, L.len.dev_len, L.len.pin_len, &w) );
   hs_pp_job* hpp = reinterpret_cast<hs_pp_job*>(w.pin + L.pp);
   hs_ppl_job* hppl = reinterpret_cast<hs_ppl_job*>(w.pin + L.ppl);
   int* dints = reinterpret_cast<int*>(w.dev + L.ints);
   const long long N = off[nb];
   for (int k = 0; k < cnt; ++k)
   {
      const Rf2Item& it = items[(size_t) start + k];
      memcpy(w.pin + L.lam + row0[k], lambda + off[it.blk], (size_t) it.n * sizeof(double));
      if ( k < nlarge )
      {
         hs_ppl_job& T = hppl[k];
         memset(&T, 0, sizeof(T));
         T.n = it.n; T.cap = it.cap; T.ntc = (it.n + HS_RF_TILE - 1) / HS_RF_TILE;
         T.A = w.dev + L.mats + mat0[k]; T.lam = w.dev + L.lam + row0[k]; T.V = F.dev + N + voff[it.blk];
         T.minev = -HUGE_VAL; T.cnt = dints + int0[k];
      }
      else
      {
         hs_pp_job& T = hpp[k - nlarge];
         memset(&T, 0, sizeof(T));
         T.n = it.n; T.cap = it.cap;
         T.A = w.dev + L.mats + mat0[k]; T.lam = w.dev + L.lam + row0[k]; T.V = F.dev + N + voff[it.blk];
         T.minev = -HUGE_VAL; T.rowoff = dints + int0[k];
      }
   }
   hipStream_t st = w.stream;
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );
   int launches = 0;
   if ( nsmall > 0 )
   {
      const hs_pp_job* dpp = reinterpret_cast<const hs_pp_job*>(w.dev + L.pp);
      int* dtot = reinterpret_cast<int*>(w.dev + L.tot);
      HS_CALL( hs_pp_recombine(st, nsmall, nmax_small, dpp, epsilon, mode, dtot) );
      HS_CALL( hs_pp_write(st, nsmall, nmax_small, dpp, dtot, epsilon, cap_small, reinterpret_cast<int*>(w.dev + L.t_small),
            reinterpret_cast<int*>(w.dev + L.r_small), reinterpret_cast<int*>(w.dev + L.c_small), w.dev + L.v_small) );
      launches += 2;
   }
   if ( nlarge > 0 )
   {
      const hs_ppl_job* dppl = reinterpret_cast<const hs_ppl_job*>(w.dev + L.ppl);
      const int nml = items[(size_t) start].n;
      HS_CALL( hs_ppl_recombine(st, nlarge, nml, dppl, epsilon, mode) );
      HS_CALL( hs_ppl_write(st, nlarge, nml, dppl, epsilon, cap_large, reinterpret_cast<int*>(w.dev + L.t_large),
            reinterpret_cast<int*>(w.dev + L.r_large), reinterpret_cast<int*>(w.dev + L.c_large), w.dev + L.v_large) );
      launches += 2;
   }
   if ( launches != hs_rf2_launches(nsmall > 0, nlarge > 0) )
      return HIPSDP_ERR_NUMERIC;
   HS_CALL( chunk_readback(w, L.len, launches, &g_rf) );
   for (int cls = 0; cls < 2; ++cls)
   {
      const int k0 = cls == 0 ? 0 : nlarge, k1 = cls == 0 ? nlarge : cnt;
      const int* tot = reinterpret_cast<const int*>(w.pin + (cls == 0 ? L.t_large : L.t_small));
      const double* val = w.pin + (cls == 0 ? L.v_large : L.v_small);
      const int* row = reinterpret_cast<const int*>(w.pin + (cls == 0 ? L.r_large : L.r_small));
      const int* col = reinterpret_cast<const int*>(w.pin + (cls == 0 ? L.c_large : L.c_small));
      const long long room = cls == 0 ? cap_large : cap_small;
      long long pos = 0;
      for (int k = k0; k < k1; ++k)
      {
         hipsdp_rounding_out& O = out[items[(size_t) start + k].blk];
         const int t = tot[k - k0];
         O.nnz_out = t;
         if ( t > O.cap )
         {
            *overflow = true;
            continue;
         }
         if ( t < 0 || pos + t > room )
            return HIPSDP_ERR_NUMERIC;
         if ( t > 0 )
         {
            memcpy(O.valout, val + pos, (size_t) t * sizeof(double));
            memcpy(O.rowout, row + pos, (size_t) t * sizeof(int));
            memcpy(O.colout, col + pos, (size_t) t * sizeof(int));
         }
         pos += t;
      }
   }
   return HIPSDP_OK;
}

}

extern "C" int hipsdp_rounding_recombine(hipsdp_solver* s, const double* lambda, double epsilon, int mode, hipsdp_rounding_out* out)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || lambda == NULL || out == NULL || mode < 0 || mode > 1 )
      return HIPSDP_ERR_ARG;
   for (int b = 0; b < nb; ++b)
      if ( out[b].cap < 0 || (out[b].cap > 0 && (out[b].rowout == NULL || out[b].colout == NULL || out[b].valout == NULL)) )
         return HIPSDP_ERR_ARG;
   hs_round_frame* F = NULL;
   HS_CALL( hs_solver_round_frame(s, 0, &F) );
   if ( !F->valid || (int) F->served.size() != nb )
      return HIPSDP_ERR_ARG;
   std::vector<Rf2Item> items;
   for (int b = 0; b < nb; ++b)
   {
      out[b].nnz_out = -1;
      if ( F->served[b] == 0 )
         items.push_back(Rf2Item{b, hs_solver_block_n(s, b), out[b].cap});
   }
   if ( items.empty() )
      return HIPSDP_OK;
   std::stable_sort(items.begin(), items.end(), [](const Rf2Item& x, const Rf2Item& y) { return x.n > y.n; });
   const std::vector<long long> off = block_sums(s, nb, NULL, n_rows), voff = block_sums(s, nb, NULL, n_full);
   std::vector<long long> len(items.size());
   for (size_t k = 0; k < items.size(); ++k)
      len[k] = hs_rf2_item_len(items[k].n, items[k].cap);
   bool overflow = false;
   HS_CALL( hs_chunks_run(len.data(), (int) items.size(), SCLR_BUDGET, hs_chunk_env("HIPSDP_ROUNDING_CHUNK"), [&](int start, int end)
      { return rf2_chunk(s, items, start, end, lambda, epsilon, mode, out, *F, off, voff, &overflow); }) );
   ++g_rf.calls;
   return overflow ? HIPSDP_ERR_ARG : HIPSDP_OK;
}

extern "C" int hipsdp_rounding_frame(hipsdp_solver* s, const int* xnnz, const int* const* xrow, const int* const* xcol,
   const double* const* xval, double* eigvals, double* obj, double* coefs, double* vecs, int* served)
{
   return rounding_frame_impl(s, RfArgs{xnnz, xrow, xcol, xval, eigvals, obj, coefs, vecs}, served);
}

extern "C" int hipsdp_rounding_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_rf.get(calls, launches, readbacks);
}

namespace {

/* ---- hipsdp_rank1_check_many: eigenvalues 1, n - 1, n and the two scans over the 2 x 2 principal minors of every Z_b(Y[j]) (kernels:
 * rank1.hip, check_many.hip, eigi.hip, syevx.hip).  The served blocks, the chunks, the workspace, Z and the eigenvalue stage are those of
 * hipsdp_check_y_many (cm_enter, cm_begin, cm_eigenvalues); the layout, the minors and the result differ. ------------------------------- */
CutStats g_r1;

/* where the four optional output groups of a chunk's candidates go (rows of nb blocks); a NULL pair is not copied out */
struct R1Dst { double* lam; double* minorev; int* minorind; double* minordet; int* detind; };

/* the layout of hipsdp_rank1_check_many, as cm_begin takes it: four doubles per matrix of at most 128 rows in L.lam */
void r1_layout(int m, int cc, int nsv, int nlarge, long long blocks_len, hs_cm_layout* L)
{ hs_r1_layout_make(m, cc, HS_CM_G, nsv, nlarge, CM_BLKW, SCLR_JOBW, HS_R1_RESW, blocks_len, L); }

/* ONE CHUNK: the candidates Y[0 .. cc): ONE upload, hs_r1_launches(..) launches whatever cc and the number of blocks are, ONE read-back.
 * The minors launch stands right behind Z(y): the column launches of the 129 .. 512 class consume their matrix. */
int r1_chunk(hipsdp_solver* s, int m, int nb, const CmBlocks& P, int cc, const double* Y, double feastol, const R1Dst& d)
{
   CmRun R;
   HS_CALL( cm_begin(s, m, P, cc, Y, true, 4, r1_layout, &R) );
   const hs_solver_cut_ws& w = R.w;
   const hs_cm_layout& L = R.L;
   hipStream_t st = w.stream;
   const int nsv = (int) P.ids.size();
   const hs_cm_blk* db = reinterpret_cast<const hs_cm_blk*>(w.dev + L.blks);
   double* dres = w.dev + L.res;
   HS_CALL( hs_r1_minors(st, nsv, cc, P.nmax, feastol, w.djobs, db, dres) );
   ++R.launches;
   /* the third class closes with the three indexed eigenvalues alone: 1 launch */
   HS_CALL( cm_eigenvalues(P, cc, hs_lsel_many_small, hs_lsel_many_mid, hs_syevx_many_index, 1, &R) );
   HS_CALL( hs_r1_result(st, nsv, cc, w.djobs, db, dres) );
   ++R.launches;
   if ( R.launches != hs_r1_launches(nsv > 0, P.nsmall > 0, P.nmid > 0, P.nmax_large) )
      return HIPSDP_ERR_NUMERIC;
   HS_CALL( chunk_readback(w, L.len, R.launches, &g_r1) );
   const double* res = w.pin + L.res;
   for (int c = 0; c < cc; ++c)
      for (int k = 0; k < nsv; ++k)
      {
         const double* row = res + ((size_t) c * nsv + k) * HS_R1_RESW;
         const size_t o = (size_t) c * nb + P.ids[k];
         int ind[4];
         memcpy(ind, row + 5, sizeof(ind));
         d.lam[3 * o] = row[0]; d.lam[3 * o + 1] = row[1]; d.lam[3 * o + 2] = row[2];
         if ( d.minorev != NULL )
         {
            d.minorev[o] = row[3];
            d.minorind[2 * o] = ind[0]; d.minorind[2 * o + 1] = ind[1];
         }
         if ( d.minordet != NULL )
         {
            d.minordet[o] = row[4];
            d.detind[2 * o] = ind[2]; d.detind[2 * o + 1] = ind[3];
         }
      }
   return HIPSDP_OK;
}

int rank1_check_many_impl(hipsdp_solver* s, int count, const double* Y, double feastol, const R1Dst& d, int* served)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || count < 0 || !(feastol >= 0.0) || (count > 0 && (Y == NULL || d.lam == NULL))
      || (d.minorev == NULL) != (d.minorind == NULL) || (d.minordet == NULL) != (d.detind == NULL) )
      return HIPSDP_ERR_ARG;
   if ( count == 0 )
      return HIPSDP_OK;
   int q = 0;                                              /* (the LP rows are not looked at) */
   const double* Dext = NULL;
   CmBlocks P;
   bool go = false;
   HS_CALL( cm_enter(s, nb, served, &P, &q, &Dext, &go) );
   if ( !go || P.ids.empty() )
      return HIPSDP_OK;
   const std::vector<long long> job_len((size_t) count, cm_candidate_len(s, m, P, 4, HS_R1_RESW));
   HS_CALL( hs_chunks_run(job_len.data(), count, SCLR_BUDGET, hs_chunk_env("HIPSDP_RANK1_CHUNK"), [&](int start, int end)
      {
         const size_t o = (size_t) start * nb;
         const R1Dst c = { d.lam + 3 * o, d.minorev != NULL ? d.minorev + o : NULL, d.minorind != NULL ? d.minorind + 2 * o : NULL,
            d.minordet != NULL ? d.minordet + o : NULL, d.detind != NULL ? d.detind + 2 * o : NULL };
         return r1_chunk(s, m, nb, P, end - start, Y + (size_t) start * m, feastol, c);
      }) );
   ++g_r1.calls;
   return HIPSDP_OK;
}

}

extern "C" int hipsdp_rank1_check_many(hipsdp_solver* s, int count, const double* Y, double feastol, double* lam, double* minorev, int* minorind,
   double* minordet, int* detind, int* served)
{
   const R1Dst d = { lam, minorev, minorind, minordet, detind };
   return rank1_check_many_impl(s, count, Y, feastol, d, served);
}

extern "C" int hipsdp_rank1_check_many_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_r1.get(calls, launches, readbacks);
}

namespace {

/* ---- hipsdp_rank1_approx: eigenpair n of Z_b(y) and the right-hand side A_0 + lambda v v^T of the rank-1 approximation heuristic for the
 * asked-for blocks (kernels: eigcuts.hip for Z(y), the batched full decomposition of eigi.hip up to 128 rows, the batched tridiagonal path
 * of syevx.hip on -Z above, rank1.hip for the rest) --------------------------------------------------------------------------------------- */
static_assert(sizeof(hs_r1a_job) == 5 * sizeof(double), "hs_r1a_layout: tabw");
#define R1A_TABW 5
CutStats g_r1a;

/* what a block of n rows takes of a chunk's workspace: Z and the slab of its decomposition, or the workspace of the tridiagonal form (Z is
 * formed into its head) and the selection output */
long long r1a_block_len(int n)
{
   return n <= HS_SC_MAXN ? hs_cut_mat_len(n) + ((hs_syev_small_scratch(n) + 1) & ~1LL) : cm_large_block(n).len;
}

/* ONE CHUNK: the asked-for served blocks `ids` (descending n): ONE upload, hs_r1a_launches(..) launches, ONE read-back, the copy-out.
 * voff / roff: where a block's vector and right-hand side start in the caller's arrays. */
int r1a_chunk(hipsdp_solver* s, int m, const std::vector<int>& ids, const double* y, const std::vector<long long>& voff,
   const std::vector<long long>& roff, double* lmax, double* vec, double* rhs)
{
   const int cnt = (int) ids.size();
   /* the tables want the blocks of at most 128 rows ordered by decomposition class; the larger ones come first in ids */
   int nlg = 0, nmax = 0, nmax_large = 0;
   for (int b : ids)
      nlg += hs_solver_block_n(s, b) > HS_SC_MAXN ? 1 : 0;
   const int nsm = cnt - nlg;
   std::vector<int> order(ids.begin(), ids.begin() + nlg);
   for (int cls = 0; cls < 3; ++cls)
      for (int j = nlg; j < cnt; ++j)
         if ( hs_syev_many_class(hs_solver_block_n(s, ids[j])) == cls )
            order.push_back(ids[j]);
   for (int j = 0; j < cnt; ++j)
   {
      nmax = std::max(nmax, hs_solver_block_n(s, order[j]));
      if ( j < nlg )
         nmax_large = std::max(nmax_large, hs_solver_block_n(s, order[j]));
   }
   /* where a block's part of the workspace, its vector and its right-hand side start in the chunk */
   const std::vector<long long> start = block_sums(s, cnt, order.data(), r1a_block_len), cvoff = block_sums(s, cnt, order.data(), n_rows),
      croff = block_sums(s, cnt, order.data(), n_tri);
   std::vector<long long> zoff((size_t) cnt);
   hs_r1a_layout L;
   hs_r1a_layout_make(m, cnt, nsm, R1A_TABW, SCLR_SJOBW, SCLR_JOBW, cvoff[cnt], croff[cnt], start[cnt], &L);
   for (int j = 0; j < cnt; ++j)
      zoff[j] = L.blocks + start[j] + (j < nlg ? cm_large_block(hs_solver_block_n(s, order[j])).ws : 0);
   hs_solver_cut_ws w;
   HS_CALL( hs_solver_cut_blocks(s, order, zoff, L.len.dev_len, L.len.pin_len, &w) );
   hipStream_t st = w.stream;
   if ( m > 0 )
      memcpy(w.pin + L.y, y, (size_t) m * sizeof(double));
   hs_r1a_job* htab = reinterpret_cast<hs_r1a_job*>(w.pin + L.tab);
   hs_eig_job* hej = reinterpret_cast<hs_eig_job*>(w.pin + L.ejobs);
   hs_sxm_job* hsx = reinterpret_cast<hs_sxm_job*>(w.pin + L.jobs);
   int* hact = reinterpret_cast<int*>(w.pin + L.act);
   for (int j = 0; j < cnt; ++j)
   {
      const int n = hs_solver_block_n(s, order[j]);
      double* base = w.dev + L.blocks + start[j];
      hs_r1a_job& T = htab[j];
      T.voff = cvoff[j]; T.roff = croff[j];
      if ( j < nlg )
      {
         const hs_ecl_block E = cm_large_block(n);
         HS_CALL( sxm_job(hs_syevx_many_job, n, base + E.ws, base + E.out, HS_SXM_ACTIVE | HS_SXM_VEC, &hsx[j], &hact[j]) );
         T.lam = base + E.out + HS_SYEVX_OUT_LAM; T.vec = base + E.out + HS_SYEVX_OUT_VEC; T.sign = -1.0;
         continue;
      }
      hs_eig_job& E = hej[j - nlg];
      memset(&E, 0, sizeof(E));
      E.n = n; E.in = base; E.ws = base + hs_cut_mat_len(n);
      T.lam = E.ws + (n - 1); T.vec = E.ws + hs_syev_many_vecpos(n) + (long long) (n - 1) * n; T.sign = 1.0;
   }
   HS_HIP( hipMemcpyAsync(w.dev, w.pin, (size_t) L.len.upload_len * sizeof(double), hipMemcpyHostToDevice, st) );
   int launches = 0;
   HS_CALL( hs_ec_form_z(st, cnt, nmax, m, w.djobs, w.dev + L.y) );
   ++launches;
   if ( nsm > 0 )
      HS_CALL( scx_syev(st, nsm, hej, reinterpret_cast<const hs_eig_job*>(w.dev + L.ejobs), &launches) );
   if ( nlg > 0 )
   {
      const hs_sxm_job* dsx = reinterpret_cast<const hs_sxm_job*>(w.dev + L.jobs);
      const int* dact = reinterpret_cast<const int*>(w.dev + L.act);
      HS_CALL( hs_r1_negate(st, nlg, nmax_large, dsx) );
      HS_CALL( hs_syevx_many_cols(st, nlg, nmax_large, hs_syevx_many_cap(nlg), dsx, dact) );
      HS_CALL( hs_syevx_many_select(st, nlg, nmax_large, 0, dsx, dact) );
      launches += 1 + (nmax_large - 1) + 3;
   }
   HS_CALL( hs_r1_rhs(st, cnt, nmax, w.djobs, reinterpret_cast<const hs_r1a_job*>(w.dev + L.tab), w.dev + L.lmax, w.dev + L.vec, w.dev + L.rhs) );
   ++launches;
   if ( launches != hs_r1a_launches(nsm > 0, nmax_large) )
      return HIPSDP_ERR_NUMERIC;
   HS_CALL( chunk_readback(w, L.len, launches, &g_r1a) );
   for (int j = 0; j < cnt; ++j)
   {
      const int b = order[j], n = hs_solver_block_n(s, b);
      lmax[b] = w.pin[L.lmax + j];
      memcpy(vec + voff[b], w.pin + L.vec + cvoff[j], (size_t) n * sizeof(double));
      memcpy(rhs + roff[b], w.pin + L.rhs + croff[j], (size_t) n * (n + 1) / 2 * sizeof(double));
   }
   return HIPSDP_OK;
}

int rank1_approx_impl(hipsdp_solver* s, const double* y, const int* want, double* lmax, double* vec, double* rhs, int* served)
{
   int m = 0, nb = 0;
   if ( !hs_solver_dims(s, &m, &nb) || y == NULL || lmax == NULL || vec == NULL || rhs == NULL )
      return HIPSDP_ERR_ARG;
   if ( served != NULL )
      for (int b = 0; b < nb; ++b)
         served[b] = (want == NULL || want[b] != 0) ? -1 : 1;
   std::vector<int> all, ids;
   HS_CALL( hs_solver_cut_enter_large(s, HS_SYEVX_MAXN, &all) );
   for (int b : all)
      if ( want == NULL || want[b] != 0 )
         ids.push_back(b);
   if ( ids.empty() )
      return HIPSDP_OK;
   std::stable_sort(ids.begin(), ids.end(), [&](int a, int c) { return hs_solver_block_n(s, a) > hs_solver_block_n(s, c); });
   const std::vector<long long> voff = block_sums(s, nb, NULL, n_rows), roff = block_sums(s, nb, NULL, n_tri);
   const int total = (int) ids.size();
   std::vector<long long> job_len((size_t) total);
   for (int k = 0; k < total; ++k)
   {
      const long long n = hs_solver_block_n(s, ids[k]);
      job_len[k] = r1a_block_len((int) n) + n + n * (n + 1) / 2 + R1A_TABW + SCLR_JOBW + 2;
   }
   HS_CALL( hs_chunks_run(job_len.data(), total, SCLR_BUDGET, hs_chunk_env("HIPSDP_RANK1_APPROX_CHUNK"), [&](int start, int end)
      {
         const std::vector<int> chunk(ids.begin() + start, ids.begin() + end);
         return r1a_chunk(s, m, chunk, y, voff, roff, lmax, vec, rhs);
      }) );
   if ( served != NULL )
      for (int b : ids)
         served[b] = 0;
   ++g_r1a.calls;
   return HIPSDP_OK;
}

}

extern "C" int hipsdp_rank1_approx(hipsdp_solver* s, const double* y, const int* want, double* lmax, double* vec, double* rhs, int* served)
{
   return rank1_approx_impl(s, y, want, lmax, vec, rhs, served);
}

extern "C" int hipsdp_rank1_approx_stats(long long* calls, long long* launches, long long* readbacks)
{
   return g_r1a.get(calls, launches, readbacks);
}
