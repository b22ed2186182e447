/* ipm.hip - the interior-point engine: homogeneous self-dual embedding, HKM direction, Mehrotra predictor-corrector.
 *
 * Replaces the third-party arithmetic behind the reference's backends (DSDPSetup/DSDPSolve/DSDPComputeX at
 * src/sdpi/sdpisolver_dsdp.c:1489-1520; SDPA::initializeSolve/solve at src/sdpi/sdpisolver_sdpa.cpp:1600-1670).
 * oracle/ipm_ref.py is the line-by-line CPU restatement used by the parity tests.
 *
 * Per iteration, per dense block (n x n, m1 = m + 1 matrices A_0..A_m stored as rows of length n^2):
 *    chol(Z), Z^-1, chol(X)                                       chol.hip   (MFMA panels)
 *    Schur  Mx_ij = tr(A_i X A_j Z^-1), i, j = 0..m               three MFMA GEMMs (below)
 *    chol(M), M = Mx[1:,1:]; solves                               chol.hip
 *    predictor / corrector right-hand sides and directions        2 passes over A each (kernels.hip) + 4 n^3 GEMMs
 *    step lengths  lambda_min(L^-1 dX L^-T)                       eig.hip (Lanczos)
 * The host thread only reads back a few dozen scalars three times per iteration and decides sigma / alpha / termination.
 */
#include "hs_kernels.h"
#include "hs_gram_cache.h"
#include "hs_sp_master.h"
#include "../../include/hipsdp.h"
#include <rocprofiler-sdk-roctx/roctx.h>
#include <vector>
#include <atomic>
#include <utility>
#include <functional>
#include <chrono>
#include <algorithm>
#include <cmath>
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <cstring>

/* ---- device scalar slots -------------------------------------------------------------------------------------- */
enum
{
   SC_AX0 = 0,     /* <A_0, X> + c^T x */
   SC_DOBJ,        /* b^T y */
   SC_XZ,          /* sum <X, Z> + x^T z */
   SC_RP2,         /* ||rp||^2 */
   SC_RD2,         /* sum_k ||Rd_k||_F^2 + ||rd||^2 */
   SC_RDLPMAX,     /* max |rd| */
   SC_HP2,         /* ||A(X, x)||^2 */
   SC_HD2,         /* ||A^T y - Z||^2 (certificate) */
   SC_S0,
   SC_BUB,         /* b^T M^-1 b */
   SC_BH,          /* sum <B_k, H_k> + beta^T hl */
   SC_WRP,         /* w^T rp */
   SC_BU1,         /* b^T u1 */
   SC_DTAU,
   SC_DKAPPA,
   SC_RATX,        /* LP ratio tests */
   SC_RATZ,
   SC_DEN,
   SC_FIXED_END = 24
};
/* per block k: SC_FIXED_END + 8 k + {0: ||Rd_k||^2, 1..3: lanczos X (theta, resid, steps), 4..6: lanczos Z} */
#define SC_BLK(k, i) (SC_FIXED_END + 8 * (k) + (i))

struct Block
{
   int     n;
   double* A;        /* (m + 1) x n^2: row i at A + i n^2.  Matrices sharded by variable: only the rows [a_r0, a_r1) of the solver exist
                      * (A = Aown - a_r0 n^2 is the address row 0 WOULD have) */
   double* Aown;     /* the allocation behind A */
   double* A0;       /* the constant matrix (row 0): A itself, or a replicated copy on the ranks that do not own row 0 */
   double* A0sep;    /* that copy (NULL where A0 == A) */
   double* Apkown;   /* the allocation behind Apk */
   double *X, *Z, *Rd, *Lz, *LzInv, *Zinv, *Lx, *LxInv, *B, *H, *G, *GZ, *dXa, *dZa, *dX, *dZ, *E, *W, *T1;
   double *dinvz, *dinvx;
   double *Xs, *Zs;  /* saved iterate for step back-off */
   double *T2, *W2;  /* scratch of the second queue */
   double *Xpre;     /* X of the preoptimal iterate (allocated at the first capture) */
   double *P2;       /* A^T([1; u2]): the part of dZ that multiplies dtau, the same for predictor and corrector (allocated on first use) */
   double *pk3;      /* 3 Lp: packed outputs of the three-vector sweep (allocated on first use) */
   double *Apk;      /* (m + 1) x Lp packed lower copy of A for the HBM-bound passes; NULL when memory is short */
   double *pkv;      /* 2 Lp: packed vector in / out */
   long long Lp;
   bool apk_valid;
   unsigned long long A_gen;   /* generation of the matrices (hs_gram_cache.h): a new number from every writer of A / A0 (a_written) */
   bool a_escaped;       /* the caller holds a device pointer to A (hipsdp_block_device_ptr) and may write at any time: never cached */
   bool derived_valid;   /* n <= 64: LxInv, LzInv (and Zinv for n <= 32) belong to the current X, Z (written by the fused factorization) */
   /* SPARSE mode (csrc/sparse.hip): the matrices of the variables are kept as the caller's nonzeros - A is NULL, A0 a dense n x n
    * array of its own; the triplets are collected on the host (sph) and built into the device structure sp before they are used */
   bool sparse;
   bool sp_dirty;
   hs_sparse* sp;
   struct SpHost* sph;
   /* sp was built on the device by hipsdp_master_gather from the triplet master block sp_master and lives in that block's workspace:
    * there are no host triplets behind it (hipsdp_add_entries takes the constant matrix only until the next set_shape) */
   bool sp_gathered;
   int sp_master;
};

struct SpHost
{
   std::vector<int> var, row, col;
   std::vector<double> val;
};

/* phases of an iteration: roctx ranges for rocprofv3 --marker-trace (always) and, with hipsdp_set_profiling, HIP events on the
 * main stream whose intervals are summed per phase (hipsdp_get_phase_times) */
enum { PH_RESID = 0, PH_FACTOR, PH_SCHUR, PH_MSOLVE, PH_PRED, PH_CORR, PH_UPDATE, PH_COUNT };
static const char* const g_phase_names[PH_COUNT] = {"residuals", "factorizations", "schur", "chol_M_solves", "predictor", "corrector",
   "update"};

struct PhaseClock
{
   bool on;
   int open;                                          /* phase whose roctx range is open, or -1 */
   std::vector<hipEvent_t> pool;
   std::vector<std::pair<int, hipEvent_t> > marks;
   double ms[PH_COUNT];
};

/* The workspace of the cut calls (csrc/cut_calls.hip, csrc/onevar.hip; layouts: hs_cut_plan.h), grow-only and
 * kept until hipsdp_free: the device buffer, its pinned host mirror (upload and read-back), the job tables on the device (the hs_ec_job
 * of a round and behind them their hs_eig_job) and the host copies they were uploaded from. */
struct CutWs
{
   double* dev = NULL; long long dev_len = 0;
   double* pin = NULL; long long pin_len = 0;
   char* tab = NULL; long long tab_len = 0;
   std::vector<hs_ec_job> jobs; std::vector<hs_eig_job> ejobs;

   /* *p (len units of `unit` bytes) holds at least `need` units afterwards; nothing is kept across a reallocation */
   static int regrow(void** p, long long* len, long long need, size_t unit, bool pinned)
   {
      if ( need <= *len )
         return HS_OK;
      if ( *p != NULL ) HS_HIP( pinned ? hipHostFree(*p) : hipFree(*p) );
      *p = NULL; *len = 0;
      HS_HIP( pinned ? hipHostMalloc(p, (size_t) need * unit, hipHostMallocDefault) : hipMalloc(p, (size_t) need * unit) );
      *len = need;
      return HS_OK;
   }
   /* lengths in doubles, the tables in bytes; a reallocated table forgets what it held */
   int grow(long long dev_need, long long pin_need, size_t tab_bytes)
   {
      HS_CALL( regrow((void**) &dev, &dev_len, dev_need, sizeof(double), false) );
      HS_CALL( regrow((void**) &pin, &pin_len, pin_need, sizeof(double), true) );
      if ( (long long) tab_bytes > tab_len ) { jobs.clear(); ejobs.clear(); }
      return regrow((void**) &tab, &tab_len, (long long) tab_bytes, 1, false);
   }
   /* the tables of a round (je may be empty), uploaded when they differ from what the device holds: first use, a new shape, another
    * storage form, a workspace laid out differently */
   int upload(const std::vector<hs_ec_job>& j, const std::vector<hs_eig_job>& je)
   {
      if ( jobs.size() == j.size() && memcmp(jobs.data(), j.data(), j.size() * sizeof(hs_ec_job)) == 0 )
         return HS_OK;
      HS_HIP( hipMemcpy(tab, j.data(), j.size() * sizeof(hs_ec_job), hipMemcpyHostToDevice) );
      if ( !je.empty() )
         HS_HIP( hipMemcpy(tab + j.size() * sizeof(hs_ec_job), je.data(), je.size() * sizeof(hs_eig_job), hipMemcpyHostToDevice) );
      jobs = j; ejobs = je;
      return HS_OK;
   }
   const hs_ec_job* djobs() const { return reinterpret_cast<const hs_ec_job*>(tab); }
   const hs_eig_job* dejobs() const { return reinterpret_cast<const hs_eig_job*>(tab + jobs.size() * sizeof(hs_ec_job)); }
   /* the two further tables of the rounds of csrc/sparsecuts_rounds.hip, in a buffer of their own under the same rules: the hs_scr_job of
    * the blocks (in the order of `jobs`) and behind them the hs_eig_job of their Z_S (ordered by decomposition class) */
   char* rtab = NULL; long long rtab_len = 0;
   std::vector<hs_scr_job> xjobs; std::vector<hs_eig_job> sjobs;
   int upload_rounds(const std::vector<hs_scr_job>& x, const std::vector<hs_eig_job>& sj)
   {
      const size_t xb = x.size() * sizeof(hs_scr_job), sb = sj.size() * sizeof(hs_eig_job);
      if ( (long long) (xb + sb) > rtab_len ) { xjobs.clear(); sjobs.clear(); }
      HS_CALL( regrow((void**) &rtab, &rtab_len, (long long) (xb + sb), 1, false) );
      if ( xjobs.size() == x.size() && sjobs.size() == sj.size() && memcmp(xjobs.data(), x.data(), xb) == 0
         && memcmp(sjobs.data(), sj.data(), sb) == 0 )
         return HS_OK;
      HS_HIP( hipMemcpy(rtab, x.data(), xb, hipMemcpyHostToDevice) );
      HS_HIP( hipMemcpy(rtab + xb, sj.data(), sb, hipMemcpyHostToDevice) );
      xjobs = x; sjobs = sj;
      return HS_OK;
   }
   const hs_scr_job* dxjobs() const { return reinterpret_cast<const hs_scr_job*>(rtab); }
   const hs_eig_job* dsjobs() const { return reinterpret_cast<const hs_eig_job*>(rtab + xjobs.size() * sizeof(hs_scr_job)); }
   /* what a cut call works with (hs_kernels.h): the buffers and the tables of `upload`, those of the rounds unset */
   void view(hipStream_t st, hs_solver_cut_ws* w) const
   {
      memset(w, 0, sizeof(*w));
      w->stream = st; w->dev = dev; w->pin = pin;
      w->djobs = djobs(); w->dejobs = dejobs(); w->ejobs = ejobs.data();
   }
   void release()
   {
      if ( dev != NULL ) (void) hipFree(dev);
      if ( tab != NULL ) (void) hipFree(tab);
      if ( rtab != NULL ) (void) hipFree(rtab);
      if ( pin != NULL ) (void) hipHostFree(pin);
      dev = NULL; tab = NULL; rtab = NULL; pin = NULL;
   }
};

struct hipsdp_solver
{
   int device;
   hipStream_t stream;
   hipStream_t stream2;          /* second queue: the Z-side chains run beside the X-side ones (both are latency bound) */
   hipEvent_t evFork, evJoin;
   bool use2;                    /* false for tiny blocks: they are launch bound and the cross-queue events only add latency */
   bool busy2;                   /* stream2 has work that stream has not joined (fork2 / join2) */
   int m, q;
   int sparse_policy;            /* 0: blocks are never kept as nonzeros, 1: when the caller's count makes it cheaper, 2: whenever a count is given */
   std::vector<Block> blk;
   double* b;        /* m */
   double* Dext;     /* q x (m + 1) */
   /* iterate */
   double *y, *x, *z;
   double tau, kappa;
   /* work vectors */
   double *yt, *dyt, *wt, *AX, *AH, *tmpe, *rp, *rd, *tmpq, *hl, *beta, *elp, *dxa, *dza, *dx, *dz, *xs, *zs, *ys;
   double *u1, *rhs2, *u2, *dy, *dya;
   double *cvec;           /* 2 (m + 1): coefficient vectors [1; u2] and [0; u1] of the split dZ = A^T([0; u1]) - dtau A^T([1; u2]) + eta Rd */
   double *Mx, *Lm, *dinvm, *Slp;
   double *pre_y, *pre_x;  /* preoptimal iterate (params.preoptgap): y and the LP multipliers; X per block in Block::Xpre */
   bool pre_valid;
   double pre_scale;       /* 1 / tau at the capture */
   int* regmask;           /* forced pivots of the last factorization of M (semidefinite pivot rule) */
   double *sc, *red_ws, *gemv_ws, *lan_ws, *lan_ws2;
   double* gemvt_ws;                   /* row-chunk partial sums of the passes A^T over blocks with few entries (hs_gemv_t_ws) */
   long long gemvt_ws_len;
   double* hsc;            /* pinned, device-visible host mirror of sc followed by the flags and a sequence number: the last kernel
                            * before a read-back stores the scalars there itself and the host waits for the number */
   double* hsc_dev;        /* device view of hsc */
   unsigned long long pub_seq;
   long long hsc_cap;      /* doubles; kept across re-shapes (pinned allocations are slow) */
   int* trsv_ws;           /* block flags of the multi-workgroup triangular solves */
   int trsv_epoch;
   int lan_rot[2];                     /* which exchange vector of the one-launch Lanczos runs is the clean one (eig.hip) */
   unsigned long long* lan_sync;       /* device: error word + exchange vectors per matrix of a pair */
   long long gemv_ws_len;
   int* flags;       /* device ints: 0 chol Z, 1 chol X, 2 chol M */
   hs_schur_ws sws;
   bool schur_mode_U, schur_mode_rows;
   bool schur_mode_cols;        /* several ranks (or HIPSDP_SCHUR=K<shards>): column slices of the W formulation + all-reduce */
   int  schur_sim_shards;       /* HIPSDP_SCHUR=K<shards> without a communicator: all slices on this device, one after the other */
   bool schur_mode_forced;      /* HIPSDP_SCHUR set: the single-launch assembly of small problems is not used either */
   double* Mgather;
   long long mx_rows;
   int nsc;
   bool shaped, solved, have_start;
   int last_status;
   double sol_scale;
   hipEvent_t ev0, ev1;
   /* device-resident master copy of the constraint matrices in ORIGINAL indices (survives set_shape) */
   int master_nvars;
   std::vector<int> master_sizes;
   std::vector<int> master_slots;         /* per master block: number of variable slots */
   std::vector<double*> master_A;         /* NULL for a block kept as triplets ... */
   std::vector<hs_spm*> master_sp;        /* ... which lives here (csrc/sp_master.hip); NULL for a dense block */
   long long mg_device_builds, mg_host_builds, mg_launches, mg_readbacks;      /* hipsdp_master_gather_stats */
   /* multi GPU */
   void* comm; int rank, nranks;
   double* passg;          /* gather buffer of the row-sharded passes: nranks * ceil(m1 / nranks) doubles */
   int shard_passes;       /* -1: by size (>= 64 MB per pass), 0 / 1: HIPSDP_SHARD_PASSES */
   int shardA_req;         /* hipsdp_shard_matrices: 0 replicated (default), 1 by variable, -1 by size against the free memory */
   int var_cw;             /* matrices sharded by variable: columns per slice of the Schur assembly */
   bool var_overlap;       /* ... and the all-to-all of a slice runs on the second queue beside the products of the next one */
   bool shardA;            /* decided by set_shape: this problem's constraint matrices are sharded by variable */
   int a_r0, a_r1;         /* rows of A (0 = constant matrix, i = variable i) this rank holds; [0, m + 1) when replicated */
   hipsdp_params par;
   PhaseClock pc;
   /* shader clock during the Schur assemblies (hipsdp_set_clock_sampling): 4 words per assembly */
   bool clk_on; unsigned long long* clk_buf; int clk_n; double clk_ghz; hipStream_t clk_stream;
   /* one-launch solve of B&B-sized problems (csrc/solve1.hip) */
   double* s1_ws;          /* device workspace (cold matrices and nonzero lists that do not fit into LDS) */
   long long s1_ws_len;
   double* s1_host;        /* pinned, device-visible: HS_S1_OUT_DOUBLES result scalars, then the sequence word, then the history */
   double* s1_host_dev;
   bool s1_sol_host;       /* y, x, z of the last solve are in s1_host too (offset S1_SOL_OFF): hipsdp_get_y / get_lp copy from there */
   bool zero_b, zero_D;    /* set_shape (same shape again) owes b / Dext their zeros: paid by set_obj / set_lp overwriting them, or before the next use */
   /* staging arena of the small uploads of a node (objective, LP rows, gather indices, triplets of the constant matrices, start
    * point): pinned, device-visible; a setter copies its data there and queues an asynchronous copy or a kernel that reads the
    * arena directly - nothing waits.  stage_pending: something queued on `stream` has not been waited for yet (every entry point
    * that touches device data outside that queue calls stage_sync first).  The offset returns to 0 when the queue has drained
    * (set_shape, end of a solve). */
   char* arena_h; char* arena_d; size_t arena_cap, stage_off; bool stage_pending;
   int m_alloc, q_alloc;   /* what the vectors and matrices indexed by variables / LP rows were allocated for (>= m, q: set_shape2) */
   int ncmd;               /* commands of the node's setters waiting in the arena (run by ONE launch before the solve, see NodeCmd) */
   hipEvent_t cmd_ev;      /* recorded behind a flushed command list: the launch reads the list from the arena when it RUNS, so the */
   bool cmd_inflight;      /* slots must not be written again before it has (cmd_new waits for the event) */
   unsigned long long s1_seq;
   int s1_last;            /* 1: the last solve ran in the single launch */
   /* the lanes of hipsdp_solve_objectives (objs_lanes): device part and pinned, device-visible part, grow-only; every call lays
    * them out for its shape and count.  They go with the problem's buffers: hipsdp_free, or a hipsdp_set_shape that does not keep
    * the allocations of the shape before.  ln_seq: their sequence numbers */
   double* ln_dev; long long ln_dev_len;
   double* ln_host; double* ln_host_dev; long long ln_host_len;
   unsigned long long ln_seq;
   /* pinned / device staging chunks of hipsdp_master_add_vars (kept until hipsdp_free) */
   void* stage_h[2]; void* stage_d[2]; hipEvent_t stage_ev[2]; long long stage_cap;
   CutWs cw;               /* the calls of csrc/cut_calls.hip and csrc/onevar.hip, through hs_solver_cut_* below */
   hs_round_frame rframe;  /* hipsdp_rounding_frame / hipsdp_rounding_recombine (csrc/cut_calls.hip), through hs_solver_round_frame below */
   /* the first assembly of a cold solve, kept across solves of the same matrices (hs_gram_cache.h; GeneralSolve::assemble_forms):
    * gc_M holds (m1 + 32) m1 doubles as the identity assemblies left them in Mx, gc_key says of what.  Allocated at the first cold
    * solve that qualifies (gc_nomem: that failed for this shape, not tried again), freed with the problem. */
   unsigned long long a_gen_next;
   double* gc_M; long long gc_len; bool gc_nomem;
   hs_gram_key gc_key;
   long long gc_hits, gc_misses;
};

/* EVERY writer of a dense block's constraint matrices (rows of A, the constant matrix A0 included) ends here: the packed copy is
 * stale and the matrices are a new generation - a cached Gram matrix of the old one no longer matches */
static void a_written(hipsdp_solver* s, Block& B)
{
   B.apk_valid = false;
   B.A_gen = hs_gen_next(&s->a_gen_next);
}

void hs_comm_phase(int phase);      /* multi.hip: the phase the next collectives are booked under */

static void phase_mark(hipsdp_solver* s, int ph)
{
   if ( s->pc.open >= 0 )
      (void) roctxRangePop();
   s->pc.open = ph;
   if ( ph >= 0 )
      (void) roctxRangePushA(g_phase_names[ph]);
   if ( !s->pc.on )
      return;
   hipEvent_t e = NULL;
   if ( !s->pc.pool.empty() )
   {
      e = s->pc.pool.back();
      s->pc.pool.pop_back();
   }
   else if ( hipEventCreate(&e) != hipSuccess )
      return;
   if ( hipEventRecord(e, s->stream) == hipSuccess )
      s->pc.marks.push_back(std::make_pair(ph, e));
   else
      s->pc.pool.push_back(e);
}

/* with profiling on: turns the recorded marks (the last one being the closing phase_mark(s, -1)) into per-phase sums; the
 * stream must be idle */
static void phase_finish(hipsdp_solver* s)
{
   for (size_t i = 0; i + 1 < s->pc.marks.size(); ++i)
   {
      float ms = 0.f;
      const int ph = s->pc.marks[i].first;
      if ( ph >= 0 && hipEventElapsedTime(&ms, s->pc.marks[i].second, s->pc.marks[i + 1].second) == hipSuccess )
         s->pc.ms[ph] += (double) ms;
   }
   for (auto& mk : s->pc.marks)
      s->pc.pool.push_back(mk.second);
   s->pc.marks.clear();
}

extern "C" const char* hipsdp_phase_name(int phase)
{
   return phase >= 0 && phase < PH_COUNT ? g_phase_names[phase] : "";
}

extern "C" int hipsdp_set_profiling(hipsdp_solver* s, int on)
{
   if ( s == NULL )
      return HIPSDP_ERR_ARG;
   s->pc.on = on != 0;
   return HIPSDP_OK;
}

extern "C" int hipsdp_get_phase_times(hipsdp_solver* s, double* ms)
{
   if ( s == NULL || ms == NULL )
      return HIPSDP_ERR_ARG;
   for (int p = 0; p < PH_COUNT; ++p)
      ms[p] = s->pc.ms[p];
   return HIPSDP_OK;
}

static thread_local char g_err[512] = "";
static int g_live_solvers = 0;      /* handles alive in this process: the device memory pool is trimmed when the last one goes */
static void set_err(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }

extern "C" const char* hipsdp_last_error(void)
{
   const char* h = hs_last_error();
   if ( g_err[0] != 0 )
      return g_err;
   return h;
}

extern "C" const char* hipsdp_version(void) { return "hipsdp 0.1 (gfx950)"; }

extern "C" int hipsdp_device_count(void)
{
   int n = 0;
   if ( hipGetDeviceCount(&n) != hipSuccess )
      return 0;
   return n;
}

extern "C" void hipsdp_default_params(hipsdp_params* p)
{
   p->gaptol = 1e-5;
   p->feastol = 1e-5;
   p->infeastol = 1e-7;
   p->objlimit = 1e20;
   p->timelimit = 0.0;
   p->gamma = 0.98;
   p->ws_gbytes = 0.0;
   p->maxiter = 100;
   p->verbose = 0;
   p->lanczos_steps = 0;        /* by block size: 24, or 16 when every block has more than 64 rows */
   p->settings = 0;
   p->pabstol = 0.0;
   p->preoptgap = 0.0;
}

template<class T>
static int dalloc(T** p, long long count)
{
   *p = NULL;
   if ( count <= 0 )
      count = 1;
   return hs_pool_alloc((void**) p, (size_t) count * sizeof(T));
}

static void dfree(void* p) { hs_pool_free(p); }

#define STAGE_BYTES (2u << 20)
/* ---- the setters of a node, deferred.  A B&B node is loaded by five or six small calls (clear, objective, gather of the active
 * matrices from the master copy, triplets of the constant matrix, LP rows, start point).  As separate copies and launches they
 * cost 4-6 us of host time each and as much again on the device's queue, one behind the other - a tenth of the solve of such a
 * node.  Instead each call leaves its data and a command in the pinned arena, and ONE launch of one workgroup runs the commands in
 * order just before the solve (or before anything else touches the device data: stage_sync).  Large operands keep the direct path. */
__global__ void __launch_bounds__(1024) k_node_cmds(const NodeCmd* __restrict__ cmds, int ncmd)
{
   __shared__ NodeCmd sc[NC_MAX];
   hs_run_node_cmds(cmds, ncmd, sc);
}

/* room for `bytes` in the staging arena: host address (NULL: does not fit - the caller takes its blocking path), *dev = the same
 * bytes as the device sees them.  The first NC_BYTES of the arena hold the command list. */
static void* stage_take(hipsdp_solver* s, size_t bytes, void** dev)
{
   if ( getenv("HIPSDP_NO_STAGING") != NULL )
      return NULL;
   if ( s->arena_h == NULL )
   {
      void* h = NULL; void* d = NULL;
      if ( hipHostMalloc(&h, STAGE_BYTES, hipHostMallocMapped) != hipSuccess )
         return NULL;
      if ( hipHostGetDevicePointer(&d, h, 0) != hipSuccess )
      {
         (void) hipHostFree(h);
         return NULL;
      }
      s->arena_h = (char*) h; s->arena_d = (char*) d; s->arena_cap = STAGE_BYTES; s->stage_off = 0; s->ncmd = 0;
   }
   if ( s->stage_off < NC_BYTES )
      s->stage_off = NC_BYTES;
   const size_t off = (s->stage_off + 63) & ~(size_t) 63;
   if ( off + bytes > s->arena_cap )
      return NULL;
   s->stage_off = off + bytes;
   if ( dev != NULL )
      *dev = s->arena_d + off;
   return s->arena_h + off;
}
/* launch the waiting commands (no wait) */
static int flush_cmds(hipsdp_solver* s)
{
   if ( s->ncmd > 0 )
   {
      hipLaunchKernelGGL(k_node_cmds, dim3(1), dim3(1024), 0, s->stream, reinterpret_cast<const NodeCmd*>(s->arena_d), s->ncmd);
      HS_LAUNCH_CHECK();
      s->ncmd = 0;
      s->stage_pending = true;
      /* the kernel fetches the list when it runs, not when it is queued: whoever writes slot 0 next waits for this event */
      if ( s->cmd_ev == NULL )
         HS_HIP( hipEventCreateWithFlags(&s->cmd_ev, hipEventDisableTiming) );
      HS_HIP( hipEventRecord(s->cmd_ev, s->stream) );
      s->cmd_inflight = true;
   }
   return HIPSDP_OK;
}
/* a slot for one more command (NULL: the arena is not available, the caller takes its direct path) */
static NodeCmd* cmd_new(hipsdp_solver* s)
{
   if ( s->arena_h == NULL && stage_take(s, 0, NULL) == NULL )
      return NULL;
   if ( s->ncmd >= NC_MAX && flush_cmds(s) != HIPSDP_OK )
      return NULL;
   if ( s->cmd_inflight )
   {
      /* a flushed list may not have been fetched yet (large gathers / clears flush in the middle of a node's setters) */
      if ( hipEventSynchronize(s->cmd_ev) != hipSuccess )
         return NULL;
      s->cmd_inflight = false;
   }
   NodeCmd* q = reinterpret_cast<NodeCmd*>(s->arena_h) + s->ncmd;
   memset(q, 0, sizeof(*q));
   ++s->ncmd;
   return q;
}
/* host -> device of a small array: data and a copy command into the arena; falls back to a blocking copy */
static int stage_upload(hipsdp_solver* s, void* dst, const void* src, size_t bytes)
{
   if ( bytes == 0 )
      return HIPSDP_OK;
   void* dv = NULL;
   void* h = (bytes <= NC_LIMIT * sizeof(double)) ? stage_take(s, bytes, &dv) : NULL;
   NodeCmd* q = (h != NULL) ? cmd_new(s) : NULL;
   if ( q == NULL )
   {
      HS_CALL( flush_cmds(s) );
      HS_HIP( hipStreamSynchronize(s->stream) );
      HS_HIP( hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice) );
      return HIPSDP_OK;
   }
   memcpy(h, src, bytes);
   q->op = NC_COPY; q->n = (long long) (bytes / sizeof(double)); q->dst = (double*) dst; q->src = (const double*) dv;
   return HIPSDP_OK;
}
/* before anything outside the solver's stream touches device data: wait for what the setters queued */
/* clear `count` doubles, in order with the waiting commands */
static int stage_zero(hipsdp_solver* s, double* dst, long long count)
{
   if ( count <= 0 )
      return HIPSDP_OK;
   NodeCmd* q = (count <= NC_LIMIT) ? cmd_new(s) : NULL;
   if ( q != NULL )
   {
      q->op = NC_ZERO; q->n = count; q->dst = dst;
      return HIPSDP_OK;
   }
   HS_CALL( flush_cmds(s) );
   HS_HIP( hipMemsetAsync(dst, 0, (size_t) count * sizeof(double), s->stream) );
   s->stage_pending = true;
   return HIPSDP_OK;
}
static int flush_zeros(hipsdp_solver* s)
{
   if ( s->zero_b )
   {
      HS_CALL( stage_zero(s, s->b, s->m) );
      s->zero_b = false;
   }
   if ( s->zero_D )
   {
      HS_CALL( stage_zero(s, s->Dext, (long long) s->q * (s->m + 1)) );
      s->zero_D = false;
   }
   return HIPSDP_OK;
}
static int stage_sync(hipsdp_solver* s)
{
   if ( s != NULL && (s->zero_b || s->zero_D) )
      HS_CALL( flush_zeros(s) );
   if ( s != NULL && s->ncmd > 0 )
      HS_CALL( flush_cmds(s) );
   if ( s != NULL && s->stage_pending )
   {
      HS_HIP( hipStreamSynchronize(s->stream) );
      s->stage_pending = false;
      s->stage_off = 0;
      s->cmd_inflight = false;
   }
   return HIPSDP_OK;
}

static void free_sparse(Block& B)
{
   if ( B.sp != NULL ) hs_sp_free(B.sp);
   B.sp = NULL;
   delete B.sph;
   B.sph = NULL;
}

static void free_problem(hipsdp_solver* s)
{
   /* blocks go back to a pool that hands them out again without a device synchronisation: nothing may still be running on them */
   if ( s->stream != NULL ) (void) hipStreamSynchronize(s->stream);
   if ( s->stream2 != NULL ) (void) hipStreamSynchronize(s->stream2);
   for (auto& B : s->blk)
   {
      double* ptrs[] = {B.Aown, B.A0sep, B.X, B.Z, B.Rd, B.Lz, B.LzInv, B.Zinv, B.Lx, B.LxInv, B.B, B.H, B.G, B.GZ, B.dXa, B.dZa, B.dX, B.dZ,
         B.E, B.W, B.T1, B.dinvz, B.dinvx, B.Xs, B.Zs, B.Apkown, B.pkv, B.T2, B.W2, B.Xpre, B.P2, B.pk3};
      for (double* p : ptrs) dfree(p);
      free_sparse(B);
   }
   s->blk.clear();
   double* ptrs[] = {s->b, s->Dext, s->y, s->x, s->z, s->yt, s->dyt, s->wt, s->AX, s->AH, s->tmpe, s->rp, s->rd, s->tmpq, s->hl,
      s->beta, s->elp, s->dxa, s->dza, s->dx, s->dz, s->xs, s->zs, s->ys, s->rhs2, s->cvec, s->u2, s->dy, s->dya, s->Mx, s->Lm,
      s->dinvm, s->Slp, s->sc, s->red_ws, s->gemv_ws, s->lan_ws, s->lan_ws2};
   for (double* p : ptrs) dfree(p);
   hs_schur_ws_free(&s->sws);
   if ( s->gc_M != NULL ) (void) hipFree(s->gc_M);
   s->gc_M = NULL; s->gc_len = 0; s->gc_nomem = false;
   hs_gram_key_clear(&s->gc_key);
   /* (the lanes of hipsdp_solve_objectives go with the problem they were laid out for) */
   if ( s->ln_dev != NULL ) (void) hipFree(s->ln_dev);
   if ( s->ln_host != NULL ) (void) hipHostFree(s->ln_host);
   s->ln_dev = NULL; s->ln_host = NULL; s->ln_host_dev = NULL; s->ln_dev_len = 0; s->ln_host_len = 0;
   dfree(s->Mgather);
   s->Mgather = NULL;
   dfree(s->passg);
   s->passg = NULL;
   dfree(s->trsv_ws);
   s->trsv_ws = NULL;
   dfree(s->gemvt_ws);
   s->gemvt_ws = NULL;
   s->gemvt_ws_len = 0;
   if ( s->lan_sync != NULL )
      (void) hipFree(s->lan_sync);
   s->lan_sync = NULL;
   dfree(s->regmask);
   s->regmask = NULL;
   dfree(s->pre_y); dfree(s->pre_x);
   s->pre_y = s->pre_x = NULL;
   s->pre_valid = false;
   s->b = s->Dext = s->y = s->x = s->z = s->yt = s->dyt = s->wt = s->AX = s->AH = s->tmpe = s->rp = s->rd = s->tmpq = s->hl = NULL;
   s->beta = s->elp = s->dxa = s->dza = s->dx = s->dz = s->xs = s->zs = s->ys = s->u1 = s->rhs2 = s->cvec = s->u2 = s->dy = s->dya = NULL;
   s->Mx = s->Lm = s->dinvm = s->Slp = s->sc = s->red_ws = s->gemv_ws = s->lan_ws = s->lan_ws2 = NULL;
   s->flags = NULL;
   s->rframe.valid = 0;          /* (the frame belongs to a shape) */
   s->rframe.served.clear();
   s->shaped = false;
   s->solved = false;
}

extern "C" int hipsdp_create(hipsdp_solver** out, int device)
{
   g_err[0] = 0;
   int nd = hipsdp_device_count();
   if ( nd <= 0 )
   {
      set_err("no HIP device available (hipsdp has no CPU fallback)");
      return HIPSDP_ERR_NODEVICE;
   }
   if ( device < 0 || device >= nd )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(device) );
   hipsdp_solver* s = new hipsdp_solver();
   memset((void*) &s->par, 0, sizeof(s->par));
   s->device = device;
   s->m = s->q = 0;
   s->b = s->Dext = s->y = s->x = s->z = NULL;
   s->shaped = s->solved = s->have_start = false;
   s->comm = NULL; s->rank = 0; s->nranks = 1;
   s->shardA_req = 0; s->shardA = false; s->a_r0 = 0; s->a_r1 = 1;
   s->passg = NULL;
   s->shard_passes = getenv("HIPSDP_SHARD_PASSES") != NULL ? atoi(getenv("HIPSDP_SHARD_PASSES")) : -1;
   s->master_nvars = 0;
   s->mg_device_builds = s->mg_host_builds = s->mg_launches = s->mg_readbacks = 0;
   s->Mgather = NULL;
   s->schur_mode_rows = false;
   s->schur_mode_cols = false; s->schur_sim_shards = 0;
   s->sws.T = s->sws.U = s->sws.K = s->sws.V = s->sws.U2 = s->sws.V2 = NULL;
   s->sws.evP[0] = s->sws.evP[1] = s->sws.evX[0] = s->sws.evX[1] = NULL; s->sws.ev_g2 = NULL; s->sws.after_g1 = NULL; s->sws.after_g1_arg = NULL;
   s->flags = NULL;
   s->hsc = NULL;
   s->hsc_dev = NULL;
   s->pub_seq = 0;
   s->hsc_cap = 0;
   s->clk_on = false; s->clk_buf = NULL; s->clk_n = 0; s->clk_ghz = 0.0; s->clk_stream = NULL;
   s->s1_ws = NULL; s->s1_ws_len = 0; s->s1_host = NULL; s->s1_host_dev = NULL; s->s1_seq = 0; s->s1_last = 0; s->s1_sol_host = false; s->zero_b = false; s->zero_D = false;
   s->arena_h = NULL; s->arena_d = NULL; s->arena_cap = 0; s->stage_off = 0; s->stage_pending = false; s->ncmd = 0; s->cmd_ev = NULL; s->cmd_inflight = false; s->m_alloc = 0; s->q_alloc = 0;
   s->ln_dev = NULL; s->ln_dev_len = 0; s->ln_host = NULL; s->ln_host_dev = NULL; s->ln_host_len = 0; s->ln_seq = 0;
   s->trsv_ws = NULL;
   s->a_gen_next = 0; s->gc_M = NULL; s->gc_len = 0; s->gc_nomem = false; s->gc_hits = s->gc_misses = 0;
   hs_gram_key_clear(&s->gc_key);
   s->pre_y = s->pre_x = NULL;
   s->pre_valid = false;
   s->pre_scale = 1.0;
   s->regmask = NULL;
   s->trsv_epoch = 0;
   s->lan_sync = NULL;
   s->lan_rot[0] = s->lan_rot[1] = 0;
   s->last_status = HIPSDP_STATUS_UNSOLVED;
   s->sol_scale = 1.0;
   s->pc.on = getenv("HIPSDP_PHASES") != NULL && atoi(getenv("HIPSDP_PHASES")) != 0;
   s->pc.open = -1;
   for (int p = 0; p < PH_COUNT; ++p) s->pc.ms[p] = 0.0;
   s->stage_h[0] = s->stage_h[1] = s->stage_d[0] = s->stage_d[1] = NULL;
   s->stage_ev[0] = s->stage_ev[1] = NULL;
   s->stage_cap = 0;
   s->b = s->Dext = s->y = s->x = s->z = s->yt = s->dyt = s->wt = s->AX = s->AH = s->tmpe = s->rp = s->rd = s->tmpq = s->hl = NULL;
   s->beta = s->elp = s->dxa = s->dza = s->dx = s->dz = s->xs = s->zs = s->ys = s->u1 = s->rhs2 = s->cvec = s->u2 = s->dy = s->dya = NULL;
   s->Mx = s->Lm = s->dinvm = s->Slp = s->sc = s->red_ws = s->gemv_ws = s->lan_ws = s->lan_ws2 = NULL;
   s->gemvt_ws = NULL;
   s->gemvt_ws_len = 0;
   hipsdp_default_params(&s->par);
   s->sparse_policy = getenv("HIPSDP_SPARSE") != NULL ? atoi(getenv("HIPSDP_SPARSE")) : 1;
   if ( s->sparse_policy < 0 || s->sparse_policy > 2 ) s->sparse_policy = 1;
   if ( hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess
      || hipStreamCreateWithFlags(&s->stream2, hipStreamNonBlocking) != hipSuccess
      || hipEventCreateWithFlags(&s->evFork, hipEventDisableTiming) != hipSuccess
      || hipEventCreateWithFlags(&s->evJoin, hipEventDisableTiming) != hipSuccess
      || hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess )
   {
      delete s;
      set_err("stream/event creation failed");
      return HIPSDP_ERR_HIP;
   }
   (void) __sync_add_and_fetch(&g_live_solvers, 1);
   *out = s;
   return HIPSDP_OK;
}

static void master_free(hipsdp_solver* s)
{
   /* a block gathered from a triplet master block points into that block's workspace: it goes with it (ensure_sparse then refuses
    * the block until it is loaded again) */
   for (auto& B : s->blk)
      if ( B.sparse && B.sp_gathered && B.sp != NULL )
      {
         hs_sp_free(B.sp);
         B.sp = NULL;
      }
   for (double* p : s->master_A) if ( p != NULL ) dfree(p);
   for (hs_spm* M : s->master_sp) hs_spm_free(M);
   s->master_sp.clear();
   s->master_A.clear();
   s->master_sizes.clear();
   s->master_slots.clear();
   s->master_nvars = 0;
}

extern "C" void hipsdp_free(hipsdp_solver** ps)
{
   if ( ps == NULL || *ps == NULL )
      return;
   hipsdp_solver* s = *ps;
   (void) hipSetDevice(s->device);
   (void) hipStreamSynchronize(s->stream);
   free_problem(s);
   master_free(s);
   if ( s->hsc != NULL ) (void) hipHostFree(s->hsc);
   s->hsc = NULL;
   if ( s->s1_host != NULL ) (void) hipHostFree(s->s1_host);
   s->s1_host = NULL;
   if ( s->arena_h != NULL ) (void) hipHostFree(s->arena_h);
   if ( s->cmd_ev != NULL ) (void) hipEventDestroy(s->cmd_ev);
   s->cmd_ev = NULL;
   s->arena_h = NULL; s->arena_d = NULL; s->arena_cap = 0;
   if ( s->s1_ws != NULL ) (void) hipFree(s->s1_ws);
   s->s1_ws = NULL;
   s->cw.release();
   if ( s->rframe.dev != NULL ) (void) hipFree(s->rframe.dev);
   s->rframe.dev = NULL; s->rframe.len = 0;
   if ( s->clk_buf != NULL ) (void) hipFree(s->clk_buf);
   s->clk_buf = NULL;
   if ( s->clk_stream != NULL ) (void) hipStreamDestroy(s->clk_stream);
   s->clk_stream = NULL;
   for (auto& mk : s->pc.marks) (void) hipEventDestroy(mk.second);
   for (hipEvent_t e : s->pc.pool) (void) hipEventDestroy(e);
   for (int b = 0; b < 2; ++b)
   {
      if ( s->stage_h[b] != NULL ) (void) hipHostFree(s->stage_h[b]);
      if ( s->stage_d[b] != NULL ) (void) hipFree(s->stage_d[b]);
      if ( s->stage_ev[b] != NULL ) (void) hipEventDestroy(s->stage_ev[b]);
   }
   (void) hipStreamSynchronize(s->stream2);
   (void) hipEventDestroy(s->ev0);
   (void) hipEventDestroy(s->ev1);
   (void) hipEventDestroy(s->evFork);
   (void) hipEventDestroy(s->evJoin);
   (void) hipStreamDestroy(s->stream2);
   (void) hipStreamDestroy(s->stream);
   delete s;
   *ps = NULL;
   if ( __sync_sub_and_fetch(&g_live_solvers, 1) <= 0 )
      hs_pool_trim();
}

/* which storage a block gets: sparse when the caller's nonzero count makes the pair formula the cheaper Schur assembly (never for
 * matrices sharded by variable: that mode exists for dense matrices that do not fit).  HIPSDP_SPARSE=0: never; =2: whenever a count
 * is given (tests) */
static bool block_wants_sparse(const hipsdp_solver* s, int n, int m, long long nnz)
{
   const int mode = s->sparse_policy;
   if ( mode == 0 || nnz < 0 || s->shardA_req > 0 )
      return false;
   if ( mode == 2 )
      return m >= 1;
   return hs_sp_prefers_sparse(n, m, nnz) != 0;
}

extern "C" int hipsdp_set_shape(hipsdp_solver* s, int m, int nblocks, const int* blocksizes, int q)
{
   return hipsdp_set_shape2(s, m, nblocks, blocksizes, q, NULL);
}

extern "C" int hipsdp_sparse_policy(hipsdp_solver* s, int mode)
{
   if ( s == NULL || mode < 0 || mode > 2 )
      return HIPSDP_ERR_ARG;
   s->sparse_policy = mode;
   return HIPSDP_OK;
}

extern "C" int hipsdp_func_attr_sets(int device)
{
   return hs_func_attr_sets(device);
}

extern "C" int hipsdp_mem_info(int device, double* free_bytes, double* total_bytes)
{
   int nd = 0;
   if ( hipGetDeviceCount(&nd) != hipSuccess || nd <= 0 )
      return HIPSDP_ERR_NODEVICE;
   if ( device < 0 || device >= nd )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(device) );
   size_t fr = 0, tot = 0;
   HS_HIP( hipMemGetInfo(&fr, &tot) );
   if ( free_bytes != NULL ) *free_bytes = (double) fr;
   if ( total_bytes != NULL ) *total_bytes = (double) tot;
   return HIPSDP_OK;
}

extern "C" int hipsdp_block_is_sparse(hipsdp_solver* s, int block)
{
   if ( s == NULL || !s->shaped || block < 0 || block >= (int) s->blk.size() )
      return 0;
   return s->blk[block].sparse ? 1 : 0;
}

extern "C" int hipsdp_set_shape2(hipsdp_solver* s, int m, int nblocks, const int* blocksizes, int q, const long long* nnz)
{
   g_err[0] = 0;
   if ( s == NULL || m < 0 || nblocks < 0 || q < 0 )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   /* (nothing of an earlier load or solve may still be queued: the arena starts over, buffers may go back to the pool) */
   if ( s->ncmd > 0 )
      HS_CALL( flush_cmds(s) );
   if ( hipStreamQuery(s->stream) != hipSuccess )
      HS_HIP( hipStreamSynchronize(s->stream) );
   if ( s->stream2 != NULL && hipStreamQuery(s->stream2) != hipSuccess )
      HS_HIP( hipStreamSynchronize(s->stream2) );
   s->stage_pending = false; s->stage_off = 0; s->ncmd = 0; s->cmd_inflight = false;
   s->zero_b = false; s->zero_D = false; s->s1_sol_host = false;
   s->rframe.valid = 0;          /* (a rounding frame belongs to the shape it was made for, the same shape set again included) */
   s->rframe.served.clear();
   /* The same shape again (the next node of a tree with the same fixings pattern, a re-load of the same problem): every
    * allocation is kept - the constraint matrices (GBs at the bench sizes), their packed copy and the Schur workspace cost tens
    * of milliseconds to free and allocate again - and only the contents are reset to what a fresh shape has. */
   /* B&B: the nodes of a tree differ in the number of active variables and LP rows by a few (fixings, tightened bounds).  Small
    * shapes are allocated with some room (m_alloc, q_alloc below), and a shape with the same blocks that fits into it takes the
    * same path: nothing is freed or allocated - sixty pool operations and a dozen clears per node otherwise. */
   const bool fits = s->shaped && (int) s->blk.size() == nblocks && !s->shardA && s->shardA_req == 0
      && ((s->m == m && s->q == q) || (m <= s->m_alloc && q <= s->q_alloc && s->comm == NULL));
   if ( fits && getenv("HIPSDP_NO_SHAPE_REUSE") == NULL )
   {
      bool same = true;
      for (int k = 0; k < nblocks; ++k)
         if ( s->blk[k].n != blocksizes[k] || s->blk[k].sparse != block_wants_sparse(s, blocksizes[k], m, nnz != NULL ? nnz[k] : -1) )
            same = false;
      if ( same )
      {
         const long long m1s = (long long) m + 1;
         if ( s->m != m || s->q != q )
         {
            /* what depends on the counts themselves */
            hs_schur_ws_free(&s->sws);
            s->sws.T = s->sws.U = s->sws.K = s->sws.V = s->sws.U2 = s->sws.V2 = NULL;
            s->sws.evP[0] = s->sws.evP[1] = s->sws.evX[0] = s->sws.evX[1] = NULL; s->sws.ev_g2 = NULL; s->sws.after_g1 = NULL; s->sws.after_g1_arg = NULL;
            s->m = m; s->q = q;
            s->a_r0 = 0; s->a_r1 = (int) m1s;
            s->u1 = s->rhs2 + 2LL * m;
         }
         for (auto& B : s->blk)
         {
            if ( B.sparse )
            {
               HS_CALL( stage_zero(s, B.A0, (long long) B.n * B.n) );
               free_sparse(B);
               B.sph = new SpHost();
               B.sp_dirty = true;
               B.sp_gathered = false;
            }
            else
               HS_CALL( stage_zero(s, B.Aown, m1s * B.n * B.n) );
            a_written(s, B);
            B.derived_valid = false;
         }
         /* (b and Dext are cleared when they are next used - unless set_obj / set_lp, which replace them whole, come first) */
         s->zero_b = true; s->zero_D = true;
         s->stage_pending = true;                 /* (no wait here: what follows is queued behind the clears) */
         s->have_start = false;
         s->solved = false;
         s->pre_valid = false;
         return HIPSDP_OK;
      }
   }
   free_problem(s);
   s->m = m;
   s->q = q;
   const long long m1 = m + 1;
   /* room for the neighbouring shapes of a tree (see above); large problems are allocated exactly */
   const bool roomy = (m <= 112) && s->comm == NULL && s->shardA_req == 0;
   const int mA = roomy ? m + 16 : m, qA = roomy ? q + 32 : q;
   const long long m1A = (long long) mA + 1;
   s->m_alloc = mA; s->q_alloc = qA;
   int nmax = 1;
   /* Constraint matrices sharded by variable (several ranks only): asked for, or - left to the sizes - when the replicated
    * matrices with their packed copy would take more than 75 % of the device memory.  Every rank decides from the same numbers. */
   s->shardA = false;
   s->a_r0 = 0; s->a_r1 = (int) m1;
   if ( s->comm != NULL && s->shardA_req != 0 && (s->nranks > 1 || s->shardA_req > 0) )
   {
      double bytes = 0.0;
      for (int k = 0; k < nblocks; ++k)
         bytes += 12.0 * (double) m1 * (double) blocksizes[k] * (double) blocksizes[k];
      size_t fr = 0, tot = 0;
      s->shardA = s->shardA_req > 0 || (hipMemGetInfo(&fr, &tot) == hipSuccess && bytes > 0.75 * (double) tot);
      if ( s->shardA )
         hs_var_rows((int) m1, s->nranks, s->rank, &s->a_r0, &s->a_r1);
   }
   const long long arows = s->a_r1 - s->a_r0;
   const long long arowsA = s->shardA ? arows : m1A;
   for (int k = 0; k < nblocks; ++k)
   {
      Block B;
      memset(&B, 0, sizeof(B));
      B.n = blocksizes[k];
      if ( B.n <= 0 )
         return HIPSDP_ERR_ARG;
      if ( B.n > nmax ) nmax = B.n;
      const long long n2 = (long long) B.n * B.n;
      s->blk.push_back(B);
      Block& R = s->blk.back();
      R.sparse = !s->shardA && block_wants_sparse(s, B.n, m, nnz != NULL ? nnz[k] : -1);
      if ( R.sparse )
      {
         /* no (m + 1) x n^2 array: the variables' matrices stay triplets, the constant matrix gets a dense array of its own */
         R.sph = new SpHost();
         R.sp_dirty = true;
         R.A = NULL;
         HS_CALL( dalloc(&R.A0sep, n2) );
         HS_HIP( hipMemsetAsync(R.A0sep, 0, (size_t) n2 * sizeof(double), s->stream) );
         R.A0 = R.A0sep;
      }
      else
      {
      HS_CALL( dalloc(&R.Aown, arowsA * n2) );
      HS_HIP( hipMemsetAsync(R.Aown, 0, (size_t) (arowsA * n2) * sizeof(double), s->stream) );
      R.A = R.Aown - (long long) s->a_r0 * n2;
      R.A0 = R.A;
      }
      if ( !R.sparse && (s->a_r0 > 0 || arows == 0) )
      {
         HS_CALL( dalloc(&R.A0sep, n2) );
         HS_HIP( hipMemsetAsync(R.A0sep, 0, (size_t) n2 * sizeof(double), s->stream) );
         R.A0 = R.A0sep;
      }
      double** mats[] = {&R.X, &R.Z, &R.Rd, &R.Lz, &R.LzInv, &R.Zinv, &R.Lx, &R.LxInv, &R.B, &R.H, &R.G, &R.GZ, &R.dXa, &R.dZa,
         &R.dX, &R.dZ, &R.E, &R.W, &R.T1, &R.Xs, &R.Zs, &R.T2, &R.W2};
      for (double** pm : mats)
         HS_CALL( dalloc(pm, n2) );
      const long long nd = hs_potrf_dinv_len(B.n);
      HS_CALL( dalloc(&R.dinvz, nd) );
      HS_CALL( dalloc(&R.dinvx, nd) );
      R.Lp = (((long long) B.n * (B.n + 1) / 2) + 1) & ~1LL;
      a_written(s, R);            /* (a fresh allocation, cleared above) */
      R.Apk = NULL;
      R.pkv = NULL;
      /* the packed copy halves the HBM traffic of the passes; small blocks are launch bound and their passes take one
       * launch less on the full storage */
      if ( B.n > 64 && !R.sparse )
      {
         if ( hipMalloc((void**) &R.Apkown, (size_t) ((arowsA > 0 ? arowsA : 1) * R.Lp) * sizeof(double)) != hipSuccess )
         {
            (void) hipGetLastError();
            R.Apkown = NULL;              /* not enough memory for the packed copy: the passes use the full storage */
         }
         else
         {
            R.Apk = R.Apkown - (long long) s->a_r0 * R.Lp;
            HS_CALL( dalloc(&R.pkv, 2 * R.Lp) );
            HS_HIP( hipMemsetAsync(R.pkv, 0, (size_t) (2 * R.Lp) * sizeof(double), s->stream) );   /* pad entries stay 0 */
         }
      }
   }
   HS_CALL( dalloc(&s->b, mA) );
   HS_CALL( dalloc(&s->Dext, (long long) qA * m1A) );
   HS_CALL( dalloc(&s->y, mA) ); HS_CALL( dalloc(&s->ys, mA) );
   double** qv[] = {&s->x, &s->z, &s->rd, &s->tmpq, &s->hl, &s->beta, &s->elp, &s->dxa, &s->dza, &s->dx, &s->dz, &s->xs, &s->zs};
   for (double** p : qv) HS_CALL( dalloc(p, qA) );
   double** ev[] = {&s->yt, &s->dyt, &s->wt, &s->AX, &s->AH, &s->tmpe};
   for (double** p : ev) HS_CALL( dalloc(p, m1A) );
   double** mv[] = {&s->rp, &s->u2, &s->dy, &s->dya};
   for (double** p : mv) HS_CALL( dalloc(p, mA) );
   /* [g ; b ; h]: the right-hand side of a direction lives behind the two of the tau elimination, so that the predictor's solve
    * can ride along with them as a third right-hand side (u1 is a view, not an allocation) */
   HS_CALL( dalloc(&s->rhs2, 3LL * mA) );
   s->u1 = s->rhs2 + 2LL * m;
   HS_CALL( dalloc(&s->cvec, 2LL * m1A) );
   HS_CALL( dalloc(&s->Mx, (m1A + 32) * m1A) );    /* row padding: the 2 G shard chunks may overhang by < 2 G rows */
   HS_CALL( dalloc(&s->Lm, (long long) mA * mA) );
   HS_CALL( dalloc(&s->dinvm, hs_potrf_dinv_len(mA)) );
   HS_CALL( dalloc(&s->Slp, (long long) qA * m1A) );
   HS_CALL( dalloc(&s->regmask, mA) );
   s->nsc = SC_FIXED_END + 8 * (nblocks > 0 ? nblocks : 1) + 8;
   HS_CALL( dalloc(&s->sc, s->nsc + 4) );          /* the 8 int flags live behind the scalars: one read-back covers both */
   s->flags = reinterpret_cast<int*>(s->sc + s->nsc);
   if ( s->hsc_cap < s->nsc + 8 )
   {
      if ( s->hsc != NULL ) (void) hipHostFree(s->hsc);
      s->hsc = NULL;
      s->hsc_cap = 2LL * (s->nsc + 8);
      HS_HIP( hipHostMalloc((void**) &s->hsc, (size_t) s->hsc_cap * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) );
      HS_HIP( hipHostGetDevicePointer((void**) &s->hsc_dev, s->hsc, 0) );
      memset(s->hsc, 0, (size_t) s->hsc_cap * sizeof(double));
   }
   HS_CALL( dalloc(&s->red_ws, HS_RED_WS_DOUBLES) );
   s->gemv_ws_len = 8192 + 4LL * 1024 * 4;
   HS_CALL( dalloc(&s->gemv_ws, s->gemv_ws_len) );
   {
      long long need = 0;
      for (auto& B : s->blk)
      {
         const long long n2 = (long long) B.n * B.n, lp = (long long) B.n * (B.n + 1) / 2;
         need = std::max(need, std::max((long long) hs_gemv_t_chunks(mA + 1, n2) * n2, (long long) hs_gemv_t_chunks(mA + 1, lp) * lp));
      }
      s->gemvt_ws_len = need;
      if ( need > 0 )
         HS_CALL( dalloc(&s->gemvt_ws, need) );
   }
   HS_CALL( dalloc(&s->lan_ws, hs_lanczos_ws(nmax, 256)) );
   HS_CALL( dalloc(&s->lan_ws2, hs_lanczos_ws(nmax, 256)) );
   if ( nmax > 64 )
   {
      if ( s->lan_sync == NULL )
         HS_HIP( hipMalloc((void**) &s->lan_sync, (size_t) hs_lanczos_sync_words() * sizeof(unsigned long long)) );
      HS_CALL( hs_lanczos_sync_reset(s->stream, s->lan_sync, s->lan_rot) );
   }
   HS_CALL( dalloc(&s->trsv_ws, hs_trsv_sync_ws(mA)) );
   if ( m > 2 * 64 )
      HS_CALL( hs_trsv_sync_init(s->stream, m, s->trsv_ws, &s->trsv_epoch) );
   s->trsv_epoch = 0;
   s->sws.T = s->sws.U = s->sws.K = s->sws.V = s->sws.U2 = s->sws.V2 = NULL;
   s->sws.evP[0] = s->sws.evP[1] = s->sws.evX[0] = s->sws.evX[1] = NULL; s->sws.ev_g2 = NULL; s->sws.after_g1 = NULL; s->sws.after_g1_arg = NULL;
   HS_HIP( hipMemsetAsync(s->Dext, 0, (size_t) ((long long) q * m1 > 0 ? (long long) q * m1 : 1) * sizeof(double), s->stream) );
   HS_HIP( hipMemsetAsync(s->b, 0, (size_t) (m > 0 ? m : 1) * sizeof(double), s->stream) );
   HS_HIP( hipStreamSynchronize(s->stream) );
   s->shaped = true;
   s->have_start = false;
   return HIPSDP_OK;
}

extern "C" int hipsdp_set_obj(hipsdp_solver* s, const double* b)
{
   if ( s == NULL || !s->shaped ) return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   if ( s->m > 0 )
      HS_CALL( stage_upload(s, s->b, b, (size_t) s->m * sizeof(double)) );
   s->zero_b = false;
   s->solved = false;
   return HIPSDP_OK;
}

__global__ void k_scatter_coo(long long nnz, int n, const int* __restrict__ var, const int* __restrict__ row,
   const int* __restrict__ col, const double* __restrict__ val, double* __restrict__ A, int r0, int r1, double* __restrict__ A0,
   int vmax, int* __restrict__ err)
{
   const long long n2 = (long long) n * n;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (long long) gridDim.x * blockDim.x)
   {
      const int r = row[e], c = col[e];
      const int v = var[e];
      /* the indices are validated here, on the device (10^8 triplets: a host loop costs as much as the upload): an entry out of
       * range is not written and raises the error flag */
      if ( v < 0 || v > vmax || r < 0 || r >= n || c < 0 || c >= n )
      {
         atomicExch(err, 1);
         continue;
      }
      /* matrices sharded by variable: rows this rank does not hold are skipped, the constant matrix goes to its replicated copy */
      double* a = (v == 0) ? A0 : A + (long long) v * n2;
      if ( v != 0 && (v < r0 || v >= r1) )
         continue;
      a[(long long) r * n + c] = val[e];
      a[(long long) c * n + r] = val[e];
   }
}

/* k_scatter_coo writes its entries in no order, and an entry writes both triangles: a position named twice in one call (as (r, c)
 * and again as (r, c) or (c, r)) would keep either value, or one value per triangle.  A block kept as nonzeros keeps the LAST entry
 * of a position (hs_sp_build), so the dense scatter is handed only that one: false when no position repeats (nothing to do), else
 * keep = the entries to scatter, in the caller's order.  Indices are in range (checked by the caller). */
static bool scatter_last_of_each_position(long long nnz, int n, const int* var, const int* row, const int* col, std::vector<long long>* keep)
{
   std::vector<std::pair<unsigned long long, long long> > key((size_t) nnz);
   for (long long e = 0; e < nnz; ++e)
   {
      const unsigned long long r = (unsigned long long) (row[e] >= col[e] ? row[e] : col[e]), c = (unsigned long long) (row[e] >= col[e] ? col[e] : row[e]);
      key[(size_t) e] = std::make_pair(((unsigned long long) var[e] * (unsigned long long) n + r) * (unsigned long long) n + c, e);
   }
   std::sort(key.begin(), key.end());
   bool repeats = false;
   for (size_t k = 0; k + 1 < key.size() && !repeats; ++k)
      repeats = key[k].first == key[k + 1].first;
   if ( !repeats )
      return false;
   keep->clear();
   for (size_t k = 0; k < key.size(); ++k)
      if ( k + 1 == key.size() || key[k].first != key[k + 1].first )
         keep->push_back(key[k].second);
   std::sort(keep->begin(), keep->end());
   return true;
}

/* the one launch of k_scatter_coo; every operand is on the device (or in the arena).  No wait */
static int scatter_launch(hipStream_t st, long long nnz, int n, const int* var, const int* row, const int* col, const double* val,
   double* A, int r0, int r1, double* A0, int vmax, int* err)
{
   long long g = (nnz + 255) / 256; if ( g > 4096 ) g = 4096;
   hipLaunchKernelGGL(k_scatter_coo, dim3((unsigned) g), dim3(256), 0, st, nnz, n, var, row, col, val, A, r0, r1, A0, vmax, err);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* the blocking route: the caller's triplets to pooled buffers, the flag cleared, the scatter, the flag back (herr == NULL: nobody
 * reads it, the indices were checked on the host) and ONE wait.  Entries in range are written even when one is not. */
static int scatter_host_triplets(hipsdp_solver* s, int n, long long nnz, const int* var, const int* row, const int* col, const double* val,
   double* A, int r0, int r1, double* A0, int vmax, int* dflag, int* herr)
{
   hipStream_t st = s->stream;
   PoolBuf<int> dv(st), dr(st), dc(st);
   PoolBuf<double> dval(st);
   HS_CALL( dv.alloc(nnz) ); HS_CALL( dr.alloc(nnz) ); HS_CALL( dc.alloc(nnz) ); HS_CALL( dval.alloc(nnz) );
   HS_HIP( hipMemcpyAsync(dv.p, var, (size_t) nnz * sizeof(int), hipMemcpyHostToDevice, st) );
   HS_HIP( hipMemcpyAsync(dr.p, row, (size_t) nnz * sizeof(int), hipMemcpyHostToDevice, st) );
   HS_HIP( hipMemcpyAsync(dc.p, col, (size_t) nnz * sizeof(int), hipMemcpyHostToDevice, st) );
   HS_HIP( hipMemcpyAsync(dval.p, val, (size_t) nnz * sizeof(double), hipMemcpyHostToDevice, st) );
   HS_HIP( hipMemsetAsync(dflag, 0, sizeof(int), st) );
   HS_CALL( scatter_launch(st, nnz, n, dv.p, dr.p, dc.p, dval.p, A, r0, r1, A0, vmax, dflag) );
   if ( herr != NULL )
      HS_HIP( hipMemcpyAsync(herr, dflag, sizeof(int), hipMemcpyDeviceToHost, st) );
   HS_HIP( hipStreamSynchronize(st) );
   return HS_OK;
}

extern "C" int hipsdp_add_entries(hipsdp_solver* s, int block, long long nnz, const int* var, const int* row, const int* col,
   const double* val)
{
   if ( s == NULL || !s->shaped || block < 0 || block >= (int) s->blk.size() || nnz < 0 )
      return HIPSDP_ERR_ARG;
   if ( nnz == 0 )
      return HIPSDP_OK;
   HS_HIP( hipSetDevice(s->device) );
   Block& B = s->blk[block];
   if ( B.sparse )
   {
      /* variables: collected on the host (built into the device structure before the next use); constant matrix: dense scatter */
      std::vector<int> cv, cr, cc; std::vector<double> cx;
      if ( B.sp_gathered )
         for (long long e = 0; e < nnz; ++e)
            if ( var[e] >= 1 )
            {
               set_err("hipsdp_add_entries: the matrices of this block were gathered from the master copy; only the constant matrix "
                  "(var 0) can be set until the next hipsdp_set_shape");
               return HIPSDP_ERR_ARG;
            }
      for (long long e = 0; e < nnz; ++e)
      {
         if ( var[e] < 0 || var[e] > s->m || row[e] < 0 || row[e] >= B.n || col[e] < 0 || col[e] >= B.n )
         {
            set_err("hipsdp_add_entries: index out of range");
            return HIPSDP_ERR_ARG;
         }
         if ( var[e] == 0 )
         {
            cv.push_back(0); cr.push_back(row[e]); cc.push_back(col[e]); cx.push_back(val[e]);
         }
         else
         {
            B.sph->var.push_back(var[e]); B.sph->row.push_back(row[e]); B.sph->col.push_back(col[e]); B.sph->val.push_back(val[e]);
         }
      }
      if ( !B.sp_gathered )
         B.sp_dirty = true;
      s->solved = false;
      if ( cv.empty() )
         return HIPSDP_OK;
      {
         std::vector<long long> keep;
         if ( scatter_last_of_each_position((long long) cv.size(), B.n, cv.data(), cr.data(), cc.data(), &keep) )
         {
            for (size_t k = 0; k < keep.size(); ++k)         /* (keep ascends: in place) */
            {
               cr[k] = cr[(size_t) keep[k]]; cc[k] = cc[(size_t) keep[k]]; cx[k] = cx[(size_t) keep[k]];
            }
            cv.resize(keep.size()); cr.resize(keep.size()); cc.resize(keep.size()); cx.resize(keep.size());
         }
      }
      nnz = (long long) cv.size();
      HS_CALL( flush_cmds(s) );
      return scatter_host_triplets(s, B.n, nnz, cv.data(), cr.data(), cc.data(), cx.data(), B.A0, 0, 1, B.A0, 0, s->flags + 6, NULL);
   }
   std::vector<int> kv, kr, kc; std::vector<double> kx;       /* (the call's entries without the overwritten ones, when there are any) */
   if ( nnz <= 16384 )
   {
      /* a few triplets (the constant matrix of a node): indices checked here, the triplets through the arena, no wait */
      bool ok = true;
      for (long long e = 0; e < nnz; ++e)
         if ( var[e] < 0 || var[e] > s->m || row[e] < 0 || row[e] >= B.n || col[e] < 0 || col[e] >= B.n )
            ok = false;
      if ( !ok )
      {
         set_err("hipsdp_add_entries: index out of range");
         return HIPSDP_ERR_ARG;
      }
      std::vector<long long> keep;
      if ( scatter_last_of_each_position(nnz, B.n, var, row, col, &keep) )
      {
         for (long long e : keep)
         {
            kv.push_back(var[e]); kr.push_back(row[e]); kc.push_back(col[e]); kx.push_back(val[e]);
         }
         nnz = (long long) keep.size();
         var = kv.data(); row = kr.data(); col = kc.data(); val = kx.data();
      }
      void* dvp = NULL;
      char* h = (char*) stage_take(s, (size_t) nnz * (3 * sizeof(int) + sizeof(double)) + 64, &dvp);
      if ( h != NULL )
      {
         /* values first (8-byte aligned), then the three index arrays */
         memcpy(h, val, (size_t) nnz * sizeof(double));
         int* hi = (int*) (h + (size_t) nnz * sizeof(double));
         memcpy(hi, var, (size_t) nnz * sizeof(int));
         memcpy(hi + nnz, row, (size_t) nnz * sizeof(int));
         memcpy(hi + 2 * nnz, col, (size_t) nnz * sizeof(int));
         const double* dval = (const double*) dvp;
         const int* di = (const int*) ((const char*) dvp + (size_t) nnz * sizeof(double));
         a_written(s, B);
         NodeCmd* q = cmd_new(s);
         if ( q != NULL )
         {
            q->op = NC_SCATTER; q->n = nnz; q->i0 = B.n; q->i1 = s->a_r0; q->i2 = s->a_r1; q->idx = di; q->src = dval; q->dst = B.A; q->dst2 = B.A0;
         }
         else
         {
            HS_CALL( flush_cmds(s) );
            HS_CALL( scatter_launch(s->stream, nnz, B.n, di, di + nnz, di + 2 * nnz, dval, B.A, s->a_r0, s->a_r1, B.A0, s->m, s->flags + 6) );
            s->stage_pending = true;
         }
         s->solved = false;
         return HIPSDP_OK;
      }
   }
   a_written(s, B);         /* (before the first call that can fail: entries in range are written even when one is not) */
   HS_CALL( flush_cmds(s) );
   int herr = 0;
   HS_CALL( scatter_host_triplets(s, B.n, nnz, var, row, col, val, B.A, s->a_r0, s->a_r1, B.A0, s->m, s->flags + 6, &herr) );
   s->solved = false;
   if ( herr != 0 )
   {
      set_err("hipsdp_add_entries: index out of range");
      return HIPSDP_ERR_ARG;
   }
   return HIPSDP_OK;
}

/* ---- master copy: the matrices A_v of ALL variables in original indices, uploaded once and kept across node solves.  A
 * node's compact block (active variables, kept rows/columns) is then gathered on the device (the
 * sdprow/sdpcol/sdpval arrays do not change between the nodes of a branch-and-bound run). */
extern "C" int hipsdp_master_define(hipsdp_solver* s, int nvars, int nblocks, const int* blocksizes, const int* nblockvars)
{
   return hipsdp_master_define2(s, nvars, nblocks, blocksizes, nblockvars, NULL);
}

extern "C" int hipsdp_master_block_is_sparse(hipsdp_solver* s, int master_block)
{
   if ( s == NULL || master_block < 0 || master_block >= (int) s->master_sp.size() )
      return 0;
   return s->master_sp[master_block] != NULL ? 1 : 0;
}

extern "C" int hipsdp_master_gather_stats(hipsdp_solver* s, long long* device_builds, long long* host_builds, long long* launches,
   long long* readbacks)
{
   if ( s == NULL )
      return HIPSDP_ERR_ARG;
   if ( device_builds != NULL ) *device_builds = s->mg_device_builds;
   if ( host_builds != NULL ) *host_builds = s->mg_host_builds;
   if ( launches != NULL ) *launches = s->mg_launches;
   if ( readbacks != NULL ) *readbacks = s->mg_readbacks;
   return HIPSDP_OK;
}

extern "C" int hipsdp_master_define2(hipsdp_solver* s, int nvars, int nblocks, const int* blocksizes, const int* nblockvars,
   const long long* nnz)
{
   if ( s == NULL || nvars < 0 || nblocks < 0 )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   HS_HIP( hipStreamSynchronize(s->stream) );
   master_free(s);
   s->master_nvars = nvars;
   for (int b = 0; b < nblocks; ++b)
   {
      if ( blocksizes[b] <= 0 )
         return HIPSDP_ERR_ARG;
      double* p = NULL;
      /* one slot per variable that appears in the block (nblockvars == NULL: one per variable) */
      const int slots = nblockvars != NULL ? nblockvars[b] : nvars;
      if ( slots < 0 || slots > nvars )
         return HIPSDP_ERR_ARG;
      if ( nnz != NULL && nnz[b] >= 0 )
      {
         /* kept as triplets: collected on the host, sorted and uploaded by the first gather (csrc/sp_master.hip) */
         hs_spm* M = NULL;
         HS_CALL( hs_spm_create(&M, blocksizes[b], slots) );
         s->master_A.push_back(NULL);
         s->master_sp.push_back(M);
         s->master_sizes.push_back(blocksizes[b]);
         s->master_slots.push_back(slots);
         continue;
      }
      const long long cnt = (long long) slots * blocksizes[b] * blocksizes[b];
      const int rc = dalloc(&p, cnt);
      if ( rc != HS_OK )
      {
         master_free(s);           /* the caller falls back to loading the node's block directly */
         return rc;
      }
      HS_HIP( hipMemsetAsync(p, 0, (size_t) (cnt > 0 ? cnt : 1) * sizeof(double), s->stream) );
      s->master_A.push_back(p);
      s->master_sp.push_back(NULL);
      s->master_sizes.push_back(blocksizes[b]);
      s->master_slots.push_back(slots);
   }
   HS_HIP( hipStreamSynchronize(s->stream) );
   return HIPSDP_OK;
}

extern "C" int hipsdp_master_add_entries(hipsdp_solver* s, int block, long long nnz, const int* var, const int* row,
   const int* col, const double* val)
{
   if ( s == NULL || block < 0 || block >= (int) s->master_A.size() || nnz < 0 )
      return HIPSDP_ERR_ARG;
   if ( nnz == 0 )
      return HIPSDP_OK;
   if ( s->master_sp[block] != NULL )
   {
      if ( hs_spm_add(s->master_sp[block], nnz, var, 0, row, col, val) != HS_OK )
      {
         set_err("hipsdp_master_add_entries: index out of range");
         return HIPSDP_ERR_ARG;
      }
      return HIPSDP_OK;
   }
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   const int n = s->master_sizes[block];
   PoolBuf<int> derr(s->stream);         /* (a master copy is defined before any shape: no s->flags yet) */
   HS_CALL( derr.alloc(1) );
   /* slot 0 of the master copy is a variable like the others: A0 = A, nothing is skipped by the row range */
   int herr = 0;
   HS_CALL( scatter_host_triplets(s, n, nnz, var, row, col, val, s->master_A[block], 0, 2147483647, s->master_A[block],
         s->master_slots[block] - 1, derr.p, &herr) );
   if ( herr != 0 )
   {
      set_err("hipsdp_master_add_entries: index out of range");
      return HIPSDP_ERR_ARG;
   }
   return HIPSDP_OK;
}

/* The same upload straight from the caller's per-variable arrays (the layout of sdpisolver.h: sdprow[b][k], sdpcol[b][k],
 * sdpval[b][k] with sdpnblockvarnonz[b][k] entries each), streamed through two pinned staging chunks: the host fills one chunk
 * (block copies) while the copy engine moves the other and the scatter kernel consumes it.  No concatenated host copy (2.25 GB
 * of freshly faulted pageable memory at n = 500, m = 1000) and no pageable H2D transfer. */
#define HS_STAGE_ENTRIES (4LL << 20)
static int stage_ensure(hipsdp_solver* s, long long want)
{
   long long cap = want < HS_STAGE_ENTRIES ? want : HS_STAGE_ENTRIES;
   if ( cap < 1024 ) cap = 1024;
   cap = (cap + 63) & ~63LL;              /* the value array follows three int arrays: keep it 8-byte aligned */
   if ( s->stage_cap >= cap )
      return HS_OK;
   for (int b = 0; b < 2; ++b)
   {
      if ( s->stage_h[b] != NULL ) (void) hipHostFree(s->stage_h[b]);
      if ( s->stage_d[b] != NULL ) (void) hipFree(s->stage_d[b]);
      s->stage_h[b] = NULL; s->stage_d[b] = NULL;
      if ( s->stage_ev[b] == NULL )
         HS_HIP( hipEventCreateWithFlags(&s->stage_ev[b], hipEventDisableTiming) );
   }
   s->stage_cap = 0;
   const size_t bytes = (size_t) cap * (3 * sizeof(int) + sizeof(double));
   for (int b = 0; b < 2; ++b)
   {
      HS_HIP( hipHostMalloc((void**) &s->stage_h[b], bytes, hipHostMallocDefault) );
      HS_HIP( hipMalloc((void**) &s->stage_d[b], bytes) );
   }
   s->stage_cap = cap;
   return HS_OK;
}

extern "C" int hipsdp_master_add_vars(hipsdp_solver* s, int block, int nslots, const int* nnz, const int* const* row,
   const int* const* col, const double* const* val)
{
   if ( s == NULL || block < 0 || block >= (int) s->master_A.size() || nslots < 0 || nslots > s->master_slots[block]
      || (nslots > 0 && (nnz == NULL || row == NULL || col == NULL || val == NULL)) )
      return HIPSDP_ERR_ARG;
   long long total = 0;
   for (int k = 0; k < nslots; ++k)
   {
      if ( nnz[k] < 0 )
         return HIPSDP_ERR_ARG;
      total += nnz[k];
   }
   if ( total == 0 )
      return HIPSDP_OK;
   if ( s->master_sp[block] != NULL )
   {
      for (int k = 0; k < nslots; ++k)
         if ( nnz[k] > 0 && hs_spm_add(s->master_sp[block], nnz[k], NULL, k, row[k], col[k], val[k]) != HS_OK )
         {
            set_err("hipsdp_master_add_vars: index out of range");
            return HIPSDP_ERR_ARG;
         }
      return HIPSDP_OK;
   }
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   HS_CALL( stage_ensure(s, total) );
   const long long cap = s->stage_cap;
   const int n = s->master_sizes[block];
   PoolBuf<int> derr(s->stream);
   HS_CALL( derr.alloc(1) );
   HS_HIP( hipMemsetAsync(derr.p, 0, sizeof(int), s->stream) );
   int k = 0;
   long long off = 0;                  /* entries of slot k already shipped */
   int set = 0;
   bool used[2] = {false, false};
   while ( k < nslots )
   {
      if ( used[set] )
         HS_HIP( hipEventSynchronize(s->stage_ev[set]) );       /* the chunk's previous contents have been consumed */
      char* hb = (char*) s->stage_h[set];
      int* hvar = (int*) hb;
      int* hrow = hvar + cap;
      int* hcol = hrow + cap;
      double* hval = (double*) (hcol + cap);
      long long fill = 0;
      while ( k < nslots && fill < cap )
      {
         const long long left = nnz[k] - off;
         const long long take = left < cap - fill ? left : cap - fill;
         if ( take > 0 )
         {
            for (long long t = 0; t < take; ++t)
               hvar[fill + t] = k;
            memcpy(hrow + fill, row[k] + off, (size_t) take * sizeof(int));
            memcpy(hcol + fill, col[k] + off, (size_t) take * sizeof(int));
            memcpy(hval + fill, val[k] + off, (size_t) take * sizeof(double));
            fill += take;
            off += take;
         }
         if ( off >= nnz[k] )
         {
            ++k;
            off = 0;
         }
      }
      if ( fill == 0 )
         break;
      char* db = (char*) s->stage_d[set];
      int* dvar = (int*) db;
      int* drow = dvar + cap;
      int* dcol = drow + cap;
      double* dval = (double*) (dcol + cap);
      HS_HIP( hipMemcpyAsync(dvar, hvar, (size_t) fill * sizeof(int), hipMemcpyHostToDevice, s->stream) );
      HS_HIP( hipMemcpyAsync(drow, hrow, (size_t) fill * sizeof(int), hipMemcpyHostToDevice, s->stream) );
      HS_HIP( hipMemcpyAsync(dcol, hcol, (size_t) fill * sizeof(int), hipMemcpyHostToDevice, s->stream) );
      HS_HIP( hipMemcpyAsync(dval, hval, (size_t) fill * sizeof(double), hipMemcpyHostToDevice, s->stream) );
      HS_CALL( scatter_launch(s->stream, fill, n, dvar, drow, dcol, dval, s->master_A[block], 0, 2147483647, s->master_A[block],
            s->master_slots[block] - 1, derr.p) );
      HS_HIP( hipEventRecord(s->stage_ev[set], s->stream) );
      used[set] = true;
      set ^= 1;
   }
   int herr = 0;
   HS_HIP( hipMemcpyAsync(&herr, derr.p, sizeof(int), hipMemcpyDeviceToHost, s->stream) );
   HS_HIP( hipStreamSynchronize(s->stream) );
   if ( herr != 0 )
   {
      set_err("hipsdp_master_add_vars: index out of range");
      return HIPSDP_ERR_ARG;
   }
   return HIPSDP_OK;
}

/* A_engine[a + 1][r'][c'] = master[slot[a]][kept[r']][kept[c']], zero for slot[a] = -1 (variable absent from the block) */
__global__ void k_master_gather(int nactive, int nk, int N, const int* __restrict__ act, const int* __restrict__ kept,
   const double* __restrict__ master, double* __restrict__ A)
{
   const long long nk2 = (long long) nk * nk;
   const long long total = (long long) nactive * nk2;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long) gridDim.x * blockDim.x)
   {
      const long long a = e / nk2;
      const long long rc = e - a * nk2;
      const int r = (int) (rc / nk), c = (int) (rc - (long long) r * nk);
      A[(a + 1) * nk2 + rc] = act[a] >= 0 ? master[((long long) act[a] * N + kept[r]) * N + kept[c]] : 0.0;
   }
}

/* The two index lists of a gather where a kernel can read them.  Through the arena when it has room: the kernel reads them there, nothing
 * is copied and nothing waits (wait = false; b follows a).  Else asynchronous copies into two pooled buffers, and the caller's launch is
 * followed by one hipStreamSynchronize (wait = true). */
struct IndexLists
{
   PoolBuf<int> da, db;
   const int *a, *b;
   bool wait;
   explicit IndexLists(hipStream_t st) : da(st), db(st), a(NULL), b(NULL), wait(false) {}
   int stage(hipsdp_solver* s, const int* ha, int na, const int* hb, int nb)
   {
      void* dv = NULL;
      int* hidx = (int*) stage_take(s, (size_t) (na + nb) * sizeof(int), &dv);
      wait = hidx == NULL;
      if ( !wait )
      {
         memcpy(hidx, ha, (size_t) na * sizeof(int));
         memcpy(hidx + na, hb, (size_t) nb * sizeof(int));
         a = (const int*) dv; b = a + na;
         return HS_OK;
      }
      HS_CALL( da.alloc(na) ); HS_CALL( db.alloc(nb) );
      HS_HIP( hipMemcpyAsync(da.p, ha, (size_t) na * sizeof(int), hipMemcpyHostToDevice, s->stream) );
      HS_HIP( hipMemcpyAsync(db.p, hb, (size_t) nb * sizeof(int), hipMemcpyHostToDevice, s->stream) );
      a = da.p; b = db.p;
      return HS_OK;
   }
};

/* from a master block kept as triplets (csrc/sp_master.hip): into a block kept as nonzeros the node's whole structure is built on the
 * device, in the master block's workspace; into a dense block the rows of the active variables are cleared and scattered */
static int master_gather_triplets(hipsdp_solver* s, int engine_block, int master_block, int nactive, const int* activevars, int nkept,
   const int* kept)
{
   hs_spm* M = s->master_sp[master_block];
   Block& B = s->blk[engine_block];
   const int N = hs_spm_size(M), S = hs_spm_slots(M);
   HS_HIP( hipSetDevice(s->device) );
   if ( B.sparse )
   {
      /* the workspace holds one node: whoever held it before (this block's last load, another block) loses it */
      for (auto& O : s->blk)
         if ( O.sparse && O.sp_gathered && O.sp_master == master_block && O.sp != NULL )
         {
            HS_HIP( hipStreamSynchronize(s->stream) );
            hs_sp_free(O.sp);
            O.sp = NULL;
         }
      if ( B.sp != NULL )
         hs_sp_free(B.sp);
      B.sp = NULL;
      if ( B.sph != NULL && !B.sph->var.empty() )
      {
         set_err("hipsdp_master_gather: the block already has entries of hipsdp_add_entries for its variables");
         return HIPSDP_ERR_ARG;
      }
      const int rc = hs_spm_gather_sparse(s->stream, M, B.n, s->m, nactive, activevars, kept, &B.sp, &s->mg_launches, &s->mg_readbacks);
      if ( rc != HS_OK )
      {
         if ( rc == HS_ERR_ARG )
            set_err("hipsdp_master_gather: slot or row out of range, a slot named twice, rows not increasing, or too many entries");
         return rc;
      }
      B.sp_gathered = true;
      B.sp_master = master_block;
      B.sp_dirty = false;
      ++s->mg_device_builds;
      s->solved = false;
      return HIPSDP_OK;
   }
   /* dense engine block: slots and the inverse of kept through the arena, one launch */
   std::vector<int> inv((size_t) N), svar((size_t) (S > 0 ? S : 1));
   int ordered = 1;
   if ( hs_spm_node_maps(N, S, nactive, activevars, nkept, kept, inv.data(), svar.data(), &ordered) != HIPSDP_OK )
   {
      set_err("hipsdp_master_gather: slot or row out of range, a slot named twice or rows not increasing");
      return HIPSDP_ERR_ARG;
   }
   if ( nactive == 0 )
      return HIPSDP_OK;
   a_written(s, B);
   HS_CALL( flush_cmds(s) );                 /* (the clears of set_shape come first) */
   IndexLists idx(s->stream);
   HS_CALL( idx.stage(s, activevars, nactive, inv.data(), N) );
   HS_CALL( hs_spm_gather_dense(s->stream, M, nkept, nactive, idx.a, idx.b, B.A, &s->mg_launches) );
   if ( idx.wait )
   {
      HS_HIP( hipStreamSynchronize(s->stream) );
      ++s->mg_readbacks;
   }
   else
      s->stage_pending = true;
   s->solved = false;
   return HIPSDP_OK;
}

extern "C" int hipsdp_master_gather(hipsdp_solver* s, int engine_block, int master_block, int nactive, const int* activevars,
   int nkept, const int* kept)
{
   if ( s == NULL || !s->shaped || engine_block < 0 || engine_block >= (int) s->blk.size() || master_block < 0
      || master_block >= (int) s->master_A.size() || nactive < 0 || nactive > s->m || nkept != s->blk[engine_block].n )
      return HIPSDP_ERR_ARG;
   if ( s->shardA || (s->blk[engine_block].sparse && s->master_sp[master_block] == NULL) )
   {
      set_err("hipsdp_master_gather: not available with matrices sharded by variable or kept as nonzeros");
      return HIPSDP_ERR_ARG;
   }
   if ( s->master_sp[master_block] != NULL )
      return master_gather_triplets(s, engine_block, master_block, nactive, activevars, nkept, kept);
   if ( nactive == 0 )
      return HIPSDP_OK;
   HS_HIP( hipSetDevice(s->device) );
   const int N = s->master_sizes[master_block];
   for (int a = 0; a < nactive; ++a)
      if ( activevars[a] < -1 || activevars[a] >= s->master_slots[master_block] )
         return HIPSDP_ERR_ARG;
   for (int r = 0; r < nkept; ++r)
      if ( kept[r] < 0 || kept[r] >= N )
         return HIPSDP_ERR_ARG;
   Block& B = s->blk[engine_block];
   a_written(s, B);
   const long long total = (long long) nactive * nkept * nkept;
   IndexLists idx(s->stream);
   HS_CALL( idx.stage(s, activevars, nactive, kept, nkept) );
   NodeCmd* q = (!idx.wait && total <= NC_LIMIT) ? cmd_new(s) : NULL;
   if ( q != NULL )
   {
      q->op = NC_GATHER; q->i0 = nactive; q->i1 = nkept; q->i2 = N; q->idx = idx.a; q->src = s->master_A[master_block]; q->dst = B.A;
   }
   else
   {
      long long g = (total + 255) / 256; if ( g > 65536 ) g = 65536;
      HS_CALL( flush_cmds(s) );
      hipLaunchKernelGGL(k_master_gather, dim3((unsigned) g), dim3(256), 0, s->stream, nactive, nkept, N, idx.a, idx.b,
         s->master_A[master_block], B.A);
      HS_LAUNCH_CHECK();
      if ( idx.wait )
         HS_HIP( hipStreamSynchronize(s->stream) );
      else
         s->stage_pending = true;
   }
   s->solved = false;
   return HIPSDP_OK;
}

extern "C" int hipsdp_set_block_dense(hipsdp_solver* s, int block, const double* A)
{
   if ( s == NULL || !s->shaped || block < 0 || block >= (int) s->blk.size() )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   Block& B = s->blk[block];
   if ( B.sparse )
   {
      set_err("hipsdp_set_block_dense: the block is kept as nonzeros (hipsdp_set_shape2 with a count): use hipsdp_add_entries");
      return HIPSDP_ERR_ARG;
   }
   const size_t n2b = (size_t) B.n * B.n * sizeof(double);
   a_written(s, B);
   if ( s->a_r1 > s->a_r0 )
      HS_HIP( hipMemcpy(B.Aown, A + (size_t) s->a_r0 * B.n * B.n, (size_t) (s->a_r1 - s->a_r0) * n2b, hipMemcpyHostToDevice) );
   if ( B.A0sep != NULL )
      HS_HIP( hipMemcpy(B.A0sep, A, n2b, hipMemcpyHostToDevice) );
   s->solved = false;
   return HIPSDP_OK;
}

extern "C" int hipsdp_set_lp(hipsdp_solver* s, const double* Dext)
{
   if ( s == NULL || !s->shaped ) return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   if ( s->q > 0 )
      HS_CALL( stage_upload(s, s->Dext, Dext, (size_t) s->q * (s->m + 1) * sizeof(double)) );
   s->zero_D = false;
   s->solved = false;
   return HIPSDP_OK;
}

int hs_gen_dense(hipStream_t s, int n, int i0, int i1, long long seed, double* A);
static int ensure_packed(hipsdp_solver* s);
static int pass_A(hipsdp_solver* s, Block& B, const double* V, double* out, bool packed = false);
static int pass_AT(hipsdp_solver* s, Block& B, const double* coef, double sa, const double* add, double* out);

extern "C" int hipsdp_gen_planted(hipsdp_solver* s, int n, int m, long long seed, const double* Xstar, const double* Zstar,
   const double* ystar, double* b_out)
{
   if ( s == NULL || !s->shaped || s->blk.size() != 1 || s->blk[0].n != n || s->m != m || s->q != 0 || s->blk[0].sparse )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   Block& B = s->blk[0];
   const long long n2 = (long long) n * n;
   const int m1 = m + 1;
   hipStream_t st = s->stream;
   a_written(s, B);         /* (first: a failure below leaves the matrices half written) */
   HS_CALL( hs_gen_dense(st, n, s->a_r0 > 1 ? s->a_r0 : 1, s->a_r1, seed, B.A) );
   /* A_0 = sum_i ystar_i A_i - Zstar : coefficient vector [0, ystar] over all m + 1 rows (row 0 is overwritten) */
   HS_HIP( hipMemcpyAsync(B.Z, Zstar, (size_t) n2 * sizeof(double), hipMemcpyHostToDevice, st) );
   HS_HIP( hipMemcpyAsync(B.X, Xstar, (size_t) n2 * sizeof(double), hipMemcpyHostToDevice, st) );
   HS_HIP( hipMemsetAsync(s->yt, 0, sizeof(double), st) );
   HS_HIP( hipMemcpyAsync(s->yt + 1, ystar, (size_t) m * sizeof(double), hipMemcpyHostToDevice, st) );
   HS_HIP( hipMemsetAsync(B.A0, 0, (size_t) n2 * sizeof(double), st) );
   if ( s->shardA )
   {
      /* every rank generated the matrices it holds; the two sums over all variables go through the sharded passes (row 0 is
       * zero and has coefficient 0 in the first, and its entry of the second is not used) */
      a_written(s, B);
      HS_CALL( ensure_packed(s) );
      HS_CALL( pass_AT(s, B, s->yt, -1.0, B.Z, B.T1) );
      HS_CALL( hs_symmetrize(st, B.T1, n) );
      HS_CALL( hs_copy(st, B.A0, B.T1, n2) );
      HS_CALL( pass_A(s, B, B.X, s->AX) );
   }
   else
   {
   HS_CALL( hs_gemv_t(st, m1, n2, B.A, n2, s->yt, -1.0, B.Z, B.T1) );
   HS_CALL( hs_symmetrize(st, B.T1, n) );
   HS_CALL( hs_copy(st, B.A, B.T1, n2) );
   /* b = A(Xstar) */
   const double* v = B.X;
   HS_CALL( hs_gemv_n(st, m1, n2, B.A, n2, 1, &v, s->AX, m1, s->gemv_ws, s->gemv_ws_len) );
   }
   HS_CALL( hs_copy(st, s->b, s->AX + 1, m) );
   HS_HIP( hipMemcpyAsync(b_out, s->b, (size_t) m * sizeof(double), hipMemcpyDeviceToHost, st) );
   HS_HIP( hipStreamSynchronize(st) );
   a_written(s, B);
   s->solved = false;
   return HIPSDP_OK;
}

void hs_gen_set_density(double density);

extern "C" int hipsdp_gen_planted_density(hipsdp_solver* s, int n, int m, long long seed, double density, const double* Xstar,
   const double* Zstar, const double* ystar, double* b_out)
{
   hs_gen_set_density(density);
   const int rc = hipsdp_gen_planted(s, n, m, seed, Xstar, Zstar, ystar, b_out);
   hs_gen_set_density(1.0);
   return rc;
}

extern "C" int hipsdp_get_block_dense(hipsdp_solver* s, int block, double* A)
{
   if ( s == NULL || !s->shaped || block < 0 || block >= (int) s->blk.size() )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   Block& B = s->blk[block];
   if ( B.sparse )
   {
      /* expanded from the triplets (later entries of the same position win, as in the device structure) */
      const size_t n2 = (size_t) B.n * B.n;
      memset(A, 0, (size_t) (s->m + 1) * n2 * sizeof(double));
      HS_HIP( hipMemcpy(A, B.A0, n2 * sizeof(double), hipMemcpyDeviceToHost) );
      if ( B.sp_gathered )
      {
         /* no host triplets: the by-variable list of the device structure */
         if ( B.sp == NULL )
            return HIPSDP_ERR_ARG;
         HS_HIP( hipStreamSynchronize(s->stream) );
         const size_t nz = (size_t) B.sp->nnz;
         std::vector<int> voff((size_t) s->m + 1), vrow(nz + 1), vcol(nz + 1);
         std::vector<double> vval(nz + 1);
         HS_HIP( hipMemcpy(voff.data(), B.sp->voff, voff.size() * sizeof(int), hipMemcpyDeviceToHost) );
         if ( nz > 0 )
         {
            HS_HIP( hipMemcpy(vrow.data(), B.sp->vrow, nz * sizeof(int), hipMemcpyDeviceToHost) );
            HS_HIP( hipMemcpy(vcol.data(), B.sp->vcol, nz * sizeof(int), hipMemcpyDeviceToHost) );
            HS_HIP( hipMemcpy(vval.data(), B.sp->vval, nz * sizeof(double), hipMemcpyDeviceToHost) );
         }
         for (int v = 1; v <= s->m; ++v)
            for (int e = voff[(size_t) v - 1]; e < voff[(size_t) v]; ++e)
            {
               double* a = A + (size_t) v * n2;
               a[(size_t) vrow[e] * B.n + vcol[e]] = vval[e];
               a[(size_t) vcol[e] * B.n + vrow[e]] = vval[e];
            }
         return HIPSDP_OK;
      }
      const SpHost& h = *B.sph;
      for (size_t e = 0; e < h.var.size(); ++e)
      {
         double* a = A + (size_t) h.var[e] * n2;
         a[(size_t) h.row[e] * B.n + h.col[e]] = h.val[e];
         a[(size_t) h.col[e] * B.n + h.row[e]] = h.val[e];
      }
      return HIPSDP_OK;
   }
   /* matrices sharded by variable: the rows this rank holds and the constant matrix are written, the rest is left alone */
   const size_t n2b = (size_t) B.n * B.n * sizeof(double);
   if ( s->a_r1 > s->a_r0 )
      HS_HIP( hipMemcpy(A + (size_t) s->a_r0 * B.n * B.n, B.Aown, (size_t) (s->a_r1 - s->a_r0) * n2b, hipMemcpyDeviceToHost) );
   if ( B.A0sep != NULL )
      HS_HIP( hipMemcpy(A, B.A0sep, n2b, hipMemcpyDeviceToHost) );
   return HIPSDP_OK;
}

extern "C" int hipsdp_block_device_ptr(hipsdp_solver* s, int block, double** dptr)
{
   if ( s == NULL || !s->shaped || block < 0 || block >= (int) s->blk.size() )
      return HIPSDP_ERR_ARG;
   HS_CALL( stage_sync(s) );
   /* whoever holds the pointer may write through it whenever it likes, unseen: the block counts as written now and its first
    * assembly is not cached for as long as this allocation lives (a hipsdp_set_shape of the same shape keeps it) */
   a_written(s, s->blk[block]);
   s->blk[block].a_escaped = true;
   *dptr = s->blk[block].Aown;
   return HIPSDP_OK;
}

extern "C" int hipsdp_set_start(hipsdp_solver* s, const double* y, const double* const* X, const double* const* Z,
   const double* x, const double* z)
{
   if ( s == NULL || !s->shaped ) return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   if ( s->m > 0 )
      HS_CALL( stage_upload(s, s->y, y, (size_t) s->m * sizeof(double)) );
   for (size_t k = 0; k < s->blk.size(); ++k)
   {
      const size_t bytes = (size_t) s->blk[k].n * s->blk[k].n * sizeof(double);
      HS_CALL( stage_upload(s, s->blk[k].X, X[k], bytes) );
      HS_CALL( stage_upload(s, s->blk[k].Z, Z[k], bytes) );
   }
   if ( s->q > 0 )
   {
      HS_CALL( stage_upload(s, s->x, x, (size_t) s->q * sizeof(double)) );
      HS_CALL( stage_upload(s, s->z, z, (size_t) s->q * sizeof(double)) );
   }
   s->have_start = true;
   s->s1_sol_host = false;
   return HIPSDP_OK;
}

/* ---- small fused kernels of the iteration ---------------------------------------------------------------------- */

/* flag = 1 when some x[i] <= 0 or z[i] <= 0 (or is not finite) */
__global__ void k_flag_nonpositive(int q, const double* __restrict__ x, const double* __restrict__ z, int* __restrict__ flag)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i < q && (!(x[i] > 0.0) || !(z[i] > 0.0) || !(x[i] < 1e300) || !(z[i] < 1e300)) )
      atomicExch(flag, 1);
}

/* rp = b * tau - AX[1:] */
__global__ void k_rp(int m, double tau, const double* __restrict__ b, const double* __restrict__ AX, double* __restrict__ rp)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i < m )
      rp[i] = b[i] * tau - AX[1 + i];
}

/* rhs2 = [g ; b] with g = Mx[0, 1:] */
__global__ void k_rhs2(int m, const double* __restrict__ Mx, const double* __restrict__ b, double* __restrict__ rhs2)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i < m )
   {
      rhs2[i] = Mx[1 + i];
      rhs2[m + i] = b[i];
   }
}

/* after the two solves: w = rhs2[0:m], ub = rhs2[m:2m];  u2 = ub - w;  wt = [1, -w] */
__global__ void k_after_solve2(int m, const double* __restrict__ rhs2, double* __restrict__ u2, double* __restrict__ wt)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i == 0 )
      wt[0] = 1.0;
   if ( i < m )
   {
      u2[i] = rhs2[m + i] - rhs2[i];
      wt[1 + i] = -rhs2[i];
   }
}

/* k_after_solve2 and, in the same thread, the two coefficient vectors of the three-vector sweep that hs_make_ext formed behind it:
 * e2 = [s20; s21 u2] from the u2 just stored, e1 = [s10; s11 u1] (u1: the predictor's right-hand side, solved with g and b) */
__global__ void k_after_solve2_ext(int m, const double* __restrict__ rhs2, double* __restrict__ u2, double* __restrict__ wt,
   double s20, double s21, double* __restrict__ e2, double s10, double s11, const double* __restrict__ u1, double* __restrict__ e1)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i == 0 )
   {
      wt[0] = 1.0;
      e2[0] = s20;
      e1[0] = s10;
   }
   if ( i < m )
   {
      const double v = rhs2[m + i] - rhs2[i];
      u2[i] = v;
      wt[1 + i] = -rhs2[i];
      e2[1 + i] = s21 * v;
      e1[1 + i] = s11 * u1[i];
   }
}

/* m <= 64 (single-block factor, dinv = inv(L) as 64 x 64, L = the factor as m x m): rhs2 = [g ; b] with g = Mx[0, 1:], both
 * solves M x = r as x = inv(L)^T (inv(L) r) with each triangular solve corrected once by the factor itself (see RB_SOLVE in
 * kernels.hip: the residual of these solves is primal infeasibility of the step), then u2 = ub - w and wt = [1, -w]: k_rhs2 + the
 * triangular solves + k_after_solve2 in one launch */
__global__ void __launch_bounds__(128) k_solve2_small(int m, const double* __restrict__ Mx, const double* __restrict__ b,
   const double* __restrict__ dinv, const double* __restrict__ L, double* __restrict__ rhs2, double* __restrict__ u2, double* __restrict__ wt,
   int subst)
{
   __shared__ double r[2][64], t[2][64], c[2][64];
   __shared__ double sL[64 * 65];
   const int k = threadIdx.x >> 6, i = threadIdx.x & 63;
   r[k][i] = (i < m) ? (k == 0 ? Mx[1 + i] : b[i]) : 0.0;
   if ( subst )
   {
      /* round 6 (HIPSDP_SMALL_SOLVE=subst): substitution with the factor itself in the oracle's order, one right-hand side per wavefront */
      for (int e = threadIdx.x; e < m * m; e += 128)
      {
         const int ii = e / m, jj = e - ii * m;
         if ( jj <= ii )
            sL[ii * 65 + jj] = L[(long long) ii * m + jj];
      }
      __syncthreads();
      const double x = hs_wl_msolve(sL, m, i, r[k][i]);
      __syncthreads();
      r[k][i] = x;
      __syncthreads();
      if ( i < m )
         rhs2[k * m + i] = x;
      if ( k == 0 )
      {
         if ( i == 0 )
            wt[0] = 1.0;
         if ( i < m )
         {
            u2[i] = r[1][i] - r[0][i];
            wt[1 + i] = -r[0][i];
         }
      }
      return;
   }
   __syncthreads();
   /* forward: t = Y r, c = r - L t, t += Y c */
   double acc = 0.0;
   if ( i < m )
      for (int j = 0; j <= i; ++j)
         acc += dinv[i * 64 + j] * r[k][j];
   t[k][i] = acc;
   __syncthreads();
   double res = 0.0;
   if ( i < m )
   {
      for (int j = 0; j <= i; ++j)
         res += L[(long long) i * m + j] * t[k][j];
      res = r[k][i] - res;
   }
   c[k][i] = res;
   __syncthreads();
   double cor = 0.0;
   if ( i < m )
      for (int j = 0; j <= i; ++j)
         cor += dinv[i * 64 + j] * c[k][j];
   __syncthreads();
   t[k][i] = acc + cor;
   __syncthreads();
   /* backward: r = Y^T t, c = t - L^T r, r += Y^T c */
   acc = 0.0;
   if ( i < m )
      for (int j = i; j < m; ++j)
         acc += dinv[j * 64 + i] * t[k][j];
   r[k][i] = acc;
   __syncthreads();
   res = 0.0;
   if ( i < m )
   {
      for (int j = i; j < m; ++j)
         res += L[(long long) j * m + i] * r[k][j];
      res = t[k][i] - res;
   }
   c[k][i] = res;
   __syncthreads();
   cor = 0.0;
   if ( i < m )
      for (int j = i; j < m; ++j)
         cor += dinv[j * 64 + i] * c[k][j];
   __syncthreads();
   r[k][i] = acc + cor;
   __syncthreads();
   if ( i < m )
      rhs2[k * m + i] = r[k][i];
   if ( k == 0 )
   {
      if ( i == 0 )
         wt[0] = 1.0;
      if ( i < m )
      {
         u2[i] = r[1][i] - r[0][i];
         wt[1 + i] = -r[0][i];
      }
   }
}

int hs_solve2_small(hipStream_t st, int m, const double* Mx, const double* b, const double* dinv, const double* L, double* rhs2, double* u2,
   double* wt, int subst)
{
   hipLaunchKernelGGL(k_solve2_small, dim3(1), dim3(128), 0, st, m, Mx, b, dinv, L, rhs2, u2, wt, subst);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

/* h = AH[1:] - eta * rp */
__global__ void k_h(int m, double eta, const double* __restrict__ AH, const double* __restrict__ rp, double* __restrict__ h)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i < m )
      h[i] = AH[1 + i] - eta * rp[i];
}

/* dtau = num / den, dy = u1 - u2 * dtau, dyt = [-dtau, dy], dkappa */
__global__ void k_finish_dir(int m, double eta, double rg, double sigmu, double tau, double kappa, double etk,
   const double* __restrict__ u1, const double* __restrict__ u2, double* __restrict__ dy, double* __restrict__ dyt,
   double* __restrict__ sc)
{
   const double den = sc[SC_S0] + kappa / tau + sc[SC_BUB];
   const double num = -eta * rg + (sigmu - tau * kappa - etk) / tau - sc[SC_BH] - eta * sc[SC_WRP] + sc[SC_BU1];
   const double dtau = num / den;
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i == 0 )
   {
      sc[SC_DTAU] = dtau;
      sc[SC_DKAPPA] = (sigmu - tau * kappa - etk - kappa * dtau) / tau;
      sc[SC_DEN] = den;
      dyt[0] = -dtau;
   }
   if ( i < m )
   {
      const double v = u1[i] - u2[i] * dtau;
      dy[i] = v;
      dyt[1 + i] = v;
   }
}

/* dZ = P1 - dtau P2 + eta Rd with dtau read from the scalar block (P1 is handed over in dZ) */
__global__ void k_dz_combine(long long n2, double* __restrict__ dZ, const double* __restrict__ P2, const double* __restrict__ sc, double eta,
   const double* __restrict__ Rd)
{
   const double dtau = sc[SC_DTAU];
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long) gridDim.x * blockDim.x)
      dZ[i] = (dZ[i] - dtau * P2[i]) + eta * Rd[i];
}

/* out = Rd + tau * A0  (certificate residual A^T y - Z) */
__global__ void k_cert(long long n2, double tau, const double* __restrict__ Rd, const double* __restrict__ A0, double* __restrict__ out)
{
   for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (long long) gridDim.x * blockDim.x)
      out[i] = Rd[i] + tau * A0[i];
}

static inline dim3 g1d(long long n) { long long g = (n + 255) / 256; if ( g < 1 ) g = 1; if ( g > 4096 ) g = 4096; return dim3((unsigned) g); }

/* The scalars of a direction and its closing kernel: BH = sum <B_k, H_k> + beta^T hl, w^T rp, b^T u1, then dtau, dkappa, dy, dyt.
 * fuse_solve: the solve with the single-block factor of M is the first record.  tail (general path, see general_tail): the first stage
 * of every <B_k, H_k> is a launch, everything else - the fill, the second stages, the dots over m, the closing kernel as a record
 * with a loop over m - is the batch's one launch; the partial sums are combined in the order of the separate launches */
int hs_ipm_dir_tail(hipStream_t st, const hs_dir_tail_args* a, int tail, int fuse_solve)
{
   const int m = a->m;
   hs_red_batch_begin(st);
   if ( fuse_solve )
      (void) hs_red_batch_solve(st, m, a->dinvm, a->Lm, 1, a->u1, m);
   HS_CALL( hs_fill_scalar(st, a->sc + SC_BH, 0.0) );
   for (int k = 0; k < a->K; ++k)
   {
      const long long n2 = (long long) a->n[k] * a->n[k];
      if ( tail )
         HS_CALL( hs_dot_deferred(st, n2, a->B[k], a->H[k], a->sc + SC_BH, 1, a->red_ws, k) );
      else
         HS_CALL( hs_dot(st, n2, a->B[k], a->H[k], a->sc + SC_BH, 1, a->red_ws) );
   }
   if ( a->q > 0 )
      HS_CALL( hs_dot(st, a->q, a->beta, a->hl, a->sc + SC_BH, 1, a->red_ws) );
   HS_CALL( hs_dot(st, m, a->rhs2, a->rp, a->sc + SC_WRP, 0, a->red_ws) );       /* w = rhs2[0:m] */
   HS_CALL( hs_dot(st, m, a->b, a->u1, a->sc + SC_BU1, 0, a->red_ws) );
   bool finished = false;
   if ( fuse_solve || tail )
   {
      hs_rb_finish F = {m, a->eta, a->rg, a->sigmu, a->tau, a->kappa, a->etk, a->u1, a->u2, a->dy, a->dyt, a->sc,
         SC_S0, SC_BUB, SC_BH, SC_WRP, SC_BU1, SC_DTAU, SC_DKAPPA, SC_DEN};
      finished = hs_red_batch_finish(st, &F, sizeof(F)) == 1;
   }
   HS_CALL( hs_red_batch_end() );
   if ( !finished )
   {
      HS_CALL( hs_red_batch_flush() );
      hipLaunchKernelGGL(k_finish_dir, g1d(m > 0 ? m : 1), dim3(256), 0, st, m, a->eta, a->rg, a->sigmu, a->tau, a->kappa, a->etk,
         a->u1, a->u2, a->dy, a->dyt, a->sc);
      HS_LAUNCH_CHECK();
   }
   return HS_OK;
}

/* after the two (three) solves with M: u2 and wt; fused: with the coefficient vectors e2 = [1; u2], e1 = [0; u1] of the three-vector
 * sweep from the same launch (hs_make_ext twice behind it otherwise; e2 == NULL: neither) */
int hs_ipm_after_solve2(hipStream_t st, int m, const double* rhs2, double* u2, double* wt, const double* u1, double* e2, double* e1, int fused)
{
   if ( fused && e2 != NULL )
   {
      hipLaunchKernelGGL(k_after_solve2_ext, g1d(m + 1), dim3(256), 0, st, m, rhs2, u2, wt, 1.0, 1.0, e2, 0.0, 1.0, u1, e1);
      HS_LAUNCH_CHECK();
      return HS_OK;
   }
   hipLaunchKernelGGL(k_after_solve2, g1d(m + 1), dim3(256), 0, st, m, rhs2, u2, wt);
   HS_LAUNCH_CHECK();
   if ( e2 != NULL )
   {
      HS_CALL( hs_make_ext(st, m, 1.0, 1.0, u2, e2) );
      HS_CALL( hs_make_ext(st, m, 0.0, 1.0, u1, e1) );
   }
   return HS_OK;
}

/* dZ = (dZ - dtau P2) + eta Rd with dtau out of the scalar block */
int hs_ipm_dz_combine(hipStream_t st, long long n2, double* dZ, const double* P2, const double* sc, double eta, const double* Rd)
{
   HS_CALL( hs_red_batch_flush() );
   hipLaunchKernelGGL(k_dz_combine, g1d(n2), dim3(256), 0, st, n2, dZ, P2, sc, eta, Rd);
   HS_LAUNCH_CHECK();
   return HS_OK;
}

int hs_ipm_sc_dtau(void) { return SC_DTAU; }
int hs_ipm_sc_len(int nblocks) { return SC_FIXED_END + 8 * (nblocks > 0 ? nblocks : 1) + 8; }

/* ---- GEMM convenience ------------------------------------------------------------------------------------------ */
static int gemm_on(hipStream_t st, int layA, int layB, int M, int N, int K, double alpha, const double* A, long long lda,
   const double* B, long long ldb, double beta, double* C, long long ldc, int flags = 0)
{
   (void) hs_red_batch_flush();          /* inside a held region: behind the records */
   hs_gemm_args g = {M, N, K, layA, layB, A, lda, 0, B, ldb, 0, C, ldc, 0, alpha, beta, 1, flags, 1, NULL};
   return hs_dgemm(st, &g);
}

static int gemm(hipsdp_solver* s, int layA, int layB, int M, int N, int K, double alpha, const double* A, long long lda,
   const double* B, long long ldb, double beta, double* C, long long ldc, int flags = 0)
{
   return gemm_on(s->stream, layA, layB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, flags);
}

/* fork: stream2 starts after everything queued on stream so far; join: stream continues after stream2 has drained */
static int fork2(hipsdp_solver* s)
{
   if ( !s->use2 )
      return HS_OK;
   s->busy2 = true;
   HS_HIP( hipEventRecord(s->evFork, s->stream) );
   HS_HIP( hipStreamWaitEvent(s->stream2, s->evFork, 0) );
   return HS_OK;
}

static int join2(hipsdp_solver* s)
{
   if ( !s->use2 )
      return HS_OK;
   s->busy2 = false;
   HS_HIP( hipEventRecord(s->evJoin, s->stream2) );
   HS_HIP( hipStreamWaitEvent(s->stream, s->evJoin, 0) );
   return HS_OK;
}

/* ---- Schur workspace ------------------------------------------------------------------------------------------------ */
static int ensure_schur_ws(hipsdp_solver* s)
{
   if ( s->sws.T != NULL )
      return HS_OK;
   {
      /* every block kept as nonzeros: the assembly needs no GEMM workspace (the split-K slabs alone would be 64 (m + 1)^2 doubles) */
      bool anydense = false;
      for (auto& B : s->blk) anydense = anydense || !B.sparse;
      if ( !anydense && !s->blk.empty() )
         return HS_OK;
   }
   const int m1 = s->m + 1;
   long long n2max = 1;
   for (auto& B : s->blk) { const long long n2 = (long long) B.n * B.n; if ( !B.sparse && n2 > n2max ) n2max = n2; }
   double budget = s->par.ws_gbytes > 0.0 ? s->par.ws_gbytes : 40.0;
   const char* env = getenv("HIPSDP_WS_GB");
   if ( env != NULL && atof(env) > 0.0 )
      budget = atof(env);
   else if ( s->par.ws_gbytes <= 0.0 && s->comm == NULL )
   {
      /* one rank, nothing prescribed: three quarters of what is free now (A and its packed copy are allocated), at least the
       * default - wider slices and fewer of them when the whole T, W pair does not fit (several ranks keep the fixed default:
       * every rank must derive the same slicing) */
      size_t fr = 0, tot = 0;
      if ( hipMemGetInfo(&fr, &tot) == hipSuccess && 0.75e-9 * (double) fr > budget )
         budget = 0.75e-9 * (double) fr;
   }
   const char* mode = getenv("HIPSDP_SCHUR");
   s->schur_mode_cols = false;
   s->schur_sim_shards = 0;
   if ( s->shardA )
   {
      /* Matrices sharded by variable: the W_j are formed where A_j lives, in S column slices of at most cw columns; the three
       * buffers of a slice (T and W of the own variables, the received row range of all W_j) take about 3 (m1 / ranks) n cw
       * doubles.  The widest slice that fits the budget (a multiple of 128, or all n columns); same numbers on every rank. */
      int nmaxb = 1;
      for (auto& B : s->blk) if ( B.n > nmaxb ) nmaxb = B.n;
      /* overlapped exchange (default; HIPSDP_VAR_OVERLAP=0: slice after slice): a second send and a second receive buffer */
      static const bool var_overlap = !(getenv("HIPSDP_VAR_OVERLAP") != NULL && getenv("HIPSDP_VAR_OVERLAP")[0] == '0');
      const double per_col = (var_overlap ? 5.0 : 3.0) * 8.0 * (double) ((m1 + s->nranks - 1) / s->nranks + 1) * (double) nmaxb;
      long long cw = (long long) (budget * 1e9 / per_col);
      const char* ecw = getenv("HIPSDP_VAR_SLICE");          /* test hook: force narrow slices */
      if ( ecw != NULL && atoi(ecw) > 0 )
         cw = atoi(ecw);
      else if ( cw < nmaxb )
         cw = cw / 128 * 128 > 0 ? cw / 128 * 128 : 128;
      if ( cw > nmaxb ) cw = nmaxb;
      s->var_cw = (int) cw;
      HS_CALL( hs_schur_ws_alloc_var(&s->sws, m1, s->nranks, nmaxb, (int) cw) );
      s->var_overlap = false;
      if ( var_overlap && cw < nmaxb )                /* (one slice: nothing to overlap with) */
         s->var_overlap = (hs_schur_ws_alloc_var_overlap(&s->sws) == HS_OK);
      s->schur_mode_U = false; s->schur_mode_rows = false; s->schur_mode_forced = true;
      return HS_OK;
   }
   /* Column slices of the W formulation: S slices in total, every rank works through S / ranks of them one after the other
    * (one rank: all of them).  S = ranks when the workspace for one slice fits the budget, otherwise the smallest multiple
    * that does - this is also how one GPU keeps the cheaper W formulation when T and W do not fit as a whole (n = 2000,
    * m = 4000: 2 x 128 GB).  The workspace holds the widest slice; every rank derives the same numbers, so all ranks take
    * the same branch (the two sharded forms use different collectives). */
   const int ranks = s->comm != NULL ? s->nranks : 1;
   auto widest = [&](int S) -> long long {
      long long w = 1;
      for (auto& B : s->blk)
         for (int g = 0; g < S; ++g)
         {
            int c0, cw;
            hs_shard_cols(m1, B.n, S, g, &c0, &cw);
            if ( (long long) B.n * cw > w ) w = (long long) B.n * cw;
         }
      return w;
   };
   int S = 0;
   if ( s->comm == NULL && mode != NULL && mode[0] == 'K' && atoi(mode + 1) >= 1 && atoi(mode + 1) <= 64 )
      S = atoi(mode + 1);
   else if ( !(mode != NULL && (mode[0] == 'R' || mode[0] == 'U')) && (mode == NULL || s->comm != NULL) )
   {
      const bool whole_fits = 2.0 * 8.0 * (double) m1 * (double) n2max <= budget * 1e9;
      if ( s->comm != NULL || !whole_fits )
         for (int k = 1; k * ranks <= 64; ++k)
            if ( (s->comm != NULL || k > 1) && 2.0 * 8.0 * (double) m1 * (double) widest(k * ranks) <= budget * 1e9 )
            {
               S = k * ranks;
               break;
            }
   }
   if ( S > 0 && 2.0 * 8.0 * (double) m1 * (double) widest(S) <= budget * 1e9 )
   {
      HS_CALL( hs_schur_ws_alloc(&s->sws, m1, widest(S), budget) );
      s->schur_mode_cols = true;
      s->schur_sim_shards = S;
   }
   if ( !s->schur_mode_cols )
      HS_CALL( hs_schur_ws_alloc(&s->sws, m1, n2max, budget) );
   s->schur_mode_U = (mode != NULL && mode[0] == 'U') || !s->sws.full || s->comm != NULL;
   s->schur_mode_rows = (mode != NULL && mode[0] == 'R');
   s->schur_mode_forced = (mode != NULL);
   if ( s->comm != NULL && s->Mgather == NULL )
   {
      const long long c = (m1 + 2 * s->nranks - 1) / (2 * s->nranks);
      HS_CALL( dalloc(&s->Mgather, c * m1 * s->nranks) );
   }
   return HS_OK;
}

/* ---- the solve ---------------------------------------------------------------------------------------------------- */

struct HostScalars
{
   std::vector<double> v;
};

int hs_bcast_doubles(void* comm, double* buf, long long count, hipStream_t stream);
int hs_bcast_ints(void* comm, int* buf, long long count, hipStream_t stream);

/* Read-back without a copy engine and without a stream synchronisation: a kernel stores n doubles of sc to the host mirror
 * and then a sequence number; the host polls the number (coherent pinned memory).  The stream is queried now and then so
 * that a failed launch cannot leave the host spinning. */
static int publish_and_wait(hipsdp_solver* s, int off, int n, const std::function<int()>* between = NULL)
{
   const unsigned long long seq = ++s->pub_seq;
   volatile unsigned long long* flag = reinterpret_cast<volatile unsigned long long*>(s->hsc + s->hsc_cap - 1);
   HS_CALL( hs_red_batch_end_publish(s->stream, n, s->sc + off, s->hsc_dev + off, seq,
         reinterpret_cast<unsigned long long*>(s->hsc_dev + s->hsc_cap - 1)) );
   /* work that does not depend on what the host is about to read goes into the queue now: the device runs it while the scalars
    * travel, the host decides and the next launches arrive */
   if ( between != NULL )
      HS_CALL( (*between)() );
   /* developer switch HIPSDP_WAIT_TIMES=1: how long the host waits here in total (at process end): the share of a solve in which the
    * device is the one being waited for */
   static int wt = -1;
   if ( wt < 0 )
      wt = (getenv("HIPSDP_WAIT_TIMES") != NULL && getenv("HIPSDP_WAIT_TIMES")[0] == '1') ? 1 : 0;
   const std::chrono::steady_clock::time_point w0 = wt ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point();
   struct WaitNote
   {
      bool on; std::chrono::steady_clock::time_point t0;
      ~WaitNote()
      {
         if ( !on ) return;
         static double total = 0.0; static long long count = 0; static bool hooked = false;
         static double* ptot = &total; static long long* pcnt = &count;
         total += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
         ++count;
         if ( !hooked )
         {
            hooked = true;
            atexit([]() { fprintf(stderr, "hipsdp: %lld read-backs, the host waited %.3f s in them (%.2f us each)\n", *pcnt, *ptot, 1e6 * *ptot / (double) (*pcnt > 0 ? *pcnt : 1)); });
         }
      }
   } note = {wt != 0, w0};
   long long spins = 0;
   while ( *flag != seq )
   {
      if ( (++spins & 0x3FFF) == 0 )
      {
         const hipError_t e = hipStreamQuery(s->stream);
         if ( e == hipSuccess )
         {
            if ( *flag == seq )
               break;
            HS_HIP( hipStreamSynchronize(s->stream) );
            if ( *flag != seq )
            {
               set_err("read-back kernel finished without publishing its results");
               return HS_ERR_HIP;
            }
            break;
         }
         if ( e != hipErrorNotReady )
         {
            hs_record_hip_error(e, "hipStreamQuery(read-back)", __FILE__, __LINE__);
            return HS_ERR_HIP;
         }
      }
   }
   __atomic_thread_fence(__ATOMIC_ACQUIRE);
   return HS_OK;
}

static int read_scalars(hipsdp_solver* s, HostScalars& h, int* flags3, const std::function<int()>* between = NULL)
{
   if ( s->comm != NULL )
      HS_CALL( hs_red_batch_end_all() );  /* recorded operations must run before the scalars are read */
   h.v.resize(s->nsc);
   if ( s->comm != NULL )
   {
      /* all ranks computed the same numbers; broadcasting rank 0's copy makes the control flow identical by construction */
      /* the flags live right behind the scalars: one broadcast covers both */
      HS_CALL( hs_bcast_doubles(s->comm, s->sc, s->nsc + (flags3 != NULL ? 2 : 0), s->stream) );
   }
   if ( s->comm == NULL )
   {
      /* the batch kernel (or a one-block kernel when the batch is empty) stores the scalars to the host mirror itself */
      HS_CALL( publish_and_wait(s, 0, s->nsc + 4, between) );
   }
   else
   {
      HS_HIP( hipMemcpyAsync(s->hsc, s->sc, (size_t) (s->nsc + (flags3 != NULL ? 4 : 0)) * sizeof(double), hipMemcpyDeviceToHost, s->stream) );
      if ( between != NULL )
         HS_CALL( (*between)() );
      HS_HIP( hipStreamSynchronize(s->stream) );
   }
   memcpy(h.v.data(), s->hsc, (size_t) s->nsc * sizeof(double));
   if ( flags3 != NULL )
      memcpy(flags3, s->hsc + s->nsc, 3 * sizeof(int));
   return HS_OK;
}

/* the two passes over the constraint matrices of one block; with a packed copy they move half the bytes */
static int ensure_sparse(hipsdp_solver* s);
static int ensure_packed(hipsdp_solver* s)
{
   HS_CALL( ensure_sparse(s) );
   for (auto& B : s->blk)
   {
      if ( B.Apk != NULL && !B.apk_valid )
      {
         if ( s->a_r1 > s->a_r0 )
            HS_CALL( hs_pack_rows(s->stream, s->a_r1 - s->a_r0, B.n, B.Lp, B.Aown, B.Apkown) );
         a_written(s, B);       /* (the packed copy is an operand of the cached assembly too: rebuilt counts as written) */
         B.apk_valid = true;
      }
   }
   return HS_OK;
}

int hs_allreduce_sum(void* comm, double* buf, long long count, hipStream_t stream);

/* Several ranks: a pass over the constraint matrices of a block is HBM-bound and every rank holds all of A, so each rank
 * sweeps only its ceil(m1 / ranks) matrices: A(V) is completed by an all-gather of m1 numbers, A^T(coef) by an all-reduce of
 * the (packed) n x n partial sums.  Every rank decides from the sizes alone (same decision everywhere). */
static bool passes_sharded(const hipsdp_solver* s, const Block& B)
{
   if ( s->comm == NULL || B.sparse )
      return false;
   if ( s->shardA )
      return true;              /* the only rows there are (hs_var_rows is the row split of the sharded passes) */
   if ( s->nranks < 2 )
      return s->shard_passes == 1;        /* a communicator of one rank: only when forced (exercises the collectives) */
   if ( s->shard_passes >= 0 )
      return s->shard_passes != 0;
   return 8.0 * (double) (s->m + 1) * (double) B.n * (double) B.n >= 64e6;
}

static void pass_rows(const hipsdp_solver* s, int* chunk, int* r0, int* r1)
{
   const int m1 = s->m + 1;
   const int c = (m1 + s->nranks - 1) / s->nranks;
   *chunk = c;
   *r0 = s->rank * c < m1 ? s->rank * c : m1;
   *r1 = *r0 + c < m1 ? *r0 + c : m1;
}

/* sparse blocks: the triplets collected since the last build become the device structure */
static int ensure_sparse(hipsdp_solver* s)
{
   for (auto& B : s->blk)
      if ( B.sparse && (B.sp_dirty || B.sp == NULL) )
      {
         if ( B.sp_gathered )
         {
            set_err("a block gathered from the master copy lost its structure (the master copy was defined again, or its master block "
               "gathered into another block): load the block again");
            return HS_ERR_ARG;
         }
         if ( B.sp != NULL ) hs_sp_free(B.sp);
         B.sp = NULL;
         HS_HIP( hipStreamSynchronize(s->stream) );
         const SpHost& h = *B.sph;
         HS_CALL( hs_sp_build(&B.sp, B.n, s->m, (long long) h.var.size(), h.var.data(), h.row.data(), h.col.data(), h.val.data()) );
         B.sp_dirty = false;
         ++s->mg_host_builds;
      }
   return HS_OK;
}

int hs_solver_sparse_block(hipsdp_solver* s, int block, const hs_sparse** sp)
{
   *sp = NULL;
   if ( s == NULL || !s->shaped || block < 0 || block >= (int) s->blk.size() || !s->blk[block].sparse )
      return HS_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   HS_CALL( ensure_sparse(s) );
   HS_HIP( hipStreamSynchronize(s->stream) );
   *sp = s->blk[block].sp;
   return HS_OK;
}

/* out = c[0] A0 + sa add (add may be NULL): the dense part of A^T(coef) of a sparse block */
__global__ void k_sp_base(long long n2, const double* __restrict__ c, const double* __restrict__ A0, double sa, const double* __restrict__ add,
   double* __restrict__ out)
{
   const double c0 = c[0];
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < n2; e += (long long) gridDim.x * blockDim.x)
      out[e] = c0 * A0[e] + (add != NULL ? sa * add[e] : 0.0);
}

/* out[0] = <a, b>: one workgroup, fixed summation order */
__global__ void __launch_bounds__(1024) k_sp_dot0(long long n, const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ out)
{
   __shared__ double part[16];
   double acc = 0.0;
   for (long long e = threadIdx.x; e < n; e += 1024)
      acc += a[e] * b[e];
#pragma unroll
   for (int off = 32; off > 0; off >>= 1)
      acc += __shfl_xor(acc, off, 64);
   if ( (threadIdx.x & 63) == 0 )
      part[threadIdx.x >> 6] = acc;
   __syncthreads();
   if ( threadIdx.x == 0 )
   {
      double t = 0.0;
      for (int w = 0; w < 16; ++w)
         t += part[w];
      out[0] = t;
   }
}

/* Mx[i][0] += v[i] (column 0 of the lower triangle) */
__global__ void k_add_col0(int m1, const double* __restrict__ v, double* __restrict__ Mx)
{
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < m1; i += gridDim.x * blockDim.x)
      Mx[(long long) i * m1] += v[i];
}

/* out[m + 1] = <A_i, V>, V symmetric; packed: B.pkv already holds the packed, weighted copy of V (hs_dirmat_pack) */
static int pass_A(hipsdp_solver* s, Block& B, const double* V, double* out, bool packed)
{
   const int m1 = s->m + 1;
   if ( B.sparse )
   {
      /* launched at once like the dense pass (hs_dot would be deferred inside a reduction batch, and callers add the result up
       * with kernels that are not) */
      /* <A_0, V> (A_0 is dense): the row-dot kernel of the dense pass with one row - split over workgroups and combined in order
       * (a single workgroup took 73 us for the 250 000 entries of a block of 500 rows) */
      HS_CALL( hs_gemv_n(s->stream, 1, (long long) B.n * B.n, B.A0, (long long) B.n * B.n, 1, &V, out, 1, s->gemv_ws, s->gemv_ws_len) );
      return hs_sp_apply_A(s->stream, B.sp, V, out + 1);
   }
   if ( passes_sharded(s, B) )
   {
      int c, r0, r1;
      pass_rows(s, &c, &r0, &r1);
      if ( s->passg == NULL )
         HS_CALL( dalloc(&s->passg, (long long) c * s->nranks) );
      double* mine = s->passg + (long long) s->rank * c;
      if ( B.Apk != NULL )
      {
         HS_CALL( hs_pack_weighted(s->stream, B.n, V, B.pkv) );
         const double* v = B.pkv;
         if ( r1 > r0 )
            HS_CALL( hs_gemv_n(s->stream, r1 - r0, B.Lp, B.Apk + (long long) r0 * B.Lp, B.Lp, 1, &v, mine, r1 - r0, s->gemv_ws, s->gemv_ws_len) );
      }
      else if ( r1 > r0 )
      {
         const long long n2 = (long long) B.n * B.n;
         HS_CALL( hs_gemv_n(s->stream, r1 - r0, n2, B.A + (long long) r0 * n2, n2, 1, &V, mine, r1 - r0, s->gemv_ws, s->gemv_ws_len) );
      }
      hs_comm_phase(1);
      const int rcg = hs_allgather_inplace(s->comm, s->passg, c, s->rank, s->stream);
      hs_comm_phase(2);
      HS_CALL( rcg );
      return hs_copy(s->stream, out, s->passg, m1);
   }
   if ( B.Apk != NULL )
   {
      if ( !packed )
         HS_CALL( hs_pack_weighted(s->stream, B.n, V, B.pkv) );
      const double* v = B.pkv;
      return hs_gemv_n(s->stream, m1, B.Lp, B.Apk, B.Lp, 1, &v, out, m1, s->gemv_ws, s->gemv_ws_len);
   }
   return hs_gemv_n(s->stream, m1, (long long) B.n * B.n, B.A, (long long) B.n * B.n, 1, &V, out, m1, s->gemv_ws, s->gemv_ws_len);
}

/* out[n x n] = sum_i coef_i A_i + sa * add */
static int pass_AT(hipsdp_solver* s, Block& B, const double* coef, double sa, const double* add, double* out)
{
   const int m1 = s->m + 1;
   const long long n2 = (long long) B.n * B.n;
   if ( B.sparse )
   {
      hipLaunchKernelGGL(k_sp_base, g1d(n2), dim3(256), 0, s->stream, n2, coef, B.A0, sa, add, out);
      HS_LAUNCH_CHECK();
      return hs_sp_apply_AT(s->stream, B.sp, coef, out);
   }
   if ( passes_sharded(s, B) )
   {
      int c, r0, r1;
      pass_rows(s, &c, &r0, &r1);
      if ( B.Apk != NULL )
      {
         HS_CALL( hs_gemv_t(s->stream, r1 - r0, B.Lp, B.Apk + (long long) r0 * B.Lp, B.Lp, coef + r0, 0.0, NULL, B.pkv + B.Lp) );
         hs_comm_phase(1);
         const int rcr = hs_allreduce_sum(s->comm, B.pkv + B.Lp, B.Lp, s->stream);
         hs_comm_phase(2);
         HS_CALL( rcr );
         return hs_unpack_sym(s->stream, B.n, B.pkv + B.Lp, sa, add, out);
      }
      /* the additive term enters once: on rank 0 */
      HS_CALL( hs_gemv_t(s->stream, r1 - r0, n2, B.A + (long long) r0 * n2, n2, coef + r0, s->rank == 0 ? sa : 0.0,
            s->rank == 0 ? add : NULL, out) );
      hs_comm_phase(1);
      const int rcr = hs_allreduce_sum(s->comm, out, n2, s->stream);
      hs_comm_phase(2);
      return rcr;
   }
   if ( B.Apk != NULL )
   {
      HS_CALL( hs_gemv_t_ws(s->stream, m1, B.Lp, B.Apk, B.Lp, coef, 0.0, NULL, B.pkv + B.Lp, s->gemvt_ws, s->gemvt_ws_len) );
      return hs_unpack_sym(s->stream, B.n, B.pkv + B.Lp, sa, add, out);
   }
   return hs_gemv_t_ws(s->stream, m1, n2, B.A, n2, coef, sa, add, out, s->gemvt_ws, s->gemvt_ws_len);
}

#define AS_MAXBLK HS_AS_MAXBLK

static bool small_problem(const hipsdp_solver* s)
{
   if ( s->blk.size() > AS_MAXBLK || s->q > 4096 || s->m + 1 > 4096 || s->shardA )
      return false;
   long long tot = 0;
   for (auto& B : s->blk)
   {
      /* a block kept as nonzeros (csrc/sparse.hip) has no dense rows A_i: the fused small-problem kernels read A + i n^2 */
      if ( B.Apk != NULL || B.sparse || B.A == NULL )
         return false;
      tot += (long long) B.n * B.n;
   }
   return tot <= 8192;
}

/* B&B-sized problems: runs of small kernels are recorded and executed by one launch (kernels.hip: hs_red_batch_hold).  A region
 * covers a whole direction, or the step of the iterate with the residual pass behind it; HIPSDP_BATCH=0 switches the regions off
 * (every kernel its own launch, as before round 3; same arithmetic either way). */
static bool batch_regions(const hipsdp_solver* s)
{
   static int on = -1;
   if ( on < 0 )
   {
      const char* env = getenv("HIPSDP_BATCH");
      on = (env != NULL && env[0] == '0') ? 0 : 1;
   }
   return on != 0 && s->comm == NULL && small_problem(s);
}

struct BatchRegion
{
   bool on;
   BatchRegion(hipsdp_solver* s, bool want) : on(want) { if ( on ) hs_red_batch_hold(s->stream); }
   int close() { if ( !on ) return HS_OK; on = false; return hs_red_batch_release(); }
   ~BatchRegion() { if ( on ) (void) hs_red_batch_release(); }
};

/* The general path proper - one rank, more than 64 variables, every block above 64 rows, no batch regions: between two Schur assemblies
 * it is a chain of launches of a few microseconds each, so neighbouring launches are merged where the arithmetic per element and
 * the order of every sum stay what they were; every other path keeps its launches */
static bool general_tail(const hipsdp_solver* s)
{
   if ( s->comm != NULL || s->m <= 64 || s->blk.empty() || batch_regions(s) )
      return false;
   for (auto& B : s->blk)
      if ( B.n <= 64 )
         return false;
   return true;
}

/* ... and a block whose sweeps run over the packed rows on this rank alone gets the packed copy of H from the kernel that forms H */
static bool pack_with_dirmat(const hipsdp_solver* s, const Block& B)
{
   return general_tail(s) && B.Apk != NULL && !B.sparse;
}

/* returns 1 when the fused launch was used */
static int apply_A_small(hipsdp_solver* s, double* const* Vk, const double* vlp, double* out, int epi, double scal,
   const double* vin, double* vout)
{
   if ( !small_problem(s) )
      return 0;
   for (auto& Bk : s->blk)
      if ( Bk.A == NULL )
         return 0;
   hs_as_args B;
   B.nblk = (int) s->blk.size();
   for (int k = 0; k < AS_MAXBLK; ++k)
   {
      B.n2[k] = 0; B.A[k] = NULL; B.V[k] = NULL;
   }
   for (size_t k = 0; k < s->blk.size(); ++k)
   {
      B.n2[k] = s->blk[k].n * s->blk[k].n;
      B.A[k] = s->blk[k].A;
      B.V[k] = Vk[k];
   }
   const int rc = hs_apply_A_small(s->stream, s->m + 1, &B, s->q, s->Dext, vlp, out, epi, scal, vin, vout);
   if ( rc != HS_OK )
      return -rc;
   return 1;
}

/* A(V) over all blocks + LP: out[m + 1] = sum_k A_k vec(V_k) + Dext^T vlp */
static int apply_A(hipsdp_solver* s, double* const* Vk, const double* vlp, double* out, bool packed = false)
{
   const int m1 = s->m + 1;
   bool first = true;
   for (size_t k = 0; k < s->blk.size(); ++k)
   {
      Block& B = s->blk[k];
      const double* v = Vk[k];
      double* dst = first ? out : s->tmpe;
      HS_CALL( pass_A(s, B, v, dst, packed && pack_with_dirmat(s, B)) );
      if ( !first )
         HS_CALL( hs_axpy(s->stream, m1, 1.0, s->tmpe, out) );
      first = false;
   }
   if ( first )
      HS_CALL( hs_fill(s->stream, out, m1, 0.0) );
   if ( s->q > 0 )
      HS_CALL( hs_gemv_t(s->stream, s->q, m1, s->Dext, m1, vlp, 1.0, out, out) );
   return HS_OK;
}

/* the engine's two queues trade places for a while: everything enqueued through s->stream goes to the second queue */
struct QueueSwap
{
   hipsdp_solver* s;
   explicit QueueSwap(hipsdp_solver* s_) : s(s_) { std::swap(s->stream, s->stream2); }
   ~QueueSwap() { std::swap(s->stream, s->stream2); }
};

/* one Newton direction; results in (dy, dyt, SC_DTAU, SC_DKAPPA), B.dX, B.dZ, s->dx, s->dz.
 * part 0: all of it.  part 1: only the right-hand side H_k, hl, A(H) and h = A(H) - eta rp (general path; it needs X, Z^-1 and the
 * residuals but not the Schur matrix, so the predictor's can run on the second queue beside the factorization of M);
 * part 2: the rest, after a part-1 call with the same arguments. */
/* split: 0 = dZ by one pass with the coefficients [-dtau; dy]; 1 = dZ = P1 - dtau P2 + eta Rd with P1 = A^T([0; u1]) computed here
 * by one pass and P2 = A^T([1; u2]) from the three-vector sweep of this iteration; 2 = P1 has been computed by that sweep as well
 * (the predictor: its u1 was solved together with the right-hand sides of the tau elimination) */
/* mode of the triangular solves with the factor of M: forward + backward (3), corrected (4).  They go block by block as
 * x = inv(L_bb) r, whose residual grows with cond(L_bb) and ends up as primal infeasibility of the step; each of them is corrected
 * once with the factor itself (about 0.3 % of a solve at n = 500, m = 1000). */
static const int SOLVE_MODE = 3 | 4;

static int direction(hipsdp_solver* s, double sigma, double eta, double mu, double rg, bool useE, double etk, int part = 0,
   bool u1_solved = false, int split = 0)
{
   const int m = s->m, m1 = s->m + 1, q = s->q;
   const double sigmu = sigma * mu;
   std::vector<double*> Hs;
   int fusedA = 0;
   BatchRegion region(s, part == 0 && batch_regions(s));
   if ( part != 2 )
   {
   for (auto& B : s->blk)
   {
      const int n = B.n;
      const long long n2 = (long long) n * n;
      if ( n <= HS_SMALL_N )
         HS_CALL( hs_dir_block_small(s->stream, n, eta, B.X, B.Rd, useE ? B.E : NULL, B.Zinv, sigmu, B.H) );
      else
      {
         if ( useE )
            HS_CALL( hs_copy(s->stream, B.G, B.E, n2) );
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, eta, B.X, n, B.Rd, n, useE ? 1.0 : 0.0, B.G, n) );
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, 1.0, B.G, n, B.Zinv, n, 0.0, B.GZ, n) );
         if ( pack_with_dirmat(s, B) )
            HS_CALL( hs_dirmat_pack(s->stream, n, sigmu, B.Zinv, B.X, B.GZ, B.H, B.pkv) );    /* (pass_A below: packed) */
         else
            HS_CALL( hs_dirmat(s->stream, n, sigmu, B.Zinv, B.X, B.GZ, B.H) );
      }
      Hs.push_back(B.H);
   }
   if ( q > 0 )
      HS_CALL( hs_lp_dir(s->stream, q, sigmu, eta, s->x, s->z, s->rd, useE ? s->elp : NULL, s->hl) );
   fusedA = part == 1 ? 0 : apply_A_small(s, Hs.data(), s->hl, s->AH, 1, eta, s->rp, s->u1);
   if ( fusedA < 0 )
      return -fusedA;
   if ( fusedA == 0 )
      HS_CALL( apply_A(s, Hs.data(), s->hl, s->AH, true) );
   if ( fusedA == 0 && m > 0 )
   {
      HS_CALL( hs_red_batch_flush() );
      hipLaunchKernelGGL(k_h, g1d(m), dim3(256), 0, s->stream, m, eta, s->AH, s->rp, s->u1);
      HS_LAUNCH_CHECK();
   }
   if ( part == 1 )
      return HS_OK;
   }
   const bool fuse_solve = (fusedA == 1) && m > 0 && m <= 64;      /* single-block factor of M: solve, reductions and closing kernel in one launch */
   if ( m > 0 && !fuse_solve && !u1_solved )
   {
      HS_CALL( hs_red_batch_flush() );
      HS_CALL( hs_trsv_sync(s->stream, m, s->Lm, s->dinvm, 1, s->u1, m, SOLVE_MODE, s->trsv_ws, &s->trsv_epoch) );
   }
   /* BH = sum <B_k, H_k> + beta^T hl ; wrp ; bu1 ; dtau, dkappa, dy */
   {
      std::vector<int> bn;
      std::vector<const double*> bB, bH;
      for (auto& B : s->blk)
      {
         bn.push_back(B.n); bB.push_back(B.B); bH.push_back(B.H);
      }
      const hs_dir_tail_args ta = {m, q, (int) s->blk.size(), bn.data(), bB.data(), bH.data(), s->beta, s->hl, s->rhs2, s->rp, s->b, s->u1, s->u2,
         s->dy, s->dyt, s->sc, s->red_ws, s->dinvm, s->Lm, eta, rg, sigmu, s->tau, s->kappa, etk};
      HS_CALL( hs_ipm_dir_tail(s->stream, &ta, general_tail(s) ? 1 : 0, fuse_solve ? 1 : 0) );
   }
   for (auto& B : s->blk)
   {
      const int n = B.n;
      const long long n2 = (long long) n * n;
      if ( split == 0 )
         HS_CALL( pass_AT(s, B, s->dyt, eta, B.Rd, B.dZ) );
      else
      {
         bool combined = false;
         if ( split == 1 )
         {
            if ( &B == &s->blk[0] )
            {
               HS_CALL( hs_make_ext(s->stream, m, 0.0, 1.0, s->u1, s->cvec + m1) );
               HS_LAUNCH_CHECK();
            }
            if ( pack_with_dirmat(s, B) )
            {
               /* pass_AT over the packed rows, its hs_unpack_sym and k_dz_combine in one launch behind the sweep */
               HS_CALL( hs_gemv_t_ws(s->stream, m1, B.Lp, B.Apk, B.Lp, s->cvec + m1, 0.0, NULL, B.pkv + B.Lp, s->gemvt_ws, s->gemvt_ws_len) );
               HS_CALL( hs_unpack_dz_combine(s->stream, n, B.pkv + B.Lp, B.P2, s->sc, SC_DTAU, eta, B.Rd, B.dZ) );
               combined = true;
            }
            else
               HS_CALL( pass_AT(s, B, s->cvec + m1, 0.0, NULL, B.dZ) );
         }
         if ( !combined )
            HS_CALL( hs_ipm_dz_combine(s->stream, n2, B.dZ, B.P2, s->sc, eta, B.Rd) );
      }
      if ( n <= HS_SMALL_N )
         HS_CALL( hs_dir_block_small(s->stream, n, 1.0, B.X, B.dZ, useE ? B.E : NULL, B.Zinv, sigmu, B.dX) );
      else
      {
         if ( useE )
            HS_CALL( hs_copy(s->stream, B.G, B.E, n2) );
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, 1.0, B.X, n, B.dZ, n, useE ? 1.0 : 0.0, B.G, n) );
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, 1.0, B.G, n, B.Zinv, n, 0.0, B.GZ, n) );
         HS_CALL( hs_dirmat(s->stream, n, sigmu, B.Zinv, B.X, B.GZ, B.dX) );
      }
   }
   if ( q > 0 )
   {
      if ( small_problem(s) )
      {
         HS_CALL( hs_lp_rows_small(s->stream, q, m1, s->Dext, s->dyt, 1, eta, sigmu, s->x, s->z,
            s->rd, useE ? s->elp : NULL, s->dz, s->dx) );
      }
      else
      {
         const double* v = s->dyt;
         HS_CALL( hs_gemv_n(s->stream, q, m1, s->Dext, m1, 1, &v, s->tmpq, q, s->gemv_ws, s->gemv_ws_len) );
         HS_CALL( hs_scale_add(s->stream, q, 1.0, s->tmpq, eta, s->rd, s->dz) );
         HS_CALL( hs_lp_dir(s->stream, q, sigmu, 1.0, s->x, s->z, s->dz, useE ? s->elp : NULL, s->dx) );
      }
   }
   return region.close();
}

/* enqueue the step-length estimates for the current direction */
static int steplen_enqueue(hipsdp_solver* s)
{
   int k = 0;
   hipStream_t st = s->stream, st2 = s->use2 ? s->stream2 : s->stream;
   HS_CALL( fork2(s) );
   for (auto& B : s->blk)
   {
      const int n = B.n;
      if ( n <= 64 )
         continue;                   /* products and eigenvalues of small blocks share one launch below */
      HS_CALL( gemm_on(st, HS_KC, HS_MC, n, n, n, 1.0, B.LxInv, n, B.dX, n, 0.0, B.T1, n) );
      HS_CALL( gemm_on(st, HS_KC, HS_KC, n, n, n, 1.0, B.T1, n, B.LxInv, n, 0.0, B.W, n) );
      HS_CALL( gemm_on(st2, HS_KC, HS_MC, n, n, n, 1.0, B.LzInv, n, B.dZ, n, 0.0, B.T2, n) );
      HS_CALL( gemm_on(st2, HS_KC, HS_KC, n, n, n, 1.0, B.T2, n, B.LzInv, n, 0.0, B.W2, n) );
   }
   HS_CALL( join2(s) );
   /* the X-side and the Z-side eigenvalue of a block run in the same launch */
   int nmax_blk = 0;
   for (auto& B : s->blk)
      if ( B.n > nmax_blk ) nmax_blk = B.n;
   /* blocks of at most 64 rows: ONE launch per size class (<= 16: exact, 17 .. 64: Lanczos in LDS) for all of them together - with
    * twenty blocks of fifty rows the forty two-workgroup launches of an iteration were 39 % of it (round 3) */
   for (int cls = 0; cls < 2; ++cls)
   {
      hs_step_jobs J;
      J.nblk = 0;
      int kk = 0;
      for (auto& B : s->blk)
      {
         const bool mine = (cls == 0) ? (B.n <= 16) : (B.n > 16 && B.n <= 64);
         if ( mine )
         {
            const int j = J.nblk++;
            J.n[j] = B.n; J.L0[j] = B.LxInv; J.D0[j] = B.dX; J.L1[j] = B.LzInv; J.D1[j] = B.dZ;
            J.res0[j] = s->sc + SC_BLK(kk, 1); J.res1[j] = s->sc + SC_BLK(kk, 4);
            if ( J.nblk == HS_STEP_MAXJOBS )
            {
               HS_CALL( hs_steplen_small_multi(st, &J, s->par.lanczos_steps) );
               J.nblk = 0;
            }
         }
         ++kk;
      }
      HS_CALL( hs_steplen_small_multi(st, &J, s->par.lanczos_steps) );
   }
   for (auto& B : s->blk)
   {
      if ( B.n > 64 )
         HS_CALL( hs_lanczos_lmin2(st, B.n, B.W, B.W2, s->par.lanczos_steps, s->sc + SC_BLK(k, 1), s->sc + SC_BLK(k, 4), s->lan_ws,
               s->lan_ws2, s->lan_rot, s->lan_sync, nmax_blk) );
      ++k;
   }
   hs_red_batch_begin(s->stream);
   HS_CALL( hs_ratio_min(s->stream, s->q, s->x, s->dx, s->sc + SC_RATX, 0, s->red_ws) );
   HS_CALL( hs_ratio_min(s->stream, s->q, s->z, s->dz, s->sc + SC_RATZ, 0, s->red_ws) );
   /* the batch stays open: both callers read the scalars next, and the read-back's launch executes the records and stores
    * the results to the host in one go (read_scalars closes the batch either way) */
   return HS_OK;
}

static double steplen_host(hipsdp_solver* s, const HostScalars& h)
{
   double a = 1e300;
   for (size_t k = 0; k < s->blk.size(); ++k)
   {
      for (int which = 0; which < 2; ++which)
      {
         const double theta = h.v[SC_BLK(k, which ? 4 : 1)];
         const double resid = h.v[SC_BLK(k, which ? 5 : 2)];
         const double lo = theta - resid;          /* pessimistic smallest eigenvalue */
         if ( lo < 0.0 )
            a = fmin(a, -1.0 / lo);
      }
   }
   a = fmin(a, fmin(h.v[SC_RATX], h.v[SC_RATZ]));
   const double dtau = h.v[SC_DTAU], dkap = h.v[SC_DKAPPA];
   if ( dtau < 0.0 ) a = fmin(a, -s->tau / dtau);
   if ( dkap < 0.0 ) a = fmin(a, -s->kappa / dkap);
   return a;
}

/* Several ranks and a small problem: sharding an assembly of less than about 2 * 10^10 flops costs more in collectives than it
 * saves, and the single-launch kernels of the B&B-sized regime only exist for one rank.  Every rank then runs the whole solve on
 * its own (identical deterministic arithmetic) and ONE exchange at the end makes rank 0's outcome the outcome everywhere - which
 * also covers the one thing that can differ between the ranks, the clock behind the time limit. */
static bool replicate_small(const hipsdp_solver* s)
{
   if ( s->comm == NULL || s->nranks < 2 || s->shardA )
      return false;
   double lim = 2e10;
   const char* e = getenv("HIPSDP_SHARD_MIN_FLOPS");
   if ( e != NULL )
      lim = atof(e);
   double fl = 0.0;
   const double m1 = (double) s->m + 1.0;
   for (auto& B : s->blk)
      fl += 4.0 * m1 * (double) B.n * (double) B.n * (double) B.n + m1 * m1 * (double) B.n * (double) B.n;
   return fl < lim;
}

struct CommOff        /* the communicator is out of sight while a replicated (small) problem is worked on */
{
   hipsdp_solver* s; void* saved; bool on;
   CommOff(hipsdp_solver* s_, bool on_) : s(s_), saved(s_->comm), on(on_) { if ( on ) s->comm = NULL; }
   ~CommOff() { if ( on ) s->comm = saved; }
};

static int solve_begin(hipsdp_solver* s, const hipsdp_params* params, hipsdp_info* info);
static int solve_run(hipsdp_solver* s, hipsdp_info* info, bool try1);

/* the buffers of the preoptimal iterate that do not exist yet (they stay until the problem is freed) */
static int ensure_preoptimal(hipsdp_solver* s)
{
   if ( s->pre_y == NULL )
      HS_CALL( dalloc(&s->pre_y, s->m_alloc > s->m ? s->m_alloc : s->m) );
   if ( s->pre_x == NULL )
      HS_CALL( dalloc(&s->pre_x, s->q_alloc > s->q ? s->q_alloc : s->q) );
   for (auto& B : s->blk)
      if ( B.Xpre == NULL )
         HS_CALL( dalloc(&B.Xpre, (long long) B.n * B.n) );
   return HS_OK;
}

static int sync_outcome(hipsdp_solver* s, int rc, hipsdp_info* info)
{
   struct Pack { int rc, solved, last_status, pre_valid; double sol_scale, tau, kappa, pre_scale; hipsdp_info info; } pk;
   memset(&pk, 0, sizeof(pk));
   pk.rc = rc; pk.solved = s->solved ? 1 : 0; pk.last_status = s->last_status; pk.pre_valid = s->pre_valid ? 1 : 0;
   pk.sol_scale = s->sol_scale; pk.tau = s->tau; pk.kappa = s->kappa; pk.pre_scale = s->pre_scale; pk.info = *info;
   const long long nint = (long long) ((sizeof(Pack) + sizeof(int) - 1) / sizeof(int));
   hipStream_t st = s->stream;
   {
      PoolBuf<int> d(st);
      HS_CALL( d.alloc(nint) );
      HS_HIP( hipMemcpyAsync(d.p, &pk, sizeof(pk), hipMemcpyHostToDevice, st) );
      HS_CALL( hs_bcast_ints(s->comm, d.p, nint, st) );
      HS_HIP( hipMemcpyAsync(&pk, d.p, sizeof(pk), hipMemcpyDeviceToHost, st) );
      HS_HIP( hipStreamSynchronize(st) );
   }
   s->solved = pk.solved != 0; s->last_status = pk.last_status; s->sol_scale = pk.sol_scale; s->tau = pk.tau; s->kappa = pk.kappa;
   s->pre_scale = pk.pre_scale;
   *info = pk.info;
   if ( pk.rc != HIPSDP_OK || !s->solved )
   {
      s->pre_valid = false;
      return pk.rc;
   }
   const int m = s->m, q = s->q;
   if ( m > 0 ) HS_CALL( hs_bcast_doubles(s->comm, s->y, m, st) );
   if ( q > 0 ) { HS_CALL( hs_bcast_doubles(s->comm, s->x, q, st) ); HS_CALL( hs_bcast_doubles(s->comm, s->z, q, st) ); }
   for (auto& B : s->blk)
   {
      const long long n2 = (long long) B.n * B.n;
      HS_CALL( hs_bcast_doubles(s->comm, B.X, n2, st) );
      HS_CALL( hs_bcast_doubles(s->comm, B.Z, n2, st) );
      B.derived_valid = false;
   }
   if ( pk.pre_valid )
   {
      HS_CALL( ensure_preoptimal(s) );
      if ( m > 0 ) HS_CALL( hs_bcast_doubles(s->comm, s->pre_y, m, st) );
      if ( q > 0 ) HS_CALL( hs_bcast_doubles(s->comm, s->pre_x, q, st) );
      for (auto& B : s->blk)
         HS_CALL( hs_bcast_doubles(s->comm, B.Xpre, (long long) B.n * B.n, st) );
   }
   s->pre_valid = pk.pre_valid != 0;
   HS_HIP( hipStreamSynchronize(st) );
   return HIPSDP_OK;
}

/* the end of every solve (hipsdp_solve, hipsdp_solve_many) */
static int solve_end(hipsdp_solver* s, int rc)
{
   /* no recorded operation and no held region outlives the call: a normal return has launched everything (the final read-back
    * ends the regions), an error return may have left records behind, which are dropped */
   if ( rc == HIPSDP_OK )
      rc = hs_red_batch_end_all();
   else
      hs_red_batch_reset();
   if ( rc != HIPSDP_OK )          /* error return inside the iteration: whatever it had queued on either queue must not outlive the call */
   {
      (void) hipStreamSynchronize(s->stream);
      (void) hipStreamSynchronize(s->stream2);
   }
   return rc;
}

extern "C" int hipsdp_solve(hipsdp_solver* s, const hipsdp_params* params, hipsdp_info* info)
{
   if ( s == NULL || !s->shaped || info == NULL )
      return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( flush_zeros(s) );
   if ( s->comm != NULL )
      HS_CALL( flush_cmds(s) );                   /* (one rank alone: the one-launch solve runs the waiting commands itself) */
   const bool alone = replicate_small(s);
   int rc;
   {
      CommOff off(s, alone);
      rc = solve_begin(s, params, info);
      if ( rc == HIPSDP_OK )
         rc = solve_run(s, info, true);
   }
   rc = solve_end(s, rc);
   if ( alone )
      rc = sync_outcome(s, rc, info);
   return rc;
}

#define CLK_MAX_ASSEMBLIES 256
/* Shader clock DURING an assembly: one thread on a queue of its own counts its cycles (clock64) and the 100 MHz wall ticks from the
 * moment the assembly is queued until a flag says it is over - ONE thread, one counter.  [First form: one (clock64, wall clock) pair
 * from a launch before and one from a launch after the assembly - they land on different XCDs, whose cycle counters are not
 * aligned: 1.98, 2.37 GHz and garbage on some boxes.  Second: 20 us of spinning right behind the assembly - the idle device is
 * back at 2.44 GHz by then.]  out[0]: flag (set by k_clock_stop behind the assembly), out[2], out[3]: cycles, ticks. */
__global__ void k_clock_window(unsigned long long* __restrict__ out)
{
   const unsigned long long w0 = wall_clock64();
   const unsigned long long c0 = clock64();
   unsigned long long w1 = w0;
   /* (at most 0.2 s: an exit every wave reaches) */
   while ( __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0ULL && w1 - w0 < 20000000ULL )
   {
      __builtin_amdgcn_s_sleep(32);
      w1 = wall_clock64();
   }
   const unsigned long long c1 = clock64();
   w1 = wall_clock64();
   out[2] = c1 - c0;
   out[3] = w1 - w0;
}
__global__ void k_clock_stop(unsigned long long* __restrict__ out)
{
   __hip_atomic_store(out, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern "C" int hipsdp_set_clock_sampling(hipsdp_solver* s, int on)
{
   if ( s == NULL ) return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   if ( on && s->clk_buf == NULL )
      HS_HIP( hipMalloc((void**) &s->clk_buf, (size_t) CLK_MAX_ASSEMBLIES * 4 * sizeof(unsigned long long)) );
   if ( on && s->clk_stream == NULL )
      HS_HIP( hipStreamCreateWithFlags(&s->clk_stream, hipStreamNonBlocking) );
   s->clk_on = on != 0;
   return HIPSDP_OK;
}

extern "C" int hipsdp_get_assembly_clock(hipsdp_solver* s, double* ghz)
{
   if ( s == NULL || ghz == NULL ) return HIPSDP_ERR_ARG;
   *ghz = s->clk_ghz;
   return HIPSDP_OK;
}

/* ---- B&B-sized problems: the whole solve in one launch of one workgroup (csrc/solve1.hip).  Returns HS_OK and *done = true when the
 * solve ran there; *done = false: not this path's problem (shape, options) or the kernel declined (too much work for one compute
 * unit) - nothing has been touched and the general path below takes over.  HIPSDP_SOLVE1=0 switches the path off. */
#define S1_HIST_MAX 256
#define S1_SOL_OFF (HS_S1_OUT_DOUBLES + 8 + 16 * S1_HIST_MAX)       /* y (128), x (4096), z (4096) */
#define S1_HOST_DOUBLES (S1_SOL_OFF + 128 + 2 * 4096)
static long long g_solve1_solves = 0;      /* solves of this process that ran in the one launch (bench.py reports the share) */
static long long g_solve1_fallbacks = 0;   /* ... that the kernel gave up on numerically and the general path solved again */
static long long g_solve1_fallbacks_warm = 0;   /* ... of these: warm-started solves (retried from the caller's start) */
static long long g_many_launches = 0;      /* hipsdp_solve_many: launches of the one-launch kernel (one per size class and call) */
static long long g_many_problems = 0;      /* ... and the problems whose results the kernel delivered there */
/* the three stages of a one-launch solve: prepare (eligibility, workspace, the kernel's arguments, the node's commands taken over),
 * wait (the sequence word), finish (the result block into the solver and info).  hipsdp_solve runs them back to back (solve1_try),
 * hipsdp_solve_many prepares many solvers, launches them together and finishes each. */
/* A LANE is what one workgroup of the kernel works on beside the matrices A[k] and Dext, which it only reads: the objective, the
 * iterate, the workspace, and in pinned host memory the result block, the sequence word behind it (at HS_S1_OUT_DOUBLES), optionally
 * the history (behind the word's 8 doubles) and y, x, z once more.  The solver's own storage is the lane of hipsdp_solve and
 * hipsdp_solve_many (solve1_own_lane); hipsdp_solve_objectives gives one solver many (objs_lanes) that share its matrices. */
struct S1Lane
{
   double *b, *y, *x, *z;
   double *X[HS_S1_MAXBLK], *Z[HS_S1_MAXBLK];
   double* gws; long long gws_len;
   double* host; double* host_dev;          /* the pinned part as the host and as the device see it */
   bool hist;                               /* it has room for the history */
   long long hy, hx, hz;                    /* offsets of y, x, z in the pinned part */
   unsigned long long* seq;                 /* the counter its sequence numbers are drawn from */
};
struct S1Prep
{
   hs_solve1_args a;
   int prof, nofb;
   std::chrono::steady_clock::time_point t_begin;
   const double* host;                      /* the pinned part of the lane the launch reports to */
   long long hy;
};
/* what a finished lane says about the solution it holds (solve1_result) */
struct S1Sol
{
   int status;
   double tau, kappa, sol_scale, pre_scale;
   bool pre_valid;
};
static void solve1_own_lane(hipsdp_solver* s, S1Lane* L)
{
   memset(L, 0, sizeof(*L));
   const int K = (int) s->blk.size();
   for (int k = 0; k < K && k < HS_S1_MAXBLK; ++k)
   {
      L->X[k] = s->blk[k].X; L->Z[k] = s->blk[k].Z;
   }
   L->b = s->b; L->y = s->y; L->x = s->x; L->z = s->z;
   L->gws = s->s1_ws; L->gws_len = s->s1_ws_len;
   L->host = s->s1_host; L->host_dev = s->s1_host_dev;
   L->hist = true;
   L->hy = S1_SOL_OFF; L->hx = L->hy + 128; L->hz = L->hx + 4096;
   L->seq = &s->s1_seq;
}
/* the lane's part of the kernel's arguments, with the next sequence number of the lane's counter */
static void solve1_bind(S1Prep* pp, const S1Lane& L, int K)
{
   hs_solve1_args& a = pp->a;
   for (int k = 0; k < K; ++k)
   {
      a.X[k] = L.X[k]; a.Z[k] = L.Z[k];
   }
   a.b = L.b; a.y = L.y; a.x = L.x; a.z = L.z;
   a.gws = L.gws; a.gws_len = L.gws_len;
   a.out = L.host_dev;
   a.hist = (L.hist && getenv("HIPSDP_SOLVE1_HIST") != NULL && getenv("HIPSDP_SOLVE1_HIST")[0] != '0') ? L.host_dev + HS_S1_OUT_DOUBLES + 8 : NULL;
   a.hist_len = S1_HIST_MAX;
   a.hy = L.host_dev + L.hy; a.hx = L.host_dev + L.hx; a.hz = L.host_dev + L.hz;
   a.seq = ++*L.seq;
   a.flag = reinterpret_cast<unsigned long long*>(L.host_dev + HS_S1_OUT_DOUBLES);
   pp->host = L.host;
   pp->hy = L.hy;
}
/* whether the one-launch path is offered the solver's problem under s->par and the environment; ns: the block sizes when it is */
static bool solve1_eligible(hipsdp_solver* s, int* ns, int* prof_out)
{
   /* (read at every solve: tests and tools switch the path between two solves of one process) */
   int on = 1, prof = 0;
   /* largest block the kernel is offered (HIPSDP_SOLVE1_MAXN): whatever fits its LDS (hs_solve1_fits) - with no LP rows one block
    * of 49 rows at m = 1, 41 at m = 64, 37 at m = 108; two of 34 / 29 / 25; eight of 16 / 13 / 12 (hipsdp_solve1_fits, units library).
    * Measured with sparse variable matrices, dense constant matrices and LP rows of density 0.3 (tests/devtools/solve1_sizes.py) it
    * is ahead of the general path at every such size: 16 rows 0.124 against 0.281 ms per iteration, 24: 0.233 / 0.360, 32: 0.360 /
    * 0.422, two of 30: 0.449 / 0.572.  [Mid-round it lost at 32 rows, 0.62 against 0.43 - a dense constant matrix went through
    * scalar loops of one wavefront and dense LP rows through a walk of their nonzeros - and the default was 24.] */
   int maxn = 64;
   /* most variables the kernel is offered (HIPSDP_SOLVE1_MAXM): with the Schur matrix as a packed triangle m = 128 fits its LDS, but
    * the factorization of M is one workgroup's (the panel recurrence one wavefront's) and grows with m^3 - against the general path
    * (tests/devtools/solve1_mbig.py, ms per iteration): m = 70: 0.227 / 0.393, 90: 0.330 / 0.426, 105: 0.424 / 0.453 (example_MkP's
    * root, two nonzeros per matrix: 0.235 / 0.450), 110: 0.520 / 0.501, 120: 0.465 / 0.436, 128: 0.541 / 0.476 */
   int maxm = 108;
   {
      if ( getenv("HIPSDP_SOLVE1_MAXM") != NULL )
         maxm = atoi(getenv("HIPSDP_SOLVE1_MAXM"));
      const char* env = getenv("HIPSDP_SOLVE1");
      on = (env != NULL && env[0] == '0') ? 0 : 1;
      prof = getenv("HIPSDP_SOLVE1_PROF") != NULL ? atoi(getenv("HIPSDP_SOLVE1_PROF")) : 0;
      if ( getenv("HIPSDP_SOLVE1_MAXN") != NULL )
         maxn = atoi(getenv("HIPSDP_SOLVE1_MAXN"));
   }
   const hipsdp_params& par = s->par;
   *prof_out = prof;
   if ( !on || s->comm != NULL || s->shardA || s->schur_mode_forced || par.verbose || s->pc.on )
      return false;
   const int K = (int) s->blk.size();
   if ( K < 1 || K > HS_S1_MAXBLK || s->m > maxm )
      return false;
   for (int k = 0; k < K; ++k)
   {
      if ( s->blk[k].sparse || s->blk[k].A == NULL || s->blk[k].n > maxn )
         return false;
      ns[k] = s->blk[k].n;
   }
   return hs_solve1_fits(s->m, s->q, K, ns) != 0;
}
/* *offered = false: not this path's problem (shape, options) - nothing has been touched.  lane = NULL: the solver's own lane, its
 * workspace and pinned part allocated here, and the node's waiting setters taken over by the launch; a lane of
 * hipsdp_solve_objectives: the setters have been flushed and the launch runs none */
static int solve1_prepare(hipsdp_solver* s, S1Prep* pp, bool* offered, const S1Lane* lane = NULL)
{
   *offered = false;
   s->s1_last = 0;
   s->s1_sol_host = false;
   const double maxwork = 3e6;
   int ns[HS_S1_MAXBLK];
   int prof = 0;
   if ( !solve1_eligible(s, ns, &prof) )
      return HS_OK;
   const hipsdp_params& par = s->par;
   const int K = (int) s->blk.size();
   hipStream_t st = s->stream;
   const long long want = hs_solve1_ws_doubles(s->m, s->q, K, ns);
   if ( lane == NULL && s->s1_ws_len < want )
   {
      if ( s->s1_ws != NULL )
      {
         HS_HIP( hipStreamSynchronize(st) );
         (void) hipFree(s->s1_ws);
         s->s1_ws = NULL; s->s1_ws_len = 0;
      }
      const long long len = want + want / 2 + 4096;
      HS_HIP( hipMalloc((void**) &s->s1_ws, (size_t) len * sizeof(double)) );
      s->s1_ws_len = len;
   }
   if ( lane == NULL && s->s1_host == NULL )
   {
      HS_HIP( hipHostMalloc((void**) &s->s1_host, (size_t) S1_HOST_DOUBLES * sizeof(double),
            hipHostMallocMapped | hipHostMallocCoherent) );
      HS_HIP( hipHostGetDevicePointer((void**) &s->s1_host_dev, s->s1_host, 0) );
      memset(s->s1_host, 0, (size_t) (HS_S1_OUT_DOUBLES + 8) * sizeof(double));
   }
   if ( par.preoptgap > 0.0 )
      HS_CALL( ensure_preoptimal(s) );
   pp->t_begin = std::chrono::steady_clock::now();
   hs_solve1_args& a = pp->a;
   memset(&a, 0, sizeof(a));
   a.m = s->m; a.q = s->q; a.nblk = K;
   for (int k = 0; k < K; ++k)
   {
      Block& B = s->blk[k];
      a.n[k] = B.n; a.A[k] = B.A; a.Xpre[k] = B.Xpre;
   }
   a.Dext = s->Dext; a.pre_y = s->pre_y; a.pre_x = s->pre_x;
   a.gaptol = par.gaptol; a.feastol = par.feastol; a.infeastol = par.infeastol; a.objlimit = par.objlimit; a.timelimit = par.timelimit;
   a.gamma = par.gamma; a.pabstol = par.pabstol; a.preoptgap = par.preoptgap; a.elapsed0 = 0.0; a.maxwork = maxwork;
   a.maxiter = par.maxiter; a.settings = par.settings; a.have_start = s->have_start ? 1 : 0;
   {
      const char* env = getenv("HIPSDP_PIVOT_RULE");
      a.pivot_rule = env != NULL ? atoi(env) : 3;
   }
   a.prof_on = prof;
   pp->prof = prof;
   const int nofb = (getenv("HIPSDP_SOLVE1_NO_FALLBACK") != NULL && getenv("HIPSDP_SOLVE1_NO_FALLBACK")[0] == '1') ? 1 : 0;    /* (read at every solve, like the other switches of this path) */
   a.keep_on_fail = nofb ? 0 : 1;
   pp->nofb = nofb;
   if ( lane != NULL )
      solve1_bind(pp, *lane, K);
   else
   {
      S1Lane own;
      solve1_own_lane(s, &own);
      solve1_bind(pp, own, K);
   }
   a.cmds = s->arena_d; a.ncmd = s->ncmd;         /* the node's setters: run by the same launch */
   if ( s->ncmd > 0 )
   {
      const size_t used = s->stage_off > NC_BYTES ? s->stage_off : NC_BYTES;
      a.cmd_bytes = (long long) ((used + 15) & ~(size_t) 15);         /* (the arena's size is a multiple of 16) */
   }
   s->ncmd = 0;
   *offered = true;
   return HS_OK;
}

/* The results of the one-launch kernels come through pinned memory: the last thing a problem's workgroup stores is its sequence word.
 * A word to wait for: the pinned part of the problem's lane, the number its launch publishes, and which of the caller's queues the
 * launch went to (< 0: never launched - not waited for, not published). */
struct SeqWord { const double* host; unsigned long long seq; int queue; };

/* Spins on all the words together; pub[i] = 1 once word i holds its number.  A launch that failed would never publish: after every
 * 0x4000 words read, each queue that still has a word missing is asked.  Not ready: keep spinning.  Finished: its missing words are
 * read once more, and what is still missing is reported.  Any other answer is recorded, and the queue's missing words count as not
 * published (pub[i] = 0); `what` names the query in that record.  No allocation: this is the wait of every B&B node solve. */
static void wait_published(const SeqWord* w, int n, const hipStream_t* queues, int nqueues, const char* what, char* pub)
{
   auto holds = [&](int i) -> bool {
      return *reinterpret_cast<const volatile unsigned long long*>(w[i].host + HS_S1_OUT_DOUBLES) == w[i].seq;
   };
   int left = 0;
   for (int i = 0; i < n; ++i)
   {
      pub[i] = 0;
      if ( w[i].queue >= 0 ) ++left;
   }
   const char GIVEN_UP = 2;
   long long reads = 0;
   while ( left > 0 )
   {
      reads += left;
      for (int i = 0; i < n; ++i)
         if ( w[i].queue >= 0 && pub[i] == 0 && holds(i) ) { pub[i] = 1; --left; }
      if ( left == 0 || reads < 0x4000 )
         continue;
      reads = 0;
      for (int c = 0; c < nqueues; ++c)
      {
         bool any = false;
         for (int i = 0; i < n && !any; ++i) any = w[i].queue == c && pub[i] == 0;
         if ( !any )
            continue;
         const hipError_t e = hipStreamQuery(queues[c]);
         if ( e == hipErrorNotReady )
            continue;
         if ( e != hipSuccess )
            hs_record_hip_error(e, what, __FILE__, __LINE__);
         for (int i = 0; i < n; ++i)
            if ( w[i].queue == c && pub[i] == 0 )
            {
               --left;
               if ( e == hipSuccess && holds(i) ) { pub[i] = 1; continue; }
               if ( e == hipSuccess )
                  set_err("the one-launch solve finished without publishing its results");
               pub[i] = GIVEN_UP;
            }
      }
   }
   for (int i = 0; i < n; ++i)
      pub[i] = pub[i] == 1;
   __atomic_thread_fence(__ATOMIC_ACQUIRE);
}

/* one word: the launch on st (host: the pinned part of its lane) */
static int solve1_wait(const double* host, unsigned long long seq, hipStream_t st)
{
   const SeqWord w = {host, seq, 0};
   char pub = 0;
   wait_published(&w, 1, &st, 1, "hipStreamQuery(one-launch solve)", &pub);
   return pub ? HS_OK : HS_ERR_HIP;
}

/* *done = true: the solve ran there; false: the kernel declined (too much work for one compute unit) or gave up numerically, and the
 * general path takes the problem from the same start */
/* the lane's part of it: the result block of the lane pp was bound to into info and sol; the solver is read (parameters, shape), the
 * process counters move, nothing of the solver's solution state is written */
static int solve1_result(hipsdp_solver* s, const S1Prep* pp, hipsdp_info* info, S1Sol* sol, bool* done)
{
   *done = false;
   const hipsdp_params& par = s->par;
   hipStream_t st = s->stream;
   const int prof = pp->prof, nofb = pp->nofb;
   const double* o = pp->host;
   const int status = (int) o[0];
   if ( status == -2 )
      return HS_OK;                              /* declined: the general path takes the problem */
   /* A numerical failure of the kernel is not final: on about 1 % of random shapes with cond(M) around
    * 1e14 one path gives up where the other converges (profiles/r04_c_solve1_fuzz.txt) - their last steps differ in how the solves
    * with M are corrected.  The general path solves the problem again before the caller escalates its settings, FROM THE SAME START:
    * with keep_on_fail the kernel has left y, x, z, X, Z in device memory as the node's setters wrote them (a caller's start point
    * stays in place and have_start stays as it was; without one the general path starts cold as it always does).
    * HIPSDP_SOLVE1_NO_FALLBACK=1 keeps the kernel's failure (and its last iterate). */
   if ( status == HIPSDP_STATUS_NUMERIC && nofb == 0 )
   {
      HS_HIP( hipStreamSynchronize(st) );
      (void) __sync_add_and_fetch(&g_solve1_fallbacks, 1);
      if ( (int) o[12] != 0 )
         (void) __sync_add_and_fetch(&g_solve1_fallbacks_warm, 1);
      return HS_OK;
   }
   /* the result block, y, x and z are in pinned memory, published before the sequence word; X and Z in device memory are complete
    * when the kernel has retired - whoever reads them waits for the queue first (stage_sync), this call does not */
   memset(info, 0, sizeof(*info));
   sol->status = status;
   sol->tau = o[9];
   sol->kappa = o[10];
   const double pobj = o[2], dobj = o[3];
   if ( status == HIPSDP_STATUS_DINF || status == HIPSDP_STATUS_DUNB || status == HIPSDP_STATUS_PDINF )
      sol->sol_scale = 1.0 / fmax(fmax(fabs(dobj), fabs(pobj)), 1e-300);
   else
      sol->sol_scale = 1.0 / sol->tau;
   sol->pre_valid = o[13] != 0.0;
   sol->pre_scale = o[14];
   info->status = status;
   info->iterations = (int) o[1];
   info->pobj = pobj * sol->sol_scale;
   info->dobj = dobj * sol->sol_scale;
   info->pinf = o[4]; info->dinf = o[5]; info->dabs = o[6]; info->gap = o[7]; info->mu = o[8];
   info->tau = sol->tau; info->kappa = sol->kappa;
   info->chol_fail = (int) o[11];
   info->warm_started = (int) o[12];
   info->settings_used = par.settings;
   info->schur_calls = info->iterations;
   for (auto& B : s->blk)
      info->schur_flops += (double) info->iterations * (4.0 * (s->m + 1) * (double) B.n * B.n * B.n + (double) (s->m + 1) * (s->m + 1) * (double) B.n * B.n);
   info->solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - pp->t_begin).count();
   if ( prof )
   {
      static const char* const names[12] = {"lists", "start", "residuals", "inverse factors + LP part", "Zinv", "Schur", "chol M + X Rd",
         "predictor rhs", "predictor step", "corrector rhs", "corrector step", "update"};
      fprintf(stderr, "hipsdp one-launch solve: %d iterations, %.1f us on the device (%.0f cycles)", info->iterations,
         o[43] / 100.0, o[17]);
      for (int i = 0; i < 12; ++i)
         fprintf(stderr, "%s %s %.0f", i ? "," : ":", names[i], o[18 + i]);
      fprintf(stderr, " | sub");
      for (int i = 12; i < 22; ++i)
         fprintf(stderr, " %.0f", o[18 + i]);
      fprintf(stderr, " | nnz A %d, LP %d\n", (int) o[40], (int) o[41]);
   }
   (void) __sync_add_and_fetch(&g_solve1_solves, 1);
   *done = true;
   return HS_OK;
}
/* the solver's own lane: the solution it holds becomes the solver's */
static int solve1_finish(hipsdp_solver* s, const S1Prep* pp, hipsdp_info* info, bool* done)
{
   S1Sol sol;
   HS_CALL( solve1_result(s, pp, info, &sol, done) );
   if ( !*done )
      return HS_OK;
   s->stage_pending = true;
   s->tau = sol.tau;
   s->kappa = sol.kappa;
   s->sol_scale = sol.sol_scale;
   s->last_status = sol.status;
   s->solved = true;
   s->have_start = false;
   s->pre_valid = sol.pre_valid;
   s->pre_scale = sol.pre_scale;
   for (auto& B : s->blk)
      B.derived_valid = false;
   s->s1_last = 1;
   s->s1_sol_host = true;
   return HS_OK;
}

static int solve1_try(hipsdp_solver* s, hipsdp_info* info, bool* done)
{
   *done = false;
   S1Prep pp;
   bool offered = false;
   HS_CALL( solve1_prepare(s, &pp, &offered) );
   if ( !offered )
      return HS_OK;
   HS_CALL( hs_solve1_launch(s->stream, &pp.a) );
   HS_CALL( solve1_wait(pp.host, pp.a.seq, s->stream) );
   return solve1_finish(s, &pp, info, done);
}

/* a solve in two parts: solve_begin checks the solver and normalises the parameters (once per solve), solve_run solves - with the
 * one-launch kernel first when try1 (hipsdp_solve), or on the general path alone (hipsdp_solve_many, which has run the kernel) */
static int solve_begin(hipsdp_solver* s, const hipsdp_params* params, hipsdp_info* info)
{
   g_err[0] = 0;
   if ( s == NULL || !s->shaped || info == NULL )
      return HIPSDP_ERR_ARG;
   if ( s->shardA && s->comm == NULL )
   {
      set_err("hipsdp_solve: the matrices of this problem are sharded by variable, the communicator is gone");
      return HIPSDP_ERR_ARG;
   }
   HS_HIP( hipSetDevice(s->device) );
   if ( params != NULL )
      s->par = *params;
   else
      hipsdp_default_params(&s->par);
   {
      if ( s->par.lanczos_steps <= 0 )
      {
         /* default: 24 steps; 16 once every block has more than 64 rows - there each step is a launch of its own and the estimate
          * (used with its residual bound subtracted, the Cholesky of the new iterate being the exact test) costs 4 % of an iteration
          * at n = 500 and 20 % at n = 200; measured on the bench instances: same iteration counts from 12 steps on */
         int nmin = 1 << 30;
         for (auto& B : s->blk) if ( B.n < nmin ) nmin = B.n;
         s->par.lanczos_steps = (!s->blk.empty() && nmin > 64) ? 16 : 24;
      }
      if ( s->par.settings < 0 ) s->par.settings = 0;
      if ( s->par.settings > 2 ) s->par.settings = 2;
      s->par.lanczos_steps <<= s->par.settings;          /* medium: twice, stable: four times the Lanczos steps */
      bool lan_used = false;                  /* blocks with more than 64 rows take their step lengths from the one-launch Lanczos */
      for (auto& B : s->blk)
         if ( B.n > 64 ) lan_used = true;
      if ( s->lan_sync != NULL && lan_used )
      {
         /* exchange vectors of the one-launch Lanczos runs: a solve starts from their initial state (a run that gave up
          * leaves them in no particular one) */
         HS_CALL( hs_lanczos_sync_reset(s->stream, s->lan_sync, s->lan_rot) );
      }
      if ( s->trsv_ws != NULL && s->m > 2 * 64 )
         HS_CALL( hs_trsv_sync_init(s->stream, s->m, s->trsv_ws, &s->trsv_epoch) );      /* likewise the triangular solves' */
      if ( s->par.lanczos_steps < 4 ) s->par.lanczos_steps = 4;
      if ( s->par.lanczos_steps > 250 ) s->par.lanczos_steps = 250;
   }
   return HIPSDP_OK;
}

/* the state every solve starts from (before the one-launch kernel is offered the problem) */
static void solve_reset(hipsdp_solver* s, hipsdp_info* info)
{
   hs_comm_phase(2);
   for (int p = 0; p < PH_COUNT; ++p) s->pc.ms[p] = 0.0;
   memset(info, 0, sizeof(*info));
   info->status = HIPSDP_STATUS_UNSOLVED;
   hs_red_batch_reset();
   s->pre_valid = false;
   s->clk_n = 0;
   s->clk_ghz = 0.0;
}

/* hs_schur_ws.after_g1 of the W form (argument: the solver): R = Lx itself is the operand of the first product and G = LzInv of the
 * second only, so the inverse factor of X follows the first product into the second queue, and ev_g2 makes the second product wait */
static int after_g1_x_inverse(void* arg)
{
   hipsdp_solver* s = static_cast<hipsdp_solver*>(arg);
   HS_CALL( fork2(s) );              /* (behind hs_zero_upper of Lx and the first product) */
   for (auto& B : s->blk)
      HS_CALL( hs_trtri(s->stream2, B.n, B.Lx, B.dinvx, B.LxInv, B.T1) );
   HS_HIP( hipEventRecord(s->evJoin, s->stream2) );
   s->sws.ev_g2 = (void*) s->evJoin;
   return HS_OK;
}

/* one solve on the general path: its constants, the bookkeeping of the iterate and one member function per phase of an iteration.
 * It lives on solve_run's stack, and every way out of it goes through close(). */
struct GeneralSolve
{
   hipsdp_solver* const s;
   hipsdp_info* const info;
   const std::chrono::steady_clock::time_point t_begin;
   const hipsdp_params& par = s->par;
   const hipStream_t st = s->stream;
   const int m = s->m, m1 = s->m + 1, q = s->q, K = (int) s->blk.size();
   /* the retry ladder of the backend (sdpisolver_sdpa.cpp:1415-1449: fast / default / stable parameter sets): more conservative
    * settings take shorter steps, keep the iterates more central and wait longer before they call a stall (oracle/ipm_ref.py:
    * Params.settings, same numbers) */
   const int settings = par.settings;
   const double gamma_eff = settings == 0 ? par.gamma : fmin(par.gamma, settings == 1 ? 0.9 : 0.75);
   const int stall_lim = settings == 0 ? 3 : (settings == 1 ? 5 : 8);
   const int nobest_lim = settings == 0 ? 6 : (settings == 1 ? 10 : 15);
   const double sigma_floor = settings == 0 ? 1e-8 : (settings == 1 ? 1e-4 : 1e-2);
   /* HIPSDP_NO_IDENTITY_START=1: the first assembly of a cold solve through the general products as well (A/B runs, tests) */
   const bool no_identity_start = getenv("HIPSDP_NO_IDENTITY_START") != NULL && getenv("HIPSDP_NO_IDENTITY_START")[0] == '1';
   const bool optimistic = (s->comm == NULL) && getenv("HIPSDP_NO_OPTIMISTIC") == NULL;
   /* (test hook, tests/test_gpu_ipm.py: HIPSDP_TEST_OVERSTEP=<factor> lengthens the step of iteration 2 beyond the boundary of the
    * cone, so that the rarely taken road - failed check, step halved, optimistic part taken back - is driven) */
   const char* const overstep = getenv("HIPSDP_TEST_OVERSTEP");

   double N1 = 0.0, normb = 0.0, normC = 0.0;
   bool small_all = false;            /* one rank, every block of at most 64 rows */
   int setf = 0;
   bool defer_ok = false;             /* the W form may await the second queue between its products (after_g1_x_inverse) */
   hipStream_t st2 = NULL;            /* the second queue, or the first when the blocks are too small for two */

   int it = 0, status = HIPSDP_STATUS_ITERLIM;
   bool stop = false;
   bool identity_start = false;
   bool factors_valid = false;        /* the Cholesky factors of X and Z are those of the current iterate */
   bool residuals_ready = false;      /* the residual pass of the current iterate has been read back */
   bool want_cert = false;
   /* The dual residual obeys an exact recurrence: dZ is DEFINED as A^T(dy~) + eta Rd, so after the update (y~, Z) += alpha
    * (dy~, dZ) the new residual is (1 - alpha eta) Rd whatever the quality of dy (forced pivots included), and likewise for the
    * LP rows.  The general path (blocks above 64 rows: each pass over A is HBM bound, 1 GB at n = 500 / m = 1000) therefore
    * scales the residual it has instead of sweeping A again; it is recomputed from scratch at the first iteration and whenever
    * the certificate residuals are needed (tau -> 0 divides the rounding the recurrence carries). */
   bool rd_have = false;             /* Rd / rd hold the residual of SOME iterate: the current one once rd_pending is worked off */
   bool rd_pending = false;
   double rd_scale = 1.0;
   bool zchain_queued = false, xchain_queued = false;      /* the chains of this iterate's factorization phase are queued */

   int certwait = 0, nstall = 0, sincebest = 0;
   double lastmu = 1e300, alpha_last = 1.0, bestmerit = 1e300;

   /* the last host scalars and what the phases of an iteration hand on */
   HostScalars hs;
   int hflags[3] = {0, 0, 0};
   double mu = 0, pinf = 0, dinf = 0, dabs = 0, gap = 0, pobj = 0, dobj = 0, rg = 0;
   double schur_ms = 0.0;
   bool defer_join = false, gram_only_used = false, schur_small = false;
   bool gram_cached = false;          /* this assembly came out of the store: no matrix-core flops were executed for it */
   bool predH_queued = false, predH_joined = false, split_dz = false;
   double dta = 0, dka = 0, sigma = 0, eta = 0, amax = 0, alpha = 0, dt = 0, dk = 0;
   double tau0 = 0, kappa0 = 0, applied = 0;

   int halt(int why) { status = why; stop = true; return HS_OK; }

   /* L = chol(M) on the queue qf, the failure flag in flags[f] */
   int factor(hipStream_t qf, int n, double* L, double* dinv, const double* M, int f)
   {
      HS_CALL( hs_copy(qf, L, M, (long long) n * n) );
      return hs_potrf(qf, n, L, dinv, s->flags + f, NULL);
   }

   /* the Z chain of the factorization phase for one block: factor (unless the step's Cholesky check has), inverse factor, Z^-1 */
   int z_chain(Block& B, hipStream_t qz)
   {
      const int n = B.n;
      if ( !factors_valid )
         HS_CALL( factor(qz, n, B.Lz, B.dinvz, B.Z, 0) );
      HS_CALL( hs_trtri(qz, n, B.Lz, B.dinvz, B.LzInv, B.T2) );
      HS_CALL( gemm_on(qz, HS_MC, HS_MC, n, n, n, 1.0, B.LzInv, n, B.LzInv, n, 0.0, B.Zinv, n, HS_GEMM_LOWER) );
      return hs_mirror_lower(qz, B.Zinv, n, n);
   }

   /* the X chain for one block: factor (likewise), zero upper triangle, inverse factor (unless after_g1_x_inverse launches it) */
   int x_chain(Block& B, bool inverse)
   {
      const int n = B.n;
      if ( !factors_valid )
         HS_CALL( factor(st, n, B.Lx, B.dinvx, B.X, 1) );
      HS_CALL( hs_zero_upper(st, B.Lx, n) );
      return inverse ? hs_trtri(st, n, B.Lx, B.dinvx, B.LxInv, B.T1) : HS_OK;
   }

   /* the Z chains need nothing from the residual pass: on the second queue, they run beside it and beside the host's read-back */
   int queue_z_chains()
   {
      HS_CALL( fork2(s) );
      for (auto& B : s->blk)
         if ( B.n > 64 )
            HS_CALL( z_chain(B, st2) );
      zchain_queued = true;
      return HS_OK;
   }

   /* Reads the scalars back.  With the Z chains under way, the X chains do not depend on the scalars either: they are queued behind
    * the kernel that publishes them and run while the host waits, decides and launches (a solve that ends here has run them in vain:
    * 0.1 ms at n = 500).
    * INVARIANT: the X chain is speculative - when the solve ends at this read-back, B.Lx, B.dinvx, B.LxInv, B.T1 and flags[1] already
    * hold the factors of the FINAL X.  Lx, LxInv, dinvx and T1 are therefore UNDEFINED after solve_run returns (nothing reads them:
    * every getter works from X, Z, y; the next solve refactors).  The chain's time is charged to PH_RESID, not PH_FACTOR, in the
    * phase anatomy (bench.py says so next to those two figures). */
   int read_back(int* flags3)
   {
      const std::function<int()> x_chains = [this]() -> int
      {
         for (auto& B : s->blk)
            if ( B.n > 64 )
               HS_CALL( x_chain(B, true) );
         xchain_queued = true;
         return HS_OK;
      };
      const bool with_x = zchain_queued && !xchain_queued && s->comm == NULL && !(factors_valid && defer_ok);
      return read_scalars(s, hs, flags3, with_x ? &x_chains : NULL);
   }

   /* blocks of at most 64 rows keep the trial iterate of a step in Xs / Zs: swapped in, and back on a failed check */
   void swap_trial()
   {
      for (auto& B : s->blk)
         if ( B.n <= 64 )
         {
            std::swap(B.X, B.Xs);
            std::swap(B.Z, B.Zs);
         }
   }

   int apply_step()
   {
      HS_CALL( hs_axpy3(st, alpha - applied, m, s->dy, s->y, q, s->dx, s->x, q, s->dz, s->z) );
      applied = alpha;
      s->tau = tau0 + alpha * dt;
      s->kappa = kappa0 + alpha * dk;
      return HS_OK;
   }

   /* no step length keeps X and Z positive definite: the step is taken back (the part applied when undo) and the solve stops */
   int give_up(bool undo)
   {
      if ( par.verbose )
         printf("hipsdp: no step length down to %g keeps X and Z positive definite\n", alpha);
      if ( undo )
      {
         HS_CALL( hs_axpy3(st, -applied, m, s->dy, s->y, q, s->dx, s->x, q, s->dz, s->z) );
         s->tau = tau0;
         s->kappa = kappa0;
      }
      for (auto& B : s->blk)
      {
         B.derived_valid = false;
         if ( B.n <= 64 )
            continue;         /* X, Z were never overwritten */
         HS_CALL( hs_copy(st, B.X, B.Xs, (long long) B.n * B.n) );
         HS_CALL( hs_copy(st, B.Z, B.Zs, (long long) B.n * B.n) );
      }
      return halt(HIPSDP_STATUS_NUMERIC);
   }

   /* ---- norms of b and of the constant part, the constants of the solve, the starting point */
   int start()
   {
      HS_CALL( stage_sync(s) );                                  /* the general path uses both queues */
      HS_CALL( ensure_schur_ws(s) );
      HS_CALL( ensure_packed(s) );
      int nmaxb = 0;
      long long N = q;
      small_all = (s->comm == NULL);
      for (auto& B : s->blk)
      {
         nmaxb = std::max(nmaxb, B.n);
         N += B.n;
         small_all = small_all && B.n <= 64;
      }
      s->use2 = nmaxb >= 128;
      st2 = s->use2 ? s->stream2 : st;
      N1 = (double) (N + 1);
      /* one block of at most 64 rows: every Cholesky flag has exactly one writing launch between two reads, which then stores its
       * result itself and the flags need no clearing */
      setf = (small_all && K == 1) ? 1 : 0;
      defer_ok = s->use2 && s->comm == NULL && !s->shardA && !s->schur_mode_cols && !s->schur_mode_rows && !s->schur_mode_U
         && !s->schur_mode_forced && K > 0;
      for (auto& B : s->blk)
         defer_ok = defer_ok && B.n > 64 && !B.sparse;

      HS_CALL( hs_dot(st, m, s->b, s->b, s->sc + 0, 0, s->red_ws) );
      HS_CALL( hs_fill(st, s->sc + 1, 1, 0.0) );
      for (auto& B : s->blk)
         HS_CALL( hs_dot(st, (long long) B.n * B.n, B.A0, B.A0, s->sc + 1, 1, s->red_ws) );
      if ( q > 0 )
      {
         /* column 0 of Dext: strided -> gather through gemv with unit vector would be overkill; copy it */
         HS_HIP( hipMemcpy2DAsync(s->tmpq, sizeof(double), s->Dext, (size_t) m1 * sizeof(double), sizeof(double), (size_t) q, hipMemcpyDeviceToDevice, st) );
         HS_CALL( hs_dot(st, q, s->tmpq, s->tmpq, s->sc + 1, 1, s->red_ws) );
      }
      /* (into the pinned mirror of the scalars: a copy into a stack variable is staged by the runtime and blocks) */
      HS_HIP( hipMemcpyAsync(s->hsc, s->sc, 2 * sizeof(double), hipMemcpyDeviceToHost, st) );
      HS_HIP( hipStreamSynchronize(st) );
      normb = sqrt(s->hsc[0]);
      normC = sqrt(s->hsc[1]);

      /* cold start: X = Z = xi I in every block until the first step - the first Schur complement is then the Gram matrix of the
       * constraint matrices themselves, M_ij = tr(A_i (xi I) A_j (I / xi)) = <A_i, A_j>, and the two n^3 products of the assembly
       * (which would multiply by sqrt(xi) I and I / sqrt(xi)) are not needed for it (single rank, dense blocks, W form) */
      for (auto& B : s->blk)
         B.derived_valid = false;
      if ( s->have_start )
      {
         /* a caller-supplied point (warm start, sdpisolver.h:160-173) is used when it is strictly interior: X_k, Z_k positive
          * definite (checked by the factorizations the first iteration needs anyway) and x, z > 0; kappa = its mean
          * complementarity (tau = 1).  Otherwise the solve falls back to the cold start below. */
         HS_HIP( hipMemsetAsync(s->flags, 0, 8 * sizeof(int), st) );
         HS_CALL( hs_fill(st, s->sc + SC_XZ, 1, 0.0) );
         for (auto& B : s->blk)
         {
            const long long n2 = (long long) B.n * B.n;
            HS_CALL( hs_symmetrize(st, B.X, B.n) );
            HS_CALL( hs_symmetrize(st, B.Z, B.n) );
            HS_CALL( factor(st, B.n, B.Lz, B.dinvz, B.Z, 0) );
            HS_CALL( factor(st, B.n, B.Lx, B.dinvx, B.X, 1) );
            HS_CALL( hs_dot(st, n2, B.X, B.Z, s->sc + SC_XZ, 1, s->red_ws) );
         }
         if ( q > 0 )
         {
            hipLaunchKernelGGL(k_flag_nonpositive, g1d(q), dim3(256), 0, st, q, s->x, s->z, s->flags + 3);
            HS_LAUNCH_CHECK();
            HS_CALL( hs_dot(st, q, s->x, s->z, s->sc + SC_XZ, 1, s->red_ws) );
         }
         int f4[4];
         HS_HIP( hipMemcpyAsync(s->hsc + 4, s->flags, 4 * sizeof(int), hipMemcpyDeviceToHost, st) );
         HS_HIP( hipMemcpyAsync(s->hsc + 8, s->sc + SC_XZ, sizeof(double), hipMemcpyDeviceToHost, st) );
         HS_HIP( hipStreamSynchronize(st) );
         memcpy(f4, s->hsc + 4, sizeof(f4));
         const double mu0 = s->hsc[8] / (double) (N > 0 ? N : 1);
         if ( f4[0] == 0 && f4[1] == 0 && f4[3] == 0 && std::isfinite(mu0) && mu0 > 0.0 )
         {
            s->tau = 1.0;
            s->kappa = mu0;
            factors_valid = true;      /* the factors of an accepted warm start are those of the first iteration */
         }
         else
            s->have_start = false;
      }
      if ( !s->have_start )
      {
         const double xi = fmax(1.0, sqrt(fmax(fmax(normb, normC), 1.0)));
         HS_CALL( hs_fill(st, s->y, m, 0.0) );
         for (auto& B : s->blk)
         {
            HS_CALL( hs_set_identity(st, B.X, B.n, xi) );
            HS_CALL( hs_set_identity(st, B.Z, B.n, xi) );
         }
         HS_CALL( hs_fill(st, s->x, q, xi) );
         HS_CALL( hs_fill(st, s->z, q, xi) );
         s->tau = 1.0;
         s->kappa = xi * xi;
         identity_start = !no_identity_start;
      }
      info->warm_started = s->have_start ? 1 : 0;
      s->have_start = false;
      return HS_OK;
   }

   /* ---- residuals of the current iterate: enqueued at the top of an iteration, or already at the end of the previous one
    * together with the step's Cholesky check, so that one read-back serves both */
   int enqueue_residuals()
   {
      const bool recur = rd_have && !want_cert;
      const bool tail = general_tail(s);
      HS_CALL( hs_make_ext(st, m, -s->tau, 1.0, s->y, s->yt) );
      HS_LAUNCH_CHECK();
      hs_red_batch_begin(st);         /* the reductions of this phase run in one launch, right before the scalars are read */
      HS_CALL( hs_fill_scalar(st, s->sc + SC_RD2, 0.0) );
      HS_CALL( hs_fill_scalar(st, s->sc + SC_XZ, 0.0) );
      HS_CALL( hs_fill_scalar(st, s->sc + SC_HD2, 0.0) );
      std::vector<double*> Xs;
      for (int k = 0; k < K; ++k)
      {
         Block& B = s->blk[k];
         const long long n2 = (long long) B.n * B.n;
         if ( !recur )
            HS_CALL( pass_AT(s, B, s->yt, -1.0, B.Z, B.Rd) );
         else if ( rd_pending )
            HS_CALL( hs_scale_add(st, n2, rd_scale, B.Rd, 0.0, NULL, B.Rd) );
         if ( tail && !want_cert )
         {
            /* (first stages now, second stages with the records: the read-back's launch) */
            HS_CALL( hs_dot_deferred(st, n2, B.Rd, B.Rd, s->sc + SC_BLK(k, 0), 0, s->red_ws, 2 * k) );
            HS_CALL( hs_dot_deferred(st, n2, B.X, B.Z, s->sc + SC_XZ, 1, s->red_ws, 2 * k + 1) );
         }
         else
         {
            HS_CALL( hs_dot(st, n2, B.Rd, B.Rd, s->sc + SC_BLK(k, 0), 0, s->red_ws) );
            HS_CALL( hs_dot(st, n2, B.X, B.Z, s->sc + SC_XZ, 1, s->red_ws) );
         }
         if ( want_cert )
         {
            HS_CALL( hs_red_batch_flush() );
            hipLaunchKernelGGL(k_cert, g1d(n2), dim3(256), 0, st, n2, s->tau, B.Rd, B.A0, B.T1);
            HS_LAUNCH_CHECK();
            HS_CALL( hs_dot(st, n2, B.T1, B.T1, s->sc + SC_HD2, 1, s->red_ws) );
         }
         Xs.push_back(B.X);
      }
      if ( q > 0 )
      {
         if ( small_problem(s) )
         {
            HS_CALL( hs_lp_rows_small(st, q, m1, s->Dext, s->yt, 0, 0.0, 0.0, s->x, s->z,
               (const double*) NULL, (const double*) NULL, s->rd, (double*) NULL) );
         }
         else if ( !recur )
         {
            const double* v = s->yt;
            HS_CALL( hs_gemv_n(st, q, m1, s->Dext, m1, 1, &v, s->tmpq, q, s->gemv_ws, s->gemv_ws_len) );
            HS_CALL( hs_scale_add(st, q, 1.0, s->tmpq, -1.0, s->z, s->rd) );
         }
         else if ( rd_pending )
            HS_CALL( hs_scale_add(st, q, rd_scale, s->rd, 0.0, NULL, s->rd) );
         HS_CALL( hs_dot(st, q, s->rd, s->rd, s->sc + SC_RD2, 1, s->red_ws) );
         HS_CALL( hs_absmax(st, q, s->rd, s->sc + SC_RDLPMAX, 0, s->red_ws) );
         HS_CALL( hs_dot(st, q, s->x, s->z, s->sc + SC_XZ, 1, s->red_ws) );
         if ( want_cert )
         {
            /* rd + tau * c */
            HS_CALL( hs_red_batch_flush() );
            HS_HIP( hipMemcpy2DAsync(s->tmpq, sizeof(double), s->Dext, (size_t) m1 * sizeof(double), sizeof(double), (size_t) q, hipMemcpyDeviceToDevice, st) );
            HS_CALL( hs_scale_add(st, q, s->tau, s->tmpq, 1.0, s->rd, s->tmpq) );
            HS_CALL( hs_dot(st, q, s->tmpq, s->tmpq, s->sc + SC_HD2, 1, s->red_ws) );
         }
      }
      else
         HS_CALL( hs_fill_scalar(st, s->sc + SC_RDLPMAX, 0.0) );
      const int fusedA = apply_A_small(s, Xs.data(), s->x, s->AX, 2, s->tau, s->b, s->rp);
      if ( fusedA < 0 )
         return -fusedA;
      if ( fusedA == 0 )
         HS_CALL( apply_A(s, Xs.data(), s->x, s->AX) );
      HS_CALL( hs_copy_scalar(st, s->sc + SC_AX0, s->AX) );
      if ( fusedA == 0 )
      {
         HS_CALL( hs_red_batch_flush() );
         hipLaunchKernelGGL(k_rp, g1d(m > 0 ? m : 1), dim3(256), 0, st, m, s->tau, s->b, s->AX, s->rp);
         HS_LAUNCH_CHECK();
      }
      HS_CALL( hs_dot(st, m, s->rp, s->rp, s->sc + SC_RP2, 0, s->red_ws) );
      HS_CALL( hs_dot(st, m, s->AX + 1, s->AX + 1, s->sc + SC_HP2, 0, s->red_ws) );
      HS_CALL( hs_dot(st, m, s->b, s->y, s->sc + SC_DOBJ, 0, s->red_ws) );
      rd_pending = false;
      return HS_OK;
   }

   int residual_pass()
   {
      phase_mark(s, PH_RESID);
      if ( s->use2 && !zchain_queued && K > 0 )
      {
         HS_HIP( hipMemsetAsync(s->flags, 0, 8 * sizeof(int), st) );
         HS_CALL( queue_z_chains() );
      }
      HS_CALL( enqueue_residuals() );
      return read_back(NULL);
   }

   /* ---- termination (mirrors oracle/ipm_ref.py) */
   int terminate()
   {
      const double tau = s->tau, kappa = s->kappa;
      pobj = hs.v[SC_AX0];
      dobj = hs.v[SC_DOBJ];
      rg = pobj - dobj - kappa;
      mu = (hs.v[SC_XZ] + tau * kappa) / N1;
      double rd2 = hs.v[SC_RD2];
      double rdmax = hs.v[SC_RDLPMAX];
      for (int k = 0; k < K; ++k)
      {
         rd2 += hs.v[SC_BLK(k, 0)];
         rdmax = fmax(rdmax, sqrt(hs.v[SC_BLK(k, 0)]));
      }
      pinf = sqrt(hs.v[SC_RP2]) / tau / (1.0 + normb);
      const double pabs = sqrt(hs.v[SC_RP2]) / tau;
      const bool pabsok = par.pabstol <= 0.0 || pabs <= par.pabstol;
      dinf = sqrt(rd2) / tau / (1.0 + normC);
      dabs = rdmax / tau;
      gap = fabs(dobj - pobj) / tau;
      if ( par.verbose )
         printf("hipsdp it %3d mu %.3e pinf %.3e dinf %.3e gap %.3e pobj %.8e dobj %.8e tau %.3e kap %.3e\n", it, mu, pinf, dinf,
            gap, pobj / tau, dobj / tau, tau, kappa);
      if ( !std::isfinite(mu) || !std::isfinite(pinf) || !std::isfinite(dinf) )
      {
         return halt(HIPSDP_STATUS_NUMERIC);
      }
      /* preoptimal iterate (warm-start point for the children of a node: relax_sdp.c "warmstartpreoptsol"): the first interior
       * iterate that is feasible to tolerance with a relative gap below preoptgap, as DSDP's monitor captures it
       * (sdpisolver_dsdp.c:323-358) */
      if ( par.preoptgap > 0.0 && !s->pre_valid && pinf <= par.feastol && dabs <= par.feastol
         && gap / (1.0 + 0.5 * fabs(pobj / tau) + 0.5 * fabs(dobj / tau)) < par.preoptgap )
      {
         HS_CALL( ensure_preoptimal(s) );
         if ( m > 0 ) HS_CALL( hs_copy(st, s->pre_y, s->y, m) );
         if ( q > 0 ) HS_CALL( hs_copy(st, s->pre_x, s->x, q) );
         for (auto& B : s->blk)
            HS_CALL( hs_copy(st, B.Xpre, B.X, (long long) B.n * B.n) );
         s->pre_scale = 1.0 / tau;
         s->pre_valid = true;
      }
      /* objective limit: with X feasible to tolerance, pobj is a lower bound of the minimisation problem
       * (SCIP_SDPPAR_OBJLIMIT, type_sdpi.h:53); tested first so that a node whose optimum lies above the limit reports it */
      if ( par.objlimit < 1e20 && pinf <= par.feastol && pobj / tau > par.objlimit + par.gaptol )
      {
         return halt(HIPSDP_STATUS_OBJLIM);
      }
      if ( pinf <= par.feastol && pabsok && dabs <= par.feastol && gap <= par.gaptol )
      {
         return halt(HIPSDP_STATUS_OPTIMAL);
      }
      const bool certzone = (tau < 1e-2 * fmin(1.0, kappa)) || (mu / (tau * tau) > 1e10);
      if ( certzone && want_cert )
      {
         const double hd = sqrt(hs.v[SC_HD2]);
         const double hp = sqrt(hs.v[SC_HP2]);
         const double big = fmax(fabs(dobj), fabs(pobj));
         const bool cand_dunb = dobj < -1e-3 * big;
         const bool cand_dinf = pobj > 1e-3 * big;
         const bool ok_dunb = cand_dunb && hd <= par.infeastol * (-dobj);
         const bool ok_dinf = cand_dinf && hp <= par.infeastol * pobj;
         if ( (ok_dunb || ok_dinf) && (ok_dunb || !cand_dunb || certwait >= 5) && (ok_dinf || !cand_dinf || certwait >= 5) )
         {
            return halt((ok_dunb && ok_dinf) ? HIPSDP_STATUS_PDINF : (ok_dunb ? HIPSDP_STATUS_DUNB : HIPSDP_STATUS_DINF));
         }
         if ( ok_dunb || ok_dinf )
            ++certwait;
      }
      if ( certzone && !want_cert )
      {
         /* the certificate residual was not computed in this pass: redo the (cheap) residual pass with it */
         want_cert = true;
         HS_CALL( residual_pass() );
         return terminate();
      }
      want_cert = certzone;
      if ( it == par.maxiter )
         return halt(status);
      if ( mu > 0.9 * lastmu && alpha_last < 1e-2 )
      {
         if ( ++nstall >= stall_lim )
         {
            return halt(HIPSDP_STATUS_NUMERIC);
         }
      }
      else
         nstall = 0;
      lastmu = mu;
      /* no progress: the worst scaled violation has not improved by 10 % for 6 iterations (accuracy limit of the problem) */
      if ( !certzone )
      {
         double merit = fmax(fmax(pinf / par.feastol, dabs / par.feastol), gap / par.gaptol);
         if ( par.pabstol > 0.0 )
            merit = fmax(merit, pabs / par.pabstol);
         if ( merit < 0.9 * bestmerit )
         {
            bestmerit = merit;
            sincebest = 0;
         }
         else if ( ++sincebest >= nobest_lim )
         {
            return halt(HIPSDP_STATUS_NUMERIC);
         }
      }
      if ( par.timelimit > 0.0 )
      {
         const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
         int over = el > par.timelimit ? 1 : 0;
         if ( s->comm != NULL )
         {
            /* the clocks of the ranks differ: rank 0's decision counts everywhere */
            HS_HIP( hipMemcpyAsync(s->flags + 7, &over, sizeof(int), hipMemcpyHostToDevice, st) );
            HS_CALL( hs_bcast_ints(s->comm, s->flags + 7, 1, st) );
            HS_HIP( hipMemcpyAsync(&over, s->flags + 7, sizeof(int), hipMemcpyDeviceToHost, st) );
            HS_HIP( hipStreamSynchronize(st) );
         }
         if ( over )
         {
            return halt(HIPSDP_STATUS_TIMELIM);
         }
      }
      return HS_OK;
   }

   /* ---- factorizations (the factors of an accepted step are re-used: they were computed by its Cholesky check) */
   int factorize()
   {
      phase_mark(s, PH_FACTOR);
      defer_join = defer_ok && !(identity_start && it == 0) && !xchain_queued;
      if ( !zchain_queued )
      {
         if ( !(setf && m <= 64) )
            HS_HIP( hipMemsetAsync(s->flags, 0, 8 * sizeof(int), st) );
         HS_CALL( fork2(s) );
      }
      for (auto& B : s->blk)
      {
         const int n = B.n;
         if ( n > 64 )
         {
            if ( !zchain_queued )
               HS_CALL( z_chain(B, st2) );
            if ( !xchain_queued )
               HS_CALL( x_chain(B, !defer_join) );
            continue;
         }
         /* single-block factors: one launch per matrix yields L (zero upper), inv(L) as n x n and, for n <= 32, the inverse of Z;
          * after an accepted step they already exist (the step's Cholesky check produced them) */
         if ( !(factors_valid && B.derived_valid) )
         {
            HS_CALL( hs_potrf_small_ext(st2, n, B.Lz, B.dinvz, s->flags + 0, B.Z, NULL, 0.0, NULL, B.LzInv, n <= 32 ? B.Zinv : NULL, setf) );
            HS_CALL( hs_potrf_small_ext(st, n, B.Lx, B.dinvx, s->flags + 1, B.X, NULL, 0.0, NULL, B.LxInv, NULL, setf) );
            B.derived_valid = true;
         }
         if ( n > 32 )
         {
            HS_CALL( gemm_on(st2, HS_MC, HS_MC, n, n, n, 1.0, B.LzInv, n, B.LzInv, n, 0.0, B.Zinv, n, HS_GEMM_LOWER) );
            HS_CALL( hs_mirror_lower(st2, B.Zinv, n, n) );
         }
      }
      zchain_queued = xchain_queued = false;
      if ( !defer_join )
         return join2(s);
      s->sws.after_g1 = after_g1_x_inverse;
      s->sws.after_g1_arg = s;
      return HS_OK;
   }

   /* ---- Schur complement (extended by the constant matrix as "variable 0") */
   int assemble()
   {
      phase_mark(s, PH_SCHUR);
      gram_only_used = gram_cached = false;
      hs_comm_phase(0);
      const bool clk_this = s->clk_on && s->clk_buf != NULL && s->clk_stream != NULL && s->clk_n < CLK_MAX_ASSEMBLIES;
      HS_HIP( hipEventRecord(s->ev0, st) );
      if ( clk_this )
      {
         /* the counting thread starts when the assembly may start (behind the event) on its own queue */
         HS_HIP( hipMemsetAsync(s->clk_buf + 4 * s->clk_n, 0, 4 * sizeof(unsigned long long), st) );
         HS_HIP( hipEventRecord(s->ev0, st) );
         HS_HIP( hipStreamWaitEvent(s->clk_stream, s->ev0, 0) );
         hipLaunchKernelGGL(k_clock_window, dim3(1), dim3(1), 0, s->clk_stream, s->clk_buf + 4 * s->clk_n);
         HS_LAUNCH_CHECK();
      }
      const double mfma_flops_before = hs_mfma_flops_total();
      schur_small = false;
      if ( s->comm == NULL && !s->shardA && !s->schur_mode_rows && !s->schur_mode_forced && K > 0 )
      {
         /* B&B-sized problems: one launch for the whole extended Schur matrix and the copies the factorization needs */
         std::vector<int> bn;
         std::vector<const double*> bA, bX, bZ;
         bool anysp = false;
         for (auto& B : s->blk)
         {
            bn.push_back(B.n); bA.push_back(B.A); bX.push_back(B.X); bZ.push_back(B.Zinv);
            anysp = anysp || B.sparse;
         }
         const int rs = anysp ? 0 : hs_schur_small(st, m1, K, bn.data(), bA.data(), bX.data(), bZ.data(), q, s->Dext, s->x, s->z, s->Mx,
            m > 0 ? s->Lm : NULL, s->dya);
         if ( rs < 0 )
            return -rs;
         schur_small = (rs == 1);
      }
      if ( !schur_small )
         HS_CALL( assemble_forms() );
      if ( defer_join )
      {
         /* (the first queue has waited for the event inside hs_schur_W; once more for whoever follows, and the hooks are taken out) */
         s->sws.ev_g2 = NULL;
         s->sws.after_g1 = NULL;
         HS_CALL( join2(s) );
      }
      HS_HIP( hipEventRecord(s->ev1, st) );
      if ( clk_this )
      {
         hipLaunchKernelGGL(k_clock_stop, dim3(1), dim3(1), 0, st, s->clk_buf + 4 * s->clk_n);
         HS_LAUNCH_CHECK();
         ++s->clk_n;
      }
      info->schur_flops_executed += hs_mfma_flops_total() - mfma_flops_before;
      hs_comm_phase(2);
      return HS_OK;
   }

   /* which identity form a dense block takes on one device (see assemble_forms) */
   bool identity_packed(const Block& B) const
   {
      return B.Apk != NULL && hs_schur_identity_packed_fits(&s->sws, m1, B.n);
   }

   /* Cold start on one device, general path, every block dense: the first assembly is a function of the constraint matrices alone and
    * is kept across solves (hs_gram_cache.h).  Fills the key of what this assembly would compute and makes sure the store exists;
    * false: this assembly is not cached (computed as ever, the store left alone) - warm start or HIPSDP_NO_IDENTITY_START, a later
    * iteration, several ranks or any sharded / forced / U form, a block kept as nonzeros, a block whose device pointer the caller
    * holds, or no memory for the store. */
   bool gram_cache_key(hs_gram_key* key)
   {
      if ( !(identity_start && it == 0) || s->comm != NULL || s->shardA || s->schur_mode_cols || s->schur_mode_rows || K < 1
         || K > HS_GRAM_MAXBLK )
         return false;
      int bn[HS_GRAM_MAXBLK], form[HS_GRAM_MAXBLK];
      unsigned long long gen[HS_GRAM_MAXBLK];
      for (int k = 0; k < K; ++k)
      {
         const Block& B = s->blk[k];
         if ( B.sparse || B.a_escaped )
            return false;
         bn[k] = B.n;
         form[k] = identity_packed(B) ? HS_GRAM_FORM_PACKED : HS_GRAM_FORM_FULL;
         gen[k] = B.A_gen;
      }
      if ( !hs_gram_key_make(key, m, K, bn, form, gen, s->sws.kws_len, s->sws.chunk_cols, s->sws.full) )
         return false;
      const long long len = (long long) (m1 + 32) * m1;
      if ( s->gc_M != NULL && s->gc_len != len )
      {
         /* (a shape of the same blocks with another m inside the same allocations: nothing is queued on the store - the copy into it
          * and every copy out of it ran in solves that have ended) */
         (void) hipFree(s->gc_M);
         s->gc_M = NULL;
         s->gc_nomem = false;
         hs_gram_key_clear(&s->gc_key);
      }
      if ( s->gc_M == NULL && !s->gc_nomem )
      {
         if ( hipMalloc((void**) &s->gc_M, (size_t) len * sizeof(double)) != hipSuccess )
         {
            (void) hipGetLastError();        /* no room: no cache, not an error */
            s->gc_M = NULL;
            s->gc_nomem = true;
         }
         s->gc_len = len;
         hs_gram_key_clear(&s->gc_key);
      }
      return s->gc_M != NULL;
   }

   /* the assembly in the form the solver's mode selects, then the sparse blocks and the LP term */
   int assemble_forms()
   {
      hs_gram_key gkey;
      const bool gram_keyed = gram_cache_key(&gkey);
      gram_cached = gram_keyed && hs_gram_key_match(&s->gc_key, &gkey);
      if ( !gram_cached )
         HS_CALL( hs_fill(st, s->Mx, (long long) m1 * m1, 0.0) );
      if ( gram_cached )
      {
         /* the same matrices as at the cold solve that stored it: the Gram matrix of all blocks as that solve's identity assemblies
          * left it in Mx (padding rows included) - no clear, no Gram launch, no summation, no D D^T */
         HS_CALL( hs_copy(st, s->Mx, s->gc_M, s->gc_len) );
         ++s->gc_hits;
         gram_only_used = true;
      }
      else if ( s->shardA )
      {
         /* matrices sharded by variable: W_j where A_j lives, all-to-all of the row ranges, partial Gram matrices summed */
         for (auto& B : s->blk)
            if ( !B.sparse )
               HS_CALL( hs_schur_Wvar_all(st, s->stream2, s->comm, s->rank, s->nranks, m1, B.n, B.A, B.Lx, B.LzInv, s->Mx, &s->sws, s->var_cw,
                     s->var_overlap ? 1 : 0) );
         HS_CALL( hs_allreduce_sum(s->comm, s->Mx, (long long) m1 * m1, st) );
      }
      else if ( s->schur_mode_cols )
      {
         /* W formulation in column slices: this rank's slices of every W_j, partial matrices summed over the ranks */
         const int S = s->schur_sim_shards;
         const int per = S / (s->comm != NULL ? s->nranks : 1);
         const int g0 = (s->comm != NULL ? s->rank : 0) * per;
         for (int g = g0; g < g0 + per; ++g)
            for (auto& B : s->blk)
            {
               if ( B.sparse )
                  continue;
               int c0, cw;
               hs_shard_cols(m1, B.n, S, g, &c0, &cw);
               if ( identity_start && it == 0 )
               {
                  /* (all column slices of this rank at once, straight from A; several ranks: the n^2 entries of the matrices in equal
                   * ranges, the partial Gram matrices are summed below like the slices' ones) */
                  if ( g == g0 )
                  {
                     const long long n2 = (long long) B.n * B.n;
                     const int G = s->comm != NULL ? s->nranks : 1, r = s->comm != NULL ? s->rank : 0;
                     const long long k0 = ((n2 * r / G) / 8) * 8, k1 = r == G - 1 ? n2 : ((n2 * (r + 1) / G) / 8) * 8;
                     HS_CALL( hs_schur_W_identity_range(st, m1, B.n, B.A, k0, k1, s->Mx, &s->sws) );
                  }
                  gram_only_used = true;
                  continue;
               }
               HS_CALL( hs_schur_Wcols(st, m1, B.n, B.A, B.Lx, B.LzInv, s->Mx, &s->sws, c0, cw) );
            }
         if ( s->comm != NULL )
            HS_CALL( hs_allreduce_sum(s->comm, s->Mx, (long long) m1 * m1, st) );
      }
      else if ( s->comm != NULL || s->schur_mode_rows )
      {
         /* sharded assembly: this rank computes two row chunks of the upper triangle, the chunks are all-gathered */
         int c, b1, b2;
         hs_shard_rows(m1, s->nranks, s->rank, &c, &b1, &b2);
         for (auto& B : s->blk)
         {
            if ( B.sparse )
               continue;
            HS_CALL( hs_schur_Urows(st, m1, B.n, B.A, B.X, B.Zinv, s->Mx, &s->sws, b1, b1 + c) );
            HS_CALL( hs_schur_Urows(st, m1, B.n, B.A, B.X, B.Zinv, s->Mx, &s->sws, b2, b2 + c) );
         }
         if ( s->comm != NULL )
         {
            const long long cnt = (long long) c * m1;
            /* chunks 0 .. G-1 sit at their final place; chunks G .. 2G-1 are owned in reverse rank order */
            HS_CALL( hs_allgather_inplace(s->comm, s->Mx, cnt, s->rank, st) );
            HS_CALL( hs_allgather(s->comm, s->Mx + (long long) b2 * m1, s->Mgather, cnt, st) );
            for (int r = 0; r < s->nranks; ++r)
            {
               const long long dstrow = (long long) (2 * s->nranks - 1 - r) * c;
               if ( dstrow >= m1 )
                  continue;
               long long rowsleft = m1 - dstrow;
               if ( rowsleft > c ) rowsleft = c;
               HS_CALL( hs_copy(st, s->Mx + dstrow * m1, s->Mgather + (long long) r * cnt, rowsleft * m1) );
            }
         }
         HS_CALL( hs_mirror_upper(st, s->Mx, m1, m1) );
      }
      else
      {
         for (auto& B : s->blk)
         {
            if ( B.sparse )
               continue;
            if ( identity_start && it == 0 )
            {
               /* one device: the Gram matrix from the packed lower triangles, half the K of the full rows.  The solve packed them ahead
                * of its first residual sweep (ensure_packed): a packed copy that exists is valid here.  The full storage serves when there
                * is no packed copy (n <= 64, or no memory for it) or when a chunked workspace is too small for the m1 x n diagonals the
                * packed form gathers into it (m1 above about 128 n).  The sharded branches above stay on the full storage: a rank's packed
                * copy covers its own rows only. */
               assert(B.Apk == NULL || B.apk_valid);
               if ( identity_packed(B) )
                  HS_CALL( hs_schur_W_identity_packed(st, m1, B.n, B.Apk, B.Lp, s->Mx, &s->sws) );
               else
                  HS_CALL( hs_schur_W_identity(st, m1, B.n, B.A, s->Mx, &s->sws) );
               gram_only_used = true;
            }
            else if ( s->schur_mode_U )
               HS_CALL( hs_schur_U(st, m1, B.n, B.A, B.X, B.Zinv, s->Mx, &s->sws, 0, m1) );
            else
               HS_CALL( hs_schur_W(st, m1, B.n, B.A, B.Lx, B.LzInv, s->Mx, &s->sws) );
         }
         if ( gram_keyed )
         {
            /* a cold solve of matrices the store does not hold: kept for the next one (before the LP term, which depends on x / z) */
            ++s->gc_misses;
            HS_CALL( hs_copy(st, s->gc_M, s->Mx, s->gc_len) );
            s->gc_key = gkey;
         }
      }
      /* blocks in sparse mode (csrc/sparse.hip), on every rank alike, behind the exchange of the sharded forms: column 0 from
       * U_0 = X A_0 Zinv (A_0 is dense) and one gather pass, the pairs of variables from the pair formula over their nonzeros */
      for (auto& B : s->blk)
      {
         if ( !B.sparse )
            continue;
         const int n = B.n;
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, 1.0, B.X, n, B.A0, n, 0.0, B.T1, n) );
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, 1.0, B.T1, n, B.Zinv, n, 0.0, B.W, n) );
         HS_CALL( pass_A(s, B, B.W, s->tmpe) );
         hipLaunchKernelGGL(k_add_col0, g1d(m1), dim3(256), 0, st, m1, s->tmpe, s->Mx);
         HS_LAUNCH_CHECK();
         HS_CALL( hs_sp_schur(st, B.sp, B.X, B.Zinv, s->Mx) );
      }
      if ( q > 0 )
      {
         HS_CALL( hs_lp_scale_rows(st, q, m1, s->x, s->z, s->Dext, s->Slp) );
         HS_CALL( gemm(s, HS_MC, HS_MC, m1, m1, q, 1.0, s->Dext, m1, s->Slp, m1, 1.0, s->Mx, m1, HS_GEMM_LOWER) );
      }
      return hs_mirror_lower(st, s->Mx, m1, m1);
   }

   /* ---- solves with M, then B_k = A_0 - sum w_i A_i ; beta = c - D w ; S0 ; b^T M^-1 b */
   int solve_m()
   {
      phase_mark(s, PH_MSOLVE);
      predH_queued = predH_joined = split_dz = false;
      if ( s->use2 && s->comm == NULL && !small_problem(s) && m > 0 )
      {
         /* the predictor's right-hand side (H_k, A(H), h) needs nothing from the Schur matrix: it runs on the second queue beside the
          * latency-bound factorization of M (one communicator serves one queue: not with several ranks) */
         HS_CALL( fork2(s) );
         {
            QueueSwap sw(s);
            HS_CALL( direction(s, 0.0, 1.0, mu, rg, false, 0.0, 1) );
         }
         predH_queued = true;
      }
      if ( m > 0 )
      {
         if ( !schur_small )
         {
            HS_HIP( hipMemcpy2DAsync(s->Lm, (size_t) m * sizeof(double), s->Mx + m1 + 1, (size_t) m1 * sizeof(double),
                  (size_t) m * sizeof(double), (size_t) m, hipMemcpyDeviceToDevice, st) );
            /* original diagonal of M for the semidefinite pivot rule */
            HS_HIP( hipMemcpy2DAsync(s->dya, sizeof(double), s->Mx + m1 + 1, (size_t) (m1 + 1) * sizeof(double), sizeof(double), (size_t) m,
                  hipMemcpyDeviceToDevice, st) );
         }
         HS_CALL( hs_potrf_psd(st, m, s->Lm, s->dinvm, s->flags + 2, s->dya, s->regmask, setf) );
         if ( m <= 64 )
         {
            HS_CALL( hs_solve2_small(st, m, s->Mx, s->b, s->dinvm, s->Lm, s->rhs2, s->u2, s->wt, hs_small_solve_by_substitution()) );
         }
         else
         {
            hipLaunchKernelGGL(k_rhs2, g1d(m), dim3(256), 0, st, m, s->Mx, s->b, s->rhs2);
            HS_LAUNCH_CHECK();
            if ( predH_queued )
            {
               /* the predictor's right-hand side h (formed on the second queue while M was factored) sits behind g and b: one
                * solve with three right-hand sides instead of a pair and, later, a single one */
               HS_CALL( join2(s) );
               predH_joined = true;
               HS_CALL( hs_trsv_sync(st, m, s->Lm, s->dinvm, 3, s->rhs2, m, SOLVE_MODE, s->trsv_ws, &s->trsv_epoch) );
            }
            else
               HS_CALL( hs_trsv_sync(st, m, s->Lm, s->dinvm, 2, s->rhs2, m, SOLVE_MODE, s->trsv_ws, &s->trsv_epoch) );
         }
      }
      split_dz = predH_joined && s->comm == NULL;
      for (auto& B : s->blk)
         if ( B.Apk == NULL )
            split_dz = false;
      const bool tail = general_tail(s);
      /* (with the three-vector sweep ahead, the coefficient vectors [1; u2] and [0; u1] come out of the same launch) */
      if ( m == 0 || m > 64 )
         HS_CALL( hs_ipm_after_solve2(st, m, s->rhs2, s->u2, s->wt, s->u1, (split_dz && tail) ? s->cvec : NULL, s->cvec + m1, 1) );
      hs_red_batch_begin(st);
      HS_CALL( hs_fill_scalar(st, s->sc + SC_S0, 0.0) );
      /* dZ = A^T([-dtau; u1 - u2 dtau]) + eta Rd is linear in dtau: A^T([0; u1]) - dtau A^T([1; u2]) + eta Rd.  u2 belongs to the
       * iteration, the predictor's u1 has just been solved with it, so B = A^T(wt), P2 = A^T([1; u2]) and the predictor's
       * P1 = A^T([0; u1]) come out of ONE sweep over A (three coefficient vectors), the corrector needs one more sweep for its P1:
       * two sweeps per iteration where B, the predictor's dZ and the corrector's dZ took three - and the dependent chain
       * B pass -> dtau -> dZ pass loses a link.  Single GPU, packed copy present, predictor solved early (else the old form). */
      if ( split_dz && !tail )
      {
         HS_CALL( hs_make_ext(st, m, 1.0, 1.0, s->u2, s->cvec) );
         HS_CALL( hs_make_ext(st, m, 0.0, 1.0, s->u1, s->cvec + m1) );
         HS_LAUNCH_CHECK();
      }
      int slot = 0;
      for (auto& B : s->blk)
      {
         const int n = B.n;
         const long long n2 = (long long) n * n;
         bool swept = false;
         if ( split_dz )
         {
            if ( B.P2 == NULL )
            {
               HS_CALL( dalloc(&B.P2, n2) );
               HS_CALL( dalloc(&B.pk3, 3 * B.Lp) );
            }
            const int r3 = hs_gemv_t3(st, m1, B.Lp, B.Apk, B.Lp, s->wt, s->cvec, s->cvec + m1, B.pk3, B.pk3 + B.Lp, B.pk3 + 2 * B.Lp);
            if ( r3 < 0 )
               return -r3;
            if ( r3 == 1 )
            {
               if ( tail )
               {
                  const double* pk[3] = {B.pk3, B.pk3 + B.Lp, B.pk3 + 2 * B.Lp};
                  double* un[3] = {B.B, B.P2, B.dZ};
                  HS_CALL( hs_unpack_sym3(st, n, 3, pk, un) );
               }
               else
               {
                  HS_CALL( hs_unpack_sym(st, n, B.pk3, 0.0, NULL, B.B) );
                  HS_CALL( hs_unpack_sym(st, n, B.pk3 + B.Lp, 0.0, NULL, B.P2) );
                  HS_CALL( hs_unpack_sym(st, n, B.pk3 + 2 * B.Lp, 0.0, NULL, B.dZ) );
               }
               swept = true;
            }
            else
            {
               HS_CALL( pass_AT(s, B, s->cvec, 0.0, NULL, B.P2) );
               HS_CALL( pass_AT(s, B, s->cvec + m1, 0.0, NULL, B.dZ) );
            }
         }
         if ( !swept )
            HS_CALL( pass_AT(s, B, s->wt, 0.0, NULL, B.B) );
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, 1.0, B.X, n, B.B, n, 0.0, B.T1, n) );
         HS_CALL( gemm(s, HS_KC, HS_MC, n, n, n, 1.0, B.T1, n, B.Zinv, n, 0.0, B.W, n) );
         if ( tail )
            HS_CALL( hs_dot_deferred(st, n2, B.B, B.W, s->sc + SC_S0, 1, s->red_ws, slot++) );
         else
            HS_CALL( hs_dot(st, n2, B.B, B.W, s->sc + SC_S0, 1, s->red_ws) );
      }
      if ( q > 0 )
      {
         const double* v = s->wt;
         HS_CALL( hs_gemv_n(st, q, m1, s->Dext, m1, 1, &v, s->beta, q, s->gemv_ws, s->gemv_ws_len) );
         HS_CALL( hs_lp_s0(st, q, s->x, s->z, s->beta, s->sc + SC_S0, 1, s->red_ws) );
      }
      HS_CALL( hs_dot(st, m, s->b, s->rhs2 + m, s->sc + SC_BUB, 0, s->red_ws) );
      return hs_red_batch_end();
   }

   /* ---- predictor: its direction, step length and the centering it leaves to the corrector */
   int predictor()
   {
      phase_mark(s, PH_PRED);
      if ( predH_queued && !predH_joined )
         HS_CALL( join2(s) );
      HS_CALL( direction(s, 0.0, 1.0, mu, rg, false, 0.0, predH_queued ? 2 : 0, predH_joined, split_dz ? 2 : 0) );
      HS_CALL( steplen_enqueue(s) );
      HS_CALL( read_scalars(s, hs, hflags) );
      float ms = 0.f;
      if ( hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess )
         schur_ms += ms;
      info->schur_calls++;
      /* (the assembly at the cold start is the Gram product alone: the count of SURVEY.md 8(d) without its n^3 part) */
      /* (... and one that came out of the store is a call, hipsdp.h, but no flops: every block of it is dense) */
      for (auto& B : s->blk)
         if ( !gram_cached )
            info->schur_flops += (gram_only_used && !B.sparse ? 0.0 : 4.0 * m1 * (double) B.n * B.n * B.n) + (double) m1 * m1 * (double) B.n * B.n;
      if ( hflags[0] != 0 || hflags[1] != 0 || hflags[2] != 0 )
      {
         if ( par.verbose )
            printf("hipsdp: Cholesky failure flags Z=%d X=%d M=%d\n", hflags[0], hflags[1], hflags[2]);
         return halt(HIPSDP_STATUS_NUMERIC);
      }
      const double aa = fmin(1.0, steplen_host(s, hs));
      dta = hs.v[SC_DTAU];
      dka = hs.v[SC_DKAPPA];
      if ( !std::isfinite(aa) || !std::isfinite(dta) )
      {
         if ( par.verbose )
            printf("hipsdp: predictor not finite (alpha %g dtau %g)\n", aa, dta);
         return halt(HIPSDP_STATUS_NUMERIC);
      }
      sigma = (1.0 - aa) * (1.0 - aa) * (1.0 - aa);
      sigma = fmin(1.0, fmax(sigma_floor, sigma));
      eta = 1.0 - sigma;
      return HS_OK;
   }

   /* ---- corrector, with the second-order terms of the predictor */
   int corrector()
   {
      phase_mark(s, PH_CORR);
      for (auto& B : s->blk)
         HS_CALL( gemm(s, HS_KC, HS_MC, B.n, B.n, B.n, 1.0, B.dX, B.n, B.dZ, B.n, 0.0, B.E, B.n) );
      {
         /* (B&B-sized: the LP term and the whole corrector direction are one launch) */
         BatchRegion region(s, batch_regions(s));
         if ( q > 0 )
            HS_CALL( hs_vec_mul(st, q, s->dx, s->dz, s->elp) );
         HS_CALL( direction(s, sigma, eta, mu, rg, true, dta * dka, 0, false, split_dz ? 1 : 0) );
         HS_CALL( region.close() );
      }
      HS_CALL( steplen_enqueue(s) );
      HS_CALL( read_scalars(s, hs, NULL) );
      amax = steplen_host(s, hs);
      alpha = fmin(1.0, gamma_eff * amax);
      dt = hs.v[SC_DTAU];
      dk = hs.v[SC_DKAPPA];
      if ( !std::isfinite(alpha) || !std::isfinite(dt) || !std::isfinite(dk) )
      {
         if ( par.verbose )
            printf("hipsdp: corrector not finite (alpha %g dtau %g dkappa %g)\n", alpha, dt, dk);
         return halt(HIPSDP_STATUS_NUMERIC);
      }
      return HS_OK;
   }

   /* ---- update, with a Cholesky check of the new X and Z (the Lanczos bound is an estimate) */
   int update()
   {
      phase_mark(s, PH_UPDATE);
      /* (blocks of at most 64 rows: the trial iterate is written to Xs / Zs and swapped in; above that the first attempt of
       * step_general saves X and Z to Xs / Zs in the launch that forms the trial iterate) */
      tau0 = s->tau;
      kappa0 = s->kappa;
      applied = 0.0;
      return (small_all && K > 0) ? step_small() : step_general();
   }

   /* small problems: the whole step is applied optimistically and the residual phase of the next iteration is enqueued behind the
    * Cholesky check, so that ONE read-back returns the flags and the new residuals; a failed check takes the step back (pointer
    * swaps, a correcting axpy) and halves it */
   int step_small()
   {
      for (int attempt = 0; attempt < 8; ++attempt)
      {
         if ( !setf )
            HS_HIP( hipMemsetAsync(s->flags, 0, 8 * sizeof(int), st) );
         for (auto& B : s->blk)
         {
            /* the Cholesky checks of the trial X and Z: one launch of two workgroups */
            double* L2[2] = {B.Lx, B.Lz};
            double* di2[2] = {B.dinvx, B.dinvz};
            int* fl2[2] = {s->flags + 1, s->flags + 0};
            const double* ba2[2] = {B.X, B.Z};
            const double* dr2[2] = {B.dX, B.dZ};
            double* mo2[2] = {B.Xs, B.Zs};
            double* li2[2] = {B.LxInv, B.LzInv};
            double* gr2[2] = {NULL, B.n <= 32 ? B.Zinv : NULL};
            HS_CALL( hs_potrf_small_ext_pair(st, B.n, L2, di2, fl2, ba2, dr2, alpha, mo2, li2, gr2, setf) );
         }
         swap_trial();
         if ( batch_regions(s) )
            hs_red_batch_hold(st);           /* (the read-back below ends the region) */
         HS_CALL( apply_step() );
         HS_CALL( enqueue_residuals() );
         HS_CALL( read_scalars(s, hs, hflags) );
         if ( hflags[0] == 0 && hflags[1] == 0 )
         {
            for (auto& B : s->blk)
               B.derived_valid = true;
            factors_valid = true;
            residuals_ready = true;
            alpha_last = alpha;
            return HS_OK;
         }
         swap_trial();
         alpha *= 0.5;
         info->chol_fail++;
      }
      return give_up(true);
   }

   /* One rank: the rest of the step (y, x, z, tau, kappa) is applied optimistically behind the Cholesky check of the new X and Z, and
    * the residual pass of the NEXT iterate (the sweep A(X), the scaled dual residual, the reductions) and the chains of its
    * factorization phase are queued behind that: ONE read-back returns the check's flags and the termination scalars of the next
    * iteration, where there were two with an idle device between them (profiles/r06_a_iter_sequence.txt: 50 us waiting for the flags,
    * then 200 us of small kernels arriving one launch at a time).  A failed check - rare: the step lengths are Lanczos estimates with
    * a safety factor - halves the step; the optimistic part is taken back by a correcting axpy and the dual residual is recomputed
    * from scratch at the next pass (its recurrence was applied in place). */
   int step_general()
   {
      if ( it == 2 && overstep != NULL )
         alpha = amax * atof(overstep);
      for (int attempt = 0; attempt < 8; ++attempt)
      {
         HS_HIP( hipMemsetAsync(s->flags, 0, 8 * sizeof(int), st) );
         /* Blocks above 64 rows: the trial iterates of X and Z and their Cholesky checks are ONE chain on the first queue - one launch
          * for X + alpha dX, Z + alpha dZ, the saved iterate and the copies to factor, then one launch per block column for both
          * matrices (seven launches and a fork in front of two chains before: profiles/r06_c_iter_sequence.txt, 1994 -> 2319 us).
          * The chain writes Z, Lz and dinvz on the first queue, so whatever the second queue still has in flight is awaited first:
          * nothing on a first attempt (solve_m or predictor joined it); after a failed check the Z chains of the iterate that was
          * given up, which read Lz and dinvz - they were ordered before the next factorization of Z by sharing its queue */
         bool large = false, small = false;
         for (auto& B : s->blk)
            (B.n > 64 ? large : small) = true;
         if ( large && s->busy2 )
            HS_CALL( join2(s) );
         for (auto& B : s->blk)
         {
            if ( B.n <= 64 )
               continue;
            const hs_trial_job tj[2] = {{B.X, B.dX, B.Xs, B.Lx}, {B.Z, B.dZ, B.Zs, B.Lz}};
            HS_CALL( hs_trial_pair(st, (long long) B.n * B.n, alpha, attempt == 0 ? 1 : 0, tj) );
            const hs_potrf_job pj[2] = {{B.Lx, B.dinvx, s->flags + 1}, {B.Lz, B.dinvz, s->flags + 0}};
            HS_CALL( hs_potrf_pair(st, B.n, pj) );
         }
         if ( small )
         {
            /* the single-launch checks of X and Z of the small blocks of a mixed problem side by side on the two queues */
            HS_CALL( fork2(s) );
            for (auto& B : s->blk)
            {
               const int n = B.n;
               if ( n > 64 )
                  continue;
               HS_CALL( hs_potrf_small_ext(st, n, B.Lx, B.dinvx, s->flags + 1, B.X, B.dX, alpha, B.Xs, B.LxInv, NULL, setf) );
               HS_CALL( hs_potrf_small_ext(st2, n, B.Lz, B.dinvz, s->flags + 0, B.Z, B.dZ, alpha, B.Zs, B.LzInv, n <= 32 ? B.Zinv : NULL, setf) );
            }
            HS_CALL( join2(s) );
         }
         if ( K == 0 )
            break;
         if ( optimistic )
         {
            swap_trial();
            HS_CALL( apply_step() );
            factors_valid = true;                    /* (what the chains below test: the check has produced the factors) */
            if ( s->use2 && !zchain_queued )
               HS_CALL( queue_z_chains() );
            if ( attempt == 0 )
            {
               rd_have = !small_problem(s);
               rd_pending = rd_have;
               rd_scale = 1.0 - alpha * eta;
            }
            HS_CALL( enqueue_residuals() );
            HS_CALL( read_back(hflags) );
            if ( hflags[0] == 0 && hflags[1] == 0 )
               break;
            /* the step was too long: everything queued behind the check ran on an iterate that is given up (the Z chains may still
             * be running: s->busy2 stays set) */
            swap_trial();
            factors_valid = zchain_queued = xchain_queued = false;
            rd_have = rd_pending = false;
         }
         else
         {
            if ( s->comm == NULL )
               HS_CALL( publish_and_wait(s, s->nsc, 2) );
            else
            {
               HS_CALL( hs_bcast_ints(s->comm, s->flags, 3, st) );
               HS_HIP( hipMemcpyAsync(s->hsc + s->nsc, s->flags, 4 * sizeof(int), hipMemcpyDeviceToHost, st) );
               HS_HIP( hipStreamSynchronize(st) );
            }
            memcpy(hflags, s->hsc + s->nsc, 3 * sizeof(int));
            if ( hflags[0] == 0 && hflags[1] == 0 )
               break;
         }
         alpha *= 0.5;
         info->chol_fail++;
      }
      if ( K > 0 && (hflags[0] != 0 || hflags[1] != 0) )
         return give_up(optimistic && applied != 0.0);
      /* accept the trial iterate: its factors, inverse factors (and inverse) are those of the fused factorization */
      if ( !optimistic )
         swap_trial();
      for (auto& B : s->blk)
         if ( B.n <= 64 )
            B.derived_valid = true;
      factors_valid = (K > 0);
      alpha_last = alpha;
      if ( optimistic && K > 0 )
      {
         residuals_ready = true;                /* (applied, queued and read above) */
         return HS_OK;
      }
      HS_CALL( hs_axpy3(st, alpha, m, s->dy, s->y, q, s->dx, s->x, q, s->dz, s->z) );
      s->tau += alpha * dt;
      s->kappa += alpha * dk;
      /* the residual the next iteration starts from: (1 - alpha eta) times the one this iteration used (general path only: the
       * single-launch kernels of small problems recompute it inside the fused launches) */
      rd_have = !small_problem(s);
      rd_pending = rd_have;
      rd_scale = 1.0 - alpha * eta;
      return HS_OK;
   }

   int run()
   {
      HS_CALL( start() );
      for (it = 0; it <= par.maxiter; ++it)
      {
         if ( !residuals_ready )
            HS_CALL( residual_pass() );
         residuals_ready = false;
         HS_CALL( terminate() );
         if ( stop )
            break;
         HS_CALL( factorize() );
         HS_CALL( assemble() );
         HS_CALL( solve_m() );
         HS_CALL( predictor() );
         if ( !stop )
            HS_CALL( corrector() );
         if ( !stop )
            HS_CALL( update() );
         if ( stop )
            break;
      }
      return HS_OK;
   }

   int finish()
   {
      HS_HIP( hipStreamSynchronize(st) );
      if ( s->clk_on && s->clk_n > 0 )
      {
         if ( s->clk_stream != NULL )
            HS_HIP( hipStreamSynchronize(s->clk_stream) );
         std::vector<unsigned long long> h((size_t) 4 * s->clk_n);
         HS_HIP( hipMemcpy(h.data(), s->clk_buf, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) );
         double dc = 0.0, dw = 0.0;
         for (int a = 0; a < s->clk_n; ++a)
         {
            dc += (double) h[4 * a + 2];
            dw += (double) h[4 * a + 3];
         }
         s->clk_ghz = dw > 0.0 ? dc / (dw * 10.0) : 0.0;
      }
      phase_finish(s);
      s->last_status = status;
      s->solved = true;
      if ( status == HIPSDP_STATUS_DINF || status == HIPSDP_STATUS_DUNB || status == HIPSDP_STATUS_PDINF )
         s->sol_scale = 1.0 / fmax(fmax(fabs(dobj), fabs(pobj)), 1e-300);
      else
         s->sol_scale = 1.0 / s->tau;
      info->status = status;
      info->iterations = it;
      info->pobj = pobj * s->sol_scale;
      info->dobj = dobj * s->sol_scale;
      info->pinf = pinf;
      info->dinf = dinf;
      info->dabs = dabs;
      info->gap = gap;
      info->mu = mu;
      info->tau = s->tau;
      info->kappa = s->kappa;
      info->settings_used = settings;
      info->schur_seconds = schur_ms * 1e-3;
      info->solve_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
      return HIPSDP_OK;
   }

   /* The one way out of run(), whatever it returned.  A stop may leave the Z chains of the abandoned iterate running on the second
    * queue (they are started before the termination decision, and behind a step's Cholesky check): they write B.Lz / B.LzInv /
    * B.Zinv / B.T2, so the solve is over - and its buffers may be re-shaped, freed or read - only when that queue has drained as well.
    * The hooks of the assembly point into this solve. */
   int close(int rc)
   {
      phase_mark(s, -1);
      const int rj = s->busy2 ? join2(s) : HS_OK;
      s->sws.ev_g2 = NULL;
      s->sws.after_g1 = NULL;
      s->sws.after_g1_arg = NULL;
      if ( rc == HIPSDP_OK && rj == HIPSDP_OK )
         return finish();
      (void) hipStreamSynchronize(st);         /* (the roctx range closed, the marks dropped) */
      phase_finish(s);
      return rc != HIPSDP_OK ? rc : rj;
   }
};

static int solve_run(hipsdp_solver* s, hipsdp_info* info, bool try1)
{
   const auto t_begin = std::chrono::steady_clock::now();
   solve_reset(s, info);
   if ( try1 )
   {
      bool done1 = false;
      HS_CALL( solve1_try(s, info, &done1) );
      if ( done1 )
      {
         s->stage_off = 0;                                      /* (the kernel ran the commands and read their data at its start) */
         return HIPSDP_OK;
      }
   }
   GeneralSolve g{s, info, t_begin};
   return g.close(g.run());
}

/* ---- many problems at once: one launch of the one-launch kernel per size class, one workgroup per problem -------------------- */

/* per host thread and grow-only (two threads may call hipsdp_solve_many at the same time): the kernels' arguments staged in pinned
 * memory and their copy in device memory (read throughout the solve: never left in coherent host memory), and the events that order
 * the launches against the solvers' queues.  A call has waited for every launch it made before it returns, so the next call may
 * write them again. */
struct ManyStage
{
   int device = -1;
   size_t cap = 0;                         /* hs_solve1_args in h and d */
   hs_solve1_args* h = NULL;
   hs_solve1_args* d = NULL;
   std::vector<hipEvent_t> ev;
   void release_args()
   {
      if ( h != NULL ) (void) hipHostFree(h);
      if ( d != NULL ) (void) hipFree(d);
      h = NULL; d = NULL; cap = 0;
   }
   void release()
   {
      release_args();
      for (hipEvent_t e : ev) (void) hipEventDestroy(e);
      ev.clear();
      device = -1;
   }
   ~ManyStage() { release(); }
};
static thread_local ManyStage g_many;

static int many_stage(int device, size_t nargs, size_t nev)
{
   ManyStage& g = g_many;
   if ( g.device != device )
   {
      g.release();
      g.device = device;
   }
   if ( g.cap < nargs )
   {
      g.release_args();
      const size_t cap = nargs + nargs / 2 + 16;
      HS_HIP( hipHostMalloc((void**) &g.h, cap * sizeof(hs_solve1_args), hipHostMallocDefault) );
      HS_HIP( hipMalloc((void**) &g.d, cap * sizeof(hs_solve1_args)) );
      g.cap = cap;
   }
   while ( g.ev.size() < nev )
   {
      hipEvent_t e = NULL;
      HS_HIP( hipEventCreateWithFlags(&e, hipEventDisableTiming) );
      g.ev.push_back(e);
   }
   return HIPSDP_OK;
}

static bool many_hip_ok(hipError_t e, const char* what, int line)
{
   if ( e == hipSuccess )
      return true;
   hs_record_hip_error(e, what, __FILE__, line);
   return false;
}

extern "C" int hipsdp_solve_many(int count, hipsdp_solver* const* solvers, const hipsdp_params* params, hipsdp_info* infos, int* rcs)
{
   g_err[0] = 0;
   if ( count < 0 )
      return HIPSDP_ERR_ARG;
   if ( count == 0 )
      return HIPSDP_OK;
   if ( solvers == NULL || infos == NULL )
      return HIPSDP_ERR_ARG;
   for (int i = 0; i < count; ++i)
   {
      const hipsdp_solver* s = solvers[i];
      if ( s == NULL || !s->shaped )
      {
         set_err("hipsdp_solve_many: a solver is NULL or has no shape");
         return HIPSDP_ERR_ARG;
      }
      if ( s->comm != NULL || s->device != solvers[0]->device )
      {
         set_err("hipsdp_solve_many: the solvers must be on one device and have no communicator");
         return HIPSDP_ERR_ARG;
      }
   }
   {
      std::vector<const hipsdp_solver*> u(solvers, solvers + count);
      std::sort(u.begin(), u.end());
      if ( std::adjacent_find(u.begin(), u.end()) != u.end() )
      {
         set_err("hipsdp_solve_many: the same solver twice");
         return HIPSDP_ERR_ARG;
      }
   }
   const int dev = solvers[0]->device;
   HS_HIP( hipSetDevice(dev) );
   HS_CALL( many_stage(dev, (size_t) count, (size_t) count + 4) );

   /* 1. what hipsdp_solve does before the kernel, for each solver, and the kernel's arguments */
   static const int classes[4] = {10, 16, 64, 1064};
   struct Item { int rc; bool offered, launched, done; int cls; S1Prep pp; };
   std::vector<Item> it((size_t) count);
   std::vector<int> members[4];
   for (int i = 0; i < count; ++i)
   {
      hipsdp_solver* s = solvers[i];
      Item& I = it[i];
      I.offered = I.launched = I.done = false;
      I.cls = -1;
      int rc = flush_zeros(s);
      if ( rc == HIPSDP_OK )
         rc = solve_begin(s, params != NULL ? &params[i] : NULL, &infos[i]);
      if ( rc == HIPSDP_OK )
      {
         solve_reset(s, &infos[i]);
         rc = solve1_prepare(s, &I.pp, &I.offered);
      }
      I.rc = rc;
      if ( rc == HIPSDP_OK && I.offered )
      {
         const int c = hs_solve1_class(&I.pp.a);
         I.cls = c == 10 ? 0 : (c == 16 ? 1 : (c == 64 ? 2 : 3));
         members[I.cls].push_back(i);
      }
   }

   /* 2. one launch per class, on the queue of its first solver, behind everything queued on every member's queue (the staged
    * setters); every member's queue then waits for the launch, so X and Z are complete once that queue has drained, as after
    * hipsdp_solve */
   ManyStage& g = g_many;
   hipStream_t lst[4] = {NULL, NULL, NULL, NULL};
   size_t off = 0, nev = 0;
   for (int c = 0; c < 4; ++c)
   {
      const std::vector<int>& mem = members[c];
      const int n = (int) mem.size();
      if ( n == 0 )
         continue;
      hipStream_t L = solvers[mem[0]]->stream;
      for (int j = 0; j < n; ++j)
         memcpy(&g.h[off + j], &it[mem[j]].pp.a, sizeof(hs_solve1_args));
      bool ok = true;
      for (int j = 1; j < n && ok; ++j)
      {
         hipEvent_t e = g.ev[nev++];
         ok = many_hip_ok(hipEventRecord(e, solvers[mem[j]]->stream), "hipEventRecord(member queue)", __LINE__) &&
              many_hip_ok(hipStreamWaitEvent(L, e, 0), "hipStreamWaitEvent(launch queue)", __LINE__);
      }
      ok = ok && many_hip_ok(hipMemcpyAsync(g.d + off, g.h + off, (size_t) n * sizeof(hs_solve1_args), hipMemcpyHostToDevice, L),
                             "hipMemcpyAsync(solve-many arguments)", __LINE__);
      ok = ok && hs_solve1_launch_many(L, classes[c], g.d + off, n) == HS_OK;
      if ( ok )
      {
         hipEvent_t e = g.ev[nev++];
         ok = many_hip_ok(hipEventRecord(e, L), "hipEventRecord(launch queue)", __LINE__);
         for (int j = 1; j < n && ok; ++j)
            ok = many_hip_ok(hipStreamWaitEvent(solvers[mem[j]]->stream, e, 0), "hipStreamWaitEvent(member queue)", __LINE__);
      }
      if ( ok )
      {
         lst[c] = L;
         (void) __sync_add_and_fetch(&g_many_launches, 1);
      }
      for (int j = 0; j < n; ++j)
      {
         it[mem[j]].launched = ok;
         if ( !ok )
            it[mem[j]].rc = HIPSDP_ERR_HIP;
      }
      off += (size_t) n;
   }

   /* 3. the sequence words of all launched problems, polled together; a launch queue that has finished while a member's word is
    * missing: that launch failed (asked at the cadence of hipsdp_solve's wait, counted in words read) */
   {
      std::vector<SeqWord> words((size_t) count);
      std::vector<char> pub((size_t) count, 0);
      for (int i = 0; i < count; ++i)
         words[i] = SeqWord{it[i].pp.host, it[i].pp.a.seq, it[i].launched ? it[i].cls : -1};
      wait_published(words.data(), count, lst, 4, "hipStreamQuery(one-launch solve of many)", pub.data());
      for (int i = 0; i < count; ++i)
         if ( it[i].launched && !pub[i] )
            it[i].rc = HIPSDP_ERR_HIP;
   }

   /* 4. the results, then the general path for the problems the kernel declined or gave up on (from the same start) and the ones
    * never offered, one after another as hipsdp_solve would solve them */
   for (int i = 0; i < count; ++i)
   {
      Item& I = it[i];
      hipsdp_solver* s = solvers[i];
      if ( I.rc == HIPSDP_OK && I.launched )
      {
         I.rc = solve1_finish(s, &I.pp, &infos[i], &I.done);
         if ( I.rc == HIPSDP_OK && I.done )
         {
            s->stage_off = 0;                                   /* (the kernel ran the commands and read their data at its start) */
            (void) __sync_add_and_fetch(&g_many_problems, 1);
         }
      }
      if ( I.rc != HIPSDP_OK || I.done )
         I.rc = solve_end(s, I.rc);
   }
   int rc_all = HIPSDP_OK;
   for (int i = 0; i < count; ++i)
   {
      Item& I = it[i];
      if ( I.rc == HIPSDP_OK && !I.done )
         I.rc = solve_end(solvers[i], solve_run(solvers[i], &infos[i], false));
      if ( rcs != NULL )
         rcs[i] = I.rc;
      if ( rc_all == HIPSDP_OK )
         rc_all = I.rc;
   }
   return rc_all;
}

/* ---- one problem, many objectives: one workgroup per objective on the matrices of ONE solver -------------------------------- */

static long long g_objs_calls = 0;         /* hipsdp_solve_objectives: calls that passed the argument checks with count > 0 */
static long long g_objs_launches = 0;      /* ... launches of the fan-out and of the one-launch kernel */
static long long g_objs_problems = 0;      /* ... jobs whose results the kernel delivered */
#define OBJS_CHUNK_MAX 512                 /* most lanes of a solver, and jobs of one launch */
#define OBJS_LANE_BYTES (256LL << 20)      /* ... fewer when that many would take more device memory than this */

/* the lanes of a call: lane 0 is the home lane (the solver's own objective and start point, saved by the fan-out: what the jobs
 * that the general path solves later start from, and what the solver gets back), lanes 1 .. nlanes the jobs of a chunk.  Device
 * part: nlanes + 1 lanes of `stride` doubles (the arrays of hs_objs_lane_layout, then the kernel's workspace), then nlanes rows of
 * mp doubles for the objectives when the staging arena cannot take them.  Pinned part: nlanes times hstride doubles (result block,
 * sequence word, y, x, z). */
struct ObjsLanes
{
   int nlanes;
   long long off[HS_FAN_MAXSEG];
   long long iter_len, stride, ws_len, mp, qp, hstride;
   double* dev; double* Bdev; double* host; double* host_dev;
};
/* with_ws = false: the home lane alone and no workspace (a problem the one-launch path is not offered; any number of blocks) */
static int objs_lanes(hipsdp_solver* s, int nlanes, bool with_ws, std::vector<long long>& off, ObjsLanes* L)
{
   const int K = (int) s->blk.size();
   std::vector<int> ns((size_t) K + 1);
   for (int k = 0; k < K; ++k) ns[k] = s->blk[k].n;
   off.assign((size_t) 4 + 2 * K, 0);
   memset(L, 0, sizeof(*L));
   L->nlanes = nlanes;
   L->iter_len = hs_objs_lane_layout(s->m, s->q, K, ns.data(), 0, off.data());
   L->mp = (s->m + 1) & ~1LL; L->qp = (s->q + 1) & ~1LL;
   long long dev_need = L->iter_len, host_need = 0;
   if ( with_ws )
   {
      for (int i = 0; i < 4 + 2 * K; ++i) L->off[i] = off[i];
      L->ws_len = (hs_solve1_ws_doubles(s->m, s->q, K, ns.data()) + 1) & ~1LL;
      L->stride = L->iter_len + L->ws_len;
      L->hstride = HS_S1_OUT_DOUBLES + 8 + L->mp + 2 * L->qp;
      dev_need = (long long) (nlanes + 1) * L->stride + (long long) nlanes * L->mp;
      host_need = (long long) nlanes * L->hstride;
   }
   if ( s->ln_dev_len < dev_need )
   {
      if ( s->ln_dev != NULL )
      {
         HS_HIP( hipStreamSynchronize(s->stream) );
         (void) hipFree(s->ln_dev);
         s->ln_dev = NULL; s->ln_dev_len = 0;
      }
      HS_HIP( hipMalloc((void**) &s->ln_dev, (size_t) dev_need * sizeof(double)) );
      s->ln_dev_len = dev_need;
   }
   if ( s->ln_host_len < host_need )
   {
      if ( s->ln_host != NULL )
      {
         HS_HIP( hipStreamSynchronize(s->stream) );
         (void) hipHostFree(s->ln_host);
         s->ln_host = NULL; s->ln_host_dev = NULL; s->ln_host_len = 0;
      }
      HS_HIP( hipHostMalloc((void**) &s->ln_host, (size_t) host_need * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) );
      HS_HIP( hipHostGetDevicePointer((void**) &s->ln_host_dev, s->ln_host, 0) );
      s->ln_host_len = host_need;
   }
   L->dev = s->ln_dev; L->Bdev = s->ln_dev + (long long) (nlanes + 1) * L->stride;
   L->host = s->ln_host; L->host_dev = s->ln_host_dev;
   return HIPSDP_OK;
}
/* lane 1 + j of a chunk as the kernel's stages see it */
static void objs_lane(const hipsdp_solver* s, const ObjsLanes& L, int j, S1Lane* o)
{
   memset(o, 0, sizeof(*o));
   double* base = L.dev + (long long) (j + 1) * L.stride;
   const int K = (int) s->blk.size();
   o->b = base + L.off[0]; o->y = base + L.off[1]; o->x = base + L.off[2]; o->z = base + L.off[3];
   for (int k = 0; k < K; ++k)
   {
      o->X[k] = base + L.off[4 + 2 * k]; o->Z[k] = base + L.off[5 + 2 * k];
   }
   o->gws = base + L.iter_len; o->gws_len = L.ws_len;
   o->host = L.host + (long long) j * L.hstride; o->host_dev = L.host_dev + (long long) j * L.hstride;
   o->hist = false;
   o->hy = HS_S1_OUT_DOUBLES + 8; o->hx = o->hy + L.mp; o->hz = o->hx + L.qp;
   o->seq = const_cast<unsigned long long*>(&s->ln_seq);
}
/* the solver's objective and, when it has one, its start point to (save) or from the home lane at `home`, on the solver's queue */
static int objs_home_copy(hipsdp_solver* s, double* home, const std::vector<long long>& off, bool warm, bool save, bool obj)
{
   hipStream_t st = s->stream;
   auto cp = [&](double* own, long long o, long long len) -> int {
      if ( len > 0 )
         HS_HIP( hipMemcpyAsync(save ? home + o : own, save ? own : home + o, (size_t) len * sizeof(double), hipMemcpyDeviceToDevice, st) );
      return HIPSDP_OK;
   };
   if ( obj )
      HS_CALL( cp(s->b, off[0], s->m) );
   if ( warm )
   {
      HS_CALL( cp(s->y, off[1], s->m) );
      HS_CALL( cp(s->x, off[2], s->q) );
      HS_CALL( cp(s->z, off[3], s->q) );
      for (size_t k = 0; k < s->blk.size(); ++k)
      {
         const long long n2 = (long long) s->blk[k].n * s->blk[k].n;
         HS_CALL( cp(s->blk[k].X, off[4 + 2 * k], n2) );
         HS_CALL( cp(s->blk[k].Z, off[5 + 2 * k], n2) );
      }
   }
   s->stage_pending = true;
   return HIPSDP_OK;
}
/* one job on the general path, on the solver's own storage, as hipsdp_set_start, hipsdp_set_obj, hipsdp_solve, hipsdp_get_y run it */
static int objs_general_job(hipsdp_solver* s, const hipsdp_params* params, const double* bj, double* home, const std::vector<long long>& off,
   bool warm, hipsdp_info* info, double* yrow)
{
   HS_CALL( objs_home_copy(s, home, off, warm, false, false) );
   s->have_start = warm;
   if ( s->m > 0 )
      HS_CALL( stage_upload(s, s->b, bj, (size_t) s->m * sizeof(double)) );
   s->solved = false;
   int rc = solve_begin(s, params, info);
   if ( rc == HIPSDP_OK )
      rc = solve_run(s, info, false);
   rc = solve_end(s, rc);
   if ( rc == HIPSDP_OK && yrow != NULL )
      rc = hipsdp_get_y(s, yrow);
   return rc;
}

extern "C" int hipsdp_solve_objectives(hipsdp_solver* s, int count, const double* B, const hipsdp_params* params, hipsdp_info* infos,
   double* Y, int* rcs)
{
   g_err[0] = 0;
   if ( s == NULL || !s->shaped || count < 0 )
      return HIPSDP_ERR_ARG;
   if ( count == 0 )
      return HIPSDP_OK;
   if ( B == NULL || infos == NULL )
      return HIPSDP_ERR_ARG;
   if ( s->comm != NULL || s->shardA )
   {
      set_err("hipsdp_solve_objectives: the solver must have no communicator and no sharded matrices");
      return HIPSDP_ERR_ARG;
   }
   if ( params != NULL && params->preoptgap > 0.0 )
   {
      set_err("hipsdp_solve_objectives: preoptgap > 0 - the preoptimal iterate is kept per solver, not per job");
      return HIPSDP_ERR_ARG;
   }
   HS_HIP( hipSetDevice(s->device) );
   (void) __sync_add_and_fetch(&g_objs_calls, 1);
   const int m = s->m, K = (int) s->blk.size();
   const bool warm = s->have_start;
   hipStream_t st = s->stream;
   std::vector<int> rc((size_t) count, HIPSDP_OK);
   auto leave = [&](int rc_call) -> int {
      int rc_all = rc_call;
      for (int j = 0; j < count; ++j)
      {
         if ( rc_call != HIPSDP_OK ) rc[j] = rc_call;
         if ( rcs != NULL ) rcs[j] = rc[j];
         if ( rc_all == HIPSDP_OK ) rc_all = rc[j];
      }
      return rc_all;
   };

   /* 1. the node's waiting setters write the shared matrices: ONE launch for them, before any lane runs (the lanes run none) */
   int r = flush_zeros(s);
   if ( r == HIPSDP_OK ) r = flush_cmds(s);
   if ( r == HIPSDP_OK ) r = solve_begin(s, params, &infos[0]);
   if ( r != HIPSDP_OK )
      return leave(solve_end(s, r));
   for (int j = 0; j < count; ++j)
      solve_reset(s, &infos[j]);
   s->solved = false;
   s->s1_last = 0;
   s->s1_sol_host = false;
   int ns[HS_S1_MAXBLK], prof = 0;
   const bool offered = solve1_eligible(s, ns, &prof);
   std::vector<long long> off;
   ObjsLanes L;
   std::vector<int> later;                      /* jobs for the general path, in job order */

   if ( !offered )
   {
      /* not the one-launch path's problem: the call is the loop */
      r = objs_lanes(s, 0, false, off, &L);
      if ( r == HIPSDP_OK ) r = objs_home_copy(s, L.dev, off, warm, true, true);
      if ( r != HIPSDP_OK )
         return leave(solve_end(s, r));
      for (int j = 0; j < count; ++j)
         later.push_back(j);
   }
   else
   {
      /* 2. the lanes: as many as a chunk has jobs */
      int chunk = OBJS_CHUNK_MAX;
      {
         const long long per = (hs_objs_lane_layout(m, s->q, K, ns, 0, L.off) + hs_solve1_ws_doubles(m, s->q, K, ns) + 2) * (long long) sizeof(double);
         if ( (long long) chunk * per > OBJS_LANE_BYTES )
            chunk = (int) (OBJS_LANE_BYTES / per);
         const char* env = getenv("HIPSDP_OBJECTIVES_CHUNK");          /* (read at every call, like the switches of the one-launch path) */
         if ( env != NULL && atoi(env) > 0 )
            chunk = atoi(env);
         if ( chunk < 1 ) chunk = 1;
         if ( chunk > count ) chunk = count;
      }
      r = objs_lanes(s, chunk, true, off, &L);
      if ( r == HIPSDP_OK ) r = many_stage(s->device, (size_t) chunk, 0);
      if ( r != HIPSDP_OK )
         return leave(solve_end(s, r));
      ManyStage& g = g_many;
      std::vector<S1Prep> pp((size_t) chunk);
      std::vector<SeqWord> words((size_t) chunk);
      std::vector<char> pub((size_t) chunk, 0);
      int cls = 0;
      bool all_published = true;
      for (int c0 = 0; c0 < count; c0 += chunk)
      {
         const int n = count - c0 < chunk ? count - c0 : chunk;
         /* 3. the objectives of the chunk, rows of mp doubles: ONE upload through the staging arena (read there by the fan-out), or,
          * when it has no room, a copy into device memory behind the lanes */
         const size_t so = s->stage_off;
         const double* Bsrc = NULL;
         if ( m > 0 )
         {
            void* dv = NULL;
            double* h = static_cast<double*>(stage_take(s, (size_t) n * L.mp * sizeof(double), &dv));
            std::vector<double> tmp;
            if ( h == NULL )
            {
               tmp.assign((size_t) n * L.mp, 0.0);
               h = tmp.data();
            }
            for (int j = 0; j < n; ++j)
            {
               memcpy(h + (size_t) j * L.mp, B + (size_t) (c0 + j) * m, (size_t) m * sizeof(double));
               if ( L.mp > m ) h[(size_t) j * L.mp + m] = 0.0;
            }
            if ( dv != NULL )
               Bsrc = static_cast<const double*>(dv);
            else
            {
               r = hipStreamSynchronize(st) == hipSuccess
                  && hipMemcpy(L.Bdev, h, (size_t) n * L.mp * sizeof(double), hipMemcpyHostToDevice) == hipSuccess ? HIPSDP_OK : HIPSDP_ERR_HIP;
               Bsrc = L.Bdev;
            }
         }
         /* 4. the fan-out: every job's objective, and the start point when there is one, into its lane; the solver's own into lane 0 */
         hs_fan_plan plan;
         memset(&plan, 0, sizeof(plan));
         {
            auto seg = [&](const double* own, const double* src, long long stride, long long dst, long long len) {
               if ( len <= 0 ) return;
               hs_fan_seg& S = plan.seg[plan.nseg++];
               S.src0 = own; S.src = src; S.stride = stride; S.dst = dst; S.len = len;
            };
            seg(s->b, Bsrc, L.mp, L.off[0], m);
            if ( warm )
            {
               seg(s->y, s->y, 0, L.off[1], m);
               seg(s->x, s->x, 0, L.off[2], s->q);
               seg(s->z, s->z, 0, L.off[3], s->q);
               for (int k = 0; k < K; ++k)
               {
                  const long long n2 = (long long) ns[k] * ns[k];
                  seg(s->blk[k].X, s->blk[k].X, 0, L.off[4 + 2 * k], n2);
                  seg(s->blk[k].Z, s->blk[k].Z, 0, L.off[5 + 2 * k], n2);
               }
            }
         }
         if ( r == HIPSDP_OK && plan.nseg > 0 )
         {
            r = hs_objs_fanout(st, &plan, L.dev, L.stride, n + 1);
            if ( r == HIPSDP_OK )
               (void) __sync_add_and_fetch(&g_objs_launches, 1);
         }
         /* 5. the kernel's arguments, one record per lane, and ONE launch of n workgroups on the solver's queue */
         bool launched = false;
         if ( r == HIPSDP_OK )
         {
            for (int j = 0; j < n && r == HIPSDP_OK; ++j)
            {
               S1Lane lane;
               objs_lane(s, L, j, &lane);
               *reinterpret_cast<volatile unsigned long long*>(lane.host + HS_S1_OUT_DOUBLES) = 0ULL;
               bool off1 = false;
               r = solve1_prepare(s, &pp[j], &off1, &lane);
               if ( r == HIPSDP_OK && !off1 )
                  r = HIPSDP_ERR_ARG;
               if ( r == HIPSDP_OK )
                  memcpy(&g.h[j], &pp[j].a, sizeof(hs_solve1_args));
            }
            if ( r == HIPSDP_OK && c0 == 0 )
               cls = hs_solve1_class(&pp[0].a);
            __atomic_thread_fence(__ATOMIC_RELEASE);
            if ( r == HIPSDP_OK )
               r = many_hip_ok(hipMemcpyAsync(g.d, g.h, (size_t) n * sizeof(hs_solve1_args), hipMemcpyHostToDevice, st),
                     "hipMemcpyAsync(solve-objectives arguments)", __LINE__) ? HIPSDP_OK : HIPSDP_ERR_HIP;
            if ( r == HIPSDP_OK )
               r = hs_solve1_launch_many(st, cls, g.d, n) == HS_OK ? HIPSDP_OK : HIPSDP_ERR_HIP;
            if ( r == HIPSDP_OK )
            {
               launched = true;
               s->stage_pending = true;
               (void) __sync_add_and_fetch(&g_objs_launches, 1);
            }
         }
         if ( !launched )
         {
            /* nothing of this chunk runs: whatever was queued drains, the jobs from here on report the error */
            (void) hipStreamSynchronize(st);
            for (int j = c0; j < count; ++j) rc[j] = r != HIPSDP_OK ? r : HIPSDP_ERR_HIP;
            all_published = false;
            break;
         }
         /* 6. the sequence words of the chunk, polled together */
         for (int j = 0; j < n; ++j)
            words[j] = SeqWord{pp[j].host, pp[j].a.seq, 0};
         wait_published(words.data(), n, &st, 1, "hipStreamQuery(one-launch solve of many objectives)", pub.data());
         /* 7. every job's results out of its lane's pinned part: no copy from the device */
         bool chunk_ok = true;
         for (int j = 0; j < n; ++j)
         {
            const int J = c0 + j;
            if ( !pub[j] ) { rc[J] = HIPSDP_ERR_HIP; chunk_ok = false; continue; }
            S1Sol sol;
            bool done = false;
            rc[J] = solve1_result(s, &pp[j], &infos[J], &sol, &done);
            if ( rc[J] != HIPSDP_OK )
               continue;
            if ( !done )
            {
               later.push_back(J);
               continue;
            }
            (void) __sync_add_and_fetch(&g_objs_problems, 1);
            if ( Y != NULL )
            {
               const double* hy = pp[j].host + pp[j].hy;
               for (int i = 0; i < m; ++i)
                  Y[(size_t) J * m + i] = hy[i] * sol.sol_scale;
            }
         }
         if ( !chunk_ok )
         {
            (void) hipStreamSynchronize(st);
            for (int j = c0 + n; j < count; ++j) rc[j] = HIPSDP_ERR_HIP;
            all_published = false;
            break;
         }
         /* (the fan-out has read the objectives: the next chunk's take their place in the arena) */
         s->stage_off = so;
      }
      if ( all_published )
         s->stage_off = 0;                 /* (everything queued before the launches has run: the setters' data has been read) */
      if ( !all_published )
         later.clear();
   }

   /* 8. the jobs of the general path, one after another on the solver's own storage, each from the start the call was given; then the
    * solver's own objective back.  The start point is consumed and the solver holds no solution. */
   double* home = L.dev;
   for (int J : later)
      rc[J] = objs_general_job(s, params, B + (size_t) J * m, home, off, warm, &infos[J], Y != NULL ? Y + (size_t) J * m : NULL);
   r = HIPSDP_OK;
   if ( !later.empty() )
      r = objs_home_copy(s, home, off, false, false, true);
   s->have_start = false;
   s->solved = false;
   s->s1_last = 0;
   s->s1_sol_host = false;
   return leave(solve_end(s, r));
}

extern "C" int hipsdp_solve_objectives_stats(long long* calls, long long* launches, long long* problems)
{
   if ( calls != NULL )
      *calls = __sync_add_and_fetch(&g_objs_calls, 0);
   if ( launches != NULL )
      *launches = __sync_add_and_fetch(&g_objs_launches, 0);
   if ( problems != NULL )
      *problems = __sync_add_and_fetch(&g_objs_problems, 0);
   return HIPSDP_OK;
}

extern "C" int hipsdp_gram_cache_stats(hipsdp_solver* s, long long* hits, long long* misses)
{
   if ( s == NULL )
      return HIPSDP_ERR_ARG;
   if ( hits != NULL ) *hits = s->gc_hits;
   if ( misses != NULL ) *misses = s->gc_misses;
   return HIPSDP_OK;
}

extern "C" int hipsdp_solve_many_stats(long long* launches, long long* problems)
{
   if ( launches != NULL )
      *launches = __sync_add_and_fetch(&g_many_launches, 0);
   if ( problems != NULL )
      *problems = __sync_add_and_fetch(&g_many_problems, 0);
   return HIPSDP_OK;
}

extern "C" long long hipsdp_solve1_fallbacks(void)
{
   return __sync_add_and_fetch(&g_solve1_fallbacks, 0);
}

extern "C" long long hipsdp_solve1_fallbacks_warm(void)
{
   return __sync_add_and_fetch(&g_solve1_fallbacks_warm, 0);
}

extern "C" long long hipsdp_solve1_solves(void)
{
   return __sync_add_and_fetch(&g_solve1_solves, 0);
}

extern "C" int hipsdp_solve1_debug_counts(unsigned int* counts2)
{
   if ( counts2 == NULL )
      return 0;
   return hs_solve1_debug_counts(counts2);
}

extern "C" int hipsdp_solve_path(hipsdp_solver* s)
{
   return (s != NULL && s->solved) ? s->s1_last : 0;
}

extern "C" int hipsdp_solve1_trace(hipsdp_solver* s, double* out64, int maxrows, double* hist)
{
   if ( s == NULL || s->s1_host == NULL )
      return HIPSDP_ERR_ARG;
   if ( out64 != NULL )
      memcpy(out64, s->s1_host, HS_S1_OUT_DOUBLES * sizeof(double));
   if ( hist != NULL && maxrows > 0 )
      memcpy(hist, s->s1_host + HS_S1_OUT_DOUBLES + 8, (size_t) (maxrows < S1_HIST_MAX ? maxrows : S1_HIST_MAX) * 16 * sizeof(double));
   return HIPSDP_OK;
}

/* ---- readback ------------------------------------------------------------------------------------------------------ */

static int read_scaled(hipsdp_solver* s, const double* d, long long n, double scale, double* out)
{
   if ( n <= 0 ) return HIPSDP_OK;
   if ( s->s1_sol_host && s->s1_host != NULL && (d == s->y || d == s->x || d == s->z) )
   {
      /* the one-launch solve left y, x, z in pinned memory as well */
      const double* h = s->s1_host + S1_SOL_OFF + (d == s->y ? 0 : (d == s->x ? 128 : 128 + 4096));
      for (long long i = 0; i < n; ++i)
         out[i] = h[i] * scale;
      return HIPSDP_OK;
   }
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   HS_HIP( hipMemcpy(out, d, (size_t) n * sizeof(double), hipMemcpyDeviceToHost) );
   for (long long i = 0; i < n; ++i)
      out[i] *= scale;
   return HIPSDP_OK;
}

extern "C" int hipsdp_get_y(hipsdp_solver* s, double* y)
{
   if ( s == NULL || !s->solved ) return HIPSDP_ERR_ARG;
   return read_scaled(s, s->y, s->m, s->sol_scale, y);
}

extern "C" int hipsdp_get_X(hipsdp_solver* s, int block, double* X)
{
   if ( s == NULL || !s->solved || block < 0 || block >= (int) s->blk.size() ) return HIPSDP_ERR_ARG;
   return read_scaled(s, s->blk[block].X, (long long) s->blk[block].n * s->blk[block].n, s->sol_scale, X);
}

extern "C" int hipsdp_get_Z(hipsdp_solver* s, int block, double* Z)
{
   if ( s == NULL || !s->solved || block < 0 || block >= (int) s->blk.size() ) return HIPSDP_ERR_ARG;
   return read_scaled(s, s->blk[block].Z, (long long) s->blk[block].n * s->blk[block].n, s->sol_scale, Z);
}

extern "C" int hipsdp_get_lp(hipsdp_solver* s, double* x, double* z)
{
   if ( s == NULL || !s->solved ) return HIPSDP_ERR_ARG;
   if ( x != NULL ) HS_CALL( read_scaled(s, s->x, s->q, s->sol_scale, x) );
   if ( z != NULL ) HS_CALL( read_scaled(s, s->z, s->q, s->sol_scale, z) );
   return HIPSDP_OK;
}

extern "C" int hipsdp_get_preoptimal(hipsdp_solver* s, int* available, double* y, double* x)
{
   if ( s == NULL || !s->solved || available == NULL ) return HIPSDP_ERR_ARG;
   *available = s->pre_valid ? 1 : 0;
   if ( !s->pre_valid )
      return HIPSDP_OK;
   if ( y != NULL ) HS_CALL( read_scaled(s, s->pre_y, s->m, s->pre_scale, y) );
   if ( x != NULL ) HS_CALL( read_scaled(s, s->pre_x, s->q, s->pre_scale, x) );
   return HIPSDP_OK;
}

extern "C" int hipsdp_get_preoptimal_X(hipsdp_solver* s, int block, double* X)
{
   if ( s == NULL || !s->solved || !s->pre_valid || X == NULL || block < 0 || block >= (int) s->blk.size() ) return HIPSDP_ERR_ARG;
   return read_scaled(s, s->blk[block].Xpre, (long long) s->blk[block].n * s->blk[block].n, s->pre_scale, X);
}

/* A[i][i] += v */
__global__ void k_shift_diag(int n, double* __restrict__ A, double v)
{
   const int i = blockIdx.x * blockDim.x + threadIdx.x;
   if ( i < n )
      A[(long long) i * n + i] += v;
}

/* SPMD: rank 0's flag everywhere (no-op for one rank) */
extern "C" int hipsdp_sync_flag(hipsdp_solver* s, int* flag)
{
   if ( s == NULL || flag == NULL )
      return HIPSDP_ERR_ARG;
   if ( s->comm == NULL || s->nranks < 2 )
      return HIPSDP_OK;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   PoolBuf<int> d(s->stream);
   HS_CALL( d.alloc(1) );
   hs_comm_phase(2);
   HS_HIP( hipMemcpyAsync(d.p, flag, sizeof(int), hipMemcpyHostToDevice, s->stream) );
   HS_CALL( hs_bcast_ints(s->comm, d.p, 1, s->stream) );
   HS_HIP( hipMemcpyAsync(flag, d.p, sizeof(int), hipMemcpyDeviceToHost, s->stream) );
   HS_HIP( hipStreamSynchronize(s->stream) );
   return HS_OK;
}

/* a point y of the host for the passes over A: y in s->ys, (-1, y) in s->dyt, the packed triangles and the device form of the blocks
 * kept as nonzeros up to date */
static int point_to_device(hipsdp_solver* s, const double* y)
{
   if ( s->m > 0 )
      HS_HIP( hipMemcpyAsync(s->ys, y, (size_t) s->m * sizeof(double), hipMemcpyHostToDevice, s->stream) );
   HS_CALL( hs_make_ext(s->stream, s->m, -1.0, 1.0, s->ys, s->dyt) );
   HS_LAUNCH_CHECK();
   HS_CALL( ensure_packed(s) );
   return HS_OK;
}

/* The full decomposition of B.W (up to 128 rows: tridiagonal reduction, multisection, inverse iteration in one launch, eigi.hip; block
 * Jacobi above): its first nlam eigenvalues (ascending) to hlam, one read-back.  Vout (may be NULL): the caller's empty
 * buffer, which gets the eigenvectors as the rows of an n x n array. */
static int decompose_W(hipsdp_solver* s, Block& B, int nlam, double* hlam, PoolBuf<double>* Vout)
{
   const int n = B.n;
   hipStream_t st = s->stream;
   PoolBuf<double> lam(st), Vown(st), ws(st);
   PoolBuf<double>& V = Vout != NULL ? *Vout : Vown;
   HS_CALL( lam.alloc(n) ); HS_CALL( V.alloc((long long) n * n) );
   HS_CALL( ws.alloc(n <= 128 ? hs_syev_small_scratch(n) : hs_syev_ws(n)) );
   HS_CALL( n <= 128 ? hs_syev_small_dev(st, n, B.W, lam.p, V.p, ws.p) : hs_syev_jacobi(st, n, B.W, lam.p, V.p, NULL, ws.p) );
   HS_HIP( hipMemcpyAsync(hlam, lam.p, (size_t) nlam * sizeof(double), hipMemcpyDeviceToHost, st) );
   HS_HIP( hipStreamSynchronize(st) );
   return HS_OK;
}

static int check_y_impl(hipsdp_solver* s, const double* y, double tol, double* lmin, double* lpviol);

extern "C" int hipsdp_check_y(hipsdp_solver* s, const double* y, double* lmin, double* lpviol)
{
   return check_y_impl(s, y, 0.0, lmin, lpviol);
}

/* the same check against a known tolerance (what the backend's re-solve loop asks: is lambda_min >= -tol?): blocks above 64 rows
 * are decided by ONE Cholesky factorization of Z(y) + 0.999 tol I - success proves lambda_min > -0.999 tol and lmin reports that
 * bound; only a failure (y really is at or beyond the tolerance) pays for the exact eigenvalue.  At an optimum Z(y) is singular
 * to rounding, i.e. a margin of tol inside the cone: the factorization succeeds and the check costs a pass over A and a Cholesky
 * instead of 250 Lanczos launches. */
extern "C" int hipsdp_check_y_tol(hipsdp_solver* s, const double* y, double tol, double* lmin, double* lpviol)
{
   return check_y_impl(s, y, tol > 0.0 ? tol : 0.0, lmin, lpviol);
}

static int check_y_impl(hipsdp_solver* s, const double* y, double tol, double* lmin, double* lpviol)
{
   if ( s == NULL || !s->shaped ) return HIPSDP_ERR_ARG;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   CommOff off(s, replicate_small(s));
   const int m1 = s->m + 1, q = s->q;
   hipStream_t st = s->stream;
   HS_CALL( point_to_device(s, y) );
   int k = 0;
   for (auto& B : s->blk)
   {
      const long long n2 = (long long) B.n * B.n;
      HS_CALL( pass_AT(s, B, s->dyt, 0.0, NULL, B.W) );
      /* run Lanczos to (numerical) convergence: up to min(n, 250) steps (not needed where the tolerance certificate decides) */
      if ( !(tol > 0.0 && B.n > 64) )
         HS_CALL( hs_lanczos_lmin(st, B.n, B.W, 250, s->sc + SC_BLK(k, 1), s->lan_ws) );
      else
      {
         HS_CALL( hs_fill(st, s->sc + SC_BLK(k, 1), 1, 0.0) );
         HS_CALL( hs_fill(st, s->sc + SC_BLK(k, 2), 1, 0.0) );
      }
      ++k;
   }
   HS_CALL( hs_fill(st, s->sc + SC_RATX, 1, 0.0) );
   if ( q > 0 )
   {
      const double* v = s->dyt;
      HS_CALL( hs_gemv_n(st, q, m1, s->Dext, m1, 1, &v, s->tmpq, q, s->gemv_ws, s->gemv_ws_len) );
      /* violation = max(0, -min(D y - c)) : use absmax on the negative part via ratio trick: min over rows */
      HS_CALL( hs_fill(st, s->hl, q, -1.0) );
      HS_CALL( hs_ratio_min(st, q, s->tmpq, s->hl, s->sc + SC_RATX, 0, s->red_ws) );   /* min_r (D y - c)_r */
   }
   HostScalars h;
   HS_CALL( read_scalars(s, h, NULL) );
   for (size_t b = 0; b < s->blk.size(); ++b)
      lmin[b] = h.v[SC_BLK(b, 1)] - h.v[SC_BLK(b, 2)];
   /* The reference accepts a solution on an EXACT eigenvalue (sdpsolchecker.c:201-257).  A Ritz value is an upper bound of
    * lambda_min and "theta - resid" only says that SOME eigenvalue lies that close to theta; once the Krylov space cannot span
    * the matrix (n above the 250 steps) an unconverged smaller eigenvalue would go unnoticed - and at an optimum Z(y) has a
    * cluster at 0, the slow case.  So above 200 rows the Lanczos estimate is not returned.  Without a tolerance and up to
    * HS_SYEVX_MAXN rows the first eigenvalue is computed (tridiagonal path, values only).  Otherwise the bound is certified: a
    * Cholesky factorization of W - sigma I succeeds only if lambda_min > sigma (then sigma is returned, a rigorous lower bound) -
    * sigma = -0.999 tol against a tolerance, estimate - 1e-9 (1 + |theta|) without one, a margin that is absolute and so not
    * relative to the norm of Z(y); if it fails the eigenvalue is computed. */
   for (size_t b = 0; b < s->blk.size(); ++b)
   {
      Block& B = s->blk[b];
      const int n = B.n;
      const bool bytol = tol > 0.0 && n > 64;
      /* A run that stopped before n steps (a breakdown: the start vector lies in an invariant subspace, as with repeated
       * eigenvalues) has not seen the whole space: its Ritz value is an eigenvalue, but not necessarily the smallest one, and its
       * residual bound is 0.  Only the run of n steps (up to 16 rows: the exact kernel, which reports n) keeps its value. */
      const bool whole = (int) h.v[SC_BLK(b, 3)] == n;
      if ( n <= 200 && !bytol && whole )
         continue;
      const long long n2 = (long long) n * n;
      if ( !bytol && n <= HS_SYEVX_MAXN )
      {
         /* tridiagonalisation and Sturm multisection for the first eigenvalue alone (syevx.hip): accurate to rounding relative to
          * the norm of Z(y) at every scale, and cheaper than the factorization */
         PoolBuf<double> out(st), ws(st);
         double l0 = 0.0;
         HS_CALL( out.alloc(HS_SYEVX_OUT_VEC) ); HS_CALL( ws.alloc((long long) hs_syevx_ws(n)) );
         HS_CALL( hs_syevx_dev(st, n, B.W, HS_SYEVX_INDEX | HS_SYEVX_NOVEC, 1, 1, 0.0, 0, out.p, ws.p) );
         HS_HIP( hipMemcpyAsync(&l0, out.p + HS_SYEVX_OUT_LAM, sizeof(double), hipMemcpyDeviceToHost, st) );
         HS_HIP( hipStreamSynchronize(st) );
         lmin[b] = l0;
         continue;
      }
      const double theta = h.v[SC_BLK(b, 1)];
      const double sigma = bytol ? -0.999 * tol : lmin[b] - 1e-9 * (1.0 + fabs(theta));
      int fl = 0;
      HS_CALL( hs_copy(st, B.T1, B.W, n2) );
      hipLaunchKernelGGL(k_shift_diag, g1d(n), dim3(256), 0, st, n, B.T1, -sigma);
      HS_LAUNCH_CHECK();
      HS_HIP( hipMemsetAsync(s->flags + 5, 0, sizeof(int), st) );
      HS_CALL( hs_potrf(st, n, B.T1, B.dinvx, s->flags + 5, NULL) );
      HS_HIP( hipMemcpyAsync(&fl, s->flags + 5, sizeof(int), hipMemcpyDeviceToHost, st) );
      HS_HIP( hipStreamSynchronize(st) );
      if ( fl == 0 && std::isfinite(sigma) )
      {
         lmin[b] = sigma;
         continue;
      }
      double l0 = 0.0;
      HS_CALL( decompose_W(s, B, 1, &l0, NULL) );
      lmin[b] = l0;
   }
   if ( lpviol != NULL )
      *lpviol = q > 0 ? fmax(0.0, -h.v[SC_RATX]) : 0.0;
   return HIPSDP_OK;
}

/* H = v v^T for row `row` of V (ld n) */
__global__ void k_outer_row(int n, const double* __restrict__ V, int row, double* __restrict__ H)
{
   const double* v = V + (long long) row * n;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < (long long) n * n; e += (long long) gridDim.x * blockDim.x)
      H[e] = v[e / n] * v[e % n];
}

/* Eigenvector cuts of one block at the point y (LP-based mode of the reference: cons_sdp.c:896-1010 produceCutFromEigenvector,
 * :1612-1803 separateSol): every eigenvector v of Z(y) = sum_i A_i y_i - A_0 with eigenvalue <= -tol gives the valid inequality
 *    sum_i (v^T A_i v) y_i >= v^T A_0 v.
 * Z(y) (one pass over A), its eigen-decomposition (one launch up to 128 rows, block Jacobi above) and the coefficients <A_i, v v^T> (one pass over A per cut) are
 * formed on the device.  The most negative eigenvalues come first; at most maxcuts cuts.
 * eigvals[maxcuts], coefs[maxcuts x m], lhs[maxcuts], vecs[maxcuts x n] (may be NULL) are host arrays.
 * Arguments checked by the caller (maxcuts may be 0: only the decomposition); lam0 (may be NULL): the block's first eigenvalue */
static int eigencuts_one(hipsdp_solver* s, int block, const double* y, double tol, int maxcuts, int* ncuts, double* eigvals,
   double* coefs, double* lhs, double* vecs, double* lam0)
{
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   CommOff off(s, replicate_small(s));
   const int m = s->m, m1 = m + 1;
   Block& B = s->blk[block];
   const int n = B.n;
   const long long n2 = (long long) n * n;
   hipStream_t st = s->stream;
   HS_CALL( point_to_device(s, y) );
   HS_CALL( pass_AT(s, B, s->dyt, 0.0, NULL, B.W) );
   PoolBuf<double> V(st), out(st);
   std::vector<double> hlam(n), hout(m1);
   HS_CALL( out.alloc(m1) );
   HS_CALL( decompose_W(s, B, n, hlam.data(), &V) );
   int k = 0;
   while ( k < n && k < maxcuts && hlam[k] <= -tol )
      ++k;
   for (int c = 0; c < k; ++c)
   {
      hipLaunchKernelGGL(k_outer_row, g1d(n2), dim3(256), 0, st, n, V.p, c, B.W2);
      HS_LAUNCH_CHECK();
      HS_CALL( pass_A(s, B, B.W2, out.p) );
      HS_HIP( hipMemcpyAsync(hout.data(), out.p, (size_t) m1 * sizeof(double), hipMemcpyDeviceToHost, st) );
      HS_HIP( hipStreamSynchronize(st) );
      eigvals[c] = hlam[c];
      lhs[c] = hout[0];
      for (int i = 0; i < m; ++i)
         coefs[(size_t) c * m + i] = hout[1 + i];
      if ( vecs != NULL )
         HS_HIP( hipMemcpy(vecs + (size_t) c * n, V.p + (size_t) c * n, (size_t) n * sizeof(double), hipMemcpyDeviceToHost) );
   }
   *ncuts = k;
   if ( lam0 != NULL )
      *lam0 = hlam[0];
   return HIPSDP_OK;
}

extern "C" int hipsdp_eigencuts(hipsdp_solver* s, int block, const double* y, double tol, int maxcuts, int* ncuts, double* eigvals,
   double* coefs, double* lhs, double* vecs)
{
   if ( s == NULL || !s->shaped || block < 0 || block >= (int) s->blk.size() || y == NULL || maxcuts < 0 || ncuts == NULL )
      return HIPSDP_ERR_ARG;
   *ncuts = 0;
   if ( maxcuts == 0 )
      return HIPSDP_OK;
   if ( eigvals == NULL || coefs == NULL || lhs == NULL )
      return HIPSDP_ERR_ARG;
   return eigencuts_one(s, block, y, tol, maxcuts, ncuts, eigvals, coefs, lhs, vecs, NULL);
}

/* ---- what the cut calls of many blocks (csrc/cut_calls.hip) and hipsdp_onevar_bounds[_all] (csrc/onevar.hip) need of a solver: its shape, the
 * blocks their shared launches serve, the cut workspace with its job tables, the per-block path (declared in hs_kernels.h) ------------ */
int hs_solver_dims(const hipsdp_solver* s, int* m, int* nblocks)
{
   if ( s == NULL || !s->shaped )
      return 0;
   *m = s->m;
   *nblocks = (int) s->blk.size();
   return 1;
}

int hs_solver_block_n(const hipsdp_solver* s, int block)
{
   return s->blk[block].n;
}

int hs_solver_lp_rows(const hipsdp_solver* s, int* q, const double** Dext)
{
   if ( s->comm != NULL || s->shardA )
      return 0;
   *q = s->q;
   *Dext = s->Dext;
   return 1;
}

/* the whole matrices of the block are on this device */
static bool ec_has_matrices(const Block& B)
{
   return B.sparse ? (B.sp != NULL && B.A0 != NULL) : B.A != NULL;
}

/* a block whose round runs in the shared launches: the whole matrices are on this device and k_syev_mid holds the block */
static bool ec_batched(const hipsdp_solver* s, const Block& B)
{
   return s->comm == NULL && !s->shardA && B.n <= 128 && ec_has_matrices(B);
}

/* the batched blocks, in the order of the decomposition's classes */
static std::vector<int> ec_batched_ids(const hipsdp_solver* s)
{
   std::vector<int> ids;
   for (int cls = 0; cls < 3; ++cls)
      for (size_t b = 0; b < s->blk.size(); ++b)
         if ( ec_batched(s, s->blk[b]) && hs_syev_many_class(s->blk[b].n) == cls )
            ids.push_back((int) b);
   return ids;
}

int hs_solver_cut_enter(hipsdp_solver* s, int only, std::vector<int>* ids)
{
   ids->clear();
   if ( only >= 0 && (s->comm != NULL || s->shardA) )
      return HS_OK;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   HS_CALL( ensure_packed(s) );          /* (also builds the device form of blocks kept as nonzeros) */
   if ( only < 0 )
      *ids = ec_batched_ids(s);
   else if ( ec_batched(s, s->blk[only]) )
      ids->assign(1, only);
   return HS_OK;
}

/* the sibling of hs_solver_cut_enter for the calls whose launches hold blocks of up to maxn rows (hipsdp_onevar_bounds_large: 512): ids
 * are ALL blocks with whole matrices on this device and at most maxn rows, in index order; hs_solver_cut_blocks then hands out the
 * table of any subset of them.  A solver with a communicator or sharded matrices: none, and it is not touched. */
int hs_solver_cut_enter_large(hipsdp_solver* s, int maxn, std::vector<int>* ids)
{
   ids->clear();
   if ( s->comm != NULL || s->shardA )
      return HS_OK;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   HS_CALL( ensure_packed(s) );
   for (size_t b = 0; b < s->blk.size(); ++b)
      if ( s->blk[b].n <= maxn && ec_has_matrices(s->blk[b]) )
         ids->push_back((int) b);
   return HS_OK;
}

/* the storage form the kernels read the block's matrices in (J zeroed by the caller) */
static void ec_job_form(const Block& B, hs_ec_job* J)
{
   J->n = B.n;
   J->ld = (long long) B.n * B.n;
   if ( B.sparse )
   {
      J->form = HS_EC_SPARSE; J->A = B.A0;
      hs_sp_get_view(B.sp, &J->sp);
   }
   else if ( B.Apk != NULL && B.apk_valid )
   {
      J->form = HS_EC_PACKED; J->A = B.Apk; J->ld = B.Lp;
   }
   else
   {
      J->form = HS_EC_DENSE; J->A = B.A;
   }
}

/* The workspace (lengths of the call's layout, its slabs from offset `slabs` on) and the job tables of a round over the batched blocks
 * `ids` (ordered by decomposition class); nmax_out: their largest n */
int hs_solver_cut_prepare(hipsdp_solver* s, const std::vector<int>& ids, const std::vector<long long>& vecoff, long long slabs,
   const hs_cut_lens& len, int* nmax_out, hs_solver_cut_ws* w)
{
   const int nj = (int) ids.size();
   HS_CALL( s->cw.grow(len.dev_len, len.pin_len, (size_t) nj * (sizeof(hs_ec_job) + sizeof(hs_eig_job))) );
   double* cur = s->cw.dev + slabs;
   std::vector<hs_ec_job> jobs((size_t) nj);
   std::vector<hs_eig_job> ejobs((size_t) nj);
   int nmax = 0;
   for (int j = 0; j < nj; ++j)
   {
      const Block& B = s->blk[ids[j]];
      hs_ec_job& J = jobs[j];
      memset(&J, 0, sizeof(J));
      memset(&ejobs[j], 0, sizeof(hs_eig_job));
      ec_job_form(B, &J);
      J.blk = ids[j];
      J.Z = cur; cur += hs_cut_mat_len(B.n);
      J.ws = cur; cur += hs_syev_small_scratch(B.n);
      J.vpos = hs_syev_many_vecpos(B.n);
      J.vecoff = vecoff[ids[j]];
      ejobs[j].n = B.n; ejobs[j].in = J.Z; ejobs[j].ws = J.ws;
      nmax = B.n > nmax ? B.n : nmax;
   }
   HS_CALL( s->cw.upload(jobs, ejobs) );
   *nmax_out = nmax;
   s->cw.view(s->stream, w);
   return HS_OK;
}

int hs_solver_cut_rounds(hipsdp_solver* s, const std::vector<hs_scr_job>& xjobs, const std::vector<hs_eig_job>& sjobs, hs_solver_cut_ws* w)
{
   HS_CALL( s->cw.upload_rounds(xjobs, sjobs) );
   w->dxjobs = s->cw.dxjobs(); w->dsjobs = s->cw.dsjobs(); w->sjobs = s->cw.sjobs.data();
   return HS_OK;
}

int hs_solver_cut_job(hipsdp_solver* s, int block, long long dev_len, long long pin_len, long long zoff, long long wsoff, hs_solver_cut_ws* w,
   int* served)
{
   *served = 0;
   if ( s->comm != NULL || s->shardA )
      return HS_OK;
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( stage_sync(s) );
   HS_CALL( ensure_packed(s) );          /* (also builds the device form of blocks kept as nonzeros) */
   const Block& B = s->blk[block];
   if ( !ec_has_matrices(B) )
      return HS_OK;
   CutWs& cw = s->cw;
   HS_CALL( cw.grow(dev_len, pin_len, sizeof(hs_ec_job)) );
   std::vector<hs_ec_job> job(1);
   memset(&job[0], 0, sizeof(hs_ec_job));
   ec_job_form(B, &job[0]);
   job[0].Z = cw.dev + zoff;
   if ( wsoff >= 0 )
      job[0].ws = cw.dev + wsoff;
   HS_CALL( cw.upload(job, std::vector<hs_eig_job>()) );
   cw.view(s->stream, w);
   *served = 1;
   return HS_OK;
}

int hs_solver_cut_blocks(hipsdp_solver* s, const std::vector<int>& ids, const std::vector<long long>& zoff, long long dev_len,
   long long pin_len, hs_solver_cut_ws* w)
{
   const int nj = (int) ids.size();
   CutWs& cw = s->cw;
   HS_CALL( cw.grow(dev_len, pin_len, (size_t) nj * sizeof(hs_ec_job)) );
   std::vector<hs_ec_job> jobs((size_t) nj);
   for (int j = 0; j < nj; ++j)
   {
      memset(&jobs[j], 0, sizeof(hs_ec_job));
      ec_job_form(s->blk[ids[j]], &jobs[j]);
      jobs[j].blk = ids[j];
      jobs[j].Z = cw.dev + zoff[j];
   }
   HS_CALL( cw.upload(jobs, std::vector<hs_eig_job>()) );
   cw.view(s->stream, w);
   return HS_OK;
}

int hs_solver_block_form(const hipsdp_solver* s, int block)
{
   hs_ec_job J;
   memset(&J, 0, sizeof(J));
   ec_job_form(s->blk[block], &J);
   return J.form;
}

int hs_solver_cut_plain(hipsdp_solver* s, long long dev_len, long long pin_len, hs_solver_cut_ws* w)
{
   HS_HIP( hipSetDevice(s->device) );
   HS_CALL( s->cw.grow(dev_len, pin_len, 0) );
   s->cw.view(s->stream, w);
   return HS_OK;
}

int hs_solver_round_frame(hipsdp_solver* s, long long need, hs_round_frame** frame)
{
   hs_round_frame& F = s->rframe;
   if ( need > F.len )
   {
      if ( F.dev != NULL ) HS_HIP( hipFree(F.dev) );
      F.dev = NULL; F.len = 0;
      HS_HIP( hipMalloc((void**) &F.dev, (size_t) need * sizeof(double)) );
      F.len = need;
   }
   *frame = &F;
   return HS_OK;
}

int hs_solver_eigencuts_block(hipsdp_solver* s, int block, const double* y, double tol, int maxcuts, int* ncuts, double* eigvals,
   double* coefs, double* lhs, double* vecs, double* lam0)
{
   return eigencuts_one(s, block, y, tol, maxcuts, ncuts, eigvals, coefs, lhs, vecs, lam0);
}

/* host-only: the column ranges of the sharded W formulation, bounds[0 .. nranks] (rank g owns [bounds[g], bounds[g + 1])) */
extern "C" int hipsdp_shard_columns(int m1, int n, int nranks, int* bounds)
{
   if ( m1 < 1 || n < 1 || nranks < 1 || nranks > 64 || bounds == NULL )
      return HIPSDP_ERR_ARG;
   for (int g = 0; g < nranks; ++g)
   {
      int c0, cw;
      hs_shard_cols(m1, n, nranks, g, &c0, &cw);
      bounds[g] = c0;
      bounds[g + 1] = c0 + cw;
   }
   return HIPSDP_OK;
}

/* mode 1: the constraint matrices of the NEXT hipsdp_set_shape are sharded by variable over the ranks of the communicator
 * (rank g holds rows [g c, (g + 1) c) of A, c = ceil((m + 1) / ranks); the constant matrix is kept everywhere); -1: only when
 * the replicated matrices would not fit; 0 (default): replicated.  Call after hipsdp_set_comm and before hipsdp_set_shape. */
extern "C" int hipsdp_shard_matrices(hipsdp_solver* s, int mode)
{
   if ( s == NULL || mode < -1 || mode > 1 )
      return HIPSDP_ERR_ARG;
   s->shardA_req = mode;
   return HIPSDP_OK;
}

/* 1 when the matrices of the current shape are sharded by variable, 0 when replicated */
extern "C" int hipsdp_matrices_sharded(hipsdp_solver* s)
{
   return s != NULL && s->shaped && s->shardA ? 1 : 0;
}

extern "C" int hipsdp_set_comm(hipsdp_solver* s, void* comm, int rank, int nranks)
{
   if ( s == NULL || nranks < 1 || nranks > 16 || rank < 0 || rank >= nranks || (nranks > 1 && comm == NULL) )
      return HIPSDP_ERR_ARG;
   s->comm = comm; s->rank = rank; s->nranks = nranks;
   /* the Schur workspace depends on the mode: drop it so that the next solve re-creates it */
   if ( s->sws.T != NULL )
   {
      HS_HIP( hipSetDevice(s->device) );
      HS_CALL( stage_sync(s) );
      HS_HIP( hipStreamSynchronize(s->stream) );
      hs_schur_ws_free(&s->sws);
   }
   return HIPSDP_OK;
}
