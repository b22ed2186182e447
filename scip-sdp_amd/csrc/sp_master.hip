/* sp_master.hip - master copy of a block KEPT AS TRIPLETS, and the gather of a node's block from it.
 *
 * A block kept as nonzeros (csrc/sparse.hip) used to be re-marshalled and rebuilt on the host at every node: three stable sorts, a
 * sort per variable, 17 blocking copies (hs_sp_build).  The solver interface guarantees that the caller's arrays do not change
 * between the nodes of a tree, so the sorting is done ONCE here, in ORIGINAL indices (hs_sp_master.cpp), and a node - a subset of the
 * slots as variables a + 1, a subset `kept` of the rows renumbered in increasing order - is a FILTER of the sorted lists: kept is
 * increasing, so (row, col) order and row-major order survive the renumbering, and the segments of the by-variable lists are the
 * filtered segments of the slots act[a] in the order of a.  Inside a position the entries are ordered by the new variable; the
 * master keeps them by slot, which is the same order whenever the slots of the active variables increase with the variable (the
 * host checks that in O(nactive)); otherwise one more launch orders each position's short segment.
 *
 * Launches of a gather into a block kept as nonzeros (7, whatever nnz, m and n are, + 1 when the orders disagree):
 *
 *   k_spm_count_var   one wavefront per variable: kept lower entries, kept mirrored entries, non-empty rows (ballot + popcount)
 *   k_spm_count_pos   one thread per master position: kept entries, and whether there is one
 *   k_spm_scan_local  exclusive scan of the five count arrays inside blocks of 1024, block sums
 *   k_spm_scan_top    scan of the block sums (one workgroup per array), the five totals
 *   k_spm_scan_add    block offsets added
 *   k_spm_write_var   the same walk as the count: voff-relative writes of vrow/vcol/vval, frow/fcol/fval, srow/sent
 *   k_spm_write_pos   poff/prow/pcol of the surviving positions, pvar/pval of their surviving entries
 *   (k_spm_order_pos  insertion sort of each position's segment by variable)
 *
 * Hazard rule: inside a launch no workgroup reads what another one writes - counts are written by the wavefront / thread that owns
 * the variable / position, every scan stage reads only what the stage before wrote, the writers read the finished offsets and
 * write disjoint ranges.  The kernel boundary is the only synchronisation; there are no atomics at all, no grid barrier, no flag.
 * One read-back per gather: the totals nnz, nfull, nslots, npos (launch sizes of the consumers live on the host).
 *
 * The results live in a grow-only workspace of the master block sized by the master's own counts (upper bounds of any node's):
 * nothing is allocated per node.  hs_sparse::borrowed keeps hs_sp_free from releasing it. */
#include "hs_kernels.h"
#include "hs_sp_master.h"
#include <vector>
#include <string.h>

#define SPM_SCAN_BLOCK 1024        /* elements per workgroup of the scan: 256 threads x 4 */
#define SPM_JOBS 5                 /* voff, foff, soff (over the variables), positions, position entries (over the master positions) */

struct hs_spm
{
   int N, S;
   std::vector<int> hslot, hrow, hcol;
   std::vector<double> hval;
   bool dirty;                      /* entries were added since the device copy was made */
   bool uploaded;
   long long L, P, F, R;
   /* device master */
   int *loff, *lrow, *lcol; double* lval;
   int *poff, *prow, *pcol, *pslot; double* pval;
   int *foff, *frow, *fcol; double* fval;
   /* workspace: index maps, counts, scans */
   int mcap;
   int* idx;                        /* act[mcap] inv[N] svar[S] */
   int* idx_h;                      /* pinned: 8 ints of totals, then the same three lists */
   int *vcnt, *pcnt, *pscan, *bsum, *tot;
   /* workspace: the node's structure */
   int *o_voff, *o_vrow, *o_vcol; double* o_vval;
   int *o_poff, *o_prow, *o_pcol, *o_pvar; double* o_pval;
   int *o_foff, *o_frow, *o_fcol; double* o_fval;
   int *o_soff, *o_srow, *o_sent; double* o_Tc;
};

struct spm_scan_jobs { const int* in[SPM_JOBS]; int* out[SPM_JOBS]; int n[SPM_JOBS]; int bs0[SPM_JOBS]; };

namespace {

template<typename T> int spm_alloc(T** p, long long count)
{
   *p = NULL;
   return hs_pool_alloc((void**) p, (size_t) (count > 0 ? count : 1) * sizeof(T));
}

template<typename T> int spm_upload(T** d, const std::vector<T>& h)
{
   HS_CALL( spm_alloc(d, (long long) h.size()) );
   if ( !h.empty() )
      HS_HIP( hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) );
   return HS_OK;
}

void spm_release_device(hs_spm* M)
{
   void* ptrs[] = {M->loff, M->lrow, M->lcol, M->lval, M->poff, M->prow, M->pcol, M->pslot, M->pval, M->foff, M->frow, M->fcol, M->fval,
      M->idx, M->vcnt, M->pcnt, M->pscan, M->bsum, M->tot, M->o_voff, M->o_vrow, M->o_vcol, M->o_vval, M->o_poff, M->o_prow, M->o_pcol,
      M->o_pvar, M->o_pval, M->o_foff, M->o_frow, M->o_fcol, M->o_fval, M->o_soff, M->o_srow, M->o_sent, M->o_Tc};
   for (void* p : ptrs)
      hs_pool_free(p);
   if ( M->idx_h != NULL )
      (void) hipHostFree(M->idx_h);
   M->loff = M->lrow = M->lcol = M->poff = M->prow = M->pcol = M->pslot = M->foff = M->frow = M->fcol = NULL;
   M->lval = M->pval = M->fval = NULL;
   M->idx = M->idx_h = M->vcnt = M->pcnt = M->pscan = M->bsum = M->tot = NULL;
   M->o_voff = M->o_vrow = M->o_vcol = M->o_poff = M->o_prow = M->o_pcol = M->o_pvar = M->o_foff = M->o_frow = M->o_fcol = NULL;
   M->o_soff = M->o_srow = M->o_sent = NULL;
   M->o_vval = M->o_pval = M->o_fval = M->o_Tc = NULL;
   M->mcap = 0;
   M->uploaded = false;
}

int spm_blocks(long long n) { return (int) ((n + SPM_SCAN_BLOCK - 1) / SPM_SCAN_BLOCK); }

}

int hs_spm_create(hs_spm** out, int N, int S)
{
   *out = NULL;
   if ( N < 1 || S < 0 )
      return HS_ERR_ARG;
   hs_spm* M = new hs_spm();
   M->N = N; M->S = S;
   M->dirty = true; M->uploaded = false;
   M->L = M->P = M->F = M->R = 0;
   M->idx_h = NULL;
   spm_release_device(M);           /* (every pointer NULL) */
   *out = M;
   return HS_OK;
}

void hs_spm_free(hs_spm* M)
{
   if ( M == NULL )
      return;
   spm_release_device(M);
   delete M;
}

int hs_spm_size(const hs_spm* M) { return M->N; }
int hs_spm_slots(const hs_spm* M) { return M->S; }

int hs_spm_add(hs_spm* M, long long nnz, const int* slot, int oneslot, const int* row, const int* col, const double* val)
{
   if ( nnz <= 0 )
      return nnz == 0 ? HS_OK : HS_ERR_ARG;
   if ( val == NULL || hs_spm_check(M->N, M->S, nnz, slot, oneslot, row, col) != HIPSDP_OK )
      return HS_ERR_ARG;
   if ( slot != NULL )
      M->hslot.insert(M->hslot.end(), slot, slot + nnz);
   else
      M->hslot.insert(M->hslot.end(), (size_t) nnz, oneslot);
   M->hrow.insert(M->hrow.end(), row, row + nnz);
   M->hcol.insert(M->hcol.end(), col, col + nnz);
   M->hval.insert(M->hval.end(), val, val + nnz);
   M->dirty = true;
   return HS_OK;
}

/* the m-sized arrays for at least m variables (grow-only; B&B shapes differ by a few variables: some room) */
static int spm_ensure_m(hs_spm* M, int m)
{
   if ( M->mcap >= m && M->idx != NULL )
      return HS_OK;
   const int cap = m + 32;
   void* old[] = {M->idx, M->vcnt, M->bsum, M->o_voff, M->o_foff, M->o_soff};
   for (void* p : old)
      hs_pool_free(p);
   if ( M->idx_h != NULL )
      (void) hipHostFree(M->idx_h);
   M->idx = M->idx_h = M->vcnt = M->bsum = M->o_voff = M->o_foff = M->o_soff = NULL;
   M->mcap = 0;
   const long long nidx = (long long) cap + M->N + M->S;
   HS_CALL( spm_alloc(&M->idx, nidx) );
   HS_HIP( hipHostMalloc((void**) &M->idx_h, (size_t) (8 + nidx) * sizeof(int), hipHostMallocDefault) );
   HS_CALL( spm_alloc(&M->vcnt, 3LL * cap) );
   HS_CALL( spm_alloc(&M->bsum, 3LL * spm_blocks(cap) + 2LL * spm_blocks(M->P) + SPM_JOBS) );
   HS_CALL( spm_alloc(&M->o_voff, (long long) cap + 1) );
   HS_CALL( spm_alloc(&M->o_foff, (long long) cap + 1) );
   HS_CALL( spm_alloc(&M->o_soff, (long long) cap + 1) );
   M->mcap = cap;
   return HS_OK;
}

/* the entries collected since the last upload become the device copy (once per master block, not per node) */
static int spm_ensure_final(hipStream_t s, hs_spm* M)
{
   if ( M->uploaded && !M->dirty )
      return HS_OK;
   HS_HIP( hipStreamSynchronize(s) );           /* nothing may still be running on what goes back to the pool */
   spm_release_device(M);
   hs_spm_final f;
   if ( hs_spm_finalize(M->N, M->S, (long long) M->hrow.size(), M->hslot.data(), M->hrow.data(), M->hcol.data(), M->hval.data(), &f) != HIPSDP_OK )
      return HS_ERR_ARG;
   M->L = f.L; M->P = f.P; M->F = f.F; M->R = f.R;
   HS_CALL( spm_upload(&M->loff, f.loff) ); HS_CALL( spm_upload(&M->lrow, f.lrow) ); HS_CALL( spm_upload(&M->lcol, f.lcol) );
   HS_CALL( spm_upload(&M->lval, f.lval) );
   HS_CALL( spm_upload(&M->poff, f.poff) ); HS_CALL( spm_upload(&M->prow, f.prow) ); HS_CALL( spm_upload(&M->pcol, f.pcol) );
   HS_CALL( spm_upload(&M->pslot, f.pslot) ); HS_CALL( spm_upload(&M->pval, f.pval) );
   HS_CALL( spm_upload(&M->foff, f.foff) ); HS_CALL( spm_upload(&M->frow, f.frow) ); HS_CALL( spm_upload(&M->fcol, f.fcol) );
   HS_CALL( spm_upload(&M->fval, f.fval) );
   /* the workspace, by the master's counts: no node has more of anything */
   HS_CALL( spm_alloc(&M->pcnt, 2 * M->P) );
   HS_CALL( spm_alloc(&M->pscan, 2 * (M->P + 1)) );
   HS_CALL( spm_alloc(&M->tot, 8) );
   HS_CALL( spm_alloc(&M->o_vrow, M->L) ); HS_CALL( spm_alloc(&M->o_vcol, M->L) ); HS_CALL( spm_alloc(&M->o_vval, M->L) );
   HS_CALL( spm_alloc(&M->o_poff, M->P + 1) ); HS_CALL( spm_alloc(&M->o_prow, M->P) ); HS_CALL( spm_alloc(&M->o_pcol, M->P) );
   HS_CALL( spm_alloc(&M->o_pvar, M->L) ); HS_CALL( spm_alloc(&M->o_pval, M->L) );
   HS_CALL( spm_alloc(&M->o_frow, M->F) ); HS_CALL( spm_alloc(&M->o_fcol, M->F) ); HS_CALL( spm_alloc(&M->o_fval, M->F) );
   HS_CALL( spm_alloc(&M->o_srow, M->R) ); HS_CALL( spm_alloc(&M->o_sent, M->R + 1) );
   HS_CALL( spm_alloc(&M->o_Tc, M->R * (long long) M->N) );
   M->uploaded = true;
   M->dirty = false;
   return HS_OK;
}

/* ---- kernels -------------------------------------------------------------------------------------------------------------- */

/* lanes of `mask` below this one */
__device__ __forceinline__ int spm_below(unsigned long long mask, int lane)
{
   return __popcll(mask & ((1ull << lane) - 1ull));
}

/* One wavefront per variable a: walks the lower and the mirrored segment of its slot in chunks of 64 and either counts what the node
 * keeps (WRITE = false: cnt[a], cnt[m + a], cnt[2 m + a]) or writes it behind the finished offsets.  A kept mirrored entry opens a
 * row slot when the kept entry before it (in this chunk: the nearest kept lane below; else the last one of the chunks before) has
 * another row. */
template<bool WRITE>
__global__ void __launch_bounds__(256) k_spm_var(int m, int nactive, const int* __restrict__ act, const int* __restrict__ inv,
   const int* __restrict__ loff, const int* __restrict__ lrow, const int* __restrict__ lcol, const double* __restrict__ lval,
   const int* __restrict__ foff, const int* __restrict__ frow, const int* __restrict__ fcol, const double* __restrict__ fval,
   int* __restrict__ cnt, const int* __restrict__ voff, int* __restrict__ vrow, int* __restrict__ vcol, double* __restrict__ vval,
   const int* __restrict__ ofoff, int* __restrict__ ofrow, int* __restrict__ ofcol, double* __restrict__ ofval,
   const int* __restrict__ osoff, int* __restrict__ osrow, int* __restrict__ osent)
{
   const int lane = threadIdx.x & 63;
   if ( WRITE && blockIdx.x == 0 && threadIdx.x == 0 )
      osent[osoff[m]] = ofoff[m];                       /* the closing offset of the row slots */
   for (int a = blockIdx.x * 4 + (threadIdx.x >> 6); a < m; a += gridDim.x * 4)
   {
      const int slot = a < nactive ? act[a] : -1;
      int cl = 0, cf = 0, cs = 0;
      if ( slot >= 0 )
      {
         const int l0 = loff[slot], l1 = loff[slot + 1];
         for (int base = l0; base < l1; base += 64)
         {
            const int e = base + lane;
            int r = -1, c = -1;
            if ( e < l1 )
            {
               r = inv[lrow[e]]; c = inv[lcol[e]];
            }
            const bool keep = r >= 0 && c >= 0;
            const unsigned long long mask = __ballot(keep);
            if ( WRITE && keep )
            {
               const int o = voff[a] + cl + spm_below(mask, lane);
               vrow[o] = r; vcol[o] = c; vval[o] = lval[e];
            }
            cl += __popcll(mask);
         }
         const int f0 = foff[slot], f1 = foff[slot + 1];
         int lastrow = -1;
         for (int base = f0; base < f1; base += 64)
         {
            const int e = base + lane;
            int r = -1, c = -1;
            if ( e < f1 )
            {
               r = inv[frow[e]]; c = inv[fcol[e]];
            }
            const bool keep = r >= 0 && c >= 0;
            const unsigned long long mask = __ballot(keep);
            const unsigned long long below = mask & ((1ull << lane) - 1ull);
            const int pl = below != 0ull ? 63 - __clzll((long long) below) : 0;
            const int pr = __shfl(r, pl, 64);
            const int prevrow = below != 0ull ? pr : lastrow;
            const bool first = keep && r != prevrow;
            const unsigned long long fmask = __ballot(first);
            if ( WRITE && keep )
            {
               const int o = ofoff[a] + cf + __popcll(below);
               ofrow[o] = r; ofcol[o] = c; ofval[o] = fval[e];
               if ( first )
               {
                  const int so = osoff[a] + cs + spm_below(fmask, lane);
                  osrow[so] = r; osent[so] = o;
               }
            }
            cf += __popcll(mask);
            cs += __popcll(fmask);
            const int hl = mask != 0ull ? 63 - __clzll((long long) mask) : 0;
            const int hr = __shfl(r, hl, 64);
            if ( mask != 0ull )
               lastrow = hr;
         }
      }
      if ( !WRITE && lane == 0 )
      {
         cnt[a] = cl; cnt[m + a] = cf; cnt[2 * m + a] = cs;
      }
   }
}

/* per master position: cnt[P + p] = entries whose slot is an active variable (0 when a row of the position is removed), cnt[p] =
 * whether there is one */
__global__ void __launch_bounds__(256) k_spm_count_pos(int P, const int* __restrict__ inv, const int* __restrict__ svar,
   const int* __restrict__ poff, const int* __restrict__ prow, const int* __restrict__ pcol, const int* __restrict__ pslot, int* __restrict__ cnt)
{
   for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x)
   {
      int c = 0;
      if ( inv[prow[p]] >= 0 && inv[pcol[p]] >= 0 )
         for (int e = poff[p]; e < poff[p + 1]; ++e)
            c += svar[pslot[e]] > 0 ? 1 : 0;
      cnt[p] = c > 0 ? 1 : 0;
      cnt[P + p] = c;
   }
}

/* scan[p], scan[P + 1 + p]: exclusive scans of the two counts (the entry behind the last one holds the total) */
__global__ void __launch_bounds__(256) k_spm_write_pos(int P, const int* __restrict__ inv, const int* __restrict__ svar,
   const int* __restrict__ poff, const int* __restrict__ prow, const int* __restrict__ pcol, const int* __restrict__ pslot,
   const double* __restrict__ pval, const int* __restrict__ scan, int* __restrict__ opoff, int* __restrict__ oprow, int* __restrict__ opcol,
   int* __restrict__ opvar, double* __restrict__ opval)
{
   const int* sp = scan;
   const int* se = scan + P + 1;
   if ( blockIdx.x == 0 && threadIdx.x == 0 )
      opoff[sp[P]] = se[P];
   for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += gridDim.x * blockDim.x)
   {
      if ( se[p + 1] == se[p] )
         continue;
      const int k = sp[p];
      int w = se[p];
      opoff[k] = w; oprow[k] = inv[prow[p]]; opcol[k] = inv[pcol[p]];
      for (int e = poff[p]; e < poff[p + 1]; ++e)
      {
         const int v = svar[pslot[e]];
         if ( v > 0 )
         {
            opvar[w] = v; opval[w] = pval[e];
            ++w;
         }
      }
   }
}

/* the slots of the active variables do not increase with the variable: every position's segment into the order of the variable */
__global__ void __launch_bounds__(256) k_spm_order_pos(int npos, const int* __restrict__ opoff, int* __restrict__ opvar, double* __restrict__ opval)
{
   for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < npos; k += gridDim.x * blockDim.x)
   {
      const int e0 = opoff[k], e1 = opoff[k + 1];
      for (int i = e0 + 1; i < e1; ++i)
      {
         const int v = opvar[i];
         const double x = opval[i];
         int j = i - 1;
         while ( j >= e0 && opvar[j] > v )
         {
            opvar[j + 1] = opvar[j]; opval[j + 1] = opval[j];
            --j;
         }
         opvar[j + 1] = v; opval[j + 1] = x;
      }
   }
}

/* stage 1: blockIdx.y = array; out[i] = exclusive scan inside the block of 1024, bsum[bs0 + block] = the block's sum */
__global__ void __launch_bounds__(256) k_spm_scan_local(spm_scan_jobs J, int* __restrict__ bsum)
{
   __shared__ int ws[4];
   const int j = blockIdx.y;
   const int n = J.n[j];
   const int* in = J.in[j];
   int* out = J.out[j];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   for (int blk = blockIdx.x; blk * SPM_SCAN_BLOCK < n; blk += gridDim.x)
   {
      const int i0 = blk * SPM_SCAN_BLOCK + threadIdx.x * 4;
      int v[4];
#pragma unroll
      for (int t = 0; t < 4; ++t)
         v[t] = i0 + t < n ? in[i0 + t] : 0;
      const int sum = v[0] + v[1] + v[2] + v[3];
      int x = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1)
      {
         const int y = __shfl_up(x, off, 64);
         if ( lane >= off )
            x += y;
      }
      if ( lane == 63 )
         ws[wave] = x;
      __syncthreads();
      int base = 0;
      for (int w = 0; w < wave; ++w)
         base += ws[w];
      int ex = base + x - sum;
#pragma unroll
      for (int t = 0; t < 4; ++t)
      {
         if ( i0 + t < n )
            out[i0 + t] = ex;
         ex += v[t];
      }
      if ( threadIdx.x == 0 )
         bsum[J.bs0[j] + blk] = ws[0] + ws[1] + ws[2] + ws[3];
      __syncthreads();
   }
}

/* stage 2: one workgroup per array: exclusive scan of its block sums in place, out[n] = tot[array] = the total */
__global__ void __launch_bounds__(256) k_spm_scan_top(spm_scan_jobs J, int* __restrict__ bsum, int* __restrict__ tot)
{
   __shared__ int ws[4];
   const int j = blockIdx.x;
   const int n = J.n[j];
   const int nb = (n + SPM_SCAN_BLOCK - 1) / SPM_SCAN_BLOCK;
   int* b = bsum + J.bs0[j];
   const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
   int carry = 0;
   for (int c0 = 0; c0 < nb; c0 += 256)
   {
      const int i = c0 + threadIdx.x;
      const int v = i < nb ? b[i] : 0;
      int x = v;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1)
      {
         const int y = __shfl_up(x, off, 64);
         if ( lane >= off )
            x += y;
      }
      if ( lane == 63 )
         ws[wave] = x;
      __syncthreads();
      int base = carry;
      for (int w = 0; w < wave; ++w)
         base += ws[w];
      if ( i < nb )
         b[i] = base + x - v;
      carry += ws[0] + ws[1] + ws[2] + ws[3];
      __syncthreads();
   }
   if ( threadIdx.x == 0 )
   {
      J.out[j][n] = carry;
      tot[j] = carry;
   }
}

/* stage 3: the offset of its block onto every entry */
__global__ void __launch_bounds__(256) k_spm_scan_add(spm_scan_jobs J, const int* __restrict__ bsum)
{
   const int j = blockIdx.y;
   const int n = J.n[j];
   int* out = J.out[j];
   for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
      out[i] += bsum[J.bs0[j] + i / SPM_SCAN_BLOCK];
}

/* A[(a + 1) n^2 ..] of a dense engine block: the workgroup that owns variable a clears its n x n slab, then scatters the kept entries
 * of slot act[a] into both triangles (the master holds every (slot, row, col) once: no two threads write one address) */
__global__ void __launch_bounds__(256) k_spm_gather_dense(int nactive, int n, const int* __restrict__ act, const int* __restrict__ inv,
   const int* __restrict__ loff, const int* __restrict__ lrow, const int* __restrict__ lcol, const double* __restrict__ lval,
   double* __restrict__ A)
{
   const long long n2 = (long long) n * n;
   for (int a = blockIdx.x; a < nactive; a += gridDim.x)
   {
      double* slab = A + (long long) (a + 1) * n2;
      for (long long t = threadIdx.x; t < n2; t += blockDim.x)
         slab[t] = 0.0;
      __syncthreads();
      const int slot = act[a];
      if ( slot >= 0 )
         for (int e = loff[slot] + threadIdx.x; e < loff[slot + 1]; e += blockDim.x)
         {
            const int r = inv[lrow[e]], c = inv[lcol[e]];
            if ( r >= 0 && c >= 0 )
            {
               slab[(long long) r * n + c] = lval[e];
               slab[(long long) c * n + r] = lval[e];
            }
         }
   }
}

/* ---- the gathers ------------------------------------------------------------------------------------------------------------ */

int hs_spm_gather_sparse(hipStream_t s, hs_spm* M, int n, int m, int nactive, const int* act, const int* kept, hs_sparse** out,
   long long* launches, long long* readbacks)
{
   *out = NULL;
   if ( n < 1 || n > M->N || m < 1 || nactive < 0 || nactive > m )
      return HS_ERR_ARG;
   HS_CALL( spm_ensure_final(s, M) );
   HS_CALL( spm_ensure_m(M, m) );
   const int N = M->N, S = M->S, P = (int) M->P;
   /* the node's maps: pinned, one copy */
   int* h = M->idx_h + 8;
   int ordered = 1;
   if ( nactive > 0 )
      memcpy(h, act, (size_t) nactive * sizeof(int));
   if ( hs_spm_node_maps(N, S, nactive, act, n, kept, h + M->mcap, h + M->mcap + N, &ordered) != HIPSDP_OK )
      return HS_ERR_ARG;
   HS_HIP( hipMemcpyAsync(M->idx, h, (size_t) (M->mcap + N + S) * sizeof(int), hipMemcpyHostToDevice, s) );
   const int* dact = M->idx;
   const int* dinv = M->idx + M->mcap;
   const int* dsvar = M->idx + M->mcap + N;
   int gv = (m + 3) / 4; if ( gv > 16384 ) gv = 16384;
   int gp = (P + 255) / 256; if ( gp > 16384 ) gp = 16384; if ( gp < 1 ) gp = 1;
   hipLaunchKernelGGL(k_spm_var<false>, dim3(gv), dim3(256), 0, s, m, nactive, dact, dinv, M->loff, M->lrow, M->lcol, M->lval, M->foff, M->frow,
      M->fcol, M->fval, M->vcnt, (const int*) NULL, (int*) NULL, (int*) NULL, (double*) NULL, (const int*) NULL, (int*) NULL, (int*) NULL,
      (double*) NULL, (const int*) NULL, (int*) NULL, (int*) NULL);
   HS_LAUNCH_CHECK();
   hipLaunchKernelGGL(k_spm_count_pos, dim3(gp), dim3(256), 0, s, P, dinv, dsvar, M->poff, M->prow, M->pcol, M->pslot, M->pcnt);
   HS_LAUNCH_CHECK();
   spm_scan_jobs J;
   J.in[0] = M->vcnt; J.in[1] = M->vcnt + m; J.in[2] = M->vcnt + 2 * m; J.in[3] = M->pcnt; J.in[4] = M->pcnt + P;
   J.out[0] = M->o_voff; J.out[1] = M->o_foff; J.out[2] = M->o_soff; J.out[3] = M->pscan; J.out[4] = M->pscan + P + 1;
   J.n[0] = J.n[1] = J.n[2] = m; J.n[3] = J.n[4] = P;
   int bs = 0, nbmax = 1;
   for (int j = 0; j < SPM_JOBS; ++j)
   {
      J.bs0[j] = bs;
      const int nb = spm_blocks(J.n[j]);
      bs += nb;
      if ( nb > nbmax ) nbmax = nb;
   }
   int gs = nbmax; if ( gs > 16384 ) gs = 16384;
   hipLaunchKernelGGL(k_spm_scan_local, dim3(gs, SPM_JOBS), dim3(256), 0, s, J, M->bsum);
   HS_LAUNCH_CHECK();
   hipLaunchKernelGGL(k_spm_scan_top, dim3(SPM_JOBS), dim3(256), 0, s, J, M->bsum, M->tot);
   HS_LAUNCH_CHECK();
   int ga = nbmax * 4; if ( ga > 16384 ) ga = 16384;
   hipLaunchKernelGGL(k_spm_scan_add, dim3(ga, SPM_JOBS), dim3(256), 0, s, J, M->bsum);
   HS_LAUNCH_CHECK();
   hipLaunchKernelGGL(k_spm_var<true>, dim3(gv), dim3(256), 0, s, m, nactive, dact, dinv, M->loff, M->lrow, M->lcol, M->lval, M->foff, M->frow,
      M->fcol, M->fval, (int*) NULL, M->o_voff, M->o_vrow, M->o_vcol, M->o_vval, M->o_foff, M->o_frow, M->o_fcol, M->o_fval, M->o_soff,
      M->o_srow, M->o_sent);
   HS_LAUNCH_CHECK();
   hipLaunchKernelGGL(k_spm_write_pos, dim3(gp), dim3(256), 0, s, P, dinv, dsvar, M->poff, M->prow, M->pcol, M->pslot, M->pval, M->pscan,
      M->o_poff, M->o_prow, M->o_pcol, M->o_pvar, M->o_pval);
   HS_LAUNCH_CHECK();
   if ( launches != NULL ) *launches += 7;
   /* the one read-back: nnz, nfull, nslots, npos (and the entries of the position list, = nnz) */
   HS_HIP( hipMemcpyAsync(M->idx_h, M->tot, SPM_JOBS * sizeof(int), hipMemcpyDeviceToHost, s) );
   HS_HIP( hipStreamSynchronize(s) );
   if ( readbacks != NULL ) *readbacks += 1;
   const int* t = M->idx_h;
   if ( t[0] != t[4] || t[0] < 0 || t[0] > M->L || t[1] > M->F || t[2] > M->R || t[3] > M->P )
      return HS_ERR_NUMERIC;
   if ( !ordered && t[3] > 0 )
   {
      int go = (t[3] + 255) / 256; if ( go > 16384 ) go = 16384;
      hipLaunchKernelGGL(k_spm_order_pos, dim3(go), dim3(256), 0, s, t[3], M->o_poff, M->o_pvar, M->o_pval);
      HS_LAUNCH_CHECK();
      if ( launches != NULL ) *launches += 1;
   }
   hs_sparse* sp = new hs_sparse();
   sp->n = n; sp->m = m;
   sp->nnz = t[0]; sp->nfull = t[1]; sp->nslots = t[2]; sp->npos = t[3];
   sp->voff = M->o_voff; sp->vrow = M->o_vrow; sp->vcol = M->o_vcol; sp->vval = M->o_vval;
   sp->poff = M->o_poff; sp->prow = M->o_prow; sp->pcol = M->o_pcol; sp->pvar = M->o_pvar; sp->pval = M->o_pval;
   sp->foff = M->o_foff; sp->frow = M->o_frow; sp->fcol = M->o_fcol; sp->fval = M->o_fval;
   sp->soff = M->o_soff; sp->srow = M->o_srow; sp->sent = M->o_sent; sp->Tc = M->o_Tc;
   sp->borrowed = 1;
   *out = sp;
   return HS_OK;
}

int hs_spm_gather_dense(hipStream_t s, hs_spm* M, int n, int nactive, const int* dact, const int* dinv, double* A, long long* launches)
{
   if ( n < 1 || n > M->N || nactive < 0 || A == NULL )
      return HS_ERR_ARG;
   HS_CALL( spm_ensure_final(s, M) );
   if ( nactive == 0 )
      return HS_OK;
   int g = nactive < 16384 ? nactive : 16384;
   hipLaunchKernelGGL(k_spm_gather_dense, dim3(g), dim3(256), 0, s, nactive, n, dact, dinv, M->loff, M->lrow, M->lcol, M->lval, A);
   HS_LAUNCH_CHECK();
   if ( launches != NULL ) *launches += 1;
   return HS_OK;
}
