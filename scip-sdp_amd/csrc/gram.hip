/* gram.hip - the Gram product of the Schur assembly, Mx += W W^T on the lower triangle (W = [W_0; ..; W_m] as rows of n^2 doubles,
 * schur.hip GEMM3; in the reference this happens inside DSDP / SDPA: sdpisolver_dsdp.c:1503, sdpisolver_sdpa.cpp:1620), round 5.
 *
 * The persistent tile kernel of dgemm2.hip gives this product one item per workgroup: 36 lower tiles x 14 K slices at m = 1000.
 * Two things it leaves on the table:
 *  - a DIAGONAL tile is computed whole, 64 slab products per K step where the lower triangle has 36 (8 of 36 tiles at m = 1000,
 *    16 of 136 at m = 2000: 11 % / 6 % of the matrix instructions of the product);
 *  - with one size of item and one item per workgroup nothing can be balanced.
 * Here
 *  - a diagonal item keeps NINE accumulators per wavefront: wavefront w owns slab rows w and 7 - w of the tile, i.e. the slabs
 *    (w, 0 .. w) and (7 - w, 0 .. 7 - w) - nine for every w, the lower triangle exactly, 18 matrix instructions per stage instead
 *    of 32.  Both operands are the same 128 rows of W: only one operand image is loaded.  The code is the same for all wavefronts:
 *    the B fragment of accumulator k comes from an LDS address that depends on w, its A fragment is chosen between the two row
 *    slabs by a wave-uniform select;
 *  - the HOST cuts the product into items (tile, K range) once per shape and deals them out as STATIC lists, one per workgroup
 *    (items g.off[wg] .. g.off[wg + 1] of a small table in device memory; longest-processing-time scheduling within each XCD's
 *    share, gr_make_plan) - the kernel contains no atomic and takes nothing dynamically.  Every tile is cut into equal K slices,
 *    the diagonal tiles into fewer, longer ones (m = 1000: 28 x 15 + 8 x 9 = 492 items, one per workgroup, where 36 x 14 whole
 *    tiles were 504), sorted by their start in K so that an XCD's workgroups read the same rows of W at about the same K (once
 *    from HBM, then from that XCD's L2, as before).  Plans with more than one item per workgroup are built by the same code but
 *    not taken by default (the lists of an XCD's workgroups drift apart in K, gr_build).  Partial tiles go to slabs and are
 *    summed in slab order by a second kernel (bitwise reproducible: the order of the sum is fixed by the plan).
 * Stage loop, LDS images and counted waits as in dgemm2.hip (two halves per stage, the DMA placed by hand behind the first matrix
 * instructions of the second half); no request crosses an item boundary.
 *
 * TWO INSTANCES of the one kernel template hs_gram_kernel<WIDE>, the same stage structure (8 K positions per stage, a ring of four):
 *  - <0>: 128 x 128 tiles, four wavefronts, two workgroups per CU, 512 lists; a stage is 16 KB of LDS.  An off-diagonal wavefront owns
 *    64 x 64 (16 accumulators, 8 fragments per K step), a diagonal one nine slabs of the 8 x 8 (above);
 *  - <1>: tile rows of 256, eight wavefronts, ONE workgroup per CU, 256 lists.  A 256 x 256 tile of FP64 accumulators is the whole
 *    register file of a CU (8 wavefronts x 32 accumulators x 8 registers = 256 each, all a wavefront has when two share a SIMD), so
 *    an OFF-DIAGONAL item is one column half of a tile, 256 x 128: 4 x 2 wavefronts of 64 x 64, 16 accumulators, the stage loop of
 *    <0> with three requests per wavefront and stage where that has four (row image 256 x 8, column image 128 x 8: 24 KB per
 *    stage, 96 KB for the ring; 12 operand doubles per matrix instruction against 16).  A DIAGONAL item is the lower triangle of
 *    256 x 256 from one row image: 16 slab rows, wavefront w owns slab rows w and 15 - w - 17 accumulators for every w, 136
 *    slabs, the lower triangle exactly -, 7.5 operand doubles per matrix instruction where the diagonal item of <0> has 14.
 * The diagonal item is compiled once per wavefront (a wave-uniform switch): the slabs of its accumulators are then constants, every
 * fragment it needs (slabs 0 .. max(w, 15 - w), its two row slabs among them) is read once per K step at a constant offset, and no
 * operand is selected at run time - 9 to 16 LDS reads and 17 matrix instructions per K step where addresses chosen at run time took
 * 19 reads, 34 selects and as many address additions.
 * Both are planned by the same host code (gr_make_plan with the instance's tile, list count and diagonal cost), summed by the same
 * second kernel, and give the same bits for the same K slicing (every element sees its K positions in ascending order).  Which one
 * takes a product is decided per shape in gr_choose (the rule stands there, its measurements in profiles/r29_gram_wide_shapes.txt:
 * m1 = 1001, K = 250000 runs on <1>, 16 / 16 K slices, 256 items); a test forces either (hs_gram_instance_force), and a forced
 * instance takes every shape the kernel can serve, whatever the size.
 */
#include "hs_common.h"
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include <map>
#include <mutex>
#include <utility>
#include <type_traits>
#include <tuple>
#include <vector>
#include <queue>
#include <algorithm>
#include <functional>

typedef double gr_v4d __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void* gr_lds_ptr;
typedef const __attribute__((address_space(1))) void* gr_gbl_ptr;

#define GR_BKS  8
#define GR_NS   4
#define GR_GPS  4
#define GR_BT(inst)  ((inst) ? 256 : 128)         /* tile rows and columns of an instance */
#define GR_NWG(inst) ((inst) ? 256 : 512)         /* its workgroups = lists: one / two per CU */
#define GR_UNI(x) __builtin_amdgcn_readfirstlane(x)

__device__ __attribute__((aligned(16))) double hs_gr_zero[2] = {0.0, 0.0};

/* one unit of work: the lower tile (ti, tj) over K positions [k0, k1), its partial result into slab `slab`; wide instance, off-diagonal
 * tiles: the column half `half` (0 / 1) of the tile */
struct gram_item
{
   int ti, tj;
   int k0, k1;
   int slab;
   int half;
};

struct gram_args
{
   const double* W;        /* [M][ldw], K contiguous */
   long long ldw;
   int M;
   double* ws;             /* slabs of M x M doubles */
   const gram_item* items; /* the lists of the 512 (wide instance: 256) workgroups, one behind the other */
   const int* off;         /* list of workgroup w of XCD x: items[off[64 x + w] .. off[64 x + w + 1]) (wide instance: 32 x + w) */
};

template<int N> __device__ __forceinline__ void gr_wait_vm()
{
   asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

/* fragment of a K-contiguous stage image: element (row 16 t + (l & 15), k = 4 ks + (l >> 4)); images are stored [slab][k / 2][row][k & 1] */
__device__ __forceinline__ double gr_frag(const double* __restrict__ img, int t, int ks, int lane)
{
   const int k = 4 * ks + (lane >> 4);
   return img[t * 128 + (k >> 1) * 32 + (lane & 15) * 2 + (k & 1)];
}

/* WIDE = 0: 128 x 128 tiles on four wavefronts (2 x 2); WIDE = 1: tile rows of 256 on eight wavefronts - an off-diagonal item is one
 * column half of a tile, 256 x 128 (4 x 2 wavefronts), a diagonal item the lower triangle of 256 x 256.  A wavefront owns 64 x 64 of an
 * off-diagonal item in both */
template<int WIDE>
__global__ void __launch_bounds__(WIDE ? 512 : 256, WIDE ? 1 : 2) hs_gram_kernel(gram_args g)
{
   constexpr int BT = GR_BT(WIDE);
   constexpr int OPA = BT * GR_BKS, OPB = 128 * GR_BKS, SLOT = OPA + OPB;    /* the two operand images of a stage, and the stage */
   constexpr int GPS = WIDE ? 3 : GR_GPS;                              /* requests per wavefront and stage of an off-diagonal item */
   constexpr int NSL = BT / 16;                                        /* slab rows of a tile */
   constexpr int NA = 4, NB = 4, NACC = NA * NB;                       /* off-diagonal: row / column slabs and accumulators of a wavefront */
   constexpr int ND = NSL + 1;                                         /* diagonal: accumulators of a wavefront */
   constexpr int NREG = ND > NACC ? ND : NACC;
   extern __shared__ __attribute__((aligned(1024))) double gr_smem[];
   const int tid = threadIdx.x, lane = tid & 63;
   const int wave = GR_UNI(tid >> 6);
   const int wm = wave >> 1, wn = wave & 1;
   const int wg = (blockIdx.x & 7) * (GR_NWG(WIDE) / 8) + (blockIdx.x >> 3);   /* (blockIdx & 7 labels the XCD: a speed assumption only) */
   const int lbeg = GR_UNI(g.off[wg]), lend = GR_UNI(g.off[wg + 1]);
   const int ar = lane & 15, ac = lane >> 4;

   /* accumulators: an off-diagonal item uses NACC (slab (4 wm + i, 4 wn + j) in acc[4 i + j]), a diagonal item the first ND */
   gr_v4d acc[NREG];
#pragma unroll
   for (int i = 0; i < NREG; ++i)
      acc[i] = (gr_v4d){0.0, 0.0, 0.0, 0.0};

   /* diagonal items: accumulator k of wavefront w is the slab (w, k) for k <= w and (NSL - 1 - w, k - w - 1) behind that */
   int dcol[ND];
   bool dlo[ND];
#pragma unroll
   for (int k = 0; k < ND; ++k)
   {
      dlo[k] = k <= wave;
      dcol[k] = k <= wave ? k : k - wave - 1;
   }

   /* ---- the item's operand rows and K range; requests of stage `st` (0 .. nst - 1) into ring slot st & 3.  Items are long (hundreds
    * of stages): no request crosses an item boundary, the ring starts empty and is drained at the end of every item - which lets
    * a diagonal item request ONE operand image per stage (two pieces per wavefront instead of four).  A piece is one slab of 16 rows:
    * pieces 0, 1 are slabs 2 w, 2 w + 1 of the row image; behind them the column image, slabs 2 w, 2 w + 1 of its eight (WIDE: its
    * eight slabs over eight wavefronts, slab w as piece 2) */
   const double* pa[2]; const double* pb[2];
   int ck0 = 0, ck1 = 0;
   pa[0] = pa[1] = pb[0] = pb[1] = hs_gr_zero;
   auto piece = [&](int st, int k) __attribute__((always_inline))
   {
      const int i = k & 1;
      const int pc = (WIDE && k >= 2) ? wave : wave * 2 + i;
      const int K0 = ck0 + GR_BKS * st;
      const double* src = (K0 + 2 * ac < ck1) ? (k < 2 ? pa[i] : pb[i]) + K0 : hs_gr_zero;
      __builtin_amdgcn_global_load_lds((gr_gbl_ptr) src, (gr_lds_ptr) (gr_smem + (st & 3) * SLOT + (k < 2 ? 0 : OPA) + pc * 128), 16, 0, 0);
   };

   /* ---- off-diagonal item */
   auto run_off = [&](int nst) __attribute__((always_inline))
   {
      double f0a[NA], f0b[NB], f1a[NA], f1b[NB];
      auto landed_frags = [&](double (&fa)[NA], double (&fb)[NB]) __attribute__((always_inline))
      {
#pragma unroll
         for (int i = 0; i < NA; ++i)
            asm volatile("" : "+v"(fa[i]));
#pragma unroll
         for (int i = 0; i < NB; ++i)
            asm volatile("" : "+v"(fb[i]));
      };
      auto read_frags = [&](double (&fa)[NA], double (&fb)[NB], const double* img, int ks) __attribute__((always_inline))
      {
#pragma unroll
         for (int i = 0; i < NA; ++i)
            fa[i] = gr_frag(img, NA * wm + i, ks, lane);
#pragma unroll
         for (int i = 0; i < NB; ++i)
            fb[i] = gr_frag(img + OPA, NB * wn + i, ks, lane);
      };
#pragma unroll
      for (int st = 0; st < GR_NS; ++st)
#pragma unroll
         for (int k = 0; k < GPS; ++k)
            piece(st, k);
      gr_wait_vm<3 * GPS>();
      __builtin_amdgcn_s_barrier();
      read_frags(f0a, f0b, gr_smem, 0);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      landed_frags(f0a, f0b);
      for (int s = 0; s < nst; ++s)
      {
         const double* sa = gr_smem + (s & 3) * SLOT;
         const double* sn = gr_smem + ((s + 1) & 3) * SLOT;
         /* first half: K step 0, the fragments of K step 1 between its matrix instructions */
         __builtin_amdgcn_sched_barrier(0);
         read_frags(f1a, f1b, sa, 1);
#pragma unroll
         for (int i = 0; i < NA; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j)
               acc[NB * i + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(f0a[i], f0b[j], acc[NB * i + j], 0, 0, 0);
#pragma unroll
         for (int q = 0; q < NA + NB; ++q)
         {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
         }
         __builtin_amdgcn_sched_group_barrier(0x008, NACC - NA - NB, 0);
         __builtin_amdgcn_sched_barrier(0);
         asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
         landed_frags(f1a, f1b);
         /* stage s + 1 must have landed; stages s + 2, s + 3 may stay in flight (requests past the item's end read the zero constant,
          * so the count is the same at the end of the item) */
         gr_wait_vm<2 * GPS>();
         __builtin_amdgcn_s_barrier();
         /* second half: K step 1; two matrix instructions, then one request of stage s + 4 per matrix instruction, then the first
          * fragments of stage s + 1 */
         __builtin_amdgcn_sched_barrier(0);
         acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(f1a[0], f1b[0], acc[0], 0, 0, 0);
         acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(f1a[0], f1b[1], acc[1], 0, 0, 0);
#pragma unroll
         for (int k = 0; k < GPS; ++k)
         {
            __builtin_amdgcn_sched_barrier(0);
            piece(s + GR_NS, k);
            acc[2 + k] = __builtin_amdgcn_mfma_f64_16x16x4f64(f1a[(2 + k) / NB], f1b[(2 + k) % NB], acc[2 + k], 0, 0, 0);
         }
         __builtin_amdgcn_sched_barrier(0);
         read_frags(f0a, f0b, sn, 0);
#pragma unroll
         for (int k = 2 + GPS; k < NACC; ++k)
            acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(f1a[k / NB], f1b[k % NB], acc[k], 0, 0, 0);
#pragma unroll
         for (int q = 0; q < NA + NB; ++q)
         {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
         }
         __builtin_amdgcn_sched_barrier(0);
         asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
         landed_frags(f0a, f0b);
      }
   };

   /* ---- diagonal item: ND accumulators (nine / seventeen), compiled once PER WAVEFRONT (wsel = its number): which slab an accumulator
    * is, is then known when the code is made.  Wavefront w needs the fragments of slabs 0 .. CM - 1, CM = max(w, NSL - 1 - w) + 1 - its
    * two row slabs are among them (both operands are the same image) -, each read once per K step at an address that is one lane
    * offset plus a constant; accumulator k takes the fragments (w, k) for k <= w and (NSL - 1 - w, k - w - 1) behind that.  One
    * operand image, two requests per wavefront and stage */
   auto run_diag = [&](auto wsel, int nst) __attribute__((always_inline))
   {
      constexpr int W0 = decltype(wsel)::value, W1 = NSL - 1 - W0;
      constexpr int CM = (W0 > W1 ? W0 : W1) + 1;
      double f0[CM], f1[CM];
      auto read_set = [&](double (&f)[CM], const double* img, int ks, int c0, int c1) __attribute__((always_inline))
      {
#pragma unroll
         for (int c = c0; c < c1; ++c)
            f[c] = gr_frag(img, c, ks, lane);
      };
      auto landed_set = [&](double (&f)[CM]) __attribute__((always_inline))
      {
#pragma unroll
         for (int c = 0; c < CM; ++c)
            asm volatile("" : "+v"(f[c]));
      };
      auto mfma_k = [&](const double (&f)[CM], int k) __attribute__((always_inline))
      {
         acc[k] = __builtin_amdgcn_mfma_f64_16x16x4f64(f[k <= W0 ? W0 : W1], f[k <= W0 ? k : k - W0 - 1], acc[k], 0, 0, 0);
      };
#pragma unroll
      for (int st = 0; st < GR_NS; ++st)
#pragma unroll
         for (int k = 0; k < 2; ++k)
            piece(st, k);
      gr_wait_vm<3 * 2>();
      __builtin_amdgcn_s_barrier();
      read_set(f0, gr_smem, 0, 0, CM);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      landed_set(f0);
      for (int s = 0; s < nst; ++s)
      {
         const double* sa = gr_smem + (s & 3) * SLOT;
         const double* sn = gr_smem + ((s + 1) & 3) * SLOT;
         /* first half: K step 0, one fragment of K step 1 behind each of its first CM < ND matrix instructions */
         __builtin_amdgcn_sched_barrier(0);
         read_set(f1, sa, 1, 0, CM);
#pragma unroll
         for (int k = 0; k < ND; ++k)
            mfma_k(f0, k);
#pragma unroll
         for (int q = 0; q < CM; ++q)
         {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
         }
         __builtin_amdgcn_sched_group_barrier(0x008, ND - CM, 0);
         __builtin_amdgcn_sched_barrier(0);
         asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
         landed_set(f1);
         gr_wait_vm<2 * 2>();
         __builtin_amdgcn_s_barrier();
         /* second half: K step 1; the first four fragments of stage s + 1 behind its first two matrix instructions, one request of
          * stage s + 4 behind each of the next two, the other fragments in pairs behind the following ones */
         __builtin_amdgcn_sched_barrier(0);
         read_set(f0, sn, 0, 0, 4);
         mfma_k(f1, 0);
         mfma_k(f1, 1);
#pragma unroll
         for (int q = 0; q < 2; ++q)
         {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
         }
#pragma unroll
         for (int k = 0; k < 2; ++k)
         {
            __builtin_amdgcn_sched_barrier(0);
            piece(s + GR_NS, k);
            mfma_k(f1, 2 + k);
         }
         __builtin_amdgcn_sched_barrier(0);
         read_set(f0, sn, 0, 4, CM);
#pragma unroll
         for (int k = 4; k < ND; ++k)
            mfma_k(f1, k);
#pragma unroll
         for (int q = 0; q < (CM - 4 + 1) / 2; ++q)
         {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
         }
         __builtin_amdgcn_sched_barrier(0);
         asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
         landed_set(f0);
      }
   };

   /* ---- the workgroup's list */
   for (int cur = lbeg; cur < lend; ++cur)
   {
      const gram_item it = g.items[cur];
      const int cti = GR_UNI(it.ti), ctj = GR_UNI(it.tj), cslab = GR_UNI(it.slab);
      ck0 = GR_UNI(it.k0); ck1 = GR_UNI(it.k1);
      const int nst = (ck1 - ck0 + GR_BKS - 1) / GR_BKS;
      const bool diag = cti == ctj;
      /* first column of the item: WIDE, an off-diagonal item is the column half it.half of its tile */
      const int n0 = ctj * BT + (WIDE ? 128 * GR_UNI(it.half) : 0);
#pragma unroll
      for (int i = 0; i < 2; ++i)
      {
         const int pc = wave * 2 + i;
         int row = cti * BT + pc * 16 + ar;
         if ( row > g.M - 1 ) row = g.M - 1;
         pa[i] = g.W + (long long) row * g.ldw + 2 * ac;
         int rowb = n0 + (WIDE ? wave : pc) * 16 + ar;
         if ( rowb > g.M - 1 ) rowb = g.M - 1;
         pb[i] = g.W + (long long) rowb * g.ldw + 2 * ac;
      }
      if ( diag )
      {
         /* (wave-uniform: every wavefront takes the copy compiled for it) */
#define GR_DIAG_CASE(w) case w: run_diag(std::integral_constant<int, w>(), nst); break
         if constexpr ( WIDE )
            switch ( wave )
            {
               GR_DIAG_CASE(0); GR_DIAG_CASE(1); GR_DIAG_CASE(2); GR_DIAG_CASE(3);
               GR_DIAG_CASE(4); GR_DIAG_CASE(5); GR_DIAG_CASE(6); default: run_diag(std::integral_constant<int, 7>(), nst); break;
            }
         else
            switch ( wave )
            {
               GR_DIAG_CASE(0); GR_DIAG_CASE(1); GR_DIAG_CASE(2); default: run_diag(std::integral_constant<int, 3>(), nst); break;
            }
#undef GR_DIAG_CASE
      }
      else
         run_off(nst);
      gr_wait_vm<0>();
      /* partial tile -> its slab; the accumulators start the next item at zero */
      {
         double* C = g.ws + (long long) cslab * (long long) g.M * g.M;
         const int m0 = cti * BT;
         if ( !diag )
         {
#pragma unroll
            for (int i = 0; i < NA; ++i)
#pragma unroll
               for (int r = 0; r < 4; ++r)
               {
                  const int row = m0 + wm * (16 * NA) + 16 * i + (lane >> 4) + 4 * r;
                  if ( row < g.M )
                  {
                     double* cr = C + (long long) row * g.M + n0 + wn * 64 + (lane & 15);
#pragma unroll
                     for (int j = 0; j < NB; ++j)
                        cr[16 * j] = acc[NB * i + j][r];
                  }
               }
         }
         else
         {
#pragma unroll
            for (int k = 0; k < ND; ++k)
            {
               const int rs = dlo[k] ? wave : NSL - 1 - wave;
#pragma unroll
               for (int r = 0; r < 4; ++r)
               {
                  const int row = m0 + 16 * rs + (lane >> 4) + 4 * r;
                  const int col = m0 + 16 * dcol[k] + (lane & 15);
                  if ( row < g.M && col < g.M )
                     C[(long long) row * g.M + col] = acc[k][r];
               }
            }
         }
#pragma unroll
         for (int i = 0; i < NREG; ++i)
            acc[i] = (gr_v4d){0.0, 0.0, 0.0, 0.0};
      }
      /* (separates this item's last LDS reads from the next item's first requests) */
      __syncthreads();
   }
}

/* C[r][c] = alpha * (sum over the partial tiles of its tile, in slab order) + beta * C[r][c] for r >= c; a diagonal tile (tiles of
 * bt rows, the instance's) has nd partial tiles (slabs 0 .. nd - 1), an off-diagonal one no */
__global__ void hs_gram_reduce_kernel(int M, int bt, int no, int nd, const double* __restrict__ ws, double* __restrict__ C, long long ldc, double alpha, double beta)
{
   const long long MM = (long long) M * M;
   for (long long e = (long long) blockIdx.x * blockDim.x + threadIdx.x; e < MM; e += (long long) gridDim.x * blockDim.x)
   {
      const int r = (int) (e / M), c = (int) (e - (long long) r * M);
      if ( c > r )
         continue;
      const int ns = (r / bt == c / bt) ? nd : no;
      double s = 0.0;
      for (int k = 0; k < ns; ++k)
         s += ws[(long long) k * MM + e];
      double* q = C + (long long) r * ldc + c;
      *q = beta != 0.0 ? alpha * s + beta * (*q) : alpha * s;
   }
}

namespace {

/* how the product is cut into items and who computes them, decided on the host once per shape and instance */
struct GramPlan
{
   std::vector<gram_item> items;       /* the lists of the instance's workgroups, one behind the other */
   std::vector<int> off;               /* GR_NWG(inst) + 1 offsets */
   int inst;                           /* 0: 128 x 128 tiles, 1: the wide instance */
   int no, nd;                         /* partial tiles per off-diagonal / diagonal tile (slabs 0 .. no - 1 / 0 .. nd - 1) */
   double span;                        /* estimated time in units of one off-diagonal tile of the instance over all of K */
   double executed;                    /* FP64 matrix-core flops of one launch */
   gram_item* dev;                     /* the table on the device */
   int* devoff;
};

/* cost of a diagonal stage relative to an off-diagonal one.  128 x 128: 18 of 32 matrix instructions, one of two operand images;
 * measured 0.71 when the diagonal item chose its fragments at run time (since it is compiled per wavefront its stages are shorter,
 * measured at m1 = 1001: 0.60 moves the product by 1 %; the figure is kept, and with it the plans and the bits of this instance).
 * Wide: the off-diagonal item is HALF a tile, 32 matrix instructions per wavefront and stage, the diagonal item 34 = 1.06; measured
 * at m1 = 1001, K = 250000: 1.06 (16 / 16 slices) 3.82 ms, 1.10 - 1.22 (15 / 17 - 19) 3.89 ms */
#ifndef GR_DIAG_COST_WIDE
#define GR_DIAG_COST_WIDE 1.06
#endif
#ifndef GR_DIAG_COST_128
#define GR_DIAG_COST_128 0.72
#endif
#define GR_DIAG_COST(inst) ((inst) ? GR_DIAG_COST_WIDE : GR_DIAG_COST_128)
/* time per unit of span of the wide instance against the 128 x 128 one (measurements at gr_choose) */
#ifndef GR_WIDE_GAIN
#define GR_WIDE_GAIN 0.96
#endif

/* Every tile in equal K slices, so for the off-diagonal tiles and sd <= so for the diagonal ones (their stages are cheaper).  The
 * items sorted by their start in K are dealt to the XCDs in runs of equal cost, so that the workgroups of an XCD read the same rows
 * of W at about the same K (once from HBM, then from that XCD's L2); inside an XCD the longest item goes to the workgroup with the
 * least work so far, and a workgroup walks its items in K order.  tm: tile rows of the instance; the wide instance has two items
 * per off-diagonal tile and slice, its column halves (both into the slice's slab).  A slice is at least 8 stages long (a product
 * shorter than that is one slice: only a forced instance meets it). */
bool gr_make_plan(GramPlan& P, int inst, int tm, long long K, int so, int sd)
{
   const double cd = GR_DIAG_COST(inst);
   const int nwg = GR_NWG(inst), wpx = nwg / 8;
   if ( so < 1 || sd < 1 )
      return false;
   long long lo = (K + so - 1) / so, ld = (K + sd - 1) / sd;
   lo = ((lo + GR_BKS - 1) / GR_BKS) * GR_BKS;
   ld = ((ld + GR_BKS - 1) / GR_BKS) * GR_BKS;
   if ( (so > 1 && (long long) (so - 1) * lo + 8 * GR_BKS > K) || (sd > 1 && (long long) (sd - 1) * ld + 8 * GR_BKS > K) )
      return false;
   std::vector<gram_item> all;
   for (int s = 0; s < so; ++s)
      for (int i = 1; i < tm; ++i)
         for (int j = 0; j < i; ++j)
            for (int h = 0; h <= inst; ++h)
            {
               gram_item it = {i, j, (int) (s * lo), (int) ((s + 1) * lo < K ? (s + 1) * lo : K), s, h};
               all.push_back(it);
            }
   for (int s = 0; s < sd; ++s)
      for (int i = 0; i < tm; ++i)
      {
         gram_item it = {i, i, (int) (s * ld), (int) ((s + 1) * ld < K ? (s + 1) * ld : K), s, 0};
         all.push_back(it);
      }
   std::stable_sort(all.begin(), all.end(), [](const gram_item& a, const gram_item& b) { return a.k0 < b.k0; });
   auto cost = [&](const gram_item& it) { return (it.ti == it.tj ? cd : 1.0) * (double) (it.k1 - it.k0) / (double) K; };
   /* matrix instructions of a stage: two K steps of 64 / 36 slabs (wide: 128 / 136) */
   const double mo = inst ? 256.0 : 128.0, md = inst ? 272.0 : 72.0;
   double total = 0.0;
   P.executed = 0.0;
   for (const gram_item& it : all)
   {
      total += cost(it);
      P.executed += 2048.0 * (double) ((it.k1 - it.k0 + GR_BKS - 1) / GR_BKS) * (it.ti == it.tj ? md : mo);
   }
   P.items.clear();
   P.off.assign(nwg + 1, 0);
   P.span = 0.0;
   size_t pos = 0;
   double done = 0.0;
   for (int x = 0; x < 8; ++x)
   {
      /* the XCD's run of the sorted list: up to its share of the total cost */
      std::vector<gram_item> mine;
      const double upto = total * (double) (x + 1) / 8.0;
      while ( pos < all.size() && (x == 7 || done + 0.5 * cost(all[pos]) <= upto) )
      {
         done += cost(all[pos]);
         mine.push_back(all[pos++]);
      }
      /* longest first onto the least loaded of the XCD's workgroups */
      std::vector<size_t> order(mine.size());
      for (size_t i = 0; i < order.size(); ++i) order[i] = i;
      std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return cost(mine[a]) > cost(mine[b]); });
      std::vector<std::vector<gram_item> > lists(wpx);
      std::vector<double> load(wpx, 0.0);
      for (size_t i : order)
      {
         int w = 0;
         for (int v = 1; v < wpx; ++v)
            if ( load[v] < load[w] ) w = v;
         load[w] += cost(mine[i]);
         lists[w].push_back(mine[i]);
      }
      for (int w = 0; w < wpx; ++w)
      {
         std::stable_sort(lists[w].begin(), lists[w].end(), [](const gram_item& a, const gram_item& b) { return a.k0 < b.k0; });
         P.off[wpx * x + w] = (int) P.items.size();
         for (const gram_item& it : lists[w])
            P.items.push_back(it);
         if ( load[w] > P.span ) P.span = load[w];
      }
   }
   P.off[nwg] = (int) P.items.size();
   P.inst = inst;
   P.no = so; P.nd = sd;
   return true;
}

/* best plan of an instance for the shape with at most nslab partial tiles per tile, on the host alone (NULL: none; the caller owns
 * it).  forced: the instance is to take the shape whatever its size - no comparison with the tile kernels, and a product too short
 * or too large for one item per workgroup gets whole tiles (one slice each, several items per workgroup where it must be). */
GramPlan* gr_build(int M, long long K, int nslab, int inst, bool forced)
{
   const int bt = GR_BT(inst), nwg = GR_NWG(inst);
   const int tm = (M + bt - 1) / bt;
   const int ntile = tm * (tm + 1) / 2;
   GramPlan* best = NULL;
   GramPlan cand;
   cand.dev = NULL; cand.devoff = NULL;
   auto consider = [&](bool ok, double penalty)
   {
      if ( !ok )
         return;
      cand.span += penalty;
      if ( best == NULL || cand.span < best->span )
      {
         if ( best == NULL )
            best = new GramPlan();
         *best = cand;
      }
   };
   /* Candidates: ONE item per workgroup (at most 512 items, wide instance 256).  With several items per workgroup the lists of an
    * XCD's workgroups drift apart in K and the rows of W are no longer shared through its L2: measured at m = 2000 (136 tiles, 8 items
    * per workgroup, balanced to 3 % below the K-sliced tile kernel's estimate) 68.6 against 66.3 ms - the tile kernel's rounds of
    * equal items stay in step by construction, and the diagonal tiles are only 6 % of that product.  The plan is taken when its
    * estimate beats the tile kernel's (whole rounds of 512 equal items) by 3 %.  Every partial tile is stored by its workgroup
    * and read again by the summation kernel: priced at 0.24 K positions of one tile. */
   /* (wide: its diagonal items are the longer ones, up to twice the slices of the off-diagonal tiles; a partial tile of a diagonal
    * item is 136 slabs where the half tile's is 128) */
   const int noff = (ntile - tm) * (inst ? 2 : 1);
   for (int so = 1; so <= nslab && (long long) noff * so + tm <= nwg; ++so)
      for (int sd = inst ? so : (so + 1) / 2; sd <= (inst ? 2 * so : so) && sd <= nslab && (long long) noff * so + (long long) tm * sd <= nwg; ++sd)
         consider(gr_make_plan(cand, inst, tm, K, so, sd), 0.24 * ((double) so * noff + (double) sd * tm) / (double) K);
   if ( forced )
   {
      if ( best == NULL )
         consider(gr_make_plan(cand, inst, tm, K, 1, 1), 0.0);
      return best;
   }
   if ( best != NULL )
   {
      /* the tile kernel's estimate counts 128 x 128 tiles on workgroups that share a CU in pairs; a wide workgroup has its CU alone
       * and its half tile is two of those: the same CU time for the same span, times what its stages were measured to save */
      const int t128 = (M + 127) / 128, n128 = t128 * (t128 + 1) / 2;
      const int sold = hs_dgemm_pick_xcd_slices(n128, K);
      const double oldspan = (double) (((long long) n128 * sold + 511) / 512) / (double) sold;
      if ( (inst ? GR_WIDE_GAIN : 1.0) * best->span * 1.03 > oldspan || (int) best->items.size() < nwg / 2 )
      {
         delete best;
         best = NULL;
      }
   }
   return best;
}

/* the same, kept per device and shape with its table on the device (NULL: none) */
GramPlan* gr_plan(int M, long long K, int nslab, int inst, bool forced)
{
   static std::mutex mu;
   static std::map<std::tuple<int, int, long long, int, int>, GramPlan*> tab;
   int dev = 0;
   if ( hipGetDevice(&dev) != hipSuccess )
      return NULL;
   std::lock_guard<std::mutex> lk(mu);
   const auto key = std::make_tuple(dev, M, K, nslab, 2 * inst + (forced ? 1 : 0));
   auto f = tab.find(key);
   if ( f != tab.end() )
      return f->second;
   GramPlan* best = gr_build(M, K, nslab, inst, forced);
   if ( best != NULL )
   {
      gram_item* d = NULL;
      int* doff = NULL;
      if ( hipMalloc((void**) &d, best->items.size() * sizeof(gram_item)) != hipSuccess
         || hipMemcpy(d, best->items.data(), best->items.size() * sizeof(gram_item), hipMemcpyHostToDevice) != hipSuccess
         || hipMalloc((void**) &doff, best->off.size() * sizeof(int)) != hipSuccess
         || hipMemcpy(doff, best->off.data(), best->off.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess )
      {
         if ( d != NULL ) (void) hipFree(d);
         if ( doff != NULL ) (void) hipFree(doff);
         delete best;
         return NULL;
      }
      best->dev = d;
      best->devoff = doff;
   }
   tab[key] = best;
   return best;
}

int gr_inst_mode = -1;
int gr_taken = 0;
int gr_wide_taken = 0;

/* The plan that takes the product (NULL: none: the tile kernels take it).  A forced instance (hs_gram_instance_force) takes every
 * shape.  Otherwise the Gram kernel takes what its 128 x 128 instance has a plan for, as before, and the wide instance runs in its
 * place
 *  - only where it pads no more rows (an even number of 128-row tiles: m1 = 1001 is 1024 rows for both), and
 *  - where its own plan is admitted (gr_build) and its span times GR_WIDE_GAIN is no more than the 128 x 128 plan's.
 * Shapes for which the 128 x 128 instance has no plan (136 tiles at m1 = 2001) stay with the tile kernels: the wide instance was
 * measured faster there too (below), but which kernel serves those shapes is left as it is.
 * GR_WIDE_GAIN: time per unit of span of the wide instance against the 128 x 128 one, both forced on one MI355X
 * (profiles/r29_gram_wide_shapes.txt): m1 = 1001, K = 250000: 3.89 ms at 0.0665 against 4.25 ms at 0.0672 = 0.92; K = 62500: 0.99 ms at
 * 0.0673 against 1.06 at 0.0686 = 0.95; m1 = 768, K = 90000: 0.85 at 0.0372 against 0.91 at 0.0398 = 1.00. */
GramPlan* gr_choose(int M, long long K, int nslab)
{
   const int mode = gr_inst_mode;
   if ( mode >= 0 )
      return gr_plan(M, K, nslab, mode, true);
   GramPlan* P = gr_plan(M, K, nslab, 0, false);
   if ( P == NULL || P->dev == NULL || (((M + 127) / 128) & 1) )
      return P;
   GramPlan* Pw = gr_plan(M, K, nslab, 1, false);
   if ( Pw != NULL && Pw->dev != NULL && GR_WIDE_GAIN * Pw->span <= P->span )
      return Pw;
   return P;
}

}

/* test hook: how many products the Gram kernel has taken so far, either instance */
int hs_gram_taken(void)
{
   return __atomic_load_n(&gr_taken, __ATOMIC_RELAXED);
}

/* test hook: which instance of the Gram kernel takes the products it is eligible for.  mode -1: chosen per shape (gr_choose), 0: the
 * 128 x 128 instance, 1: the wide instance; forced (0, 1), the kernel also takes products below the size from which it is used by
 * default.  Any other mode changes nothing.  Returns how many products the wide instance has taken so far. */
int hs_gram_instance_force(int mode)
{
   if ( mode >= -1 && mode <= 1 )
      gr_inst_mode = mode;
   return __atomic_load_n(&gr_wide_taken, __ATOMIC_RELAXED);
}

/* C (M x M, lower triangle) = alpha W W^T + beta C with W [M][K] (K contiguous, leading dimension ldw), through `nslab` slabs of
 * M x M doubles at ws.  1: done, 0: not eligible (the caller takes hs_dgemm), < 0: error code negated.  *executed: the FP64
 * matrix-core flops the launch executes (the tiles and K ranges of the instance that ran). */
int hs_gram_try(hipStream_t stream, int M, long long K, const double* W, long long ldw, double* C, long long ldc, double alpha, double beta,
   double* ws, int nslab, double* executed)
{
   const bool forced = gr_inst_mode >= 0;
   if ( ws == NULL || nslab < 2 || M < 1 || K < 2 || (!forced && (M < 256 || K < 16384)) )
      return 0;
   if ( (ldw & 1) || (K & 1) || (((uintptr_t) W) & 15) || K > 2000000000LL )
      return 0;
   if ( nslab > 64 ) nslab = 64;
   GramPlan* P = gr_choose(M, K, nslab);
   if ( P == NULL || P->dev == NULL || P->items.empty() )
      return 0;
   gram_args g;
   g.W = W; g.ldw = ldw; g.M = M; g.ws = ws; g.items = P->dev; g.off = P->devoff;
   const size_t smem = (size_t) GR_NS * (GR_BT(P->inst) + 128) * GR_BKS * sizeof(double);
   if ( P->inst )
   {
      static hs_attr_mask attr_wide;
      if ( hs_func_max_lds(reinterpret_cast<const void*>(&hs_gram_kernel<1>), (int) smem, &attr_wide) != HS_OK )
         return -HS_ERR_HIP;
      hipLaunchKernelGGL(hs_gram_kernel<1>, dim3(GR_NWG(1)), dim3(512), smem, stream, g);
   }
   else
   {
      static hs_attr_mask attr_done;
      if ( hs_func_max_lds(reinterpret_cast<const void*>(&hs_gram_kernel<0>), (int) smem, &attr_done) != HS_OK )
         return -HS_ERR_HIP;
      hipLaunchKernelGGL(hs_gram_kernel<0>, dim3(GR_NWG(0)), dim3(256), smem, stream, g);
   }
   if ( hipGetLastError() != hipSuccess )
      return -HS_ERR_HIP;
   {
      int blocks = (int) (((long long) M * M + 255) / 256);
      if ( blocks > 2048 ) blocks = 2048;
      hipLaunchKernelGGL(hs_gram_reduce_kernel, dim3(blocks), dim3(256), 0, stream, M, GR_BT(P->inst), P->no, P->nd, ws, C, ldc, alpha, beta);
      if ( hipGetLastError() != hipSuccess )
         return -HS_ERR_HIP;
   }
   if ( executed != NULL )
      *executed = P->executed;
   (void) __atomic_add_fetch(&gr_taken, 1, __ATOMIC_RELAXED);
   if ( P->inst )
      (void) __atomic_add_fetch(&gr_wide_taken, 1, __ATOMIC_RELAXED);
   return 1;
}

/* developer tool: the plan chosen for a shape (as hs_gram_try chooses it: a forced instance is followed) */
int hs_gram_plan_info(int M, long long K, int nslab, int* no, int* nd, int* nitems, double* span)
{
   GramPlan* P = gr_choose(M, K, nslab > 64 ? 64 : nslab);
   if ( P == NULL )
      return 0;
   *no = P->no; *nd = P->nd; *nitems = (int) P->items.size(); *span = P->span;
   return 1;
}

/* test entry, host only: the plan of instance `inst` for a shape as gr_build makes it (forced as above).  info[4] = items, lists,
 * partial tiles per off-diagonal and per diagonal tile; off[lists + 1]; the first `cap` items as six ints each (ti, tj, k0, k1,
 * slab, half).  1: there is a plan, 0: none */
int hs_gram_plan_host(int inst, int forced, int M, long long K, int nslab, int cap, int* items, int* off, int* info)
{
   if ( inst < 0 || inst > 1 || M < 1 || K < 2 || nslab < 1 )
      return 0;
   GramPlan* P = gr_build(M, K, nslab > 64 ? 64 : nslab, inst, forced != 0);
   if ( P == NULL )
      return 0;
   info[0] = (int) P->items.size(); info[1] = GR_NWG(inst); info[2] = P->no; info[3] = P->nd;
   for (size_t i = 0; i < P->off.size(); ++i)
      off[i] = P->off[i];
   for (int i = 0; i < info[0] && i < cap; ++i)
      memcpy(items + 6 * (size_t) i, &P->items[i], sizeof(gram_item));
   delete P;
   return 1;
}
