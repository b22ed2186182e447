/* hs_wave.h - what the kernels of csrc/ share below the level of an algorithm: moving a double between the lanes of a wavefront, the
 * sums over lanes, and the reciprocals built on the hardware seeds.  The sums are NOT interchangeable: each adds in its own order, a
 * kernel's results are reproducible to the bit only while it keeps the one it has, and the names say which is which. */
#ifndef HS_WAVE_H
#define HS_WAVE_H

#include <hip/hip_runtime.h>

/* ---- lane exchange ------------------------------------------------------------------------------------------------------------- */

/* The value of another lane of the same row of 16 lanes, on the data-parallel-primitive path (no LDS crossbar round trip as with
 * __shfl): CTRL = 0xB1 quad_perm [1, 0, 3, 2] (lane ^ 1), 0x4E quad_perm [2, 3, 0, 1] (lane ^ 2), 0x141 row_half_mirror (7 - lane
 * within the eight), 0x140 row_mirror (15 - lane within the row).  Valid in every lane; all lanes of the row must be active. */
template<int CTRL>
__device__ __forceinline__ int hs_dpp(int v)
{
   return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}
template<int CTRL>
__device__ __forceinline__ double hs_dpp(double v)
{
   int lo = __double2loint(v), hi = __double2hiint(v);
   lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
   hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
   return __hiloint2double(hi, lo);
}

/* The value lane l holds, as a wavefront-uniform (scalar) operand; l must itself be wavefront-uniform.  Valid in every lane. */
__device__ __forceinline__ double hs_lane(double v, int l)
{
   const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
   return __hiloint2double(hi, lo);
}

/* ---- sums by DPP: inside the rows of 16 first ------------------------------------------------------------------------------------ */

/* Sum over the four lanes of a quad, valid in every lane: (v + v[lane ^ 1]), then that plus the same of lane ^ 2. */
__device__ __forceinline__ double hs_quad_sum_dpp(double v)
{
   v += hs_dpp<0xB1>(v);
   v += hs_dpp<0x4E>(v);
   return v;
}

/* Sum over the 16 lanes of a row, valid in every lane of the row: the quad sum, then plus the quad mirrored within the eight, then
 * plus the eight mirrored within the row. */
__device__ __forceinline__ double hs_row_sum_dpp(double v)
{
   v += hs_dpp<0xB1>(v);              /* quad_perm [1, 0, 3, 2] */
   v += hs_dpp<0x4E>(v);              /* quad_perm [2, 3, 0, 1] */
   v += hs_dpp<0x141>(v);             /* row_half_mirror */
   v += hs_dpp<0x140>(v);             /* row_mirror */
   return v;
}

/* Sum over the 64 lanes, valid (and wavefront-uniform) in every lane: the four row sums of hs_row_sum_dpp read as scalars and added
 * as ((row 0 + row 1) + row 2) + row 3. */
__device__ __forceinline__ double hs_wave_sum_dpp(double v)
{
   v = hs_row_sum_dpp(v);
   return ((hs_lane(v, 0) + hs_lane(v, 16)) + hs_lane(v, 32)) + hs_lane(v, 48);
}

/* ---- sums by __shfl ------------------------------------------------------------------------------------------------------------- */

/* Sum over the aligned groups of W lanes (W = 4, 16, 64), valid in every lane with the same bits throughout a group: the butterfly
 * v += v[lane ^ m] for m = 1, 2, .., W / 2 ascending - pairs first, the two halves of the group last.  Up to a row of 16
 * every step adds the same two partial sums as the DPP sums above; over 64 lanes it is (row 0 + row 1) + (row 2 + row 3), other bits
 * than hs_wave_sum_dpp.  The same steps stand written out for W = 4 and 16 in chol.hip, kernels.hip and eig.hip (quad_sum): as this
 * loop the compiler orders the instructions of those kernels differently, so they stay as they are. */
template<int W>
__device__ __forceinline__ double hs_xsum(double v)
{
#pragma unroll
   for (int m = 1; m < W; m <<= 1)
      v += __shfl_xor(v, m, 64);
   return v;
}

/* Sum over the 64 lanes, valid in LANE 0 ONLY: v += v[lane + off] for off = 32, 16, .., 1 descending - the two halves of the wavefront
 * first, neighbours last; a lane whose partner lies behind lane 63 adds its own value instead, so the other lanes hold no sum. */
__device__ __forceinline__ double hs_wave_sum_down(double v)
{
#pragma unroll
   for (int off = 32; off > 0; off >>= 1)
      v += __shfl_down(v, off, 64);
   return v;
}

/* Sum over a workgroup of NW wavefronts, valid in every thread with the same bits: hs_xsum<64> per wavefront, then
 * ((red[0] + red[1]) + red[2]) + .. in the order of the wavefronts.  Contains ONE barrier, behind the stores to red[0 .. NW - 1] -
 * red must not be written again before the next barrier of the caller. */
template<int NW>
__device__ __forceinline__ double hs_block_sum(double v, double* red)
{
   v = hs_xsum<64>(v);
   if ( (threadIdx.x & 63) == 0 )
      red[threadIdx.x >> 6] = v;
   __syncthreads();
   double s = red[0];
#pragma unroll
   for (int w = 1; w < NW; ++w)
      s += red[w];
   return s;
}

/* ---- reciprocals without the division and square-root expansions ------------------------------------------------------------------ */

/* 1 / t by v_rcp_f64 and ONE Newton step r += (1 - t r) r: full precision for finite, normal t at a third of the latency of a
 * division - for the sequential recurrences (Sturm counts in quotient form). */
__device__ __forceinline__ double hs_rcp1(double t)
{
   double r = __builtin_amdgcn_rcp(t);
   r = fma(fma(-t, r, 1.0), r, r);
   return r;
}

/* 1 / t by v_rcp_f64 and TWO Newton steps. */
__device__ __forceinline__ double hs_rcp2(double t)
{
   double r = __builtin_amdgcn_rcp(t);
   r = fma(fma(-t, r, 1.0), r, r);
   r = fma(fma(-t, r, 1.0), r, r);
   return r;
}

/* 1 / sqrt(x) by v_rsq_f64 (a low-precision seed) and two coupled Newton steps on g -> sqrt(x), h -> 1 / (2 sqrt(x)); returns 2 h. */
__device__ __forceinline__ double hs_rsqrt2(double x)
{
   double y = __builtin_amdgcn_rsq(x);
   double h = 0.5 * y, g = x * y;
   double r = fma(-h, g, 0.5);
   g = fma(g, r, g); h = fma(h, r, h);
   r = fma(-h, g, 0.5);
   h = fma(h, r, h);
   return 2.0 * h;
}

#endif
