/* hs_syevx_index_many.h - part of syevx.hip (included inside its anonymous namespace, behind the bodies of the four stages): the values
 * launch of hipsdp_rank1_check_many for MANY matrices on the forms hs_syevx_many_cols leaves. */
#ifndef HS_SYEVX_INDEX_MANY_H
#define HS_SYEVX_INDEX_MANY_H

/* the several-indices values form (hipsdp_rank1_check_many), grid (matrices, 2): row 0 the range [1, 1] to out - the launch and the bits
 * of row 0 of k_syevx_values_many -, row 1 the range [n - 1, n] to out2 (eigenvalue n - 1 at out2[HS_SYEVX_OUT_LAM], n behind it) */
__global__ void __launch_bounds__(SX_VT) k_syevx_values_index_many(const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act)
{
   const int job = blockIdx.x, which = blockIdx.y;
   if ( act[job] == 0 )
      return;
   const int n = jobs[job].n;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   if ( which == 0 )
      d_syevx_values(n, 0, 1, 1, 0.0, 0, w.d, w.e, jobs[job].out);
   else
      d_syevx_values(n, 0, n - 1, n, 0.0, 0, w.d, w.e, jobs[job].out2);
}

#endif
