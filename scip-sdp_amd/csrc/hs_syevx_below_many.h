/* hs_syevx_below_many.h - a PART of syevx.hip, included there inside its unnamed namespace and nowhere else (it uses sx_layout and the
 * stage bodies of that file): the kernels of the BELOW selection for many matrices per launch. */
#ifndef HS_SYEVX_BELOW_MANY_H
#define HS_SYEVX_BELOW_MANY_H

/* ---- the BELOW selection for many matrices per launch (hs_syevx_many_below; caller: hipsdp_eigencuts_all_large, cut_calls.hip): on the
 * tridiagonal forms k_syevx_col_many leaves, the eigenvalues <= bound of every active matrix, at most maxk of them, with their vectors,
 * into out in the layout HS_SYEVX_OUT(n) of the single-matrix path - and eigenvalue 1 by index into out2, the value a matrix without
 * an eigenvalue below the bound still has to report.  Wrappers like the four above: the bodies are those of the single matrix. */
__global__ void __launch_bounds__(SX_VT) k_syevx_values_below_many(const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act, double bound,
   int maxk)
{
   const int job = blockIdx.x, which = blockIdx.y;
   if ( act[job] == 0 )
      return;
   const int n = jobs[job].n;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   if ( which == 0 )
      d_syevx_values(n, 0, 1, 1, 0.0, 0, w.d, w.e, jobs[job].out2);
   else
      d_syevx_values(n, 1, 0, 0, bound, maxk, w.d, w.e, jobs[job].out);
}

/* dynamic LDS: maxk x (nmax | 1) doubles */
__global__ void __launch_bounds__(SX_VT) k_syevx_tvec_below_many(const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act)
{
   extern __shared__ __attribute__((aligned(16))) double Z[];
   const int job = blockIdx.x;
   if ( act[job] == 0 )
      return;
   const int n = jobs[job].n;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   d_syevx_tvec(n, w.d, w.e, jobs[job].out, w.Zt, w.G0, w.G1, w.G2, Z);
}

/* grid (matrices, maxk): one wavefront per vector; vector k >= the matrix's count returns at once (d_syevx_back) */
__global__ void __launch_bounds__(64) k_syevx_back_below_many(const hs_sxm_job* __restrict__ jobs, const int* __restrict__ act)
{
   const int job = blockIdx.x;
   if ( act[job] == 0 )
      return;
   const int n = jobs[job].n;
   const sx_ws w = sx_layout(n, jobs[job].ws);
   d_syevx_back(n, (int) blockIdx.y, w.R, w.tau, w.Zt, jobs[job].out);
}

#endif
