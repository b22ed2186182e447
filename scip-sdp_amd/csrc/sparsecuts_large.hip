/* sparsecuts_large.hip - sparse eigenvector cuts of ONE SDP block of 129 .. 512 rows (the large path of hipsdp_sparsecuts).
 *
 * The algorithm is that of sparsecuts.hip (cons_sdp.c:1340-1607, truncated power method :1140-1234, default configuration); there the
 * matrix M = maxeig I - Z of a block lies in the LDS of one compute unit, which ends at 128 rows.  Here Z(y) comes from k_ec_form_z,
 * (lmin, v0) and maxeig from ONE tridiagonalisation (hs_syevx_tridiag_dev) and two requests on it (hs_syevx_select_dev); behind them
 *
 *    k_sc_tpower_large   ONE workgroup of 512 threads   thread i = row i, eight wavefronts: the whole loop over cuts and iterations
 *    k_sc_coefs_large    grid (m + 1), 256 threads      workgroup i: x_c^T A_i x_c of every cut c over the pairs of its support (a
 *                                                       block kept as nonzeros: over the variable's nonzeros)
 *
 * The bodies of both kernels are device functions of hs_scl_tpower.h (scl_tpower_loop, scl_coefs_block), which the kernels of
 * sparsecuts_large_rounds.hip - all such blocks of a solver per launch - instantiate as well.
 * An iteration is a chain of dependent steps (|w| -> ranks -> norm -> product -> Rayleigh quotient), not a throughput problem, and
 * the only synchronisation between the rows is the workgroup barrier.  HAZARD RULE: one workgroup, so there is no grid barrier, no
 * flag, no waiting on another workgroup and no atomic operation; MT is read and written by this workgroup alone, and a workgroup
 * barrier stands between its global stores to MT (the initial fill, every deflation, every new diagonal) and its later loads.
 *
 * M stays EXPLICIT (m_ii = maxeig - z_ii, m_ij = -z_ij), in a global workspace of n^2 doubles, stored TRANSPOSED: MT[c n + r] =
 * M[r][c].  The product (M x)_i = sum_p M[i][s_p] x_p over the ascending support s then reads `size` contiguous rows of MT, one
 * coalesced load per support entry with thread i at column i, and keeps the summands and their order of the row-major product of the
 * reference.  The diagonal of Z, x on its support, |w|, v0, the two lists and the partial sums are in LDS (about 23 KB).  A cut
 * (Z -= scalar x x^T, maxeig -= scalar) adds scalar x_p x_q to MT[s_q n + s_p] for the size^2 pairs of the support - the expression
 * of k_sc_tpower for M[s_p][s_q] - and forms the diagonal again.  The truncation keeps entry i when fewer than `size` entries j have
 * |w_j| > |w_i|, or |w_j| == |w_i| and j < i.  The ascending support list comes from a ballot per wavefront and the kept counts of
 * the wavefronts before it.  All sums: hs_wave_sum_dpp per wavefront, then the eight wavefronts in index order.  Every loop
 * condition is false for a NaN, and every loop is bounded by maxit or maxcuts. */
#include "hs_kernels.h"
#define SCL_NT 512         /* k_sc_tpower_large: one thread per row, HS_SCL_MAXN rows at most */
#include "hs_scl_tpower.h"

__global__ void __launch_bounds__(SCL_NT) k_sc_tpower_large(int n, int size, const double* __restrict__ Z, const double* __restrict__ plmin,
   const double* __restrict__ pmaxeig, const double* __restrict__ v0, double* MT, hs_sc_par par, hs_sc_out out)
{
   SCL_LDS_DECL(L);
   scl_tpower_loop(n, size, Z, plmin[0], pmaxeig[0], v0, MT, par, out, L);
}

/* k_sc_coefs with room for 512 rows: scl_coefs_block for matrix blockIdx.x of the one block */
__global__ void __launch_bounds__(SCL_CT) k_sc_coefs_large(int m, int maxcuts, int size, const hs_ec_job* __restrict__ jobs, hs_sc_out out)
{
   __shared__ double xs[HS_SCL_MAXN];
   __shared__ int sup[HS_SCL_MAXN];
   __shared__ double part[SCL_CT / 64];
   scl_coefs_block(m, maxcuts, size, (int) blockIdx.x, jobs[0], out, xs, sup, part);
}

int hs_scl_tpower(hipStream_t st, int n, int size, const double* Z, const double* lmin, const double* maxeig, const double* v0, double* MT,
   const hs_sc_par* par, const hs_sc_out* out)
{
   if ( n < 1 || n > HS_SCL_MAXN || size < 1 || Z == NULL || lmin == NULL || maxeig == NULL || v0 == NULL || MT == NULL )
      return HS_ERR_ARG;
   if ( out->smax < 1 || out->smax > HS_SCL_MAXN || (size <= n && size > out->smax) )
      return HS_ERR_ARG;
   hipLaunchKernelGGL(k_sc_tpower_large, dim3(1), dim3(SCL_NT), 0, st, n, size, Z, lmin, maxeig, v0, MT, *par, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}

int hs_scl_coefs(hipStream_t st, int m, int maxcuts, int size, const hs_ec_job* job, const hs_sc_out* out)
{
   if ( maxcuts <= 0 )
      return HS_OK;
   hipLaunchKernelGGL(k_sc_coefs_large, dim3(m + 1), dim3(SCL_CT), 0, st, m, maxcuts, size, job, *out);
   HS_HIP( hipGetLastError() );
   return HS_OK;
}
