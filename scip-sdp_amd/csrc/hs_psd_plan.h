/* hs_psd_plan.h - host-side planning of hipsdp_psd_project_many (csrc/psd_many.hip): argument checks, the sort of the jobs into the
 * classes of the batched decomposition, and the offsets of every job's slabs.  Host only: nothing here includes or calls HIP, so
 * the file compiles with the host compiler alone (tests/harness/psd_plan_check.cpp runs it under the sanitizers). */
#ifndef HS_PSD_PLAN_H
#define HS_PSD_PLAN_H

#include "../../include/hipsdp.h"
#include <vector>

#define HS_PP_MAXN  128      /* jobs of at most this many rows are batched */
#define HS_PP_ALIGN 32       /* slabs start at multiples of this many doubles (256 bytes, what the pool hands the single call) */

/* a batched job, in launch order (class 0 first) */
struct hs_pp_item
{
   int job;                  /* index in the caller's array */
   int n, nnz, cap;
   long long trip;           /* first triplet in the packed upload */
   long long a_off;          /* doubles: the n x n slab of the matrix, later of the result */
   long long ws_off;         /* doubles: the slab of the decomposition (hs_eig_job.ws) */
   long long row_off;        /* ints: n + 1 row offsets of the result */
};

struct hs_pp_plan
{
   std::vector<hs_pp_item> items;       /* batched jobs, sorted by class, caller's order inside a class */
   std::vector<int> big;                /* jobs above HS_PP_MAXN rows, caller's order */
   long long trips, a_len, ws_len, row_len;
   long long out_len;                   /* entries the packed result can need at most: sum of min(cap, n (n + 1) / 2) */
   int nmax;                            /* largest batched n */
};

/* the two rules of the batched decomposition the plan depends on (csrc/eigi.hip: hs_syev_many_class, hs_syev_small_scratch) */
struct hs_pp_rules { int (*cls)(int n); long long (*scratch)(int n); };

/* HIPSDP_OK, or HIPSDP_ERR_ARG (the plan is then not to be used): count outside 0 .. HIPSDP_PSD_MANY_MAXJOBS,
 * jobs NULL with count > 0, a bad mode, n < 1, nnz < 0, cap < 0, a NULL array where a length is positive, a triplet index outside
 * the matrix */
int hs_pp_plan_make(int count, const hipsdp_psd_job* jobs, int mode, const hs_pp_rules* rules, hs_pp_plan* plan);

#endif
