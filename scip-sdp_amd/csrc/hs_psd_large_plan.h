/* hs_psd_large_plan.h - host-side planning of hipsdp_psd_project_many_large (csrc/psd_large.hip): argument checks, which jobs are
 * served, the chunks the served jobs are taken in and the offsets of every job's slabs inside its chunk, and the launch count of a
 * chunk.  Host only: nothing here includes or calls HIP, so the file compiles with the host compiler alone
 * (tests/harness/psd_large_plan_check.cpp runs it under the sanitizers). */
#ifndef HS_PSD_LARGE_PLAN_H
#define HS_PSD_LARGE_PLAN_H

#include "../../include/hipsdp.h"
#include <vector>

#define HS_PPL_TILE  64      /* rows and columns of an output tile of the recombination */
#define HS_PPL_ALIGN 32      /* slabs start at multiples of this many doubles (256 bytes) */

/* a served job; the offsets are relative to the start of the part of the chunk's device block they belong to */
struct hs_ppl_item
{
   int job;                  /* index in the caller's array */
   int n, nnz, cap;
   int ntc;                  /* tile columns (= tile rows) of the recombination: ceil(n / HS_PPL_TILE) */
   long long len;            /* bytes of workspace the job takes in a chunk (what the chunk limit counts) */
   long long trip;           /* first triplet in the chunk's packed upload */
   long long ws_off;         /* doubles: the workspace of the decomposition (ws_len(n)) */
   long long out_off;        /* doubles: eigenvalues and eigenvectors (out_len(n)) */
   long long cnt_off;        /* ints: n x ntc row counts, then ntc x ntc tile totals */
};

/* the two lengths of the batched decomposition the plan depends on (csrc/syevr.hip: hs_syevr_ws, HS_SYEVR_OUT), in doubles */
struct hs_ppl_rules { long long (*ws_len)(int n); long long (*out_len)(int n); };

struct hs_ppl_chunk
{
   int first, end;           /* items [first, end) of the plan */
   int nmax;                 /* largest n of the chunk */
   long long trips;          /* triplets of the chunk */
   long long ws_len, out_len;/* doubles */
   long long cnt_len;        /* ints */
   long long res_len;        /* entries the packed result can need at most: sum of min(cap, n (n + 1) / 2) */
};

/* HIPSDP_OK, or HIPSDP_ERR_ARG: the argument-error list of hipsdp_psd_project_many (hs_psd_plan.h) */
int hs_ppl_check(int count, const hipsdp_psd_job* jobs, int mode);
/* the served jobs (HIPSDP_PSD_LARGE_MINN <= n <= HIPSDP_PSD_LARGE_MAXN), largest first, caller's order among equal sizes, with
 * job, n, nnz, cap, ntc and len filled in; jobs must have passed hs_ppl_check */
int hs_ppl_items(int count, const hipsdp_psd_job* jobs, const hs_ppl_rules* rules, std::vector<hs_ppl_item>* items);
/* the chunk that starts at item `start`: as many items as fit `budget` bytes of workspace, at least one (hs_chunk_end of hs_chunks.h
 * over the items' len); fills the offsets of its items and returns its description */
int hs_ppl_chunk_make(std::vector<hs_ppl_item>* items, int start, long long budget, const hs_ppl_rules* rules, hs_ppl_chunk* chunk);
/* kernel launches of a chunk whose largest job has nmax rows: nmax + 8 + 6 ceil(nmax / 32)
 *    1 expand, nmax - 1 columns of the tridiagonalisation, 2 for the eigenvalues and their order, 3 + 6 ceil(nmax / 32) for the
 *    eigenvectors of T, 1 back-transformation, 1 recombination, 1 write */
int hs_ppl_launches(int nmax);

#endif
