/* hs_sp_master.h - host side of a master block kept as triplets (csrc/sp_master.hip): the one-time sort of the collected entries
 * into the three orders the gather kernels read, and the index maps of a node.  Host only: nothing here includes or calls HIP, so
 * the file compiles with the host compiler alone (tests/harness/sp_master_check.cpp runs it under the sanitizers).
 *
 * The rule is that of hs_sp_build (csrc/sparse.hip): the larger index of an entry is its row, and a later entry at the same
 * (slot, row, col) replaces an earlier one.  All indices are ORIGINAL ones (rows 0 .. N - 1 of the block, slots 0 .. S - 1). */
#ifndef HS_SP_MASTER_H
#define HS_SP_MASTER_H

#include "../../include/hipsdp.h"
#include <vector>

struct hs_spm_final
{
   int N, S;
   long long L, P, F, R;                /* lower entries, positions, mirrored entries, non-empty rows summed over the slots */
   /* lower triplets sorted by (slot, row, col): slot k has [loff[k], loff[k + 1]) */
   std::vector<int> loff, lrow, lcol;
   std::vector<double> lval;
   /* the same entries sorted by (row, col, slot): position p = (prow[p], pcol[p]) has [poff[p], poff[p + 1]) */
   std::vector<int> poff, prow, pcol, pslot;
   std::vector<double> pval;
   /* both triangles per slot, row-major: slot k has [foff[k], foff[k + 1]) */
   std::vector<int> foff, frow, fcol;
   std::vector<double> fval;
};

/* HIPSDP_OK, or HIPSDP_ERR_ARG: an index outside the block (slot == NULL: every entry belongs to slot `oneslot`) */
int hs_spm_check(int N, int S, long long nnz, const int* slot, int oneslot, const int* row, const int* col);

/* HIPSDP_OK, or HIPSDP_ERR_ARG: an index outside the block, or more mirrored entries than an int offset counts (out is then
 * not to be used) */
int hs_spm_finalize(int N, int S, long long nnz, const int* slot, const int* row, const int* col, const double* val, hs_spm_final* out);

/* the maps of a node: inv[N] = new index of an original row (-1: removed), svar[S] = new 1-based variable of a slot (0: not
 * active); *ordered = 1 when the slots of the active variables increase with the variable, so that the master's order inside a
 * position is the node's.  HIPSDP_ERR_ARG: a slot outside -1 .. S - 1 or named twice, kept not increasing or outside the block.
 * O(N + S + nactive). */
int hs_spm_node_maps(int N, int S, int nactive, const int* act, int nkept, const int* kept, int* inv, int* svar, int* ordered);

#endif
