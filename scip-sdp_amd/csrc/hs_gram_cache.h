/* hs_gram_cache.h - host bookkeeping of the cached cold-start Gram matrix (csrc/ipm.hip: GeneralSolve::assemble_forms).  Plain C++, no
 * device call: what decides whether the stored first assembly M_ij = <A_i, A_j> may stand in for a computed one.
 *
 * Every dense block carries a generation number of its constraint matrices.  Numbers are drawn from ONE counter per solver that only
 * grows (hs_gen_next), so a number is never handed out twice in the life of a solver: a block that is freed and allocated again, or
 * written and written back, cannot meet an old key again.  Whoever writes, gathers, generates, clears, re-shapes or frees the matrices
 * of a block (or cannot prove that it wrote nothing) draws a new number for it.
 *
 * The stored matrix is the bits of Mx after the identity assemblies of all blocks, in block order, before the LP term.  Those bits are
 * a function of: the matrices (generation numbers), the shape (m, the block sizes in order), which identity form each block took
 * (packed lower triangles or full rows: different K, different summation) and the workspace the Gram kernel summed in (number of
 * slabs from kws_len; full / chunk_cols decide whether the packed form fits).  The key holds exactly these. */
#ifndef HS_GRAM_CACHE_H
#define HS_GRAM_CACHE_H

#define HS_GRAM_FORM_FULL   1      /* hs_schur_W_identity: the full rows */
#define HS_GRAM_FORM_PACKED 2      /* hs_schur_W_identity_packed: 2 P P^T - D D^T */
#define HS_GRAM_MAXBLK 64          /* problems with more dense blocks are not cached */

struct hs_gram_key
{
   int valid;                                   /* 0: nothing stored */
   int m, nblk;
   int n[HS_GRAM_MAXBLK];
   int form[HS_GRAM_MAXBLK];
   unsigned long long gen[HS_GRAM_MAXBLK];
   long long kws_len, chunk_cols;
   int ws_full;
};

/* a generation number nobody has had: 1, 2, ... (0 is "never written": no block carries it once it exists) */
static inline unsigned long long hs_gen_next(unsigned long long* counter)
{
   return ++*counter;
}

static inline void hs_gram_key_clear(hs_gram_key* k)
{
   k->valid = 0;
   k->m = 0;
   k->nblk = 0;
   k->kws_len = k->chunk_cols = 0;
   k->ws_full = 0;
}

/* the key of what a cold solve is about to assemble: 0 when such a problem is not cached (no blocks, too many, a form that is none) */
static inline int hs_gram_key_make(hs_gram_key* k, int m, int nblk, const int* n, const int* form, const unsigned long long* gen,
   long long kws_len, long long chunk_cols, int ws_full)
{
   hs_gram_key_clear(k);
   if ( m < 0 || nblk < 1 || nblk > HS_GRAM_MAXBLK )
      return 0;
   for (int b = 0; b < nblk; ++b)
   {
      if ( n[b] < 1 || gen[b] == 0 || (form[b] != HS_GRAM_FORM_FULL && form[b] != HS_GRAM_FORM_PACKED) )
         return 0;
      k->n[b] = n[b];
      k->form[b] = form[b];
      k->gen[b] = gen[b];
   }
   k->m = m;
   k->nblk = nblk;
   k->kws_len = kws_len;
   k->chunk_cols = chunk_cols;
   k->ws_full = ws_full;
   k->valid = 1;
   return 1;
}

/* 1 when the stored matrix (key `have`) is bit for bit what a solve with key `want` would compute */
static inline int hs_gram_key_match(const hs_gram_key* have, const hs_gram_key* want)
{
   if ( !have->valid || !want->valid || have->m != want->m || have->nblk != want->nblk || have->kws_len != want->kws_len
      || have->chunk_cols != want->chunk_cols || have->ws_full != want->ws_full )
      return 0;
   for (int b = 0; b < have->nblk; ++b)
      if ( have->n[b] != want->n[b] || have->form[b] != want->form[b] || have->gen[b] != want->gen[b] )
         return 0;
   return 1;
}

#endif
