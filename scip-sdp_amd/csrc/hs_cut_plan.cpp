/* hs_cut_plan.cpp - see hs_cut_plan.h */
#include "hs_cut_plan.h"

static long long even(long long len) { return (len + 1) & ~1LL; }

/* lmin .. vec from offset `at` on; returns the offset behind the vectors */
static long long res_arrays(long long at, int nb, int m, int maxcuts, long long vec_len, hs_cut_res* r)
{
   const long long slots = (long long) nb * maxcuts;
   r->nb = nb; r->smax = 0;
   r->ints = r->sup = -1;
   r->lmin = at; r->eig = r->lmin + nb; r->lhs = r->eig + slots; r->coef = r->lhs + slots; r->vec = r->coef + slots * m;
   return r->vec + vec_len;
}

void hs_ec_layout_make(int nb, int m, int maxcuts, long long vec_len, long long slab_len, hs_ec_layout* L)
{
   L->y = 0;
   L->ncuts = (m + 2) & ~1LL;
   L->slabs = res_arrays(L->ncuts + nb, nb, m, maxcuts, vec_len, &L->r);
   L->len.res_off = L->ncuts; L->len.res_len = L->slabs - L->ncuts;
   L->len.upload_len = m; L->len.pin_len = L->slabs; L->len.dev_len = L->slabs + slab_len;
}

void hs_sc_layout_make(int nb, int m, int maxcuts, int smax, long long vec_len, long long slab_len, hs_sc_layout* L)
{
   L->y = 0;
   L->sizes = (m + 2) & ~1LL;
   L->len.res_off = L->sizes + ((long long) nb + 1) / 2;
   L->r.ints = res_arrays(L->len.res_off, nb, m, maxcuts, vec_len, &L->r);
   L->r.smax = smax;
   L->r.sup = L->r.ints + (3LL * nb + 1) / 2;
   L->slabs = L->r.sup + ((long long) nb * maxcuts * smax + 1) / 2;
   L->len.res_len = L->r.sup - L->len.res_off;
   L->len.upload_len = L->len.res_off; L->len.pin_len = L->r.sup; L->len.dev_len = L->slabs + slab_len;
}

void hs_scr_layout_make(int nb, int m, int maxcuts, int smax, long long vec_len, long long slab_len, long long state_len, hs_scr_layout* L)
{
   hs_sc_layout_make(nb, m, maxcuts, smax, vec_len, slab_len, &L->sc);
   L->state = even(L->sc.len.dev_len);
   L->len = L->sc.len;
   L->len.dev_len = L->state + state_len;
}

void hs_scl_layout_make(int n, int m, int maxcuts, int smax, long long ws_len, long long out_len, long long out_vec, hs_scl_layout* L)
{
   const long long ylen = (m + 2) & ~1LL;
   L->y = 0;
   L->len.res_off = ylen;
   L->r.ints = res_arrays(ylen, 1, m, maxcuts, (long long) maxcuts * n, &L->r);
   L->r.smax = smax;
   L->len.res_len = even(L->r.ints + 2 - ylen);          /* three ints, and an even length */
   L->r.sup = ylen + L->len.res_len;
   L->Z = L->r.sup + even(((long long) maxcuts * smax + 1) / 2);
   L->ws = L->Z + hs_cut_mat_len(n);
   L->o1 = L->ws + even(ws_len);
   L->o2 = L->o1 + even(out_len);
   L->MT = L->o2 + out_vec;
   L->len.upload_len = m;
   L->len.pin_len = ylen + (L->len.res_len > out_vec ? L->len.res_len : out_vec);      /* maxcuts = 0 reads the head of o1 back */
   L->len.dev_len = L->MT + hs_cut_mat_len(n);
}

void hs_ova_layout_make(int m, int count, int tabw, int resw, long long z_len, int mid_grid, int mid_nmax, hs_ova_layout* L)
{
   L->u = 0;
   L->tab = even(m);
   L->res = L->tab + (long long) count * tabw;
   L->Z = even(L->res + (long long) count * resw);
   L->slabs = L->Z + even(z_len);
   L->len.res_off = L->res; L->len.res_len = (long long) count * resw;
   L->len.upload_len = L->res; L->len.pin_len = L->res + L->len.res_len;
   L->len.dev_len = L->slabs + 2LL * mid_grid * mid_nmax * mid_nmax;
}

void hs_ovl_layout_make(int m, int count, int tabw, int jobw, int resw, int statew, long long z_len, const long long* ws_len,
   const long long* out_len, long long* ws, long long* out, hs_ovl_layout* L)
{
   L->u = 0;
   L->tab = even(m);
   L->jobs = even(L->tab + (long long) count * tabw);
   L->act = even(L->jobs + (long long) count * jobw);
   L->nactive = L->act + even(((long long) count + 1) / 2);
   L->res = L->nactive + 2;
   L->state = even(L->res + (long long) count * resw);
   L->Z = even(L->state + (long long) count * statew);
   L->slabs = L->Z + even(z_len);
   long long at = L->slabs;
   for (int k = 0; k < count; ++k)
   {
      ws[k] = at;
      at += even(ws_len[k]);
      out[k] = at;
      at += even(out_len[k]);
   }
   L->len.res_off = L->res; L->len.res_len = (long long) count * resw;
   L->len.upload_len = L->res; L->len.pin_len = L->res + L->len.res_len;
   L->len.dev_len = at;
}

hs_sclr_block hs_sclr_block_make(int n, int ns, long long scratch, long long ws_len, long long out_len)
{
   hs_sclr_block B;
   B.st = 0;
   B.v0 = HS_SCR_STATE_LEN;
   B.Z = B.v0 + even(n);
   B.MT = B.Z + hs_cut_mat_len(n);
   B.ZS = B.MT + hs_cut_mat_len(n);
   B.wsS = B.ZS + (ns > 0 ? hs_cut_mat_len(ns) : 0);
   B.ws = B.wsS + (ns > 0 ? even(scratch) : 0);
   B.out = B.ws + even(ws_len);
   B.len = B.out + even(out_len);
   return B;
}

void hs_sclr_layout_make(int nb, int m, int maxcuts, int smax, long long vec_len, int count, int jobw, int xjobw, int sjobw,
   long long blocks_len, hs_sclr_layout* L)
{
   L->y = 0;
   L->sizes = even(m);
   L->jobs = L->sizes + even(((long long) nb + 1) / 2);
   L->xjobs = L->jobs + even((long long) count * jobw);
   L->sjobs = L->xjobs + even((long long) count * xjobw);
   L->act = L->sjobs + even((long long) count * sjobw);
   L->len.res_off = L->act + even(((long long) count + 1) / 2);
   L->r.ints = res_arrays(L->len.res_off, nb, m, maxcuts, vec_len, &L->r);
   L->r.smax = smax;
   L->r.sup = L->r.ints + (3LL * nb + 1) / 2;
   L->blocks = even(L->r.sup + ((long long) nb * maxcuts * smax + 1) / 2);
   L->len.res_len = L->r.sup - L->len.res_off;
   L->len.upload_len = L->len.res_off; L->len.pin_len = L->r.sup; L->len.dev_len = L->blocks + blocks_len;
}

void hs_cm_layout_make(int m, int cc, int group, int nsv, int nlarge, int blkw, int jobw, long long blocks_len, hs_cm_layout* L)
{
   const long long groups = ((long long) cc + group - 1) / group, jobs = (long long) cc * nlarge;
   L->Yg = 0;
   L->blks = even(groups * m * group);
   L->jobs = L->blks + even((long long) nsv * blkw);
   L->act = L->jobs + even(jobs * jobw);
   L->res = L->act + even((jobs + 1) / 2);
   L->lam = L->res + even((long long) cc * nsv + cc);
   L->blocks = L->lam + 2LL * cc * (nsv - nlarge);
   L->len.res_off = L->res; L->len.res_len = L->lam - L->res;
   L->len.upload_len = L->res; L->len.pin_len = L->lam; L->len.dev_len = L->blocks + blocks_len;
}

void hs_r1_layout_make(int m, int cc, int group, int nsv, int nlarge, int blkw, int jobw, int resw, long long blocks_len, hs_cm_layout* L)
{
   hs_cm_layout_make(m, cc, group, nsv, nlarge, blkw, jobw, blocks_len, L);
   L->lam = L->res + even((long long) cc * nsv * resw);
   L->blocks = L->lam + 4LL * cc * (nsv - nlarge);
   L->len.res_len = L->lam - L->res;
   L->len.pin_len = L->lam; L->len.dev_len = L->blocks + blocks_len;
}

hs_ecl_block hs_ecl_block_make(long long ws_len, long long out_len)
{
   hs_ecl_block B;
   B.ws = 0;
   B.out = even(ws_len);
   B.len = B.out + even(out_len);
   return B;
}

void hs_ecl_layout_make(int nb, int m, int maxcuts, long long vec_len, int count, int jobw, long long blocks_len, hs_ecl_layout* L)
{
   L->y = 0;
   L->jobs = even(m);
   L->vecoff = L->jobs + even((long long) count * jobw);
   L->act = L->vecoff + even(count);
   L->len.res_off = L->act + even(((long long) count + 1) / 2);
   L->r.ints = even(res_arrays(L->len.res_off, nb, m, maxcuts, vec_len, &L->r));
   L->r.sup = L->r.ints + even((3LL * nb + 1) / 2);            /* (no supports: where the result ends) */
   L->blocks = L->r.sup;
   L->len.res_len = L->r.sup - L->len.res_off;
   L->len.upload_len = L->len.res_off; L->len.pin_len = L->r.sup; L->len.dev_len = L->blocks + blocks_len;
}
