"""Case table of tests/test_gpu_small_path.py: the shapes at which the small-problem passes of scip-sdp_amd/csrc/kernels.hip and their
recorded forms inside k_red_batch take another path.  Every case names the branch it is there for and carries a predicate over the
constants of the sources (read from their #define lines) that says it reaches that branch; tests/test_small_path_cases_cpu.py evaluates
the predicates, so that a later change of RB_ROWS or RB_MAXWORK fails there instead of silently moving a case off its branch.

A case is a dict: op, branch, pred (a function of the constants K), records (">=1": the recorded form must have run; 0: the call
declines and is launched) and the parameters of the operation."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "scip-sdp_amd", "csrc")
NAMES = ("RB_MAX", "RB_MAXN", "RB_ROWS", "RB_MATS", "RB_MAXWORK", "HS_SMALL_N", "HS_AS_MAXBLK", "DB_PR", "DB_PC", "RED_STAGE_N")


def constants():
    text = ""
    for f in ("kernels.hip", "hs_kernels.h", "hs_lds_product.h"):
        with open(os.path.join(CSRC, f)) as fh:
            text += fh.read()
    K = {}
    for nm in NAMES:
        found = set(re.findall(r"^#define[ \t]+%s[ \t]+(\d+)\b" % nm, text, re.M))
        assert len(found) == 1, "%s: expected one #define with a number, found %s" % (nm, sorted(found))
        K[nm] = int(found.pop())
    return K


CASES = []


def case(op, branch, pred, records=">=1", **par):
    c = dict(op=op, branch=branch, pred=pred, records=records)
    c.update(par)
    c["id"] = "%s-%s-%s" % (op, branch, "-".join("%s%s" % (k, str(v).replace(" ", "")) for k, v in sorted(par.items())))
    CASES.append(c)


# ---- hs_dir_block_small / RB_DIRBLK: one entry per thread up to n^2 = 256, above it a DB_PR x DB_PC patch per thread -----------------
def _tails(K, n):
    return n % K["DB_PR"], n % K["DB_PC"]


case("dir_block", "dirblk_single_entry", lambda K, n=1: n * n <= 256, n=1)
case("dir_block", "dirblk_entry_per_thread", lambda K, n=2: n * n <= 256, n=2)
case("dir_block", "dirblk_entry_per_thread", lambda K, n=15: n * n <= 256, n=15)
case("dir_block", "dirblk_entry_per_thread_last", lambda K, n=16: n * n == 256, n=16)
case("dir_block", "dirblk_patches_first", lambda K, n=17: (n - 1) ** 2 <= 256 < n * n <= K["HS_SMALL_N"] ** 2 and _tails(K, n) == (1, 2), n=17)
case("dir_block", "dirblk_patches_row_and_column_tail", lambda K, n=33: 256 < n * n and n <= K["HS_SMALL_N"] and _tails(K, n) == (1, 3), n=33)
case("dir_block", "dirblk_patches_row_and_column_tail", lambda K, n=47: 256 < n * n and n <= K["HS_SMALL_N"] and _tails(K, n) == (1, 2), n=47)
case("dir_block", "dirblk_largest", lambda K, n=48: n == K["HS_SMALL_N"] and _tails(K, n) == (0, 3), n=48)
DIR_BLOCK_TOO_LARGE = 49          # HS_ERR_ARG: checked by the CPU test to be HS_SMALL_N + 1


# ---- hs_lp_rows_small / RB_LPROWS: rows are staged RB_ROWS at a time; m1 <= 64 is straight-line (a wavefront and eight rows per step:
# 32 rows per trip of its loop), above it every lane sum is a strided loop ----------------------------------------------------------
def _lp_ok(K, q, m1):
    return q * m1 <= K["RB_MAXWORK"]


for m1 in (1, 2, 63, 64):
    for q in (1, 4, 5, 31):
        case("lp_rows", "lprows_straight_one_trip", lambda K, q=q, m1=m1: m1 <= 64 and q <= 32 and q <= K["RB_ROWS"] and _lp_ok(K, q, m1), q=q, m1=m1)
    for q in (33, 63, 64):
        case("lp_rows", "lprows_straight_second_trip", lambda K, q=q, m1=m1: m1 <= 64 and 32 < q <= K["RB_ROWS"] and _lp_ok(K, q, m1), q=q, m1=m1)
    for q in (65, 129):
        case("lp_rows", "lprows_straight_full_pass_and_more", lambda K, q=q, m1=m1: m1 <= 64 and q > K["RB_ROWS"] and _lp_ok(K, q, m1), q=q, m1=m1)
for m1 in (65, 127, 129):
    for q in (1, 4, 5, 31, 33, 63, 64, 65, 129):
        if (q, m1) != (129, 129):
            case("lp_rows", "lprows_strided", lambda K, q=q, m1=m1: m1 > 64 and _lp_ok(K, q, m1), q=q, m1=m1)
case("lp_rows", "lprows_declines", lambda K: 129 * 129 > K["RB_MAXWORK"], records=0, q=129, m1=129)
case("lp_rows", "lprows_declines_just_above", lambda K: 257 * 64 > K["RB_MAXWORK"] >= 256 * 64, records=0, q=257, m1=64)
case("lp_rows", "lprows_recorded_just_below", lambda K: 256 * 64 <= K["RB_MAXWORK"] < 257 * 64, q=256, m1=64)


# ---- hs_apply_A_small / RB_APPLYA: matrices are staged RB_MATS at a time; one block of at most 256 entries with at most 256 LP rows is
# straight-line (eight matrices per step), everything else the general loops; more than two blocks are not recorded ----------------
def _aa_work(K, n2, q, m1):
    return (sum(n2) + q) * m1 <= K["RB_MAXWORK"]


def _aa_straight(K, n2, q, m1):
    return len(n2) == 1 and n2[0] <= 256 and q <= 256 and _aa_work(K, n2, q, m1)


def _aa_general(K, n2, q, m1):
    return len(n2) <= 2 and not (len(n2) == 1 and n2[0] <= 256 and q <= 256) and _aa_work(K, n2, q, m1)


for n2 in (1, 255, 256):
    for q in (0, 1, 255, 256):
        case("apply_A", "applya_straight", lambda K, n2=n2, q=q: _aa_straight(K, (n2,), q, 9) and 9 % 8 != 0, n2=(n2,), q=q, m1=9)
case("apply_A", "applya_general_long_block", lambda K: _aa_general(K, (257,), 3, 9) and 257 > 256, n2=(257,), q=3, m1=9)
case("apply_A", "applya_general_many_lp_rows", lambda K: _aa_general(K, (9,), 257, 9) and 257 > 256, n2=(9,), q=257, m1=9)
case("apply_A", "applya_two_blocks", lambda K: _aa_general(K, (289, 9), 0, 9), n2=(289, 9), q=0, m1=9)
case("apply_A", "applya_two_blocks", lambda K: _aa_general(K, (289, 9), 7, 33), n2=(289, 9), q=7, m1=33)
case("apply_A", "applya_three_blocks_decline", lambda K: 3 > 2 and 3 <= K["HS_AS_MAXBLK"], records=0, n2=(16, 9, 4), q=3, m1=5)
case("apply_A", "applya_eight_blocks_decline", lambda K: 8 == K["HS_AS_MAXBLK"], records=0, n2=(4, 1, 9, 16, 4, 25, 1, 9), q=0, m1=3)
for form, n2, q in (("straight", (9,), 5), ("general", (16, 9), 3)):
    ok = _aa_straight if form == "straight" else _aa_general
    case("apply_A", "applya_%s_no_epilogue_row" % form, lambda K, ok=ok, n2=n2, q=q: ok(K, n2, q, 1), n2=n2, q=q, m1=1)
    for m1 in (2, 31):
        case("apply_A", "applya_%s_unroll_tail" % form, lambda K, ok=ok, n2=n2, q=q, m1=m1: ok(K, n2, q, m1) and m1 < K["RB_MATS"] and m1 % 8 != 0, n2=n2, q=q, m1=m1)
    case("apply_A", "applya_%s_one_full_stage" % form, lambda K, ok=ok, n2=n2, q=q: ok(K, n2, q, 32) and 32 == K["RB_MATS"], n2=n2, q=q, m1=32)
    case("apply_A", "applya_%s_stage_tail_of_one" % form, lambda K, ok=ok, n2=n2, q=q: ok(K, n2, q, 33) and 33 == K["RB_MATS"] + 1, n2=n2, q=q, m1=33)
    case("apply_A", "applya_%s_two_full_stages" % form, lambda K, ok=ok, n2=n2, q=q: ok(K, n2, q, 64) and 64 == 2 * K["RB_MATS"], n2=n2, q=q, m1=64)
    case("apply_A", "applya_%s_third_stage" % form, lambda K, ok=ok, n2=n2, q=q: ok(K, n2, q, 65) and 65 == 2 * K["RB_MATS"] + 1, n2=n2, q=q, m1=65)
case("apply_A", "applya_recorded_just_below", lambda K: 256 * 64 <= K["RB_MAXWORK"] < 257 * 64 and _aa_straight(K, (256,), 0, 64), n2=(256,), q=0, m1=64)
case("apply_A", "applya_declines_just_above", lambda K: 257 * 64 > K["RB_MAXWORK"] >= 256 * 64, records=0, n2=(256,), q=1, m1=64)


# ---- hs_gemv_t / RB_GEMVT: one thread per entry (stride 256), rows eight at a time and a tail -------------------------------------
def _gt_ok(K, R, E):
    return E <= K["RB_MAXN"] and R * E <= K["RB_MAXWORK"]


for R in (1, 7, 8, 9, 17):
    rb = "rows_tail_only" if R < 8 else ("rows_eight" if R == 8 else "rows_eight_and_tail")
    rp = (lambda R: R < 8) if R < 8 else ((lambda R: R == 8) if R == 8 else (lambda R: R > 8 and R % 8 != 0))
    for E in (1, 255, 257):
        eb = "one_entry" if E == 1 else ("one_trip" if E <= 256 else "second_trip")
        ep = (lambda E: E == 1) if E == 1 else ((lambda E: 1 < E <= 256) if E <= 256 else (lambda E: E > 256))
        case("gemv_t", "gemvt_%s_%s" % (rb, eb), lambda K, R=R, E=E, rp=rp, ep=ep: _gt_ok(K, R, E) and rp(R) and ep(E), R=R, E=E)
case("gemv_t", "gemvt_recorded_just_below", lambda K: 16 * 1024 <= K["RB_MAXWORK"] < 17 * 964 and 1024 <= K["RB_MAXN"], R=16, E=1024)
case("gemv_t", "gemvt_declines_just_above", lambda K: 17 * 964 > K["RB_MAXWORK"] >= 17 * 963, records=0, R=17, E=964)


# ---- the four reductions: recorded up to RB_MAXN entries; runs of up to four with distinct outputs and at most 1024 entries each go
# one per wavefront (rb_run_wave), everything else through the whole workgroup (rb_run).  The fills of the slots are records too. -----
def _red_groups(K, lens, slots):
    """the groups k_red_batch forms over a run of reductions: the while loop in front of its switch"""
    groups, t = [], 0
    while t < len(lens):
        g = 0
        while g < 4 and t + g < len(lens) and lens[t + g] <= 1024 and slots[t + g] not in slots[t:t + g]:
            g += 1
        g = max(g, 1)
        groups.append(g)
        t += g
    return groups


def _red_all_recorded(K, lens, nslots):
    return all(n <= K["RB_MAXN"] for n in lens) and nslots + len(lens) <= K["RB_MAX"]


def red(branch, pred, lens, slots, acc, nslots, records=">=1", positive_d=False):
    case("reductions", branch, pred, records=records, lens=tuple(lens), slots=tuple(slots), acc=tuple(acc), nslots=nslots, positive_d=positive_d)


def _red_stages(K, L):
    """workgroups of the launch's first stage; above one, a second stage combines their partial results and the record re-enacts both"""
    return -(-L // K["RED_STAGE_N"])


for L in (1, 63, 64, 65, 255, 256, 257, 1024, 1025):
    for a in (0, 1):
        red("red_workgroup_form" + ("_accumulate" if a else ""),
            lambda K, L=L: _red_all_recorded(K, (L,), 2) and _red_groups(K, (L,), (0,)) == [1] and _red_stages(K, L) == 1, (L,), (0,), (a,), 2)
# (2048: the longest one-stage launch; 2049: two workgroups, the second with one entry; 5000: three, the last one short in its second
# trip; 16384: RB_MAXN / RED_STAGE_N full ones)
red("red_one_stage_longest", lambda K: _red_stages(K, 2048) == 1 and _red_stages(K, 2049) == 2 and _red_all_recorded(K, (2048,), 2), (2048,), (0,), (0,), 2)
for L, g in ((2049, 2), (5000, 3), (16384, 8)):
    for a in (0, 1):
        red("red_two_stage_form" + ("_accumulate" if a else ""), lambda K, L=L, g=g: _red_all_recorded(K, (L,), 2) and _red_stages(K, L) == g,
            (L,), (0,), (a,), 2)
red("red_longest_recorded", lambda K: 16384 == K["RB_MAXN"], (16384,), (1,), (0,), 2)
red("red_not_recorded", lambda K: 16385 == K["RB_MAXN"] + 1, (16385,), (0,), (0,), 2, records=0)
red("red_group_of_four", lambda K: _red_groups(K, (5, 64, 257, 1024), (0, 1, 2, 3)) == [4] and _red_all_recorded(K, (5, 64, 257, 1024), 4),
    (5, 64, 257, 1024), (0, 1, 2, 3), (0, 0, 0, 0), 4)
red("red_group_of_four_then_one", lambda K: _red_groups(K, (1, 63, 65, 255, 256), (0, 1, 2, 3, 4)) == [4, 1] and _red_all_recorded(K, (1, 63, 65, 255, 256), 5),
    (1, 63, 65, 255, 256), (0, 1, 2, 3, 4), (0, 0, 0, 0, 0), 5)
red("red_group_accumulates", lambda K: _red_groups(K, (64, 65, 3), (2, 0, 1)) == [3], (64, 65, 3), (2, 0, 1), (1, 1, 1), 3)
red("red_same_slot_not_grouped", lambda K: _red_groups(K, (64, 65), (0, 0)) == [1, 1], (64, 65), (0, 0), (0, 1), 1)
red("red_short_then_long_not_grouped", lambda K: _red_groups(K, (63, 1025), (0, 1)) == [1, 1] and 1025 <= K["RB_MAXN"], (63, 1025), (0, 1), (0, 0), 2)
# (17 fills and 7 reductions fill the batch: it is launched when the eighth reduction arrives, which then waits alone)
red("red_mid_batch_flush", lambda K: 17 + 8 == K["RB_MAX"] + 1 and _red_groups(K, (3, 64, 65, 255, 7, 256, 257), tuple(range(7))) == [4, 3],
    (3, 64, 65, 255, 7, 256, 257, 9), tuple(range(8)), (0, 1, 0, 1, 0, 1, 0, 1), 17)
red("red_ratio_min_without_negative_direction", lambda K: True, (65,), (0,), (0,), 1, positive_d=True)


# ---- the small solves with the factor of M: RB_SOLVE (form 0, every row split over four lanes) and k_solve2_small (form 1) -------------
for m in (1, 2, 3, 4, 5, 31, 63, 64):
    br = "solve_fewer_rows_than_lanes_of_a_row" if m < 4 else ("solve_full_tile" if m == 64 else "solve_rows_over_four_lanes")
    pr = (lambda m: m < 4) if m < 4 else ((lambda m: m == 64) if m == 64 else (lambda m: 4 <= m < 64))
    case("solve", br, lambda K, m=m, pr=pr: m <= 64 and pr(m), m=m)


# ---- hs_gemv_t3: E and lda even; rows eight at a time, then four, then one; 256 threads of two entries per workgroup ------------------
def _t3_rows(R):
    return (R // 8, (R % 8) // 4, R % 4)


for R, rows in ((1, (0, 0, 1)), (3, (0, 0, 3)), (4, (0, 1, 0)), (7, (0, 1, 3)), (8, (1, 0, 0)), (9, (1, 0, 1)), (12, (1, 1, 0)), (13, (1, 1, 1))):
    for E, eb, ep in ((2, "one_thread", lambda E: E == 2), (510, "partial_workgroup", lambda E: 2 < E < 512), (512, "full_workgroup", lambda E: E == 512),
                      (514, "second_workgroup", lambda E: E > 512)):
        case("gemv_t3", "t3_rows_%d_%d_%d_%s" % (rows + (eb,)), lambda K, R=R, rows=rows, E=E, ep=ep: _t3_rows(R) == rows and E % 2 == 0 and ep(E), R=R, E=E)
case("gemv_t3", "t3_declines_odd_E", lambda K: 511 % 2 == 1, records=0, R=9, E=511, lda=512)
case("gemv_t3", "t3_declines_odd_lda", lambda K: 511 % 2 == 1 and 510 % 2 == 0, records=0, R=9, E=510, lda=511)


# ---- hs_gemv_n (pass A): the launcher's rule (gemv_n_launch), restated ---------------------------------------------------------------
def gemvn_plan(R, E, lda, nv, voff, ws):
    """-> (slices, two-at-a-time kernel, lengths of the slices)"""
    vec = lda % 2 == 0 and voff % 2 == 0
    ns = 1
    if R < 512 and E >= 16384:
        ns = max(1, min((1024 + R - 1) // R, E // 8192))
        if ns * nv * R > ws:
            ns = 1
    chunk = (E + ns - 1) // ns
    chunk = (chunk + 1) & ~1
    return ns, vec, [min(E, (k + 1) * chunk) - k * chunk for k in range(ns)]


def pa(branch, pred, R, E, lda, nv, voff=0, ws=0):
    case("pass_a", branch, lambda K: pred(*gemvn_plan(R, E, lda, nv, voff, ws)), R=R, E=E, lda=lda, nv=nv, voff=voff, ws=ws)


for nv in (1, 2, 4):
    pa("gemvn_scalar_odd_pitch", lambda ns, vec, ln: ns == 1 and not vec, 150, 201, 201, nv)
pa("gemvn_scalar_unaligned_vector", lambda ns, vec, ln: ns == 1 and not vec, 20, 300, 300, 2, voff=1)
pa("gemvn_vector_one_slice", lambda ns, vec, ln: ns == 1 and vec and ln[0] % 2 == 0, 20, 300, 304, 2, voff=2)
pa("gemvn_vector_one_slice_odd_tail", lambda ns, vec, ln: ns == 1 and vec and ln[0] % 2 == 1, 20, 301, 304, 1)
pa("gemvn_vector_split", lambda ns, vec, ln: ns == 2 and vec and all(v % 2 == 0 for v in ln), 37, 16384, 16384, 1, ws=2 * 37)
pa("gemvn_vector_split", lambda ns, vec, ln: ns == 4 and vec and all(v % 2 == 0 for v in ln), 300, 40000, 40000, 2, ws=4 * 2 * 300)
pa("gemvn_scalar_split", lambda ns, vec, ln: ns == 4 and not vec and ln[-1] < ln[0], 300, 40001, 40001, 1, ws=4 * 300)
pa("gemvn_workspace_too_short_for_split", lambda ns, vec, ln: ns == 1 and vec, 37, 16384, 16384, 4, ws=2 * 4 * 37 - 1)
pa("gemvn_vector_split_chunk_rounded_up", lambda ns, vec, ln: ns == 2 and vec and ln[0] == 8194 and ln[1] == 8192, 37, 16386, 16386, 1, ws=2 * 37)
pa("gemvn_vector_split_odd_tail", lambda ns, vec, ln: ns == 2 and vec and ln[1] % 2 == 1, 37, 16385, 16386, 1, ws=2 * 37)


def cases(op):
    return [c for c in CASES if c["op"] == op]


def ids(op):
    return [c["id"] for c in cases(op)]


# every branch the table is meant to cover (tests/test_small_path_cases_cpu.py: each has at least one case)
BRANCHES = (
    "dirblk_single_entry", "dirblk_entry_per_thread", "dirblk_entry_per_thread_last", "dirblk_patches_first",
    "dirblk_patches_row_and_column_tail", "dirblk_largest",
    "lprows_straight_one_trip", "lprows_straight_second_trip", "lprows_straight_full_pass_and_more", "lprows_strided", "lprows_declines",
    "lprows_declines_just_above", "lprows_recorded_just_below",
    "applya_straight", "applya_general_long_block", "applya_general_many_lp_rows", "applya_two_blocks", "applya_three_blocks_decline",
    "applya_straight_no_epilogue_row", "applya_straight_unroll_tail", "applya_straight_one_full_stage", "applya_straight_stage_tail_of_one",
    "applya_straight_two_full_stages", "applya_straight_third_stage", "applya_general_no_epilogue_row", "applya_general_unroll_tail",
    "applya_general_one_full_stage", "applya_general_stage_tail_of_one", "applya_general_two_full_stages", "applya_general_third_stage",
    "applya_recorded_just_below", "applya_declines_just_above",
    "gemvt_rows_tail_only_one_entry", "gemvt_rows_eight_one_trip", "gemvt_rows_eight_and_tail_second_trip", "gemvt_recorded_just_below",
    "gemvt_declines_just_above",
    "red_workgroup_form", "red_workgroup_form_accumulate", "red_longest_recorded", "red_not_recorded", "red_group_of_four",
    "red_group_of_four_then_one", "red_group_accumulates", "red_same_slot_not_grouped", "red_short_then_long_not_grouped",
    "red_mid_batch_flush", "red_ratio_min_without_negative_direction",
    "solve_fewer_rows_than_lanes_of_a_row", "solve_rows_over_four_lanes", "solve_full_tile",
    "t3_rows_0_0_1_one_thread", "t3_rows_0_1_3_partial_workgroup", "t3_rows_1_0_0_full_workgroup", "t3_rows_1_1_1_second_workgroup",
    "t3_declines_odd_E", "t3_declines_odd_lda",
    "gemvn_scalar_odd_pitch", "gemvn_scalar_unaligned_vector", "gemvn_vector_one_slice", "gemvn_vector_one_slice_odd_tail",
    "gemvn_vector_split", "gemvn_scalar_split", "gemvn_workspace_too_short_for_split", "gemvn_vector_split_chunk_rounded_up",
    "gemvn_vector_split_odd_tail",
)
