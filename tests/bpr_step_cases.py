"""Inputs, references and checks of the hogwild BPR step tests, in ONE place: tests/test_bpr_step_gpu.py runs the cases on
the device, tests/test_bpr_step_cpu.py proves — from the restatements and the float64 step alone — that every case is a
fair test, that the tolerances below follow their rules, and that the checks reject nine deliberately wrong updates (and,
for the conveyor's block buffers, four wrong uses of them; for the XCD-strata form, seven wrong merges, write paths and
lane masks of its own, and two wrong racy rows; for the resident exchange, eight wrong protocols of publishing and applying).

A case = Zipf interactions + normal tables with real scores (z well away from 0.5) + ONE launch of `n` samples at sample
offset `s_begin` of epoch 0 (conveyor cases: ONE conveyor_enqueue over 1 to 8 blocks, whose item rows live in block
buffers: `pack` / `unpack` / `conveyor_tables`), whose non-skipped triplets oracle.hogwild_triplets names before anything
runs.  The launch is made three times from the same start tables:

  Z  lr = 0             tables bit-identical; skip counter == the restatement's; `correct` == #(x > 0) in float64, give or
                        take the triplets whose |x| is below the float32 score's a-priori error bound
  A  lr = 0.05          rows of CLEAN triplets (no row shared with another triplet of the launch) == the float64 step
     reg = 0.01         within T_CLEAN; rows no triplet touches (those beyond n_items, every bias without use_bias) bit-identical
  B  lr = 2^-12         EVERY touched row: |got - start - jacobi sum| <= C[case] x path + floor (Euclidean over the row),
     reg = 0.01         path = sum over the row's triplets of |delta|, floor = touches x ulp(max |row|) / 2 x sqrt(k)

T_CLEAN.  Rule: 4 x the largest |float32 step - float64 step| over the clean rows of all cases (the device sums the dot
product in DPP / butterfly order and uses __expf and __frcp_rn), rounded up to one significant digit.

C[case].  Rule: 4 x the largest |sequential - jacobi| / path over all touched rows and three orders of application (the
restatement's and two seeded permutations), float64, rounded up to one significant digit.  It is the share of a row's
path by which ANY order of exact updates may differ from the Jacobi sum, so it bounds a correct kernel whatever its
scheduling; a lost or doubled update moves a row by path / touches, visible where that exceeds 2 x the tolerance.
tests/test_bpr_step_cpu.py asserts both rules and prints every figure.

The XCD-strata form (csrc/bpr_strata.inc; a launch = one or two whole phases of an epoch) stores its cold item rows with
plain read-modify-write among the CUs of one XCD, by design: of two waves that touch such a row in one phase, one may
overwrite the other's store.  Launch B therefore holds a strata case under TWO rules (check_b_strata), the rows' classes
decided on the CPU from the triplets alone: every U row, every hot item row and every cold item row that ONE wave per
phase touches, each with its bias, under the rule above, unchanged — that class carries the in-step merge (UNR triplets
of a wave share one load of a row; its lead reference stores every delta of the step) and the same-wave store-then-load
order; a cold item row that two or more waves of a phase touch under the racy rule (racy_rows): element by element,
got - start within tolerance / sqrt(k) of the sum of a non-empty subset of the row's (phase, wave, step) groups.

The resident exchange (the EXCH instantiations of csrc/bpr_ldsbin.inc; a launch = the WHOLE epoch, driven through
cornac_amd.dist.ShardedBprTrainer on one rank without a process group) is held under launch Z, A and B as above and, in
launch B, under a second rule on what the launch PUBLISHES (check_exch_b): P = sum over the exchanges of keeps + (table -
base) is what the other ranks receive plus what the closing exchange still owes them, and every touched item row and bias
of P lies within tolerance_b of the Jacobi sum, n_ex more roundings in its floor term; only hot rows may differ from their
base afterwards, bucket e holds keep e (twice it where a twin rank is played on the communication stream) with the rule's
weights, and base - start is the sum of the keeps.  With a twin under the "sqrt" rule the corrections c = rule(S) - keep are
not zero and reach a row whenever the run lets them: the table rule gives way to the accounting, from the buffers read
back — table - start - sum c = P and base - start - sum c = sum keeps — and P is held to the Jacobi sum under a C of its own.
"""
import functools

import numpy as np

from cornac_amd import _lib, synth
from oracle import bpr_step_oracle as step
from oracle import oracle as orc

MI355X_CUS = 256
LR_A, LR_B, REG = 0.05, 2.0 ** -12, 0.01

# ---- measured (tests/test_bpr_step_cpu.py prints the CPU figures, tests/test_bpr_step_gpu.py the MI355X ones) ------------
# float32 step vs float64 step over the clean rows of all cases: 1.17e-7 (fused_k3, whose rows reach 2.1: ulp / 2 = 1.2e-7;
#   5e-8 .. 1e-7 elsewhere)  ->  T_CLEAN = 5e-7.
# |sequential - jacobi| / path, three orders: 0.0027 .. 0.0054 for the 2 048-sample launches with biases (0.0007 .. 0.0011
#   without: the bias deltas are what moves a score most), 0.030 / 0.035 passing, 0.035 wide, 0.0053 / 0.0058 owned (one
#   tile of each of 4 096 / 6 144 waves: 262 138 / 393 207 triplets)  ->  C below.
# MI355X, launch Z: `correct` inside the float64 interval in every case (the interval is one number in 21 of 27 cases).
# MI355X, launch A, largest |got - float64 step| over clean rows: U 6.0e-8, V 1.17e-7 (fused_k3), B 8.6e-8 — the float32
#   step's own error, a quarter of T_CLEAN.
# MI355X, launch B, largest error / tolerance over touched rows: U 0.18, V 0.26, B 0.41 (owned_k100; 0.39 lds_k64) — the
#   device is one more order of application, a quarter of C like the three measured ones.  Owned kernel, error / PATH:
#   U 0.0035 / 0.0046, V 0.0080 / 0.0058, B 0.033 / 0.022 (k = 64 / 100).  The bias figure belongs to rows touched ONCE whose
#   delta lr (z - reg b) is small (z = 0.01: path 1e-6) beside the rounding of its one float32 add onto |b| = 1.4 (3.4e-8,
#   under ulp / 2 = 6e-8): that is the floor term of the tolerance; net of it the bias rows lie within 0.0041 / 0.0049 of
#   their path, like U, V and the float64 orders.
# Conveyor (cornac_hip_bpr_conveyor_enqueue; a launch = the whole epoch of its blocks' bins, 1 527 .. 3 234 triplets):
#   float32 step vs float64 step over the clean rows 2.9e-8 .. 6.1e-8; |sequential - jacobi| / path, three orders: 0.0023
#   (k = 40) .. 0.0056 (k = 256, popularity), 0.0065 heavy  ->  C = 0.01 .. 0.03 below.  33 .. 37 % of the triplets clean (a
#   bin draws its positives with replacement: at most 1 / e can be), 1 % with popularity negatives, 12 % heavy.
# MI355X, conveyor: `correct` inside the float64 interval in all 15 cases (one number in 13); launch A, clean rows: U 5.9e-8,
#   V 5.9e-8, B 6.1e-8; launch B, error / tolerance: U 0.14, V 0.22 (conv_k40), B 0.59 (conv_k192; 0.43 conv_k40, 0.40
#   conv_ranges8_k64: rows touched once, the floor term as above); layouts equal to the oracle's, no lock time-outs.
# XCD strata (one phase of 4 096 / 5 120 / 7 168 waves at k <= 64 / <= 192 / above: 65 158 .. 65 961 triplets, two phases 131 000):
#   float32 step vs float64 step over the clean rows 5.9e-8 .. 8.5e-8 (T_CLEAN stays); |sequential - jacobi| / path, three
#   orders: 0.0046 .. 0.0097 (0.0137 two phases at k = 64, 0.0196 strata_rehash2_k100)  ->  C = 0.02 .. 0.08 below.  14 % of the
#   triplets clean (6 % at 100 000 x 200 000, 20 % at 1 048 583 items); racy rows 10.6 .. 10.9 % of the touched item rows (13.2 %
#   without hot items, 12.1 % over two phases, 23.2 % at 200 000 items, 4.1 % at 1 048 583), 2 .. 11 groups each; at UNR = 4 /
#   2 some 4 200 / 2 000 steps name a cold item twice and 7 900 / 4 200 repeat an exclusive user, 3 000 / 2 500 are partial.
# MI355X, strata: `correct` inside the float64 interval in all 16 cases (one number in 2); launch A, clean rows: U 6.1e-8,
#   V 6.1e-8, B 8.5e-8; launch B, exact rule, error / tolerance: U 0.15 (strata_k33), V 0.19 (strata_k128), B 0.80
#   (strata_k64; 0.75 strata_partial_k64); racy rule: every racy row passes; ONE
#   subset explains 94 .. 97 % of them as a whole (9 585 of 9 991 at k = 64, 18 300 of 19 377 at k = 200: on the others the
#   elements of one row come from different subsets, so two waves' stores of a row interleave below the row), and a third
#   lost at least one group at UNR = 4 (3 342 of 9 991; 31 .. 35 % over the cases), 20 .. 24 % at UNR = 2, 13 % at UNR = 1 (2 529 of 19 377) — a phase of
#   these launches is one tile per wave, every wave of the grid at once; packed and unpacked records alike (6 695 / 6 845 of
#   20 424 at k = 64).  Hot set, epoch key and bucket tables equal to their restatements; misplaced workgroups 0 in every case.
# Resident exchange (a launch = the whole epoch: 299 977 .. 299 999 triplets, 1 .. 23 draws skipped; plans 1 024 bins of 293 / 157 / 108
#   / 79 rows, 256 bins of 256 / 257; 2.5 (300 000 items) .. 9.2 (65 536) touches of a touched item row; 60 .. 103 triplets with a hot
#   positive on 1 .. 3 hot items, 508 .. 547 on 19 at k = 100, 1 268 / 1 371 on 46 at k = 192, 2 853 / 2 933 on 101 at k = 200 / 256;
#   0 .. 1 398 clean triplets): float32 step vs float64 step over the clean rows 2.8e-8 .. 6.1e-8; |sequential - jacobi| / path,
#   three orders: 0.0020 without biases, 0.0052 .. 0.0100  ->  C = 0.009, 0.03 .. 0.04; the "sqrt" twin, |P - jacobi| / path over three
#   host runs of the protocol (an exchange applied 0, 1, n_ex boundaries after its publication): 0.0097  ->  C = 0.04 (the order
#   share of that case alone: 0.0075).  One lost update shows on >= 0.82 of the touched rows of every table (n_ex = 32 and the twin,
#   C = 0.04 over 9.2 touches; 0.92 at k = 192 / 256 with popularity negatives; >= 0.95 elsewhere).
# MI355X, resident exchange: `correct` inside the float64 interval in all 17 cases; launch A, clean rows: U 5.9e-8, V 5.7e-8, B
#   6.1e-8; launch B, table rule, error / tolerance: U 0.24 (exch_k40), V 0.24, B 0.92 (exch_k64: bias rows touched once, the floor
#   term as above; 0.35 and less elsewhere); published-delta rule: V 0.21, B 0.24 (exch_pop_k256); base - start - sum of keeps
#   within 0.2 of its floor, the twin accounting within 0.31 .. 0.38; "align" weights within 0.03 of (k + 2) 2^-24; exchanges applied
#   inside the launch: 0 .. 3 of 4, 1 .. 7 of 8, 0 .. 24 of 32, none of 11 (ex_per = 0) — the flush applies the others; rows apart
#   from their base afterwards: exactly the n_hot hot rows on the 1 024-bin plans, none on the 256-bin ones; no lock time-outs.
#   The floor of the identities takes max |row| = |start| + path (tolerance_b(reach=True)): with the start-and-end ulp a bias of
#   5e-6 carried to 1e-4 and back missed it, 1.1e-11 against 2.5e-12 (exch_align_k100, bias 73 025), 9.1e-13 against 6.8e-13
#   (exch_pop_k256, bias 21 132) — float32 roundings at the ulp of where the row has been, which C x path covers in the rules.
T_CLEAN = 5e-7
C = {
    "fused_k3": 0.03, "fused_k7": 0.02, "fused_k16": 0.02, "fused_k20": 0.02,
    "fused_k50": 0.02, "fused_k100": 0.02, "fused_k192": 0.02, "fused_k200": 0.02,
    "fused_generic_k300": 0.02, "fused_vec4_k12": 0.02, "fused_vec4_k64": 0.02, "fused_dense_bias_k50": 0.02,
    "fused_nobias_k100": 0.003, "fused_pop_k16": 0.01, "lds_k40": 0.02, "lds_k64": 0.02,
    "lds_k100": 0.02, "lds_k192": 0.02, "lds_k200": 0.02, "lds_nobias_k64": 0.005,
    "lds_pop_k100": 0.007, "lds_partial_k64": 0.02, "lds_wide_k64": 0.2, "pass_k128": 0.2, "pass_k64": 0.2,
    "owned_k64": 0.03, "owned_k100": 0.03,
    "conv_k40": 0.01, "conv_k64": 0.02, "conv_k100": 0.02, "conv_k192": 0.03, "conv_k256": 0.02,
    "conv_pop_k64": 0.02, "conv_pop_k100": 0.02, "conv_pop_k192": 0.02, "conv_pop_k256": 0.03, "conv_nobias_k192": 0.02,
    "conv_ranges3_k100": 0.02, "conv_ranges8_k64": 0.02, "conv_pad_k64": 0.02, "conv_order_k64": 0.02, "conv_heavy_k64": 0.03,
    "strata_k33": 0.02, "strata_k64": 0.04, "strata_k100": 0.04, "strata_k128": 0.04, "strata_k192": 0.04, "strata_k200": 0.04,
    "strata_allhot_k64": 0.03, "strata_allhot_k100": 0.03, "strata_nohot_k64": 0.03, "strata_packed_k64": 0.06,
    "strata_packed_k100": 0.04, "strata_nobias_k100": 0.03, "strata_partial_k64": 0.03, "strata_epoch1_k64": 0.03,
    "strata_rehash2_k100": 0.08, "strata_auto_k33": 0.02,
    "exch_k64": 0.03, "exch_k100": 0.04, "exch_k192": 0.04, "exch_k200": 0.03, "exch_pop_k64": 0.03, "exch_pop_k100": 0.03,
    "exch_pop_k192": 0.04, "exch_pop_k256": 0.03, "exch_k40": 0.03, "exch_nobias_k64": 0.009, "exch_partial_k64": 0.03,
    "exch_one_k64": 0.03, "exch_ex32_k64": 0.04, "exch_short_k64": 0.03, "exch_align_k100": 0.03,
    "exch_twin_sqrt_k64": 0.04,  # (its own rule: the share of three host runs of the protocol, tests/test_bpr_step_cpu.py)
    "exch_twin_align_k100": 0.03,
}


def _fused(k, flags=0, **kw):
    return dict(dict(form="fused", k=k, nu=20_000, ni=30_720, nnz=300_000, zipf=0.8, n=2048,
                     flags=_lib.FORM_FUSED | _lib.HOG_NO_OWNERSHIP | flags), **kw)


def _owned(k, **kw):
    return dict(dict(form="owned", k=k, nu=200_000, ni=400_000, nnz=524_288, zipf=0.3, n=None, flags=_lib.HOG_FUSED_OPT_OUT,
                     clean_share=False), **kw)


def _lds(k, **kw):
    return dict(dict(form="ldsbin", k=k, nu=20_000, ni=30_720, nnz=300_000, zipf=0.8, n=2048, flags=_lib.FORM_LDSBIN), **kw)


def _exch(k, **kw):
    """ONE resident-exchange launch (csrc/bpr_ldsbin.inc, EXCH instantiations; cornac_amd.dist.ShardedBprTrainer.run_epoch with
    resident = True): the WHOLE epoch, s_begin = 0 and n = nnz (Case sets n), with n_ex exchange points inside it.  A plan needs
    nnz >= CUs x 16 x 64 = 262 144, so the launch is 300 000 draws and the catalogue as large as the LDS lets a resident plan
    be: rows are touched few times and one lost update shows.  Next to no triplet of a whole epoch is clean (clean_share=False:
    the clean triplets that exist are checked all the same) and launch B carries the family.  rule: the exchange's delta rule;
    twin: a second rank with the same deltas is played on the communication stream (bucket *= 2)."""
    return dict(dict(form="ldsbin", exch=True, k=k, nu=200_000, ni=300_000, nnz=300_000, zipf=0.3, user_sigma=0.5, n=None, s_begin=0,
                     flags=_lib.FORM_LDSBIN, clean_share=False, n_ex=4, rule="sqrt", twin=False), **kw)


def _exch256(k, **kw):
    # 100 000 x 65 536: 256 bins of 256 rows, 1 172 draws = 37 tiles of 32 per bin
    return _exch(k, **dict(dict(nu=100_000, ni=65_536, n_ex=8), **kw))


def _conv(k, **kw):
    """ONE conveyor launch (cornac_hip_bpr_conveyor_enqueue) over `blocks` of `n_blocks`: the whole epoch of those blocks'
    bins, so the data are sparse (8 192 interactions over 131 072 items) to keep the launch at some 2 000 triplets.  The
    draws are keyed by (seed, epoch), the deal by (deal_seed, layout_epoch): all four differ in every case."""
    return dict(dict(form="conveyor", kind="sparse", k=k, nu=100_000, ni=131_072, nnz=8_192, zipf=0.1, user_sigma=0.5, n=None,
                     s_begin=0, flags=0, n_blocks=4, blocks=(2,), epoch=5, layout_epoch=3, deal_seed=0xDEA10000 + k,
                     order_seed=None, heavy=None), **kw)


def _conv_pop(k, **kw):
    # the negative of a popularity draw is the item of another interaction of the bin, and every such item is a positive
    # of the same launch too: next to no triplet is clean, so launch B carries these cases (clean_share=False: the clean
    # triplets that exist are checked all the same)
    return _conv(k, kind="pop", neg_pop=True, clean_share=False, **kw)


def strata_waves(k, cus=MI355X_CUS):
    """the strata kernel's persistent grid on an MI355X, in waves: 4 / 5 / 5 / 7 workgroups of 4 waves per CU for the
    instantiations <1,4> / <2,2> / <3,2> / <4,1> (98 / 81 / 94 / 71 VGPRs of 512).  The device test takes the count from
    debug_ownership() and rebuilds the case if the device runs another grid."""
    return cus * 4 * (4 if k <= 64 else 5 if k <= 192 else 7)


def _strata(k, **kw):
    """ONE phase of the XCD-strata form (csrc/bpr_strata.inc): s_begin = the nominal start of `phase`, n = 1 (Case computes
    both).  The form needs 33 <= k <= 256 and nnz >= CUs x 8 x 4 x 64, so the problem is the owned cases': a phase is an eighth
    of the epoch, some 65 700 triplets, 14 % of them clean, and launch B carries the form (clean_share=False: the clean
    triplets that exist are checked all the same).  hot_cfg = strata_config's (hot_permille, hot_min_mult_x100, rehash_period);
    phases = 2: a second phase, enqueued by a second call without a sync in between; packed: chunk_records(True) first."""
    return dict(dict(form="strata", k=k, nu=200_000, ni=400_000, nnz=524_288, zipf=0.3, n=1, phase=2, epoch=0, phases=1,
                     flags=_lib.FORM_STRATA, clean_share=False, hot_cfg=(120, 200, 1), packed=False, racy_cap=0.15), **kw)


# One case per kernel instantiation the dispatchers return (csrc/bpr.hip pick_hogwild_kernel, pick_ldsbin_kernel,
# pick_strata_kernel).
SPECS = {
    # fused, unowned: every (G, R) of the row-wise kernel, the generic kernel, two float4 layouts, the switches
    "fused_k3": _fused(3), "fused_k7": _fused(7), "fused_k16": _fused(16), "fused_k20": _fused(20),
    "fused_k50": _fused(50), "fused_k100": _fused(100), "fused_k192": _fused(192), "fused_k200": _fused(200),
    "fused_generic_k300": _fused(300),
    "fused_vec4_k12": _fused(12, _lib.HOG_VEC4_LAYOUT), "fused_vec4_k64": _fused(64, _lib.HOG_VEC4_LAYOUT),
    "fused_dense_bias_k50": _fused(50, _lib.HOG_DENSE_BIAS),
    "fused_nobias_k100": _fused(100, use_bias=False),
    "fused_pop_k16": _fused(16, neg_pop=True, ni=61_440, n=1536),  # (as lds_pop_k100 below)
    # LDS bins, resident: R = 1..4, without biases, popularity negatives, a partial last group (30 733 = 120 x 256 + 13)
    "lds_k40": _lds(40), "lds_k64": _lds(64), "lds_k100": _lds(100), "lds_k192": _lds(192), "lds_k200": _lds(200),
    "lds_nobias_k64": _lds(64, use_bias=False),
    # (popularity negatives land on the popular items again and again: a larger catalogue and a shorter launch keep a third clean)
    "lds_pop_k100": _lds(100, neg_pop=True, ni=61_440, n=1536),
    "lds_partial_k64": _lds(64, ni=30_733),
    # 64-draw tiles (csrc/bpr_ldsbin.inc ldsbin_launch_range: >= 8 192 draws per bin and launch): the rest of an epoch of
    # 2.4 M interactions, flat distributions so that C stays at 0.2 (at Zipf 0.8: 3).  No triplet of such a launch is clean
    # and a row is touched 100 times and more, so only launch B applies and it shows wrong factors and lost SHARES of a
    # row's updates, not a single lost update (visibility 0).
    "lds_wide_k64": _lds(64, nu=100_000, zipf=0.3, user_sigma=0.5, nnz=2_400_000, n=2_400_000 - 12_345, clean_share=False,
                         only_b=True),
    # LDS bins, passing: max_rounds = 1 turns a catalogue just past one round of resident bins into passing bins.  A
    # passing launch is at least a quarter of an epoch (csrc/bpr.hip ldsbin_can_run): 75 000 samples over these small
    # catalogues leave few clean triplets, so launch A's share condition is not asked of them (clean_share=False) — the
    # clean triplets that exist are checked all the same — and launch B carries the form.  Next to none of the clean
    # triplets has a hot positive (1 and 0 do): the 10 700 hot positives of such a launch fall on 950 hot items, a median of
    # 14 touches on such a row, and the launch cannot be shorter.
    "pass_k128": _lds(128, nu=100_000, ni=80_000, nnz=262_144, zipf=0.6, user_sigma=0.5, n=65_536, max_rounds=1, clean_share=False),
    "pass_k64": _lds(64, nu=100_000, ni=80_000, nnz=262_144, zipf=0.6, user_sigma=0.5, n=65_536, max_rounds=1, clean_share=False),
    # fused, OWNED (k > 32, nnz >= 8 workgroups x 4 waves x 64 samples per CU): every wave draws from its own users' slice,
    # exclusive users take plain stores and users split over the waves ("shared") atomics.  The smallest launch is one
    # 64-sample tile of EVERY wave of the persistent grid (Case computes n), so no third of it is clean (clean_share=False:
    # the clean triplets that exist are checked all the same) and launch B carries the form; a flat 200 000 x 400 000
    # problem keeps the mean touches per row below 4.  `waves`: the persistent grid on an MI355X, 256 CUs x 4 workgroups
    # x 4 waves at k = 64 (R = 1) and x 6 x 4 at k = 100 (R = 2), the occupancy of the two instantiations; the device test
    # takes the count from debug_ownership() and rebuilds the case if the device runs another grid.
    "owned_k64": _owned(64, waves=4096), "owned_k100": _owned(100, waves=6144),
    # the conveyor (csrc/bpr.hip pick_ldsbin_kernel(conv = true)): R = 1..4 with uniform and with popularity negatives, and
    # the address arithmetic of the block buffers
    "conv_k40": _conv(40), "conv_k64": _conv(64), "conv_k100": _conv(100), "conv_k192": _conv(192),
    "conv_k256": _conv(256),  # (2 344 bins of 56 rows: the LDS decides the plan, not the candidates)
    "conv_pop_k64": _conv_pop(64), "conv_pop_k100": _conv_pop(100), "conv_pop_k192": _conv_pop(192),
    "conv_pop_k256": _conv_pop(256),
    "conv_nobias_k192": _conv(192, use_bias=False),
    "conv_ranges3_k100": _conv(100, n_blocks=16, blocks=(11, 2, 7)),  # three ranges, not in ascending order
    "conv_ranges8_k64": _conv(64, n_blocks=32, blocks=(30, 1, 17, 8, 0, 31, 12, 5)),  # kLbMaxRanges
    "conv_pad_k64": _conv(64, ni=130_072),  # 2 032 bins of 65 slots: the last group has 24 items, so most bins end in a pad slot
    "conv_order_k64": _conv(64, order_seed=77),  # conveyor_setup's explicit item order: a seeded permutation
    # skipped draws and hot user rows: 8 users of 600 interactions each on top (denser data would leave nothing clean)
    "conv_heavy_k64": _conv(64, kind="heavy", ni=65_536, heavy=(8, 600), clean_share=False),
    # XCD strata (csrc/bpr.hip pick_strata_kernel): <1,4> at k = 33 and 64, <2,2> at 100 and 128, <3,2> at 192, <4,1> at 200
    # (a 100 000 x 200 000 problem, so that its float64 tables are the size of owned_k100's; twice the rows race there)
    "strata_k33": _strata(33), "strata_k64": _strata(64), "strata_k100": _strata(100), "strata_k128": _strata(128, seed=0x5EED0080),
    "strata_k192": _strata(192), "strata_k200": _strata(200, nu=100_000, ni=200_000, racy_cap=0.30),
    # every item hot: the whole launch goes through atomics and every row is under the exact rule; no item hot
    "strata_allhot_k64": _strata(64, hot_cfg=(1000, 0, 1)), "strata_allhot_k100": _strata(100, hot_cfg=(1000, 0, 1)),
    "strata_nohot_k64": _strata(64, hot_cfg=(0, 200, 1)),
    # packed records (pitch kp + 32, bias at column kp): kp = 64, and kp = 128 with 28 pad columns; two phases, the second
    # launched from the records the first left (the device test runs the same two phases unpacked as well)
    "strata_packed_k64": _strata(64, packed=True, phases=2, phase=3), "strata_packed_k100": _strata(100, packed=True, phases=2, phase=6),
    "strata_nobias_k100": _strata(100, use_bias=False),
    "strata_partial_k64": _strata(64, ni=400_003, phase=5),  # 400 003 = 8 x 50 000 + 3: three partitions hold one item more
    "strata_epoch1_k64": _strata(64, epoch=1, phase=0),  # the re-deal under the key of epoch 1
    "strata_rehash2_k100": _strata(100, epoch=1, phase=7, hot_cfg=(120, 200, 2)),  # epoch 1 draws from the buckets of epoch 0's key
    # flags = 0: 2^20 items and more, no LDS-bin plan -> the strata form by itself
    "strata_auto_k33": _strata(33, ni=1_048_583, flags=0, phase=4),
    # the resident exchange (csrc/bpr.hip pick_ldsbin_kernel(exch = true)): R = 1..4 with uniform and with popularity negatives;
    # the wide instantiations take 1 024 bins (the largest catalogue whose rows fit the LDS in four rounds)
    "exch_k64": _exch(64), "exch_k100": _exch(100, ni=160_000), "exch_k192": _exch(192, ni=110_000), "exch_k200": _exch(200, ni=80_000),
    "exch_pop_k64": _exch(64, neg_pop=True), "exch_pop_k100": _exch(100, ni=160_000, neg_pop=True),
    "exch_pop_k192": _exch(192, ni=110_000, neg_pop=True), "exch_pop_k256": _exch(256, ni=80_000, neg_pop=True, seed=0x5EED0100),
    "exch_k40": _exch256(40),  # R = 1 with lanes beyond k
    "exch_nobias_k64": _exch256(64, use_bias=False),
    "exch_partial_k64": _exch256(64, ni=65_549),  # 65 549 = 256 x 256 + 13: a partial last group, 257 rows per bin
    "exch_one_k64": _exch256(64, n_ex=1),  # only the end-of-launch duty
    "exch_ex32_k64": _exch256(64, n_ex=32),  # kLbMaxExchanges: 37 tiles per bin, so ex_per = 1 and ex_parts = 1
    "exch_short_k64": _exch(64, n_ex=11),  # 10 tiles per bin: ex_per = 0, every boundary is met at the end of the launch
    "exch_align_k100": _exch(100, ni=160_000, rule="align"),
    # a twin rank: S = 2 d.  "align": the factor is exactly 1 / 2 and c an exact zero; "sqrt": c = (sqrt(2) - 1) d, the accounting
    "exch_twin_sqrt_k64": _exch256(64, twin=True), "exch_twin_align_k100": _exch(100, ni=160_000, rule="align", twin=True),
}
NAMES = list(SPECS)
EXCH_NAMES = [name for name in NAMES if SPECS[name].get("exch")]
CONVEYOR_NAMES = [name for name in NAMES if SPECS[name]["form"] == "conveyor"]
STRATA_NAMES = [name for name in NAMES if SPECS[name]["form"] == "strata"]
PAD = -7.75  # what the pad slots of the block buffers hold (finite: a pad slot read as a row shows in the checks, not as a NaN)


def ldsbin_plan(ni, nnz, k, cus=MI355X_CUS, min_candidates=48, max_rounds=4, pass_min_draws_x100=200):
    """csrc/bpr.hip ldsbin_plan restated (defaults of the pass config), LDS byte count included: dict(bins, cap, passing) or
    None.  tests/test_bpr_step_gpu.py holds it against ldsbin_stats() before it launches; the CPU test has no device to
    ask, so a change of the kernel's plan that this function misses shows there, on the device, not on the CPU."""
    if k > 256 or nnz < cus * 16 * 64:
        return None
    kp = (k + 63) // 64 * 64
    lds = lambda cap, waves: (cap * (kp + 5) + 1) * 4 + waves * 3 * 64 * 4
    for rounds in range(1, max_rounds + 1):
        bins = cus * rounds
        cap = -(-ni // bins)
        if cap < min_candidates:
            return None
        if lds(cap, 16) <= 96 * 1024:
            return dict(bins=bins, cap=cap, passing=False)
    if nnz * 100 < ni * pass_min_draws_x100:
        return None
    cap = (64 * 1024 - (4 + 8 * 3 * 64 * 4)) // ((kp + 5) * 4)
    if cap < min_candidates:
        return None
    bins = -(-(-(-ni // cap)) // cus) * cus
    cap = -(-ni // bins)
    if cap < min_candidates:
        return None
    return dict(bins=bins, cap=cap, passing=True)


def conveyor_plan(ni, k, n_blocks, cus=MI355X_CUS, min_candidates=48, pass_waves=8, pass_kb=64):
    """the conveyor branch of csrc/bpr.hip ldsbin_plan restated (defaults of the pass config): dict(bins, bpb, cap) or None.
    tests/test_bpr_step_gpu.py holds it against what conveyor_setup returns before it launches.  The cases' shapes keep
    n_items / 64 <= 2 x CUs x n_blocks, so their plans do not depend on the device's CU count."""
    if k > 256:
        return None
    kp = (k + 63) // 64 * 64
    fixed = 4 + pass_waves * 3 * 64 * 4
    if pass_kb * 1024 <= fixed:
        return None
    cap_lds = (pass_kb * 1024 - fixed) // ((kp + 5) * 4)
    cap_min = max(min_candidates, 16)
    if cap_lds < cap_min:
        return None
    bins = max(-(-ni // cap_lds), min(ni // (cap_min + cap_min // 3), 2 * cus * n_blocks))
    bins = max(1, -(-bins // n_blocks)) * n_blocks
    cap = -(-ni // bins)
    if cap > cap_lds or bins > 1 << 22 or bins * cap >= 1 << 31:
        return None
    return dict(bins=bins, bpb=bins // n_blocks, cap=cap)


def pack(V, B, slot_item, blocks, bpb, cap, into=None, bias_at=None):
    """the block buffers of `blocks` (csrc/bpr_ldsbin.inc LdsBinArgs::conv_rows): per block bpb x cap x k row floats in (bin,
    slot) order, then bpb x cap biases; slot s of the deal holds item slot_item[s], pad slots (-1) hold PAD.  into = existing
    buffers, one per block of `blocks`: only the slots that hold an item are written.  bias_at: where the bias area begins (a
    deliberately wrong kernel's; default bpb x cap x k).  Returns a list of float32 arrays."""
    k, w = V.shape[1], bpb * cap
    bias_at = w * k if bias_at is None else bias_at
    out = []
    for n, blk in enumerate(blocks):
        items = slot_item[blk * w:(blk + 1) * w]
        ok = np.flatnonzero(items >= 0)
        buf = np.full(w * k + w, PAD, np.float32) if into is None else into[n]
        buf[:w * k].reshape(w, k)[ok] = V[items[ok]]
        buf[bias_at + ok] = B[items[ok]]
        out.append(buf)
    return out


def unpack(bufs, V, B, slot_item, blocks, bpb, cap, bias_at=None):
    """copies of (V, B) with the rows and biases of the items of `blocks` taken from their buffers"""
    k, w = V.shape[1], bpb * cap
    bias_at = w * k if bias_at is None else bias_at
    V, B = np.array(V, np.float32), np.array(B, np.float32)
    for buf, blk in zip(bufs, blocks):
        items = slot_item[blk * w:(blk + 1) * w]
        ok = np.flatnonzero(items >= 0)
        V[items[ok]] = buf[:w * k].reshape(w, k)[ok]
        B[items[ok]] = buf[bias_at + ok]
    return V, B


@functools.lru_cache(maxsize=4)
def _data(nu, ni, nnz, zipf, user_sigma=1.0, heavy=None):
    users, items = synth.zipf_interactions(nu, ni, nnz, zipf, 11, user_sigma)
    if heavy is not None:  # (count, degree): that many users get `degree` further items each
        rs = np.random.RandomState(13)
        hu = rs.choice(nu, heavy[0], replace=False)
        keys = np.concatenate([users * ni + items] + [int(u) * ni + rs.choice(ni, heavy[1], replace=False) for u in hu])
        keys = np.unique(keys)
        users, items = keys // ni, keys % ni
    return synth.csr_from_sorted(users, items, nu)


def _tables(name, nu, total_items, k):
    """normal tables whose scores have unit spread whatever k (x = u.(vi - vj) + bi - bj: variance 2 k s^4 + 2 s_b^2 = 1
    with s_b = 0.5): float32 values, so exactly representable on the device"""
    rs = np.random.RandomState(sum(map(ord, name)) + 1000 * k)
    s = (0.25 / k) ** 0.25
    return (rs.normal(0, s, (nu, k)).astype(np.float32), rs.normal(0, s, (total_items, k)).astype(np.float32),
            rs.normal(0, 0.5, total_items).astype(np.float32))


class Case:
    """the inputs of one case and, computed once and never modified, its triplets and float64 references"""

    def __init__(self, name, cus=MI355X_CUS, waves=None):
        sp = dict(dict(use_bias=True, neg_pop=False, s_begin=12_345, seed=0x5EED0000 + len(name), max_rounds=4,
                       min_candidates=48, clean_share=True, only_b=False, user_sigma=1.0, heavy=None, kind=None, exch=False,
                       n_ex=0, rule="sqrt", twin=False), **SPECS[name])
        self.name, self.spec = name, sp
        for key, v in sp.items():
            setattr(self, key, v)
        self.total_items = self.ni + 37  # item rows beyond the trained range: no launch may touch them
        self.indptr, self.indices = _data(self.nu, self.ni, self.nnz, self.zipf, self.user_sigma, self.heavy)
        self.nnz = len(self.indices)
        self.tables = _tables(name, self.nu, self.total_items, self.k)
        self.neg_population = _lib.NEG_POPULARITY if self.neg_pop else _lib.NEG_UNIFORM
        kw = {}
        self.plan = self.ownership = None
        if self.form == "ldsbin":
            self.plan = ldsbin_plan(self.ni, self.nnz, self.k, cus, self.min_candidates, self.max_rounds)
            assert self.plan is not None, "%s: no LDS-bin plan" % name
            kw = dict(n_bins=self.plan["bins"], share=self.nnz / (4.0 * cus) if self.plan["passing"] else None)
        if self.exch:  # the whole epoch; the hot items (their rows stay in the global table: the atomic branch of ex_row_duty)
            assert not self.plan["passing"] and self.s_begin == 0 and 1 <= self.n_ex <= 32
            self.n = self.nnz
            self.lds_tables = orc.ldsbin_tables(self.indptr, self.indices, self.ni, self.plan["bins"], 75)
            self.n_hot = int(self.lds_tables["n_hot"])
            self.hot_items = np.sort(self.lds_tables["rank_item"][:self.n_hot].astype(np.int64))
            kw["tables"] = self.lds_tables
        if self.form == "owned":
            # the smallest launch of this form: one 64-sample tile of every wave (csrc/bpr.hip: a launch covers the tiles
            # [tmax s_begin / nnz, tmax (s_begin + n) / nnz) of every wave's slice, tmax = the longest slice's tile count)
            self.ownership = orc.hogwild_ownership(self.indptr, self.indices, waves or self.waves)
            tmax = int((np.diff(self.ownership[0]).max() + 63) // 64)
            self.n = -(-self.nnz // tmax) - self.s_begin
            assert tmax * self.s_begin // self.nnz == 0 and (tmax == 1 or tmax * (self.s_begin + self.n) // self.nnz == 1)
            kw = dict(ownership=self.ownership)
        form, epoch = self.form, 0
        if self.form == "strata":
            assert self.nnz >= cus * 8 * 4 * 64 and 33 <= self.k <= 256
            if self.flags == 0:  # FORM_AUTO takes the strata form by itself: 2^20 items and more, and no LDS-bin plan
                assert self.ni >= 1 << 20 and ldsbin_plan(self.ni, self.nnz, self.k, cus) is None
            self.waves = waves or strata_waves(self.k, cus)
            self.ownership = orc.hogwild_ownership(self.indptr, self.indices, self.waves)
            # phase ph begins at sample ceil(ph nnz / 8); the first call enqueues 1 sample there, every further call the samples
            # up to and including the next phase's first one (csrc/bpr.hip strata_enqueue: a launch runs the phases that begin inside it)
            first = [-(-(self.phase + q) * self.nnz // 8) for q in range(self.phases)]
            assert self.phase + self.phases <= 8
            self.s_begin, self.launch_ns = first[0], [1] + [b - a for a, b in zip(first, first[1:])]
            self.n, epoch = sum(self.launch_ns), self.epoch
            kw = dict(ownership=self.ownership, k=self.k, hot_permille=self.hot_cfg[0], hot_min_mult_x100=self.hot_cfg[1],
                      rehash_period=self.hot_cfg[2])
        if self.form == "conveyor":
            self.plan = conveyor_plan(self.ni, self.k, self.n_blocks, cus, self.min_candidates)
            assert self.plan is not None, "%s: no conveyor plan" % name
            assert self.epoch != self.layout_epoch and self.seed != self.deal_seed and 1 <= len(self.blocks) <= 8
            bins, bpb, cap = self.plan["bins"], self.plan["bpb"], self.plan["cap"]
            tables = orc.ldsbin_tables(self.indptr, self.indices, self.ni, bins, 10 ** 9)  # (no hot items in this layout)
            self.rank_item = None if self.order_seed is None else np.random.RandomState(self.order_seed).permutation(
                self.ni).astype(np.int32)
            order = tables["rank_item"] if self.rank_item is None else self.rank_item
            self.slot_item, self.item_slot = orc.ldsbin_layout(self.deal_seed, self.layout_epoch, bins, self.ni, order)
            form, epoch, self.n = "ldsbin", self.epoch, self.nnz
            kw = dict(n_bins=bins, tables=tables, deal=(self.deal_seed, self.layout_epoch), rank_item=self.rank_item,
                      bins=[(b * bpb, (b + 1) * bpb) for b in self.blocks])
            # all blocks' buffers as the launches find them, from the ORACLE's layout
            self.bufs = pack(self.tables[1], self.tables[2], self.slot_item, range(self.n_blocks), bpb, cap)
            for buf in self.bufs:
                buf.setflags(write=False)
        t = orc.hogwild_triplets(form, self.seed, epoch, self.s_begin, self.n, self.indptr, self.indices, self.ni,
                                 neg_pop=self.neg_pop, **kw)
        if self.form == "conveyor":
            t.pop("hot")  # (none is)
            self.draws = t["draws"]
        self.trip = (t["u"], t["i"], t["j"])
        self.skipped, self.hot, self.bin, self.shared = t["skipped"], t.get("hot"), t.get("bin"), t.get("shared")
        self.racy = None
        if self.form == "strata":
            self.strata = t
            self._classify_item_rows(t)
        # launch B: the Jacobi sum of every row; launch A: the float64 step of the clean triplets alone (their rows have no
        # other delta, so no sum is needed); launch Z: the float64 scores (they do not depend on lr)
        self.jac = step.jacobi(self.trip, self.tables, LR_B, REG, self.use_bias)
        for tab in "UVB":
            for a in self.jac[tab].values():
                a.setflags(write=False)
        self.touches = {tab: self.jac[tab]["touches"] for tab in "UVB"}
        u, i, j = self.trip
        self.clean = (self.touches["U"][u] == 1) & (self.touches["V"][i] == 1) & (self.touches["V"][j] == 1)
        cu, ci, cj = (a[self.clean] for a in self.trip)
        _, _, dU, dVi, dVj, dBi, dBj = step.deltas((cu, ci, cj), *self.tables, LR_A, REG, self.use_bias)
        cij = np.concatenate([ci, cj])
        self.clean_rows = {"U": cu, "V": cij, "B": cij}
        self.clean_want = {tab: start[rows].astype(np.float64) + d for tab, start, rows, d in (
            ("U", self.tables[0], cu, dU), ("V", self.tables[1], cij, np.concatenate([dVi, dVj])),
            ("B", self.tables[2], cij, np.concatenate([dBi, dBj])))}
        self.x, self.z = self.jac["x"], self.jac["z"]
        self.x_bound = step.score_error_bound(self.trip, self.tables)

    def _classify_item_rows(self, t):
        """the classes of the strata form's item rows, from the triplets alone: hot (device-scope atomics), cold and touched
        by ONE wave per phase (plain stores in program order), cold and touched by two or more waves of one phase (`racy`:
        plain read-modify-write among the CUs of one XCD; two phases never race, the kernel boundary lies between them).  A
        reference = one naming of an item row by a triplet (its i, then its j); its group = the (phase, wave, step) it is
        loaded and stored in."""
        W, n = self.waves, len(t["i"])
        self.ref_row = np.concatenate([t["i"], t["j"]])
        self.ref_hot = np.concatenate([t["hot_i"], t["hot_j"]])
        self.ref_trip = np.concatenate([np.arange(n), np.arange(n)])
        self.ref_isj = np.concatenate([np.zeros(n, bool), np.ones(n, bool)])
        self.item_hot = np.zeros(self.total_items, bool)
        self.item_hot[self.ref_row[self.ref_hot]] = True
        assert not self.item_hot[self.ref_row[~self.ref_hot]].any(), "an item is hot in every reference or in none"
        phase, wave = np.concatenate([t["phase"]] * 2), np.concatenate([t["wave"]] * 2)
        pairs = np.unique((self.ref_row * 8 + phase) * W + wave)  # distinct (row, phase, wave)
        rp, waves_of = np.unique(pairs // W, return_counts=True)  # per (row, phase)
        self.racy = np.zeros(self.total_items, bool)
        self.racy[np.unique(rp[waves_of >= 2] // 8)] = True
        self.racy &= ~self.item_hot
        self.trip_group = np.unique((t["phase"] * W + t["wave"]) * (1 << 24) + t["step"], return_inverse=True)[1]
        self.ref_group = np.concatenate([self.trip_group] * 2)
        self._racy_groups = None

    def racy_groups(self):
        """{m: (rows [n], dV [n, m, k], dB [n, m])}: the racy rows that m groups name, with every group's float64 delta of
        launch B (the sum over the group's references of the row: what the in-step merge stores at once)"""
        if self._racy_groups is not None:
            return self._racy_groups
        sel = np.flatnonzero(self.racy[self.ref_row])
        if len(sel) == 0:
            self._racy_groups = {}
            return self._racy_groups
        trips, inv = np.unique(self.ref_trip[sel], return_inverse=True)
        _, _, _, dVi, dVj, dBi, dBj = step.deltas(tuple(a[trips] for a in self.trip), *self.tables, LR_B, REG, self.use_bias)
        isj = self.ref_isj[sel]
        dv, db = np.where(isj[:, None], dVj[inv], dVi[inv]), np.where(isj, dBj[inv], dBi[inv])
        row, grp = self.ref_row[sel], self.ref_group[sel]
        order = np.lexsort((grp, row))
        row, grp, dv, db = row[order], grp[order], dv[order], db[order]
        starts = np.flatnonzero(np.r_[True, (row[1:] != row[:-1]) | (grp[1:] != grp[:-1])])
        gdv, gdb, grow = np.add.reduceat(dv, starts, axis=0), np.add.reduceat(db, starts), row[starts]
        rows, first, m = np.unique(grow, return_index=True, return_counts=True)
        out = {}
        for mm in np.unique(m):
            pick = np.flatnonzero(m == mm)
            idx = first[pick][:, None] + np.arange(mm)[None, :]
            out[int(mm)] = (rows[pick], gdv[idx], gdb[idx])
        self._racy_groups = out
        return out

    def exch_tiles(self):
        """per bin of a resident-exchange launch: (draws, tile width, tiles), csrc/bpr_ldsbin.inc ldsbin_launch_range restated
        for a whole epoch and a 16-wave workgroup"""
        t, bins = self.lds_tables, self.plan["bins"]
        key = int(orc.lib().oracle_ldsbin_key(int(self.seed), 0))
        _, cold, off = orc.ldsbin_deal_key(key, bins, self.ni, t["n_hot"], orc.ldsbin_n_strata(self.ni, bins, 16), 32,
                                           t["rank_item"], t["cptr"], t["n_hot_inter"])
        draws = cold.astype(np.int64) + np.diff(off.astype(np.int64))
        tile_w = np.where(draws < 8 * 16 * 64, 32, 64)
        return draws, tile_w, -(-draws // tile_w)

    def exch_segments(self, n_ex):
        """per triplet: how many exchange boundaries of its bin lie before it.  Boundary e < n_ex - 1 sits at the bin's draw
        (e + 1) (n_tiles // n_ex) tile_w, the last one (every one of a bin with fewer tiles than exchanges) at the end of the
        launch.  The restatement names a bin's triplets in draw order but not their draws: the m-th triplet stands for draw
        m, so a boundary sits late by the bin's skipped draws before it (a few in a thousand)."""
        _, tile_w, tiles = self.exch_tiles()
        per = (tiles // n_ex) * tile_w
        first = np.flatnonzero(np.r_[True, self.bin[1:] != self.bin[:-1]])
        assert len(np.unique(self.bin[first])) == len(first), "the restatement goes bin by bin"
        m = np.arange(len(self.bin)) - np.repeat(first, np.diff(np.r_[first, len(self.bin)]))
        p = per[self.bin]
        return np.where(p > 0, np.minimum(m // np.maximum(p, 1), n_ex - 1), 0)

    def triplets_of(self, table, row):
        u, i, j = self.trip
        return np.flatnonzero(u == row if table == "U" else (i == row) | (j == row))

    def describe(self, table, row):
        ids = self.triplets_of(table, row)
        u, i, j = self.trip
        return "%s: table %s row %d, %d touches, triplets %s" % (
            self.name, table, row, len(ids), ", ".join("#%d (u %d, i %d, j %d)" % (t, u[t], i[t], j[t]) for t in ids[:8]) +
            (" ..." if len(ids) > 8 else ""))


@functools.lru_cache(maxsize=2)
def case(name, cus=MI355X_CUS, waves=None):
    return Case(name, cus, waves)


# ---- the checks: `got` = (U, V, B) as the device (or a deliberately wrong reference) returns them --------------------------
def _untouched_identical(c, launch, got):
    for tab, start, g in zip("UVB", c.tables, got):
        same = (g == start).reshape(len(start), -1).all(axis=1) | (c.touches[tab] > 0)
        assert same.all(), "launch %s changed a row no triplet touches: %s" % (launch, c.describe(tab, int(np.flatnonzero(~same)[0])))


def conveyor_tables(c, launch, bufs, U):
    """(U, V, B) as a conveyor launch left them: `bufs` = the buffers of ALL blocks after the launch.  The buffers of the
    blocks the launch was not given and the pad slots of those it was given must be bit-identical; what the launched
    blocks' item slots hold goes back to the items' rows, where check_a / check_b hold every row to its rule (rows no
    triplet touches, those beyond n_items among them: bit-identical)."""
    bpb, cap = c.plan["bpb"], c.plan["cap"]
    w = bpb * cap
    for blk, (start, buf) in enumerate(zip(c.bufs, bufs)):
        assert buf.dtype == np.float32 and buf.shape == start.shape
        if blk not in c.blocks:
            assert np.array_equal(start, buf), "%s, launch %s changed the buffer of block %d, which it was not given" % (c.name, launch, blk)
            continue
        pad = np.flatnonzero(c.slot_item[blk * w:(blk + 1) * w] < 0)
        rows, bias = buf[:w * c.k].reshape(w, c.k)[pad], buf[w * c.k + pad]
        assert (rows == np.float32(PAD)).all() and (bias == np.float32(PAD)).all(), "%s, launch %s changed a pad slot of block %d" % (
            c.name, launch, blk)
    V, B = unpack([bufs[b] for b in c.blocks], c.tables[1], c.tables[2], c.slot_item, c.blocks, bpb, cap)
    return U, V, B


def check_z(c, got, correct, skipped):
    for tab, start, g in zip("UVB", c.tables, got):
        assert np.array_equal(start, g), "%s: lr = 0 changed table %s" % (c.name, tab)
    assert skipped == c.skipped, "%s: skip counter %d, restatement %d" % (c.name, skipped, c.skipped)
    lo, hi = int((c.x > c.x_bound).sum()), int((c.x > -c.x_bound).sum())
    assert lo <= correct <= hi, "%s: `correct` = %d, float64 scores give %d..%d" % (c.name, correct, lo, hi)
    return dict(correct=correct, lo=lo, hi=hi)


def check_a(c, got):
    """launch A: clean rows against the float64 step at T_CLEAN, untouched rows bit-identical.  Returns the largest
    clean-row error per table."""
    _untouched_identical(c, "A", got)
    worst = {}
    for tab, g in zip("UVB", got):
        rows, want = c.clean_rows[tab], c.clean_want[tab]
        err = np.abs(g[rows].astype(np.float64) - want).reshape(len(rows), -1).max(axis=1) if len(rows) else np.zeros(0)
        worst[tab] = float(err.max()) if len(err) else 0.0
        bad = np.flatnonzero(err > T_CLEAN)
        assert len(bad) == 0, "launch A, clean row off by %.3g > T_CLEAN = %.3g (%d such rows): %s" % (
            err[bad[0]], T_CLEAN, len(bad), c.describe(tab, int(rows[bad[0]])))
    return worst


def tolerance_b(c, tab, coeff=None, extra=0, reach=False):
    """per-row tolerance of launch B for one table: C x path + touches x ulp(max |row|) / 2 x sqrt(k), max |row| taken from the
    row's start and its Jacobi end.  extra: further float32 roundings of the row to add to `touches` in the floor term (the
    resident exchange: one per exchange).  reach: max |row| = max |start| + path instead, which bounds the row at EVERY moment
    of the launch — for the identities that have the floor term alone (coeff = 0): a bias of 5e-6 that steps of 1e-4 carry
    away and back is rounded at the ulp of 1e-4 on the way, which C x path covers in the rules and nothing in an identity"""
    coeff = C[c.name] if coeff is None else coeff
    j = c.jac[tab]
    start = c.tables["UVB".index(tab)].astype(np.float64).reshape(len(j["touches"]), -1)
    top = np.maximum(np.abs(start), np.abs(start + j["sum"].reshape(start.shape))).max(axis=1)
    if reach:
        top = np.abs(start).max(axis=1) + j["path"]
    half_ulp = np.spacing(top.astype(np.float32)).astype(np.float64) / 2
    return coeff * j["path"] + (j["touches"] + extra) * half_ulp * np.sqrt(start.shape[1])


def check_b(c, got, coeff=None, other_rule=None):
    """launch B: every touched row against the Jacobi sum.  Returns the largest error / tolerance per table.  other_rule =
    {table: mask of the rows that another rule holds} (check_b_strata: the racy rows)."""
    _untouched_identical(c, "B", got)
    worst = {}
    for tab, start, g in zip("UVB", c.tables, got):
        j = c.jac[tab]
        rows = np.flatnonzero((j["touches"] > 0) & ~other_rule[tab] if other_rule and tab in other_rule else j["touches"] > 0)
        if len(rows) == 0:
            worst[tab] = 0.0
            continue
        moved = g[rows].astype(np.float64) - start[rows].astype(np.float64)
        err = np.linalg.norm((moved - j["sum"][rows]).reshape(len(rows), -1), axis=1)
        tol = tolerance_b(c, tab, coeff)[rows]
        worst[tab] = float((err / tol).max())
        bad = np.flatnonzero(err > tol)
        assert len(bad) == 0, "launch B, |got - start - jacobi| = %.3g > %.3g (path %.3g; %d such rows): %s" % (
            err[bad[0]], tol[bad[0]], j["path"][rows[bad[0]]], len(bad), c.describe(tab, int(rows[bad[0]])))
    return worst


def visibility(c, tab, coeff=None):
    """share of the touched rows of a table on which ONE lost or doubled update shows: path / touches > 2 x tolerance"""
    j = c.jac[tab]
    rows = np.flatnonzero(j["touches"] > 0)
    if len(rows) == 0:
        return 1.0
    return float((j["path"][rows] / j["touches"][rows] > 2 * tolerance_b(c, tab, coeff)[rows]).mean())


def round_up_1sig(v):
    e = np.floor(np.log10(v))
    return float(np.ceil(v / 10 ** e - 1e-9) * 10 ** e)


# ---- the XCD-strata form: launch B under two rules ----------------------------------------------------------------------------
MAX_RACY_GROUPS = 16


def racy_rows(c, got, coeff=None):
    """The racy rule, row by row.  A cold item row that two or more waves of one phase touch is plain read-modify-write among
    the CUs of one XCD: a store may overwrite another wave's, so what arrives is the sum of SOME of the row's (phase, wave,
    step) groups — at least one, the last store's.  Element by element (nobody has measured at what granularity two waves'
    stores of one row interleave), got - start must lie within the row's tolerance_b / sqrt(k) of the sum of a non-empty
    subset of its groups' float64 deltas; the bias, one element, within its own tolerance_b.  Returns per racy row: rows,
    groups, ok (the rule holds), whole (ONE subset explains the row and its bias), full (the subset of all groups does)."""
    tol_v, tol_b = tolerance_b(c, "V", coeff) / np.sqrt(c.k), tolerance_b(c, "B", coeff)
    out = dict(rows=[], groups=[], ok=[], whole=[], full=[])
    for m, (rows, dv, db) in sorted(c.racy_groups().items()):
        assert 2 <= m <= MAX_RACY_GROUPS, "%s: a racy row of %d groups" % (c.name, m)
        subsets = ((np.arange(1, 1 << m)[:, None] >> np.arange(m)[None, :]) & 1).astype(np.float64)  # (the last one: all groups)
        chunk = max(1, (1 << 22) // (len(subsets) * c.k))
        for a in range(0, len(rows), chunk):
            r = rows[a:a + chunk]
            moved = got[1][r].astype(np.float64) - c.tables[1][r].astype(np.float64)
            sums = np.einsum("sm,nmk->nsk", subsets, dv[a:a + chunk])
            within = np.abs(moved[:, None, :] - sums) <= tol_v[r][:, None, None]
            if c.use_bias:
                moved_b = got[2][r].astype(np.float64) - c.tables[2][r].astype(np.float64)
                within_b = np.abs(moved_b[:, None] - db[a:a + chunk] @ subsets.T) <= tol_b[r][:, None]
            else:
                within_b = np.ones(within.shape[:2], bool)
            each = within.all(axis=2) & within_b
            out["rows"].append(r)
            out["groups"].append(np.full(len(r), m))
            out["ok"].append(within.any(axis=1).all(axis=1) & within_b.any(axis=1))
            out["whole"].append(each.any(axis=1))
            out["full"].append(each[:, -1])
    return {key: (np.concatenate(v) if v else np.zeros(0, bool if key in ("ok", "whole", "full") else np.int64))
            for key, v in out.items()}


def check_b_strata(c, got, coeff=None):
    """launch B of a strata case: check_b, unchanged, on every U row, every hot item row and every cold item row that one
    wave per phase touches (with their biases); the racy rule on the others.  Returns check_b's figures and: racy (rows
    under the racy rule), whole (explained by one subset as a whole), lost (not explained by the sum of all their groups:
    at least one group's store was overwritten)."""
    worst = check_b(c, got, coeff, other_rule={"V": c.racy, "B": c.racy})
    r = racy_rows(c, got, coeff)
    bad = np.flatnonzero(~r["ok"])
    assert len(bad) == 0, "launch B, racy rule: no subset of the row's %d groups explains an element (%d such rows of %d): %s" % (
        r["groups"][bad[0]], len(bad), len(r["ok"]), c.describe("V", int(r["rows"][bad[0]])))
    worst.update(racy=len(r["ok"]), whole=int(r["whole"].sum()), lost=int((~r["full"]).sum()))
    return worst


def racy_visible(c, coeff=None):
    """per racy row (the order of racy_rows): a single group's loss shows, path / groups > 2 x tolerance"""
    tol, path = tolerance_b(c, "V", coeff), c.jac["V"]["path"]
    rows = [(r, np.full(len(r), m)) for m, (r, _, _) in sorted(c.racy_groups().items())]
    if not rows:
        return np.zeros(0, bool)
    r, m = np.concatenate([a for a, _ in rows]), np.concatenate([b for _, b in rows])
    return path[r] / m > 2 * tol[r]


# ---- the resident exchange: the table, and what the launch publishes ------------------------------------------------------------
# `res` = what a launch left, as the device test reads it back (and the host model of tests/test_bpr_step_cpu.py returns it):
# U [nu, k]; flat, base [nt k + nt] (the replicated item table [V | B] and its base, read BEFORE the driver's closing exchange);
# signals [2 n_ex + 1] (arrivals | landed flags | error word); applied [nt]; red = exch_reduce(keeps, buckets).
class ExchReducer:
    """What the checks need of the keeps [n_ex][nt k + nt] and buckets [n_ex][nt k + 3 nt] of a launch, taken in exchange by
    exchange where the buffers are (torch tensors on the device: float32; the float64 host model's arrays as they are), in
    float64: ksum = sum_e keeps[e]; csum = sum_e (rule(buckets[e]) - keeps[e]), the corrections the launch and the flush apply
    between them; all_zero; bucket_is_keep (buckets[e][:width] == keeps[e], or 2 keeps[e] with a twin, bit for bit); under
    "sqrt" w_exact (wV[e][i] == ranks x (row i of keeps[e] has a non-zero), wB likewise), under "align" w_rel (largest |w -
    ranks x sum d^2| / that, the sum in float64)."""

    def __init__(self, c):
        self.c, self.n, self.ksum, self.csum = c, 0, None, None
        self.out = dict(all_zero=True, bucket_is_keep=True, w_exact=True, w_rel=0.0)

    def add(self, keep, bucket):
        import torch

        c, out = self.c, self.out
        K, Bk = torch.as_tensor(keep), torch.as_tensor(bucket)
        nt, k = c.total_items, c.k
        nk, width, ranks = nt * k, nt * k + nt, 2.0 if c.twin else 1.0
        assert K.shape == (width,) and Bk.shape == (width + 2 * nt,) and K.dtype == Bk.dtype
        if self.ksum is None:
            self.ksum = torch.zeros(width, dtype=torch.float64, device=K.device)
            self.csum = torch.zeros_like(self.ksum)
        self.n += 1
        S, wV, wB, Kd = Bk[:width].double(), Bk[width:width + nt], Bk[width + nt:], K.double()
        self.ksum += Kd
        out["all_zero"] &= not bool(K.any()) and not bool(Bk.any())
        out["bucket_is_keep"] &= bool(torch.equal(Bk[:width], K * ranks))
        dV, dB = Kd[:nk].view(nt, k), Kd[nk:]
        if c.rule == "sqrt":
            out["w_exact"] &= bool(torch.equal(wV.double(), ranks * (dV != 0).any(dim=1).double())) and bool(
                torch.equal(wB.double(), ranks * (dB != 0).double()))
            fV, fB = wV.double().clamp(min=1.0).rsqrt(), wB.double().clamp(min=1.0).rsqrt()
        else:
            for w, want in ((wV, ranks * (dV * dV).sum(dim=1)), (wB, ranks * dB * dB)):
                out["w_exact"] &= bool((w[want == 0] == 0).all())
                rel = ((w.double() - want).abs() / want)[want > 0]
                out["w_rel"] = max(out["w_rel"], float(rel.max()) if rel.numel() else 0.0)
            n2V, n2B = (S[:nk].view(nt, k) ** 2).sum(dim=1), S[nk:] ** 2
            fV = torch.where(n2V > 0, (wV.double() / n2V).clamp(max=1.0), torch.ones_like(n2V))
            fB = torch.where(n2B > 0, (wB.double() / n2B).clamp(max=1.0), torch.ones_like(n2B))
        self.csum[:nk] += (S[:nk].view(nt, k) * fV[:, None]).reshape(-1) - Kd[:nk]
        self.csum[nk:] += S[nk:] * fB - Kd[nk:]

    def result(self):
        assert self.n == self.c.n_ex
        return dict(self.out, ksum=self.ksum.cpu().numpy(), csum=self.csum.cpu().numpy())


def exch_reduce(c, keeps, buckets):
    red = ExchReducer(c)
    for e in range(c.n_ex):
        red.add(keeps[e], buckets[e])
    return red.result()


def _exch_vb(c, flat):
    nk = c.total_items * c.k
    return flat[:nk].reshape(c.total_items, c.k), flat[nk:]


def exch_tables(c, res, uncorrected=False):
    """(U, V, B) of a launch; uncorrected: with the corrections the buffers name taken out again (float64 sum, one rounding)"""
    flat = (res["flat"].astype(np.float64) - res["red"]["csum"]).astype(np.float32) if uncorrected else res["flat"]
    return (res["U"],) + _exch_vb(c, flat)


def check_exch_signals(c, res):
    sig, n_ex = np.asarray(res["signals"]), c.n_ex
    assert (sig[:n_ex] == c.plan["bins"]).all(), "%s: arrivals %s, bins %d" % (c.name, sig[:n_ex], c.plan["bins"])
    assert (sig[n_ex:2 * n_ex] == 1).all() and sig[2 * n_ex] == 0, "%s: landed flags %s, error word %d" % (c.name, sig[n_ex:2 * n_ex], sig[2 * n_ex])
    ap = np.asarray(res["applied"])
    assert ((ap >= 0) & (ap <= n_ex)).all() and (ap[c.ni:] == 0).all(), "%s: the applied[] record" % c.name


def check_exch_z(c, res):
    """launch Z of a resident-exchange case beyond check_z: nothing published but exact zeros, the base is the table"""
    check_exch_signals(c, res)
    assert res["red"]["all_zero"], "%s: lr = 0 published a non-zero keep or bucket word" % c.name
    assert np.array_equal(res["flat"], res["base"]), "%s: lr = 0 left table and base apart" % c.name


def check_exch_a(c, res):
    """launch A: check_a, unchanged — on the table less its corrections where they are not zero (twin, "sqrt": a clean row
    holds (sqrt(2) - 1) of its own step on top, sooner or later)"""
    check_exch_signals(c, res)
    return check_a(c, exch_tables(c, res, uncorrected=c.twin and c.rule == "sqrt"))


def _exch_rows(c, tab, got, want, coeff, what):
    """per row of V (or element of B): |got - want| <= tolerance_b(coeff) with n_ex more roundings (coeff = 0: its floor term
    alone, max |row| by its reach), Euclidean over the row; `want` None = the Jacobi sum, on the touched rows, and an exact zero
    on the others.
    Returns the largest error / tolerance."""
    j = c.jac[tab]
    tol = tolerance_b(c, tab, coeff, extra=c.n_ex, reach=want is not None)
    if want is None:
        quiet = np.flatnonzero((j["touches"] == 0) & (got != 0).reshape(len(tol), -1).any(axis=1))
        assert len(quiet) == 0, "%s: %s of a row no triplet touches is not zero: %s" % (c.name, what, c.describe(tab, int(quiet[0])))
        rows, want = np.flatnonzero(j["touches"] > 0), j["sum"]
    else:
        rows = np.arange(len(tol))
    if len(rows) == 0:
        return 0.0
    err = np.linalg.norm((got[rows] - want[rows]).reshape(len(rows), -1), axis=1)
    bad = np.flatnonzero(err > tol[rows])
    assert len(bad) == 0, "launch B, %s off by %.3g > %.3g (path %.3g; %d such rows): %s" % (
        what, err[bad[0]], tol[rows][bad[0]], j["path"][rows[bad[0]]], len(bad), c.describe(tab, int(rows[bad[0]])))
    return float((err / tol[rows]).max()) if len(rows) else 0.0


def check_exch_b(c, res, coeff=None, lock_timeouts=0):
    """launch B of a resident-exchange case.  Returns the largest error / tolerance of the table rule (U, V, B), of the
    published-delta rule (PV, PB) and of the floor-only identities (floor), and the rows left apart from their base (left)."""
    check_exch_signals(c, res)
    red = res["red"]
    start = np.concatenate([c.tables[1].ravel(), c.tables[2]]).astype(np.float64)
    flat, base = res["flat"].astype(np.float64), res["base"].astype(np.float64)
    owed = flat - base
    P = red["ksum"] + owed
    accounting = c.twin and c.rule == "sqrt"
    if accounting:
        # whatever the timing: the table is its start, the rank's steps and the corrections; the base lacks what is still owed.
        # U takes no correction, but its steps saw rows displaced by them: the same C as P
        out = check_b(c, exch_tables(c, res), coeff, other_rule={tab: np.ones(c.total_items, bool) for tab in "VB"})
        steps, published = flat - start - red["csum"], base - start - red["csum"]
    else:
        out = check_b(c, exch_tables(c, res), coeff)  # 1: one rank alone makes the exchange the identity
        steps, published = flat - start, base - start
    # 2: what the other ranks receive, and what the closing exchange still owes them
    for tab, p in zip("VB", _exch_vb(c, P)):
        out["P" + tab] = _exch_rows(c, tab, p, None, coeff, "the published delta")
    # 3: only hot rows are stepped after their last publication
    apart = np.flatnonzero((_exch_vb(c, owed)[0] != 0).any(axis=1) | (_exch_vb(c, owed)[1] != 0))
    cold = np.setdiff1d(apart, c.hot_items)
    assert len(cold) == 0 and len(apart) <= c.n_hot, "%s: %d rows differ from their base, %d of them cold (n_hot %d): %s" % (
        c.name, len(apart), len(cold), c.n_hot, c.describe("V", int(cold[0])) if len(cold) else "")
    out["left"] = len(apart)
    # 4: the bucket of one rank is its keep (of two equal ranks: twice it), with the rule's weights
    assert red["bucket_is_keep"], "%s: buckets[:, :width] != %s keeps" % (c.name, "2 x" if c.twin else "")
    assert red["w_exact"], "%s: a weight word differs from what its keep row says" % c.name
    w_tol = (c.k + 2) * 2.0 ** -24
    assert red["w_rel"] <= w_tol, "%s: a weight is %.3g (relative) off the float64 sum of squares, tolerance %.3g" % (c.name, red["w_rel"], w_tol)
    out["w_rel"] = red["w_rel"] / w_tol
    # 5 / the accounting: no delta published twice or never, no correction applied twice or never — within the roundings
    worst = 0.0
    for tab, s, p, pub, ks in zip("VB", _exch_vb(c, steps), _exch_vb(c, P), _exch_vb(c, published), _exch_vb(c, red["ksum"])):
        worst = max(worst, _exch_rows(c, tab, pub, ks, 0.0, "base - start%s - sum of keeps" % (" - corrections" if accounting else "")))
        worst = max(worst, _exch_rows(c, tab, s, p, 0.0, "table - start%s - P" % (" - corrections" if accounting else "")))
    out["floor"] = worst
    assert lock_timeouts == 0, "%s: %d lock time-outs" % (c.name, lock_timeouts)
    return out
