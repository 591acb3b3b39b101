"""Every ranking path of csrc/score.hip at its dispatch boundaries, against the oracle: the cases, the rule and the checker
are tests/rank_cases.py (tests/test_rank_cases_cpu.py holds them to account); this file only calls the device."""
import contextlib

import numpy as np
import pytest

import rank_cases as rc
from cornac_amd import _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _subnormals_are_numbers():
    with rc.ieee_subnormals():      # (whatever an earlier test of the session loaded: see rank_cases.ieee_subnormals)
        yield


@contextlib.contextmanager
def scorer(case):
    t = case.t
    sc = _lib.Scorer(t.U, t.V, t.ib, t.ub)
    try:
        yield sc
    finally:
        sc.close()


def rank_and_check(case):
    with scorer(case) as sc:
        items, scores = sc.rank_topk(case.users, case.topk, exclude=case.excl)
    rc.check_rank(case, items, scores)


@pytest.mark.parametrize("with_ub", [False, True])
@pytest.mark.parametrize("k", rc.SCORE_KS)
def test_scores_at_the_padding_boundaries(k, with_ub):
    """A: score_gemm_mfma_kernel<8,2> (k 16), <16,2> (17, 24, 31, 32), <32,2> (33, 64), <64,1> (65, 128) and
    score_valu_kernel (129) through score_block on all 257 users and on a permuted list with repeats; score_user and
    score_pairs at the same k: the oracle's bits"""
    case = rc.score_case(k, with_ub)
    with scorer(case) as sc:
        block = sc.score_block(case.users)
        subset = sc.score_block(case.props["subset"])
        one = sc.score_user(case.props["single_user"])
        pu, pi = case.props["pairs"]
        pairs = sc.score_pairs(pu, pi)
    assert np.array_equal(block, case.scores), case
    assert np.array_equal(subset, case.scores[case.props["subset"]]), case
    assert np.array_equal(one, case.scores[case.props["single_user"]]), case
    assert np.array_equal(pairs, case.scores[pu, pi]), case


@pytest.mark.parametrize("k,topk,with_ub,with_excl", rc.FUSED)
def test_every_fused_instantiation(k, topk, with_ub, with_excl):
    """B: rank_fused_kernel<KT, CAP, UB> for every (KT, CAP, UB) the dispatch can select (rank_cases.FUSED lists which case
    runs which), rank_merge_kernel, excl_bitmap_kernel"""
    rank_and_check(rc.fused_case(k, topk, with_ub, with_excl))


@pytest.mark.parametrize("topk", [10, 32])
@pytest.mark.parametrize("n_items", rc.LIMIT_ITEMS)
def test_fused_exclusions_on_both_sides_of_the_bitmap_limit(n_items, topk):
    """C: 262 144 items rank with the exclusion bitmap, 262 145 and 262 177 with the binary search at compaction"""
    rank_and_check(rc.limit_case(n_items, topk))


def test_no_bitmap_catalogue_refuses_unsorted_and_resident_lists():
    """C: the two host checks of a catalogue beyond the bitmap"""
    case = rc.limit_case(rc.LIMIT_ITEMS[1], 10)
    indptr, indices = case.excl
    unsorted = indices.copy()
    lo = indptr[rc.LIMIT_ENDS_ROW]
    unsorted[lo], unsorted[lo + 1] = indices[lo + 1], indices[lo]
    with scorer(case) as sc:
        with pytest.raises(_lib.HipError, match="not strictly sorted"):
            sc.rank_topk(case.users, case.topk, exclude=(indptr, unsorted))
        sc.set_exclusions(indptr, indices)
        with pytest.raises(_lib.HipError, match="resident exclusion lists"):
            sc.rank_topk_resident((0, case.n_rows), case.topk)


@pytest.mark.parametrize("with_excl", [False, True])
@pytest.mark.parametrize("n_items,topk,k", rc.SELECT)
def test_radix_select(n_items, topk, k, with_excl):
    """D: topk_select_kernel over MFMA scores (k 16) and VALU scores (k 129, 200), mark_excluded_kernel"""
    rank_and_check(rc.select_case(n_items, topk, k, with_excl))


@pytest.mark.parametrize("with_excl", [False, True])
@pytest.mark.parametrize("n_items,topk", rc.SORT)
def test_full_sort(n_items, topk, with_excl):
    """E: full_sort_kernel on less than one chunk, one chunk, and 2, 4 and 16 chunks (phase B)"""
    rank_and_check(rc.sort_case(n_items, topk, with_excl))


def test_full_sort_second_batch():
    """E: cornac_hip_rank_topk's batch loop at 1024 rows per batch (topk > 2048)"""
    rank_and_check(rc.sort_batch_case())


def test_select_second_batch():
    """F: cornac_hip_rank_topk's batch loop at 16 384 rows per batch"""
    rank_and_check(rc.batch_case())


def test_positions_second_batch():
    """F: cornac_hip_rank_positions' batch loop"""
    case = rc.batch_case()
    with scorer(case) as sc:
        got = sc.rank_positions(case.users, rc.csr(case.props["targets"]), exclude=case.excl)
    rc.check_positions(case, *got)


def test_score_block_second_batch():
    """F: cornac_hip_score_block's batch loop"""
    case = rc.batch_case()
    with scorer(case) as sc:
        got = sc.score_block(case.users)
    assert np.array_equal(got, case.scores), case


@pytest.mark.parametrize("consumer", sorted(rc.SPECIAL_CONSUMERS))
@pytest.mark.parametrize("k", [16, 10])
def test_special_values_rank(k, consumer):
    """G: +inf, -inf, zeros of either sign and subnormal scores through the fused kernel, the select and the full sort"""
    rank_and_check(rc.special_case(k, consumer))


@pytest.mark.parametrize("k", [16, 10])
def test_special_values_positions_and_scores(k):
    """G: the same tables through rank_positions, and the subnormal scores of score_block as bits"""
    case = rc.special_case(k, "positions")
    with scorer(case) as sc:
        got = sc.rank_positions(case.users, rc.csr(case.props["targets"]))
        block = sc.score_block(case.users)
    rc.check_positions(case, *got)
    assert np.array_equal(block, case.scores), case
    sub = list(rc.SUBNORMAL)
    assert np.array_equal(block[:, sub].view(np.uint32), case.scores[:, sub].view(np.uint32)), case
