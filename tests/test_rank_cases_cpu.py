"""tests/rank_cases.py held to account, without a device: every case has the property it is named for (computed from the
oracle's scores); a NumPy restatement of each ranking path's STRUCTURE — radix select on the 64-bit key, per-chunk sort +
merge, per-segment top-k + merge, position counts on the keys — passes the checker on the cases of that path; and each
restatement with one of the mistakes such a kernel can make fails the checker on the case meant to catch it."""
import re

import numpy as np
import pytest

import rank_cases as rc

U64 = np.uint64


@pytest.fixture(autouse=True)
def _subnormals_are_numbers():
    with rc.ieee_subnormals():      # (whatever an earlier test of the session loaded: see rank_cases.ieee_subnormals)
        yield


# ---- the kernels' key -----------------------------------------------------------------------------------------------------
def order_key(s, signed_zeros=False):
    s = np.asarray(s, np.float32)
    if not signed_zeros:
        s = s + np.float32(0.0)                       # -0.0 -> +0.0: one key for both
    b = s.view(np.uint32)
    k = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    return np.where(k == 0, 1, k).astype(np.uint32)


def key_to_float(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def row_keys(scores_row, dead_row, mutant):
    """[order key | item index], 0 for an excluded item"""
    n = len(scores_row)
    idx = np.arange(n, dtype=U64)
    low = U64(0xFFFFFFFF) - idx if mutant == "ascending_ties" else idx
    keys = (order_key(scores_row, mutant == "signed_zeros").astype(U64) << U64(32)) | low
    if dead_row is not None:
        keys[dead_row] = 0
    if mutant == "drop_last" and n % 32 == 1:
        keys[-1] = 0
    return keys


def unpack(keys, topk, mutant):
    keys = np.concatenate([keys[:topk], np.zeros(max(0, topk - len(keys)), U64)])
    low = (keys & U64(0xFFFFFFFF)).astype(np.int64)
    items = (0xFFFFFFFF - low if mutant == "ascending_ties" else low).astype(np.int32)
    scores = key_to_float((keys >> U64(32)).astype(np.uint32))
    items[keys == 0] = 0 if mutant == "pad_item_0" else -1
    scores[keys == 0] = -np.inf
    return items, scores


def desc(keys):
    return np.sort(keys)[::-1]


# ---- the three ranking structures, one row at a time ---------------------------------------------------------------------
def radix_select(keys, scores_row, topk, mutant):
    """topk_select_kernel: 8 passes of an MSB radix select find the topk-th largest key, the keys at or above it are sorted"""
    prefix, rem = 0, topk
    for p in range(8):
        shift = 56 - 8 * p
        sel = keys if p == 0 else keys[(keys >> U64(shift + 8)) == U64(prefix)]
        hist = np.bincount(((sel >> U64(shift)) & U64(255)).astype(np.int64), minlength=256)
        acc, b = 0, 255
        while b > 0 and acc + hist[b] < rem:
            acc += hist[b]
            b -= 1
        rem -= acc
        prefix = (prefix << 8) | b
    return desc(keys[(keys >= U64(prefix)) & (keys != 0)])


def chunk_sort_merge(keys, scores_row, topk, mutant, chunk=rc.SORT_CHUNK):
    """full_sort_kernel: keys padded to a power of two, every chunk sorted, sorted runs merged pairwise"""
    n_pad = 1 << (len(keys) - 1).bit_length()
    keys = np.concatenate([keys, np.zeros(n_pad - len(keys), U64)])
    run = min(chunk, n_pad)
    keys = np.concatenate([desc(keys[c:c + run]) for c in range(0, n_pad, run)])
    while run < n_pad and mutant != "not_merged":
        run *= 2
        keys = np.concatenate([desc(keys[c:c + run]) for c in range(0, n_pad, run)])   # (a merge of two sorted halves)
    return keys


def segment_topk_merge(keys, scores_row, topk, mutant, dead_row=None, n_segments=4):
    """rank_fused_kernel + rank_merge_kernel: the items in a visit order of their own, cut into segments; every segment
    keeps its topk best candidates among those at or above the running threshold (the topk-th score of a list seen so far:
    a lower bound of the row's topk-th, so nothing that belongs to the result is lost); the lists are merged.
    (late_exclusions: `keys` come without the exclusions; they are applied to each list after it raised the threshold)"""
    n = len(keys)
    visit = np.random.RandomState(n).permutation(n)
    seg = -(-n // n_segments)
    parts, tau = [], -np.inf
    for s0 in range(0, n, seg):
        it = visit[s0:s0 + seg]
        it = it[scores_row[it] >= tau]
        top = desc(keys[it])[:topk]
        top = top[top != 0]
        if len(top) == topk:
            tau = max(tau, key_to_float(np.uint32(top[-1] >> U64(32)))[()])
        if mutant == "late_exclusions" and dead_row is not None:
            top = top[~dead_row[(top & U64(0xFFFFFFFF)).astype(np.int64)]]
        parts.append(top)
    return desc(np.concatenate(parts))


def rank_restated(case, path, mutant=None, rows=None):
    """a case through one of the structures, in batches of case.props['batch'] rows where the case has any"""
    batch = case.props.get("batch", case.n_rows)
    rows = range(case.n_rows) if rows is None else rows
    items = np.empty((case.n_rows, case.topk), np.int32)
    scores = np.empty((case.n_rows, case.topk), np.float32)
    for r in rows:
        b0 = r // batch * batch
        dead = None if case.mask is None else case.mask[r - b0 if mutant == "first_batch_lists" else r]
        if path is segment_topk_merge:
            keys = row_keys(case.scores[r], None if mutant == "late_exclusions" else dead, mutant)
            out = path(keys, case.scores[r], case.topk, mutant, dead_row=dead)
        else:
            out = path(row_keys(case.scores[r], dead, mutant), case.scores[r], case.topk, mutant)
        items[r], scores[r] = unpack(out, case.topk, mutant)
    return items, scores


def check_rows(case, path, mutant=None, rows=None):
    """check_rank on all rows, or on some: the other rows are given the expected result"""
    items, scores = rank_restated(case, path, mutant, rows)
    if rows is not None:
        other = np.setdiff1d(np.arange(case.n_rows), rows)
        items[other], scores[other] = case.want[0][other], case.want[1][other]
    rc.check_rank(case, items, scores)


def caught(case, path, mutant, rows=None):
    with pytest.raises(AssertionError, match=re.escape(case.name)):
        check_rows(case, path, mutant, rows)


def positions_restated(case, mutant=None):
    """rank_positions_kernel: integer compares of the order keys"""
    batch = case.props["batch"] if "batch" in case.props else case.n_rows
    g, p, ge, sc = [], [], [], []
    for r, tg in enumerate(case.props["targets"]):
        b0 = r // batch * batch
        dead = None if case.mask is None else case.mask[r - b0 if mutant == "first_batch_lists" else r]
        keys = row_keys(case.scores[r], dead, mutant)
        hi = keys >> U64(32)
        for t in tg:
            if t < 0 or t >= case.n_items or keys[t] == 0:
                g.append(-1), p.append(-1), ge.append(-1), sc.append(-np.inf)
                continue
            g.append(int((hi > hi[t]).sum())), p.append(int((keys > keys[t]).sum()))
            ge.append(int(((hi >= hi[t]) & (keys != 0)).sum())), sc.append(case.scores[r][t])
    return np.array(g), np.array(p), np.array(ge), np.array(sc, np.float32)


# ---- the rule and the checker themselves -----------------------------------------------------------------------------------
def test_vectorised_rule_equals_the_row_rule_and_oracle_rank():
    from oracle import oracle as orc

    for case in (rc.special_case(16, "select"), rc.select_case(2500, 64, 16, True), rc.sort_case(8193, 2049, True)):
        items, scores = case.want
        for r in range(case.n_rows):
            cand = np.arange(case.n_items) if case.mask is None else np.flatnonzero(~case.mask[r])
            it, sc = rc.expected(case.scores[r], cand, case.topk)
            assert np.array_equal(items[r], it) and np.array_equal(scores[r], sc), (case, r)
            ranked, _ = orc.rank(case.scores[r], case.n_items, case.n_items, item_indices=cand, k=case.topk)
            assert np.array_equal(it[:len(ranked)], ranked), (case, r)


def test_checker_names_case_row_and_position():
    case = rc.select_case(2500, 33, 16, True)
    items, scores = (a.copy() for a in case.want)
    rc.check_rank(case, items, scores)
    items[7, 4], items[7, 5] = items[7, 5], items[7, 4]
    with pytest.raises(AssertionError, match=r"D/2500x33/k16\+excl: row 7 position 4"):
        rc.check_rank(case, items, scores)
    items, scores = (a.copy() for a in case.want)
    scores[9, 2] = np.nextafter(scores[9, 2], np.float32(np.inf))
    with pytest.raises(AssertionError, match="row 9 position 2"):
        rc.check_rank(case, items, scores)
    short = rc.SELECT_SHORT_ROWS[0]
    scores = case.want[1].copy()
    scores[short, 5] = np.finfo(np.float32).min                       # padding must be -inf, not merely low
    with pytest.raises(AssertionError, match="row %d position 5" % short):
        rc.check_rank(case, case.want[0], scores)
    # a zero of the other sign passes (the MFMA chain over padded factors returns +0.0), a flushed subnormal does not
    case = rc.special_case(16, "select")
    items, scores = (a.copy() for a in case.want)
    zero = np.isin(items, rc.NEG_ZERO)
    assert zero.any()
    scores[zero] = 0.0
    rc.check_rank(case, items, scores)
    sub = np.isin(items, rc.SUBNORMAL)
    scores[sub] = 0.0
    with pytest.raises(AssertionError, match="G/k16/select"):
        rc.check_rank(case, items, scores)


# ---- A ---------------------------------------------------------------------------------------------------------------------
def test_score_cases_sit_on_the_padding_boundaries():
    lds = {}
    for k in rc.SCORE_KS:
        case = rc.score_case(k, True)
        lds.setdefault(case.t.ld, []).append(k)
        assert case.n_rows == 2 * 4 * 32 + 1 and case.n_items % 32 != 0
        sub = case.props["subset"]
        assert len(np.unique(sub)) < len(sub) and not np.array_equal(sub, np.sort(sub)) and sub.max() == 256
        assert case.scores.shape == (257, 333) and np.isfinite(case.scores).all()
    assert lds == {16: [16], 32: [17, 24, 31, 32], 64: [33, 64], 128: [65, 128], 129: [129]}
    assert rc.score_case(16, False).t.ub is None


# ---- B ---------------------------------------------------------------------------------------------------------------------
def test_fused_cases_cover_every_instantiation_once():
    inst = [rc.fused_instantiation(k, topk, ub) for k, topk, ub, _ in rc.FUSED]
    want = {(kt, cap, ub) for kt in (8, 16, 32, 64) for cap in (56, 64) for ub in (False, True)}
    want |= {(64, 42, False), (64, 42, True)}
    assert len(inst) == len(set(inst)) and set(inst) == want
    assert {k for k, _, _, _ in rc.FUSED} == {16, 24, 32, 33, 64, 128}
    assert {t for _, t, _, _ in rc.FUSED} == {10, 11, 24, 25, 32}
    assert sum(e for _, _, _, e in rc.FUSED) * 2 == len(rc.FUSED)
    assert rc.FUSED_USERS == 128 + 2 and rc.FUSED_ITEMS // 32 == 625


@pytest.mark.parametrize("k,topk,with_ub,with_excl", rc.FUSED)
def test_fused_case_is_fair_and_sharp(k, topk, with_ub, with_excl):
    case = rc.fused_case(k, topk, with_ub, with_excl)
    assert (case.t.ub is not None) == with_ub
    rows = [0, 1, 2, 64, 129] if with_excl else [5, 129]
    items = case.want[0]
    tied = (np.isin(items, np.arange(1000, 1040)) | np.isin(items, np.arange(15000, 15040))).any(1)
    rows += list(np.flatnonzero(tied)[:3])
    assert tied.sum() >= 10, "exact ties between distant tiles must reach the top of some rows"
    check_rows(case, segment_topk_merge, rows=rows)
    caught(case, segment_topk_merge, "ascending_ties", rows)
    if with_excl:
        for r in case.props["wall_rows"]:
            wall = case.excl_rows[r]
            assert len(wall) == rc.WALL and case.scores[r][wall].min() >= np.delete(case.scores[r], wall).max()
        assert len(case.excl_rows[1]) == 0 and list(case.excl_rows[2]) == [0, case.n_items - 1]
        caught(case, segment_topk_merge, "late_exclusions", list(case.props["wall_rows"]))


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_items", rc.LIMIT_ITEMS)
def test_limit_case_is_fair_and_sharp(n_items):
    tiles = -(-n_items // 32)
    assert (tiles <= 8192) == (n_items == rc.N_BITMAP_ITEMS)
    for topk in (10, 32):
        case = rc.limit_case(n_items, topk)
        assert case.props["bitmap"] == (tiles <= 8192) and case.n_rows == 40 and case.t.k == 16
        assert all((np.diff(r) > 0).all() for r in case.excl_rows), "the no-bitmap path needs strictly sorted lists"
        wall = case.excl_rows[rc.LIMIT_WALL_ROW]
        s = case.scores[rc.LIMIT_WALL_ROW]
        assert len(wall) == rc.LIMIT_WALL and s[wall].min() >= np.delete(s, wall).max()
        assert case.n_live[rc.LIMIT_SHORT_ROW] == 3 < topk and case.n_live[rc.LIMIT_EMPTY_ROW] == n_items
        assert (case.want[0][rc.LIMIT_SHORT_ROW][3:] == -1).all() and n_items - 1 in case.want[0][rc.LIMIT_SHORT_ROW][:3]
        assert list(case.excl_rows[rc.LIMIT_ENDS_ROW]) == [0, n_items - 1]
        rows = [rc.LIMIT_WALL_ROW, rc.LIMIT_EMPTY_ROW, rc.LIMIT_ENDS_ROW, rc.LIMIT_SHORT_ROW, 17]
        check_rows(case, segment_topk_merge, rows=rows)
        caught(case, segment_topk_merge, "late_exclusions", [rc.LIMIT_WALL_ROW])
        caught(case, segment_topk_merge, "pad_item_0", [rc.LIMIT_SHORT_ROW])
        if n_items % 32 == 1:
            caught(case, segment_topk_merge, "drop_last", [rc.LIMIT_SHORT_ROW])
    # the same lists on both sides of the limit, but for the rows that are about the catalogue's own size
    a, b = rc.limit_case(rc.LIMIT_ITEMS[0], 10).excl_rows, rc.limit_case(rc.LIMIT_ITEMS[1], 10).excl_rows
    own = (rc.LIMIT_WALL_ROW, rc.LIMIT_ENDS_ROW, rc.LIMIT_SHORT_ROW)
    assert all(np.array_equal(a[r], b[r]) for r in range(40) if r not in own)


# ---- D ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_excl", [False, True])
@pytest.mark.parametrize("n_items,topk,k", rc.SELECT)
def test_select_case_is_fair_and_sharp(n_items, topk, k, with_excl):
    case = rc.select_case(n_items, topk, k, with_excl)
    assert rc.FUSED_MAX < topk <= rc.SELECT_MAX or k > 128, "neither the fused kernel nor the full sort"
    run = case.props["run"]
    S = case.scores
    assert len(run) == min(rc.RUN, n_items // 3) and (S[:, run] == S[:, run[:1]]).all()
    if topk < n_items:
        live = np.ones_like(S, bool) if case.mask is None else ~case.mask
        above = ((S > S[:, run[:1]]) & live).sum(1)
        in_run = live[:, run].sum(1)
        straddles = (above < topk) & (above + in_run > topk)
        assert straddles.mean() >= 0.5, "the run of equal scores must straddle topk in half the rows: %r" % straddles.mean()
    if with_excl:
        assert all(case.n_live[r] == 5 < topk for r in case.props["short_rows"])
    check_rows(case, radix_select)
    caught(case, radix_select, "ascending_ties")
    if with_excl:
        caught(case, radix_select, "pad_item_0", list(case.props["short_rows"]))
    if n_items % 32 == 1:
        caught(case, radix_select, "drop_last")


# ---- E ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_excl", [False, True])
@pytest.mark.parametrize("n_items,topk", rc.SORT)
def test_sort_case_is_fair_and_sharp(n_items, topk, with_excl):
    case = rc.sort_case(n_items, topk, with_excl)
    assert topk > rc.SELECT_MAX and case.n_rows == 6 and case.t.k == 12
    assert case.props["n_pad"] == {2049: 4096, 8192: 8192, 8193: 16384, 20_000: 32768, 70_000: 131072}[n_items]
    S = case.scores
    if n_items >= rc.SORT_CHUNK + rc.SORT_DUP[1]:
        i = np.arange(*rc.SORT_DUP)
        assert (S[:, i] == S[:, i + rc.SORT_CHUNK]).all() and (i // rc.SORT_CHUNK != (i + rc.SORT_CHUNK) // rc.SORT_CHUNK).all()
    if n_items > rc.SORT_CHUNK:
        lo, hi = rc.SORT_RUN[0], min(rc.SORT_RUN[1], n_items)
        assert (S[:, lo:hi] == S[:, lo:lo + 1]).all() and lo // rc.SORT_CHUNK != (hi - 1) // rc.SORT_CHUNK
    if with_excl:
        assert case.n_live[5] == 7 < topk and (case.want[0][5][7:] == -1).all()
    check_rows(case, chunk_sort_merge)
    caught(case, chunk_sort_merge, "ascending_ties")
    if case.props["n_pad"] > rc.SORT_CHUNK:
        caught(case, chunk_sort_merge, "not_merged")
    if with_excl:
        caught(case, chunk_sort_merge, "pad_item_0", [5])
    if n_items % 32 == 1 and topk == n_items:
        caught(case, chunk_sort_merge, "drop_last")


def test_sort_batch_case_is_fair_and_sharp():
    case = rc.sort_batch_case()
    b = case.props["batch"]
    assert case.n_rows > b == rc.SORT_BATCH_ROWS and case.topk > rc.SELECT_MAX
    assert all(len(case.excl_rows[r]) >= 100 for r in range(b - 4, case.n_rows))
    rows = list(range(b - 4, case.n_rows)) + [0, 1, 500]
    check_rows(case, chunk_sort_merge, rows=rows)
    caught(case, chunk_sort_merge, "first_batch_lists", rows)


# ---- F ---------------------------------------------------------------------------------------------------------------------
def test_batch_case_is_fair_and_sharp():
    case = rc.batch_case()
    b = case.props["batch"]
    assert case.n_rows == b + 37 and b == rc.BATCH_ROWS and rc.FUSED_MAX < case.topk <= rc.SELECT_MAX
    second = range(b, case.n_rows)
    assert sum(not np.array_equal(case.excl_rows[r], case.excl_rows[r - b]) for r in second) >= 30
    assert {len(t) for t in case.props["targets"]} == set(range(10))
    assert not np.array_equal(case.users, np.sort(case.users))
    rows = list(second) + list(range(0, 200))
    check_rows(case, radix_select, rows=rows)
    caught(case, radix_select, "first_batch_lists", rows)
    rc.check_positions(case, *positions_restated(case))
    with pytest.raises(AssertionError, match="F/batch: row") as e:
        rc.check_positions(case, *positions_restated(case, "first_batch_lists"))
    assert int(re.search(r"row (\d+)", str(e.value)).group(1)) >= b


# ---- G ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 10])
def test_special_case_is_fair_and_sharp(k):
    t = rc.special_case(k, "sort").t
    S = t.scores
    assert not np.isnan(S).any()
    assert (S[:, list(rc.NEG_ZERO)].view(np.uint32) == 0x80000000).all(), "the oracle scores these -0.0"
    assert (S[:, list(rc.POS_ZERO)].view(np.uint32) == 0).all()
    sub = S[:, list(rc.SUBNORMAL)]
    assert (sub != 0).all() and (np.abs(sub) < 2.0 ** -126).all()
    assert np.isposinf(S[:, list(rc.POS_INF)]).all() and np.isneginf(S[:, list(rc.NEG_INF)]).all()
    ordinary = np.delete(S, list(rc.POS_INF + rc.NEG_INF + rc.NEG_ZERO + rc.POS_ZERO + rc.SUBNORMAL), axis=1)
    assert (ordinary > 1).sum(1).min() == len(rc.POSITIVE) and ((ordinary < -1).sum(1) == ordinary.shape[1] - 2).all()
    zeros = np.array(sorted(rc.NEG_ZERO + rc.POS_ZERO, reverse=True))
    full = rc.special_case(k, "sort")
    for r in range(full.n_rows):
        at = int(np.flatnonzero(full.want[0][r] == zeros[0])[0])
        assert np.array_equal(full.want[0][r][at:at + 12], zeros), "the twelve zeros tie: descending index"
    assert list(full.want[0][0][-3:]) == sorted(rc.NEG_INF, reverse=True) and np.isneginf(full.want[1][0][-3:]).all()
    fused = rc.special_case(k, "fused")
    inside = np.isin(fused.want[0][:, 9], zeros)              # (twelve zeros, at most ten places: the next one is a zero too)
    assert inside.mean() >= 0.5, "topk 10 must end inside the tied zeros in half the rows: %r" % inside.mean()
    assert np.isin(rc.special_case(k, "select").want[0], zeros).sum(1).min() == 12
    for consumer, path in (("fused", segment_topk_merge), ("select", radix_select), ("sort", chunk_sort_merge)):
        case = rc.special_case(k, consumer)
        check_rows(case, path)
        caught(case, path, "signed_zeros")
        caught(case, path, "ascending_ties")
    case = rc.special_case(k, "positions")
    hit = np.concatenate(case.props["targets"])
    assert all(np.isin(g, hit).any() for g in (rc.POS_INF, rc.NEG_INF, rc.NEG_ZERO, rc.POS_ZERO, rc.SUBNORMAL))
    rc.check_positions(case, *positions_restated(case))
    with pytest.raises(AssertionError, match="G/k%d/positions" % k):
        rc.check_positions(case, *positions_restated(case, "signed_zeros"))
