"""The ranking checks' rule, cases and checker, in ONE place: tests/test_rank_cases_cpu.py holds the cases to the property
each is named for and shows that the checker catches the mistakes a ranking kernel can make; tests/test_rank_paths_gpu.py
runs every case through the device and hands the result to the checker.  NumPy only, plus `oracle.score_block` (the
index-ordered fmaf chain in C) for the scores.

The pinned rule (`oracle.rank`): descending score, ties by descending item index, `-0.0 == +0.0` a tie; excluded items
are no candidates; a row with fewer than `topk` candidates is padded with `(-1, -inf)`.  `expected` states it for one
row, `expected_rows` for a block of rows (a stable ascending argsort of each row, read backwards).

Everything is exact: items are integers, scores are compared with `np.array_equal` against the oracle's scores of the
returned items (`bit_items`: as `uint32` where the case says so), so there are no tolerances here, only shapes.  Every
shape is the smallest at which the path it is named for is taken; the docstring of each builder says which.
"""
import contextlib
import ctypes
import functools

import numpy as np

N_BITMAP_ITEMS = 262_144      # 8192 tiles of 32 items: the largest catalogue that ranks with the exclusion bitmap
SORT_CHUNK = 8192             # keys per LDS chunk of the full sort
SELECT_MAX = 2048             # largest topk of the radix select
FUSED_MAX = 32                # largest topk of the fused kernel
BATCH_ROWS = 16_384           # rows per batch of the materialised paths (small catalogue)
SORT_BATCH_ROWS = 1024        # ... of the full sort


def _orc():
    from oracle import oracle as orc

    orc.build()
    return orc


@contextlib.contextmanager
def ieee_subnormals():
    """Loading a shared library that was linked with -ffast-math (the oracle's timing build, the reference's extensions)
    switches the loading thread to flush-to-zero / denormals-are-zero for the rest of the process; NumPy and the oracle then
    compute and COMPARE subnormals as zeros.  Inside this block the calling thread has the default floating-point
    environment; the previous one is put back afterwards.  (The oracle's worker threads keep the mode they were created in:
    a case with subnormal scores has the oracle score one user per call, which the calling thread executes.)"""
    try:
        libm = ctypes.CDLL("libm.so.6")
        saved = ctypes.create_string_buffer(64)           # fenv_t
        libm.fegetenv(saved)
        libm.fesetenv(ctypes.c_void_p(-1))                # FE_DFL_ENV
    except (OSError, AttributeError):
        libm = None
    try:
        yield
    finally:
        if libm is not None:
            libm.fesetenv(saved)


# ---- the rule ------------------------------------------------------------------------------------------------------------
def expected(scores_row, cand, topk):
    """the first `topk` of the candidates `cand` (item ids) of one row: (items int32[topk], scores float32[topk])"""
    cand = np.asarray(cand, np.int64)
    order = np.argsort(scores_row[cand], kind="stable")[::-1]
    top = cand[order][:topk]
    items = np.full(topk, -1, np.int32)
    scores = np.full(topk, -np.inf, np.float32)
    items[:len(top)] = top
    scores[:len(top)] = scores_row[top]
    return items, scores


def csr(rows):
    """lists per row -> (indptr int64, indices int32)"""
    indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    indices = np.concatenate([np.asarray(r, np.int32) for r in rows] + [np.empty(0, np.int32)]).astype(np.int32)
    return indptr, indices


def csr_mask(lists, n_rows, n_items):
    """CSR of item lists -> bool [n_rows, n_items]"""
    mask = np.zeros((n_rows, n_items), bool)
    if lists is not None:
        indptr, indices = lists
        mask[np.repeat(np.arange(n_rows), np.diff(indptr)), indices] = True
    return mask


def expected_rows(scores, mask, topk):
    """`expected` over the rows of `scores` [rows, n_items]; `mask` (bool, same shape, or None) marks excluded items"""
    n_rows, n_items = scores.shape
    order = np.argsort(scores, axis=1, kind="stable")[:, ::-1]
    n_live = np.full(n_rows, n_items, np.int64)
    if mask is not None and mask.any():
        dead = np.take_along_axis(mask, order, 1)
        live_first = np.argsort(dead, axis=1, kind="stable")[:, :topk]    # the live ones first, their order kept
        order = np.take_along_axis(order, live_first, 1)
        n_live -= mask.sum(1)
    order = np.ascontiguousarray(order[:, :topk])
    pad = np.arange(topk)[None, :] >= n_live[:, None]
    want_scores = np.take_along_axis(scores, order, 1).astype(np.float32)
    items = order.astype(np.int32)
    items[pad] = -1
    want_scores[pad] = -np.inf
    return items, want_scores


# ---- a case --------------------------------------------------------------------------------------------------------------
class Tables:
    """factor tables, the users ranked, and the oracle's scores of those users (computed once)"""

    def __init__(self, U, V, ib, ub, users, user_by_user=False):
        self.U, self.V, self.ib, self.ub, self.user_by_user = U, V, ib, ub, user_by_user
        self.users = np.ascontiguousarray(users, np.int32)
        self.n_items, self.k = V.shape
        self.ld = next((p for p in (16, 32, 64, 128) if self.k <= p), self.k)   # padded row length on the device

    @functools.cached_property
    def scores(self):
        orc = _orc()
        with ieee_subnormals():
            if self.user_by_user:
                s = np.concatenate([orc.score_block(self.U, self.V, self.ib, self.ub, self.users[r:r + 1])
                                    for r in range(len(self.users))])
            else:
                s = orc.score_block(self.U, self.V, self.ib, self.ub, self.users)
        s.setflags(write=False)
        return s


class Case:
    """one ranking call: tables, users, topk, optional exclusion CSR (per row of the call), and what it is for"""

    def __init__(self, name, tables, topk, excl_rows=None, bit_items=None, **props):
        self.name, self.t, self.topk = name, tables, topk
        self.excl_rows = excl_rows
        self.excl = None if excl_rows is None else csr(excl_rows)
        self.bit_items = bit_items      # bool [n_items]: items whose scores must match the oracle's as uint32
        self.props = props

    users = property(lambda self: self.t.users)
    scores = property(lambda self: self.t.scores)
    n_rows = property(lambda self: len(self.t.users))
    n_items = property(lambda self: self.t.n_items)

    @functools.cached_property
    def mask(self):
        return None if self.excl is None else csr_mask(self.excl, self.n_rows, self.n_items)

    @functools.cached_property
    def want(self):
        scores = self.scores
        with ieee_subnormals():
            return expected_rows(scores, self.mask, self.topk)

    @property
    def n_live(self):
        return np.full(self.n_rows, self.n_items) if self.mask is None else self.n_items - self.mask.sum(1)

    def __repr__(self):
        return self.name


def check_rank(case, items, scores):
    """a [rows, topk] result against the rule: items exactly, scores equal to the oracle's scores of the returned items,
    padding exactly (-1, -inf); names the case, the row and the first differing position"""
    want_items, want_scores = case.want
    with ieee_subnormals():
        _check_rank(case, want_items, want_scores, np.asarray(items), np.asarray(scores))


def _check_rank(case, want_items, want_scores, items, scores):
    assert items.shape == want_items.shape and scores.shape == want_scores.shape, \
        "%s: result shape %r / %r, wanted %r" % (case.name, items.shape, scores.shape, want_items.shape)
    bad = items != want_items
    if bad.any():
        r = int(np.flatnonzero(bad.any(1))[0])
        p = int(np.flatnonzero(bad[r])[0])
        raise AssertionError("%s: row %d position %d: item %d (score %r), wanted item %d (score %r); row has %d candidates"
                             % (case.name, r, p, items[r, p], scores[r, p], want_items[r, p], want_scores[r, p],
                                case.n_live[r]))
    pad = want_items < 0
    ref = np.take_along_axis(case.scores, np.where(pad, 0, items).astype(np.int64), 1)
    ref[pad] = -np.inf
    same = (scores == ref)
    if case.bit_items is not None:
        strict = ~pad & case.bit_items[np.where(pad, 0, items)]
        same &= ~strict | (scores.view(np.uint32) == ref.view(np.uint32))
    if not same.all():
        r = int(np.flatnonzero(~same.all(1))[0])
        p = int(np.flatnonzero(~same[r])[0])
        raise AssertionError("%s: row %d position %d (item %d): score %r (0x%08x), the oracle's is %r (0x%08x)"
                             % (case.name, r, p, items[r, p], scores[r, p], scores.view(np.uint32)[r, p], ref[r, p],
                                ref.view(np.uint32)[r, p]))


def expected_positions(case):
    """per target of `case.props['targets']`: (greater, pos, ge, score); an excluded or out-of-range target gets
    (-1, -1, -1, -inf).  greater = candidates scored strictly higher, pos = place in the ranked order, ge = candidates scored
    at least as high (the target included)"""
    S, mask = case.scores, case.mask
    out = []
    for r, tg in enumerate(case.props["targets"]):
        live = np.ones(case.n_items, bool) if mask is None else ~mask[r]
        cand = np.flatnonzero(live)
        s_c = S[r][cand]
        for t in tg:
            if t < 0 or t >= case.n_items or not live[t]:
                out.append((-1, -1, -1, -np.inf))
                continue
            s = S[r][t]
            g = int((s_c > s).sum())
            out.append((g, g + int(((s_c == s) & (cand > t)).sum()), int((s_c >= s).sum()), s))
    return out


def check_positions(case, greater, pos, ge, tgt_scores):
    with ieee_subnormals():
        _check_positions(case, greater, pos, ge, tgt_scores)


def _check_positions(case, greater, pos, ge, tgt_scores):
    want = case.props.get("want_positions")
    if want is None:
        want = case.props["want_positions"] = expected_positions(case)
    assert len(greater) == len(pos) == len(ge) == len(tgt_scores) == len(want), "%s: %d targets, wanted %d" % (
        case.name, len(greater), len(want))
    p = 0
    for r, tg in enumerate(case.props["targets"]):
        for t in tg:
            got = (int(greater[p]), int(pos[p]), int(ge[p]))
            assert got == want[p][:3] and tgt_scores[p] == want[p][3], \
                "%s: row %d target %d: (greater, pos, ge, score) = %r + (%r,), wanted %r" % (case.name, r, t, got,
                                                                                           tgt_scores[p], want[p])
            p += 1


# ---- ingredients ---------------------------------------------------------------------------------------------------------
def _normal_tables(n_users, n_items, k, seed, with_ub, ib_std=0.2):
    rs = np.random.RandomState(seed)
    U = rs.normal(0, 0.3, (n_users, k)).astype(np.float32)
    V = rs.normal(0, 0.3, (n_items, k)).astype(np.float32)
    ib = rs.normal(0, ib_std, n_items).astype(np.float32)
    ub = rs.normal(0, 0.2, n_users).astype(np.float32) if with_ub else None
    return rs, U, V, ib, ub


def _random_rows(rs, n_rows, n_items, max_len):
    return [np.sort(rs.choice(n_items, rs.randint(0, max_len + 1), replace=False)).astype(np.int32) for _ in range(n_rows)]


def best_of(scores_row, n, cand=None):
    """the row's `n` best items by the rule, as a sorted list"""
    cand = np.arange(len(scores_row)) if cand is None else cand
    return np.sort(expected(scores_row, cand, n)[0]).astype(np.int32)


# ---- A: the score kernels at the padding boundaries ----------------------------------------------------------------------
SCORE_KS = (16, 17, 24, 31, 32, 33, 64, 65, 128, 129)


@functools.lru_cache(maxsize=None)
def score_case(k, with_ub):
    """257 users x 333 items: one row over a full workgroup of the two-row-tile MFMA kernels (4 waves x 2 x 32 rows), ragged
    last row and item tiles.  k = 16 | 17..32 | 33..64 | 65..128 | 129 run score_gemm_mfma_kernel<8,2> | <16,2> | <32,2> |
    <64,1> | score_valu_kernel through score_block; score_user and score_pairs are the VALU chains at the same k."""
    rs, U, V, ib, ub = _normal_tables(257, 333, k, 1000 + k, with_ub)
    t = Tables(U, V, ib, ub, np.arange(257))
    subset = np.concatenate([rs.permutation(257)[:90], [256, 0, 256, 5, 5]]).astype(np.int32)   # permuted, with repeats
    pu, pi = rs.randint(0, 257, 500).astype(np.int32), rs.randint(0, 333, 500).astype(np.int32)
    return Case("A/k%d%s" % (k, "+ub" if with_ub else ""), t, 1, subset=subset, pairs=(pu, pi), single_user=256)


# ---- B: every instantiation of the fused kernel --------------------------------------------------------------------------
# (k, topk, user base, exclusions) -> rank_fused_kernel<KT = ld / 2, CAP, UB>; one line per instantiation
FUSED = (
    (16, 10, False, True),     # < 8, 56, false>
    (16, 24, True, False),     # < 8, 56, true>
    (16, 25, False, False),    # < 8, 64, false>
    (16, 32, True, True),      # < 8, 64, true>
    (24, 24, False, False),    # <16, 56, false>
    (32, 11, True, True),      # <16, 56, true>
    (32, 32, False, False),    # <16, 64, false>
    (24, 25, True, True),      # <16, 64, true>
    (64, 10, False, True),     # <32, 56, false>
    (33, 24, True, False),     # <32, 56, true>
    (33, 25, False, True),     # <32, 64, false>
    (64, 32, True, False),     # <32, 64, true>
    (128, 10, False, False),   # <64, 42, false>
    (128, 10, True, True),     # <64, 42, true>
    (128, 11, False, True),    # <64, 56, false>: one over the topk that takes the 42-slot buffers
    (128, 24, True, False),    # <64, 56, true>
    (128, 32, False, False),   # <64, 64, false>
    (128, 25, True, True),     # <64, 64, true>
)
FUSED_USERS, FUSED_ITEMS, WALL = 130, 20_000, 200
FUSED_WALL_ROWS = (0, 129)


def fused_instantiation(k, topk, with_ub):
    ld = next(p for p in (16, 32, 64, 128) if k <= p)
    cap = 42 if (topk <= 10 and ld == 128) else 56 if topk <= 24 else 64
    return ld // 2, cap, with_ub


@functools.lru_cache(maxsize=4)
def _fused_tables(k, with_ub):
    rs, U, V, ib, ub = _normal_tables(FUSED_USERS, FUSED_ITEMS, k, 2000 + k, with_ub)
    ib[15000:15040] += np.float32(1.0)                                # (high enough to reach the top of many rows)
    V[1000:1040], ib[1000:1040] = V[15000:15040], ib[15000:15040]     # exact ties between distant tiles
    return Tables(U, V, ib, ub, np.arange(FUSED_USERS))


@functools.lru_cache(maxsize=4)
def fused_case(k, topk, with_ub, with_excl):
    """130 users (the second row block has 2 live rows of 128) x 20 000 items (625 tiles: tens of segments per row block,
    the threshold hand-off between them, rank_merge_kernel over a list padded to a power of two).  With exclusions
    (through the bitmap): rows 0 and 129 exclude their own 200 best items, row 1 nothing, row 2 items 0 and n_items - 1."""
    t = _fused_tables(k, with_ub)
    rows = None
    if with_excl:
        rs = np.random.RandomState(k * 100 + topk)
        rows = _random_rows(rs, FUSED_USERS, FUSED_ITEMS, 60)
        for r in FUSED_WALL_ROWS:
            rows[r] = best_of(t.scores[r], WALL)
        rows[1] = np.empty(0, np.int32)
        rows[2] = np.array([0, FUSED_ITEMS - 1], np.int32)
    return Case("B/k%d/top%d%s%s" % (k, topk, "+ub" if with_ub else "", "+excl" if with_excl else ""), t, topk, rows,
                instantiation=fused_instantiation(k, topk, with_ub), wall_rows=FUSED_WALL_ROWS if with_excl else ())


# ---- C: the bitmap limit ---------------------------------------------------------------------------------------------------
LIMIT_ITEMS = (N_BITMAP_ITEMS, N_BITMAP_ITEMS + 1, N_BITMAP_ITEMS + 33)
LIMIT_USERS, LIMIT_WALL = 40, 500
LIMIT_WALL_ROW, LIMIT_SHORT_ROW, LIMIT_EMPTY_ROW, LIMIT_ENDS_ROW = 0, 3, 1, 2


@functools.lru_cache(maxsize=1)
def _limit_all():
    return _normal_tables(LIMIT_USERS, LIMIT_ITEMS[-1], 16, 3000, False)[1:]


@functools.lru_cache(maxsize=2)
def _limit_tables(n_items):
    U, V, ib, ub = _limit_all()
    return Tables(U, np.ascontiguousarray(V[:n_items]), np.ascontiguousarray(ib[:n_items]), None, np.arange(LIMIT_USERS))


@functools.lru_cache(maxsize=2)
def _limit_rows(n_items):
    t = _limit_tables(n_items)
    rows = _random_rows(np.random.RandomState(3001), LIMIT_USERS, N_BITMAP_ITEMS, 80)   # the same lists at every size
    rows[LIMIT_WALL_ROW] = best_of(t.scores[LIMIT_WALL_ROW], LIMIT_WALL)
    rows[LIMIT_EMPTY_ROW] = np.empty(0, np.int32)
    rows[LIMIT_ENDS_ROW] = np.array([0, n_items - 1], np.int32)
    rows[LIMIT_SHORT_ROW] = np.setdiff1d(np.arange(n_items), [0, n_items // 2, n_items - 1]).astype(np.int32)
    return rows


def limit_case(n_items, topk):
    """k = 16, 40 users; 262 144 items are exactly 8192 tiles (exclusion bitmap), 262 145 and 262 177 one item and one tile
    more (no bitmap: the lists are binary-searched when a row's candidate buffer is compacted).  Row 0 excludes its 500 best
    items (every true winner sits behind excluded survivors at compaction), row 3 keeps three candidates (item 0, the middle
    one and the LAST item), row 1 excludes nothing, row 2 items 0 and n_items - 1; the other rows carry the same sorted
    lists at every size.  rank_fused_kernel<8, 56, false> at topk 10, <8, 64, false> at topk 32."""
    return Case("C/%d/top%d" % (n_items, topk), _limit_tables(n_items), topk, _limit_rows(n_items),
                wall_rows=(LIMIT_WALL_ROW,), short_rows=(LIMIT_SHORT_ROW,), bitmap=n_items <= N_BITMAP_ITEMS)


# ---- D: the radix select ---------------------------------------------------------------------------------------------------
SELECT = ((33, 33, 16), (2048, 2048, 16), (2500, 33, 16), (2500, 64, 16), (2500, 65, 16), (9001, 2047, 16),
          (9001, 2048, 16), (3000, 10, 129), (3000, 10, 200))
SELECT_USERS, RUN = 50, 300


@functools.lru_cache(maxsize=2)
def _select_tables(n_items, topk, k):
    """item bases dominate the scores (sd 1 against 0.03 of the products), so one item has about the same rank for
    every user; the V row and base of the item whose rank is most often inside (topk - run, topk) are copied into a run of
    item slots: `run` bit-equal scores per row, with the topk boundary inside the run"""
    rs, U, V, ib, ub = _normal_tables(SELECT_USERS, n_items, k, 4000 + n_items + topk + k, False, ib_std=1.0)
    U *= np.float32(1.0 / (3.0 * np.sqrt(k)))         # products: sd 0.03
    run = min(RUN, n_items // 3)
    s0 = n_items // 3
    users = np.arange(SELECT_USERS)
    if topk < n_items:
        S = _orc().score_block(U, V, ib, None, users.astype(np.int32))
        keep = np.ones(n_items, bool)
        keep[s0:s0 + run] = False                       # these slots are overwritten
        above = np.empty((SELECT_USERS, n_items), np.int64)   # kept items scored above each item, row by row
        for r in range(SELECT_USERS):
            above[r] = keep.sum() - np.searchsorted(np.sort(S[r][keep]), S[r], side="right")
        inside = ((above < topk) & (above + run > topk)).sum(0)
        src = int(np.argmax(inside))
    else:
        src = 0
    V[s0:s0 + run], ib[s0:s0 + run] = V[src], ib[src]
    t = Tables(U, V, ib, None, users)
    t.run = np.arange(s0, s0 + run)
    return t


SELECT_SHORT_ROWS = (3, 47)


@functools.lru_cache(maxsize=4)
def select_case(n_items, topk, k, with_excl):
    """50 users, 33 <= topk <= 2048 (k = 16, MFMA scores) or k > 128 with topk = 10 (VALU scores): topk_select_kernel, with
    exclusions behind mark_excluded_kernel.  topk 33 and 2048 are the ends of its range, 64 | 65 and 2047 | 2048 the two
    sides of a power-of-two sort list.  With exclusions rows 3 and 47 keep 5 candidates, row 4 excludes half of the run."""
    t = _select_tables(n_items, topk, k)
    rows = None
    if with_excl:
        rs = np.random.RandomState(n_items + topk)
        rows = _random_rows(rs, SELECT_USERS, n_items, min(40, n_items // 2))
        for r in SELECT_SHORT_ROWS:
            rows[r] = np.sort(rs.permutation(n_items)[5:]).astype(np.int32)
        rows[4] = t.run[::2].astype(np.int32)
    return Case("D/%dx%d/k%d%s" % (n_items, topk, k, "+excl" if with_excl else ""), t, topk, rows, run=t.run,
                short_rows=SELECT_SHORT_ROWS if with_excl else ())


# ---- E: the full sort ------------------------------------------------------------------------------------------------------
SORT = ((2049, 2049), (8192, 8192), (8193, 8193), (8193, 2049), (20_000, 20_000), (70_000, 70_000))
SORT_DUP, SORT_RUN = (100, 150), (8140, 8240)


def _sort_ties(V, ib):
    n = len(ib)
    V[1000:1010], ib[1000:1010] = V[1000], ib[1000]
    a, b = SORT_DUP
    if n >= SORT_CHUNK + b:
        V[SORT_CHUNK + a:SORT_CHUNK + b], ib[SORT_CHUNK + a:SORT_CHUNK + b] = V[a:b], ib[a:b]
    lo, hi = SORT_RUN[0], min(SORT_RUN[1], n)
    if hi > lo:
        ib[lo] += np.float32(0.5)          # (near the top of every row: inside a topk below n_items, too)
        V[lo:hi], ib[lo:hi] = V[lo], ib[lo]


@functools.lru_cache(maxsize=2)
def _sort_tables(n_items):
    rs, U, V, ib, ub = _normal_tables(6, n_items, 12, 5000 + n_items, False)
    _sort_ties(V, ib)
    return Tables(U, V, ib, None, np.arange(6))


def sort_case(n_items, topk, with_excl):
    """6 users, k = 12, topk > 2048: full_sort_kernel.  n_items 2049 | 8192 | 8193 | 20 000 | 70 000 pad to 4096 | 8192 |
    16 384 | 32 768 | 131 072 keys: less than one LDS chunk, exactly one, 2, 4 and 16 chunks (phase B: the merge across
    chunks through the global scratch).  Items 1000..1009 tie, items i and i + 8192 (100 <= i < 150) share a V row, items
    8140..8239 are one run of equal scores across the chunk boundary.  Excluded keys sort to the end and come back as padding; row 5 keeps 7 candidates."""
    t = _sort_tables(n_items)
    rows = None
    if with_excl:
        rs = np.random.RandomState(n_items + topk)
        rows = _random_rows(rs, 6, n_items, 300)
        rows[0] = np.arange(8100, min(8200, n_items), 2, dtype=np.int32) if n_items > 8100 else rows[0]
        rows[5] = np.sort(rs.permutation(n_items)[7:]).astype(np.int32)
    return Case("E/%dx%d%s" % (n_items, topk, "+excl" if with_excl else ""), t, topk, rows,
                n_pad=1 << (n_items - 1).bit_length(), short_rows=(5,) if with_excl else ())


SORT_BATCH_USERS = SORT_BATCH_ROWS + 6


@functools.lru_cache(maxsize=1)
def sort_batch_case():
    """1030 users x 2049 items, topk = 2049: the full sort takes 1024 rows per batch, rows 1024..1029 are a second batch
    (b0 = 1024 offsets the exclusion rows).  Every row has a list of its own; rows 1020..1029 are long ones."""
    rs, U, V, ib, ub = _normal_tables(SORT_BATCH_USERS, 2049, 12, 5999, False)
    t = Tables(U, V, ib, None, np.arange(SORT_BATCH_USERS))
    rows = _random_rows(rs, SORT_BATCH_USERS, 2049, 12)
    for r in range(SORT_BATCH_ROWS - 4, SORT_BATCH_USERS):
        rows[r] = np.sort(rs.choice(2049, 100 + r % 7, replace=False)).astype(np.int32)
    return Case("E/batch", t, 2049, rows, batch=SORT_BATCH_ROWS)


# ---- F: the second batch of the materialised paths -------------------------------------------------------------------------
BATCH_USERS = BATCH_ROWS + 37


@functools.lru_cache(maxsize=1)
def batch_case():
    """16 384 + 37 users x 40 items, k = 8, topk = 33: the select path, score_block and rank_positions each with a second
    batch (b0 = 16 384 offsets the exclusion and target rows).  Every row has its own exclusion list (0..6 items) and
    0..9 targets."""
    rs, U, V, ib, ub = _normal_tables(BATCH_USERS, 40, 8, 6000, True)
    V[30:34], ib[30:34] = V[3], ib[3]
    t = Tables(U, V, ib, ub, rs.permutation(BATCH_USERS))
    lens = rs.randint(0, 7, BATCH_USERS)
    rows = [np.sort(rs.permutation(40)[:n]).astype(np.int32) for n in lens]
    targets = [rs.permutation(40)[:r % 10].astype(np.int32) for r in range(BATCH_USERS)]
    return Case("F/batch", t, 33, rows, targets=targets, batch=BATCH_ROWS)


# ---- G: scores that are not ordinary numbers -------------------------------------------------------------------------------
SPECIAL_ITEMS, SPECIAL_USERS = 2100, 40
POS_INF, NEG_INF = (7, 1033, 2099), (0, 64, 2050)
POSITIVE = (500, 1500)                              # ordinary items above zero; every other ordinary item is below
NEG_ZERO = (100, 102, 104, 1200, 1202, 2090)        # all factors 0 but the last: its product underflows to -0.0
POS_ZERO = (101, 103, 105, 1201, 1203, 2091)        # all factors 0: +0.0
SUBNORMAL = (40, 41, 300, 1700, 1701, 2080)
SPECIAL_CONSUMERS = {"fused": 10, "select": 40, "sort": SPECIAL_ITEMS}


@functools.lru_cache(maxsize=2)
def _special_tables(k):
    """U is about 2^-70 and the ordinary items' V about 2^70, so their products are ordinary numbers; item bases of -5 put
    every ordinary item below zero but two (+5).  user_base is -0.0 for every user and U[:, k - 1] negative, so that
      * a NEG_ZERO item (item base -0.0, V = 0 but V[k - 1] = 2^-100) scores (-0.0 + -0.0) + fma(.., -2^-170 -> -0.0);
      * a POS_ZERO item (item base -0.0, V = 0) scores (-0.0 + -0.0) + (+0.0) = +0.0;
      * a SUBNORMAL item (item base 0, V about 2^-64) has products about 2^-137 and sums below 2^-126;
      * +inf / -inf item bases over finite factors give +inf / -inf (no inf - inf)."""
    rs = np.random.RandomState(7000 + k)
    U = np.ldexp(rs.normal(0, 0.3, (SPECIAL_USERS, k)), -70).astype(np.float32)
    U[:, k - 1] = -np.abs(U[:, k - 1])
    V = np.ldexp(rs.normal(0, 0.3, (SPECIAL_ITEMS, k)), 70).astype(np.float32)
    ib = (rs.normal(0, 0.2, SPECIAL_ITEMS) - 5.0).astype(np.float32)
    ib[list(POSITIVE)] += 10.0
    ib[list(POS_INF)], ib[list(NEG_INF)] = np.inf, -np.inf
    zeros = list(NEG_ZERO + POS_ZERO)
    V[zeros], ib[zeros] = 0.0, -0.0
    V[list(NEG_ZERO), k - 1] = np.float32(2.0 ** -100)
    V[list(SUBNORMAL)] = np.ldexp(rs.normal(0, 0.3, (len(SUBNORMAL), k)), -64).astype(np.float32)
    ib[list(SUBNORMAL)] = 0.0
    ub = np.full(SPECIAL_USERS, -0.0, np.float32)
    return Tables(U, V, ib, ub, np.arange(SPECIAL_USERS), user_by_user=True)


@functools.lru_cache(maxsize=8)
def special_case(k, consumer):
    """40 users x 2100 items at k = 16 (ld == k) and k = 10 (ld != k: the MFMA chain ends in fma(0, 0, acc), which turns a
    -0.0 accumulator into +0.0), ranked by the fused kernel (topk 10: three +inf items, two ordinary ones, the positive
    subnormals, then the boundary inside the twelve tied zeros), the select (topk 40), the full sort (everything: a real item
    scored -inf comes back with its id, last) and rank_positions (targets in every group).  The twelve zeros tie and come in
    descending item index whatever their sign; the subnormal items' scores must match the oracle's bit for bit."""
    t = _special_tables(k)
    bits = np.zeros(SPECIAL_ITEMS, bool)
    bits[list(SUBNORMAL)] = True
    props = {}
    if consumer == "positions":
        rs = np.random.RandomState(k)
        groups = POS_INF + NEG_INF + POSITIVE + NEG_ZERO + POS_ZERO + SUBNORMAL
        props["targets"] = [np.concatenate([rs.permutation(groups)[:r % 9], rs.randint(0, SPECIAL_ITEMS, r % 3)]).astype(np.int32)
                            for r in range(SPECIAL_USERS)]
    return Case("G/k%d/%s" % (k, consumer), t, SPECIAL_CONSUMERS.get(consumer, 1), None, bit_items=bits, **props)
