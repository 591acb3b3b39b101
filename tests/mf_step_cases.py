"""Inputs, references and checks of the hogwild MF step tests, in ONE place: tests/test_mf_step_gpu.py runs the cases on the
device, tests/test_mf_step_cpu.py proves — from the restatements and the float64 step alone — that every case is a fair
test, that the tolerances below follow their rules, and that the checks reject deliberately wrong updates.

MF has no sampler: a launch cornac_hip_mf_epoch_enqueue(part, n_parts, ...) processes exactly the ratings
[nnz part / n_parts, nnz (part + 1) / n_parts) of the stored COO order, so the updates of a launch are known from the
inputs alone.  A case = Zipf pairs in a seeded random order + ratings 1..5 with mu = 3 + normal tables with unit-spread
predictions and two non-zero bias tables + ONE such launch, made three times from the same start tables:

  Z  lr = 0             all four tables bit-identical (so the bias_pad / bias_unpad round trip and the copies' fold-back are
                        identities); the returned sum of squared errors within sum (2 |err| b + b^2) of float64, b = the
                        a-priori error bound of a float32 err (oracle/mf_step_oracle.py error_bound)
  A  lr = 0.01          rows of CLEAN ratings (no other rating of the launch names their user or their item) == the float64
     reg = 0.02         step within T_CLEAN; rows no rating touches (and every bias without use_bias) bit-identical
  B  lr = LR_B[case]    EVERY touched row: |got - start - jacobi sum| <= C[case] x path+ + floor (Euclidean over the row),
     reg = 0.02         floor = touches x ulp(max |row|) / 2 x sqrt(k)

The path of launch B.  path+ = sum over the row's ratings of lr (max(|err_t|, E) |other row| + reg |own row|), E = the rms
error of the case's ratings.  The floor E is needed: a rating whose error happens to vanish contributes no path of its own,
yet its delta still moves with the drift of its partner row — with the unfloored path |sequential - jacobi| / path reached
0.97 (k = 16) and 7.5 (k = 64) on user rows of the 300-item epoch at lr = 2^-12, against 0.22 and 0.18 with the floor.

Split rows (csrc/mf.hip mf_build_split: the hot rows of a step handle, form 3, and of >= 2^20 ratings) train through
copies that a hash of the rating's position names.  Their reference is the "align" merge of the per-copy Jacobi sums, their
path the sum of the copies' paths.  Under the block rotation the copies are merged after each of 8 phases and which phase a
hot rating runs in is the host's deal, so that one case (blocks_split_k64) EXEMPTS the split items' item rows and biases,
named, and checks every other row.

T_CLEAN.  Rule: 4 x the largest |float32 step - float64 step| over the clean rows of all cases, rounded up to one
significant digit.
C[case].  Rule: 4 x the largest |sequential - jacobi| / path+ over all touched rows and three orders of application (the
stored order and two seeded permutations), float64, rounded up to one significant digit; split rows: measured on the merged
row.  It is the share of a row's path by which ANY order of exact updates may differ from the Jacobi sum.
LR_B[case].  Rule: the largest power of two <= 2^-12 for which that C is <= 0.05.
tests/test_mf_step_cpu.py asserts the rules and prints every figure.
"""
import functools

import numpy as np

from cornac_amd import synth
from oracle import mf_step_oracle as step

MI355X_CUS = 256
LR_A, REG, MU = 0.01, 0.02, 3.0
TABLES = step.TABLES

# ---- measured (tests/test_mf_step_cpu.py prints the CPU figures, tests/test_mf_step_gpu.py the MI355X ones) ------------
# float32 step vs float64 step over the clean rows of all cases: 1.18e-7 (slice_k3, whose rows reach 2: ulp / 2 = 1.2e-7;
#   3e-8 .. 1.1e-7 elsewhere)  ->  T_CLEAN = 5e-7.  49 % of a 2 054-rating slice is clean (53 % of the last one), 66 of the 937
#   ratings of step_short_k64, 320 of the flat epoch, none of the other step cases and of the 2^20-rating epochs: there launch A
#   checks the untouched rows alone and launch B carries the case.
# |sequential - jacobi| / path+, three orders, largest over the rows at 2^-12 (it is proportional to lr): 0.003 .. 0.011 on
#   the slices (U and Bu; V and Bi a third of that); 7 500-rating step slices 0.012 .. 0.027; 300-item epoch U 0.22 (k = 16),
#   V 0.004, Bi 0.07; flat epoch 0.011 .. 0.018; the 300 000-rating epoch 0.4 .. 0.6 and the 2^20-rating epoch 0.16 .. 0.19 — the
#   row that sets it is the heaviest user's (hundreds of ratings: its own drift reaches every one of its deltas)  ->  LR_B
#   from 2^-12 down to 2^-18, and C below.
# Single-update visibility at those constants (share of the judged rows with path+ / touches > 2 x tolerance): slices and
#   flat epochs U 0.99 .. 1.0, V 0.92 .. 1.0; 7 500-rating step slices U 0.99 .. 1.0, V 0.2 .. 0.56; whole epochs over the
#   log-normal(1) users U 0.44 .. 0.76 (300-item epochs 0.63 .. 0.76, 300 000 ratings 0.46 .. 0.55, 2^20 ratings 0.44 .. 0.51) and
#   V 0 .. 0.84: a third and more of those users have over 1 / (2 C) ratings, and a smaller step sinks one update under the
#   floor — these launches show wrong factors and lost shares of a row's updates, the slices show single updates.
# MI355X, launch Z: all tables bit-identical; sum of squared errors off by 9e-7 .. 2e-3, 1e-4 .. 1e-5 of its bound.
# MI355X, launch A, largest |got - float64 step| over clean rows: U 9.8e-8, V 1.18e-7 (slice_k3), Bu 6.3e-8, Bi 6.4e-8 — the
#   float32 step's own error, a quarter of T_CLEAN.
# MI355X, launch B, largest error / tolerance over judged rows: U 0.26 (blocks_split_k64; 0.12 .. 0.24 elsewhere), V 0.11
#   (blocks_k64; 0.004 .. 0.07 on the fused kernel), Bu 0.26 (owned_split_k64), Bi 0.23 (blocks_k128; 0.02 .. 0.11 on the fused
#   kernel) — the device is one more order of application, a quarter of C like the three measured ones.  The owned
#   kernel's grid there: 6 144 / 7 168 / 6 144 / 8 192 waves at k = 64 / 100 / 192 / 200, the ownership tables equal to their
#   restatement at each; 28 081 batches of 4 (k = 64), 11 955 and 10 431 of 2 name one exclusive user twice.
T_CLEAN = 5e-7
LR_B = {
    "slice_k3": 2.0 ** -12, "slice_k7": 2.0 ** -12, "slice_k16": 2.0 ** -12, "slice_k20": 2.0 ** -12,
    "slice_k50": 2.0 ** -12, "slice_k100": 2.0 ** -12, "slice_k192": 2.0 ** -12, "slice_k200": 2.0 ** -12,
    "slice_generic_k300": 2.0 ** -12, "slice_nobias_k100": 2.0 ** -12, "slice_last_k64": 2.0 ** -12,
    "step_slice_k16": 2.0 ** -14, "step_slice_k64": 2.0 ** -14, "step_slice_generic_k300": 2.0 ** -13,
    "step_epoch_k16": 2.0 ** -17, "step_epoch_k64": 2.0 ** -17, "step_epoch_generic_k300": 2.0 ** -15,
    "owned_k64": 2.0 ** -13, "owned_k100": 2.0 ** -12, "owned_k192": 2.0 ** -12, "owned_k200": 2.0 ** -13,
    "owned_split_k64": 2.0 ** -16, "blocks_k64": 2.0 ** -18, "blocks_k128": 2.0 ** -18, "blocks_k192": 2.0 ** -18,
    "blocks_k200": 2.0 ** -18, "blocks_split_k64": 2.0 ** -16,
 "step_short_k64": 2.0 ** -12,
}
C = {
    "slice_k3": 0.05, "slice_k7": 0.04, "slice_k16": 0.03, "slice_k20": 0.03, "slice_k50": 0.03, "slice_k100": 0.03,
    "slice_k192": 0.03, "slice_k200": 0.03, "slice_generic_k300": 0.03, "slice_nobias_k100": 0.02,
    "slice_last_k64": 0.05, "step_slice_k16": 0.03, "step_slice_k64": 0.04, "step_slice_generic_k300": 0.05,
    "step_epoch_k16": 0.04, "step_epoch_k64": 0.03, "step_epoch_generic_k300": 0.05, "owned_k64": 0.03,
    "owned_k100": 0.05, "owned_k192": 0.05, "owned_k200": 0.04, "owned_split_k64": 0.04, "blocks_k64": 0.04,
    "blocks_k128": 0.03, "blocks_k192": 0.04, "blocks_k200": 0.04, "blocks_split_k64": 0.05,
 "step_short_k64": 0.02,
}

DATA = {  # name: (n_users, n_items, nnz, zipf, user_sigma)
    "mid": (20_000, 30_720, 300_000, 0.8, 1.0),
    "few_items": (6_000, 300, 60_000, 0.8, 1.0),
    "flat": (200_000, 100_000, 524_288, 0.3, 0.5),
    "big": (60_000, 30_720, 1 << 20, 0.8, 1.0),
}


def _slice(k, **kw):
    return dict(dict(data="mid", k=k, form=0, part=73, n_parts=146, clean_share=True), **kw)


def _step(k, whole, **kw):
    return dict(dict(data="few_items", k=k, form=3, part=0 if whole else 4, n_parts=1 if whole else 8), **kw)


# One case per kernel instantiation the dispatchers return (csrc/mf.hip pick_mf_kernel, pick_blocks_kernel).
SPECS = {
    # fused, unowned, a middle slice of ~2 055 ratings: every (G, R) of the row-wise kernel and the generic kernel
    "slice_k3": _slice(3), "slice_k7": _slice(7), "slice_k16": _slice(16), "slice_k20": _slice(20), "slice_k50": _slice(50),
    "slice_k100": _slice(100), "slice_k192": _slice(192), "slice_k200": _slice(200), "slice_generic_k300": _slice(300),
    "slice_nobias_k100": _slice(100, use_bias=False),
    # the last part of the epoch: 2 055 = 32 x 64 + 7 ratings, a partial final tile
    "slice_last_k64": _slice(64, part=145),
    # split rows through the step form (form 3): 3 of 300 items train through 6 copies; a slice and the whole epoch
    "step_slice_k16": _step(16, False), "step_slice_k64": _step(64, False), "step_slice_generic_k300": _step(300, False),
    "step_epoch_k16": _step(16, True), "step_epoch_k64": _step(64, True), "step_epoch_generic_k300": _step(300, True),
    # ... and a SHORT slice (937 ratings, ~17 on each copy): the copies' deltas are still nearly orthogonal, so the align merge
    # is the plain sum there and a merge by the MEAN shows (over a long launch the copies' deltas agree, align approaches
    # the mean, and only the plain sum shows)
    "step_short_k64": _step(64, False, part=32, n_parts=64),
    # fused, OWNED (the whole epoch, k > 32, nnz >= CUs x 8 x 4 x 64): exclusive users take plain stores, the deltas of a batch's
    # ratings of one user summed first; R = 1..4
    "owned_k64": dict(data="flat", k=64, owned=True), "owned_k100": dict(data="flat", k=100, owned=True),
    "owned_k192": dict(data="flat", k=192, owned=True), "owned_k200": dict(data="flat", k=200, owned=True),
    # ... with split rows (>= 2^20 ratings: an item holding > 0.1 % of them)
    "owned_split_k64": dict(data="big", k=64, owned=True),
    # block rotation (form 2), the whole epoch: item bins in LDS and hot items under atomics
    "blocks_k64": dict(data="mid", k=64, form=2), "blocks_k128": dict(data="mid", k=128, form=2),
    "blocks_k192": dict(data="mid", k=192, form=2), "blocks_k200": dict(data="mid", k=200, form=2),
    # ... with split rows, merged after each of the 8 phases: the split items' rows are exempt (module docstring)
    "blocks_split_k64": dict(data="big", k=64, form=2, exempt_split=True),
}
NAMES = list(SPECS)
OWNED_UNR = {64: 4, 100: 2, 192: 2, 200: 1}  # pick_mf_kernel: ratings a wave of the owned kernel has in flight together
# the owned kernel's persistent grid on an MI355X (256 CUs x the instantiation's workgroups per CU x 4 waves); the device
# test takes the count from debug_ownership() and restates the tables for whatever grid the device runs
OWNED_WAVES = {64: 6144, 100: 7168, 192: 6144, 200: 8192}


@functools.lru_cache(maxsize=2)
def _data(name):
    """(rid, cid, val): synth.zipf_interactions in a seeded random order — a slice of the stored order is a random sample,
    not one user's run — with ratings 1..5"""
    nu, ni, nnz, zipf, sigma = DATA[name]
    users, items = synth.zipf_interactions(nu, ni, nnz, zipf, 11, sigma)
    rs = np.random.RandomState(12)
    perm = rs.permutation(nnz)
    return users[perm].astype(np.int64), items[perm].astype(np.int64), rs.randint(1, 6, nnz).astype(np.float32)


def _tables(name, nu, ni, k):
    """normal tables whose predictions have unit spread whatever k (mu + bu + bi + u.v: variance k s^4 + 2 s_b^2 = 1 with
    s_b = 0.5): float32 values, so exactly representable on the device"""
    rs = np.random.RandomState(sum(map(ord, name)) + 1000 * k)
    s = (0.5 / k) ** 0.25
    return (rs.normal(0, s, (nu, k)).astype(np.float32), rs.normal(0, s, (ni, k)).astype(np.float32),
            rs.normal(0, 0.5, nu).astype(np.float32), rs.normal(0, 0.5, ni).astype(np.float32))


def blocks_hot(cid, n_items):
    """csrc/mf.hip mf_build_blocks: the items that stay in global memory under atomics (more than a tenth of a bin's share
    of the ratings); the others are dealt to the 256 LDS bins"""
    return np.bincount(cid, minlength=n_items) * 10 * 256 > len(cid)


class Case:
    """the inputs of one case and, computed once and never modified, its ratings and float64 references"""

    def __init__(self, name, lr_b=None, cus=MI355X_CUS, blocks_per_cu=8):
        sp = dict(dict(use_bias=True, form=0, part=0, n_parts=1, clean_share=False, owned=False, exempt_split=False), **SPECS[name])
        self.name, self.spec = name, sp
        for key, v in sp.items():
            setattr(self, key, v)
        self.nu, self.ni, self.nnz = DATA[self.data][:3]
        self.rid, self.cid, self.val = _data(self.data)
        self.tables = _tables(name, self.nu, self.ni, self.k)
        self.lr_b = LR_B[name] if lr_b is None else lr_b
        # what the handle will decide: the split (csrc/mf.hip mf_build_split) and the renamed item ids
        self.inflight = step.step_inflight(self.ni, self.k, cus, blocks_per_cu) if self.form == 3 else None
        self.per_copy = step.split_per_copy(self.nnz, self.inflight[1] if self.inflight else None)
        self.split = step.split_plan(self.cid, self.ni, self.per_copy)
        self.n_virtual = int(self.split[1][-1])
        self.cid_ext = step.split_id(np.arange(self.nnz), self.cid, *self.split, self.ni)
        self.s0, self.s1 = self.nnz * self.part // self.n_parts, self.nnz * (self.part + 1) // self.n_parts
        s = slice(self.s0, self.s1)
        self.rat = (self.rid[s], self.cid_ext[s], self.val[s])  # the launch's ratings, item ids naming copies
        self.items = self.cid[s]
        # launch B: the Jacobi sum of every row (split rows: the align merge of their copies'); launch A: the float64 step of
        # the clean ratings alone; launch Z: the float64 errors (they do not depend on lr)
        ext = step.extend(self.tables, self.split)
        self.jac = step.fold(step.jacobi(self.rat, ext, self.lr_b, REG, MU, self.use_bias), self.split, self.ni)
        for tab in TABLES:
            for a in self.jac[tab].values():
                a.setflags(write=False)
        self.err, self.sse, self.E = self.jac["err"], self.jac["sse"], self.jac["E"]
        self.touches = {tab: self.jac[tab]["touches"] for tab in TABLES}  # (biases off: theirs are all 0)
        u, it = self.rat[0], self.items
        self.clean = (self.touches["U"][u] == 1) & (self.touches["V"][it] == 1)
        cu, ci = u[self.clean], it[self.clean]
        self.clean_rat = (cu, ci, self.rat[2][self.clean])
        _, dU, dV, dBu, dBi = step.deltas(self.clean_rat, self.tables, LR_A, REG, MU, self.use_bias)
        self.clean_rows = {"U": cu, "V": ci, "Bu": cu, "Bi": ci}
        self.clean_want = {tab: start[self.clean_rows[tab]].astype(np.float64) + d
                           for tab, start, d in zip(TABLES, self.tables, (dU, dV, dBu, dBi))}
        b = step.error_bound(self.rat, ext, MU)
        self.sse_bound = float(np.sum(2 * np.abs(self.err) * b + b * b))
        # rows launch B does not judge: the split items' item rows and biases under the block rotation
        self.exempt = {tab: np.zeros(len(t), bool) for tab, t in zip(TABLES, self.tables)}
        if self.exempt_split:
            self.exempt["V"][self.split[0]] = self.exempt["Bi"][self.split[0]] = True

    def ratings_of(self, table, row):
        return np.flatnonzero((self.rat[0] if table in ("U", "Bu") else self.items) == row)

    def describe(self, table, row):
        ids = self.ratings_of(table, row)
        return "%s: table %s row %d%s, %d touches, ratings %s" % (
            self.name, table, row, " (split)" if table in ("V", "Bi") and row in self.split[0] else "", len(ids),
            ", ".join("#%d (u %d, i %d -> %d, r %g)" % (self.s0 + t, self.rat[0][t], self.items[t], self.rat[1][t], self.rat[2][t])
                      for t in ids[:8]) + (" ..." if len(ids) > 8 else ""))


@functools.lru_cache(maxsize=2)
def case(name, lr_b=None, cus=MI355X_CUS, blocks_per_cu=8):
    return Case(name, lr_b, cus, blocks_per_cu)


# ---- the checks: `got` = (U, V, Bu, Bi) as the device (or a deliberately wrong reference) returns them -------------------
def _untouched_identical(c, launch, got):
    for tab, start, g in zip(TABLES, c.tables, got):
        same = (g == start).reshape(len(start), -1).all(axis=1) | (c.touches[tab] > 0)  # (biases off: no touches)
        assert same.all(), "launch %s changed a row no rating touches: %s" % (launch, c.describe(tab, int(np.flatnonzero(~same)[0])))


def check_z(c, got, sse):
    for tab, start, g in zip(TABLES, c.tables, got):
        assert np.array_equal(start, g), "%s: lr = 0 changed table %s" % (c.name, tab)
    assert abs(sse - c.sse) <= c.sse_bound, "%s: sum of squared errors %.17g, float64 %.17g, bound %.3g" % (c.name, sse, c.sse, c.sse_bound)
    return dict(sse_err=abs(sse - c.sse), sse_bound=c.sse_bound)


def check_a(c, got):
    """launch A: clean rows against the float64 step at T_CLEAN, untouched rows bit-identical.  Returns the largest
    clean-row error per table."""
    _untouched_identical(c, "A", got)
    worst = {}
    for tab, g in zip(TABLES, got):
        rows, want = c.clean_rows[tab], c.clean_want[tab]
        err = np.abs(g[rows].astype(np.float64) - want).reshape(len(rows), -1).max(axis=1) if len(rows) else np.zeros(0)
        worst[tab] = float(err.max()) if len(err) else 0.0
        bad = np.flatnonzero(err > T_CLEAN)
        assert len(bad) == 0, "launch A, clean row off by %.3g > T_CLEAN = %.3g (%d such rows): %s" % (
            err[bad[0]], T_CLEAN, len(bad), c.describe(tab, int(rows[bad[0]])))
    return worst


def tolerance_b(c, tab, coeff=None):
    """per-row tolerance of launch B for one table: C x path+ + touches x ulp(max |row|) / 2 x sqrt(k)"""
    coeff = C[c.name] if coeff is None else coeff
    j = c.jac[tab]
    start = c.tables[TABLES.index(tab)].astype(np.float64).reshape(len(j["touches"]), -1)
    top = np.maximum(np.abs(start), np.abs(start + j["sum"].reshape(start.shape))).max(axis=1)
    half_ulp = np.spacing(top.astype(np.float32)).astype(np.float64) / 2
    return coeff * j["path"] + j["touches"] * half_ulp * np.sqrt(start.shape[1])


def judged_rows(c, tab):
    return np.flatnonzero((c.jac[tab]["touches"] > 0) & ~c.exempt[tab])


def deviation_b(c, tab, got_tab):
    """(rows, |got - start - jacobi sum| per judged row) of one table"""
    rows = judged_rows(c, tab)
    if len(rows) == 0:
        return rows, np.zeros(0)
    start = c.tables[TABLES.index(tab)]
    moved = got_tab[rows].astype(np.float64) - start[rows].astype(np.float64)
    return rows, np.linalg.norm((moved - c.jac[tab]["sum"][rows]).reshape(len(rows), -1), axis=1)


def check_b(c, got, coeff=None):
    """launch B: every touched row against the Jacobi sum.  Returns the largest error / tolerance per table."""
    _untouched_identical(c, "B", got)
    worst = {}
    for tab, g in zip(TABLES, got):
        rows, err = deviation_b(c, tab, g)
        if len(rows) == 0:
            worst[tab] = 0.0
            continue
        tol = tolerance_b(c, tab, coeff)[rows]
        worst[tab] = float((err / tol).max())
        bad = np.flatnonzero(err > tol)
        assert len(bad) == 0, "launch B, |got - start - jacobi| = %.3g > %.3g (path %.3g; %d such rows): %s" % (
            err[bad[0]], tol[bad[0]], c.jac[tab]["path"][rows[bad[0]]], len(bad), c.describe(tab, int(rows[bad[0]])))
    return worst


def visibility(c, tab, coeff=None):
    """share of the judged rows of a table on which ONE lost or doubled update shows: path+ / touches > 2 x tolerance"""
    j = c.jac[tab]
    rows = judged_rows(c, tab)
    if len(rows) == 0:
        return 1.0
    return float((j["path"][rows] / j["touches"][rows] > 2 * tolerance_b(c, tab, coeff)[rows]).mean())


def round_up_1sig(v):
    e = np.floor(np.log10(v))
    return float(np.ceil(v / 10 ** e - 1e-9) * 10 ** e)
