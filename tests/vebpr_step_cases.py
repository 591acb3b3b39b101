"""Inputs, references and checks of the hogwild VEBPR step tests, in ONE place: tests/test_vebpr_step_gpu.py runs the cases
on the device, tests/test_vebpr_step_cpu.py proves — from the restatement of the sampler and the float64 step alone — that
every case is a fair test, that the tolerances below follow their rules, and that the checks reject ten deliberately wrong
updates.  The VEBPR counterpart of tests/bpr_step_cases.py: same launches, same rules, four rows per sample.

A case = a purchase matrix and a view matrix + normal tables with real scores + ONE epoch of vebpr_hogwild_kernel
(cornac_hip_vebpr_fit_epochs(1, ...) is always a whole epoch, and seed_hogwild makes it epoch 0), whose non-skipped
quadruples (u, i, v, j) oracle.hogwild_quadruples names before anything runs.  The epoch is made three times from the same
start tables, alpha = 0.3 (so that a swap with 1 - alpha = 0.7 shows):

  Z  lr = 0             tables bit-identical; skip counter == the restatement's; `correct` == #(every applicable score > 0)
                        in float64, give or take the quadruples with a score below the float32 score's a-priori error bound
  A  lr = 0.05          rows of CLEAN quadruples (none of its rows touched by another quadruple of the epoch; v != i) == the
     reg = 0.01         float64 step within T_CLEAN; rows no quadruple touches (those beyond n_items among them) bit-identical
  B  lr = 2^-12         EVERY touched row: |got - start - jacobi sum| <= C[case] x path + floor (Euclidean over the row),
     reg = 0.01         path = sum over the deltas landing on the row of |delta|, floor = touches x ulp(max |row|) / 2 x sqrt(k)

v == i: the kernel adds dVi and dVv onto the one row, and so does the float64 step (oracle/vebpr_step_oracle.py); such a
row counts two touches.

T_CLEAN.  Rule: 4 x the largest |float32 step - float64 step| over the clean rows of all cases with a launch A (the device
sums the dot products in butterfly order and uses __expf and __frcp_rn), rounded up to one significant digit.

C[case].  Rule: 4 x the largest |sequential - jacobi| / path over all touched rows and three orders of application (the
restatement's and two seeded permutations), float64, rounded up to one significant digit.  It is the share of a row's
path by which ANY order of exact updates may differ from the Jacobi sum, so it bounds a correct kernel whatever its
scheduling; a lost or doubled update moves a row by path / touches, visible where that exceeds 2 x the tolerance.
tests/test_vebpr_step_cpu.py asserts both rules and prints every figure.
"""
import functools

import numpy as np

import bpr_step_cases as bc
from cornac_amd import synth
from oracle import oracle as orc
from oracle import vebpr_step_oracle as step

MI355X_CUS = 256
LR_A, LR_B, REG, ALPHA = 0.05, 2.0 ** -12, 0.01, 0.3
PAD_ROWS = 37  # item rows beyond n_items: no launch may touch them
LARGE_NNZ = 524_288  # the owned cases' interactions: the ownership threshold of 256 CUs x 8 x 4 waves x 64 (debug_ownership)

# ---- measured (tests/test_vebpr_step_cpu.py prints the CPU figures, tests/test_vebpr_step_gpu.py the MI355X ones) ---------
# float32 step vs float64 step over the clean rows of all cases: 1.18e-7 (unowned_k3, whose rows reach 2.1: ulp / 2 = 1.2e-7;
#   3.6e-8 .. 9e-8 elsewhere)  ->  T_CLEAN = 5e-7.
# |sequential - jacobi| / path, three orders: 0.029 .. 0.055 for the small cases, 0.020 / 0.014 / 0.026 owned (k = 64 / 100 /
#   136), 0.014 for the stride case  ->  C below.  What sets it is a view row whose alpha d_iv u and (1 - alpha) d_vj u
#   cancel: its delta is then all reg, a path 25 times shorter than its neighbours', and the two to four other updates of
#   its user in the epoch move d_iv and d_vj by a few per cent of THAT.  One view row in a thousand does; hence few
#   purchases per view-dense user and few view users in the large data (see _small_data, _large_data).
# Single-update visibility at these C: U 0.85 .. 0.87, V 0.91 .. 0.92 for the small cases (0.57 / 0.75 at k = 20, C = 0.3),
#   owned U 0.89 / 0.94 / 0.52, V 0.98 / 0.99 / 0.65, stride 0.77 / 0.91.
# MI355X, launch Z: skip counter equal to the restatement's in every case; `correct` inside the float64 interval (one number
#   in 7 of the 8 small cases, 8 .. 31 wide in the large ones).
# MI355X, launch A, largest |got - float64 step| over clean rows: U 1.01e-7, V 1.18e-7 (unowned_k3), 3.1e-8 .. 9.0e-8 elsewhere
#   — the float32 step's own error, a quarter of T_CLEAN.
# MI355X, launch B, largest error / tolerance over touched rows: small cases U 0.008 .. 0.089, V 0.087 .. 0.217; owned U 0.062 /
#   0.067 / 0.028, V 0.146 / 0.225 / 0.108 (k = 64 / 100 / 136; 6 144 waves, ownership tables equal to their restatement);
#   stride U 0.076, V 0.142 — the device is one more order of application, a quarter of C like the three measured ones.
T_CLEAN = 5e-7
C = {
    "unowned_k3": 0.2, "unowned_k7": 0.2, "unowned_k12": 0.2, "unowned_k20": 0.3,
    "unowned_k50": 0.2, "unowned_k100": 0.2, "unowned_k200": 0.2, "unowned_k256": 0.2,
    "owned_k64": 0.08, "owned_k100": 0.06, "owned_k136": 0.2,
    "unowned_stride_k64": 0.06,
}


def _small(k, **kw):
    return dict(form="unowned", data="small", k=k, ownership=True, **kw)  # (the dispatcher itself picks the unowned kernels here)


def _owned(k):
    return dict(form="owned", data="large", k=k, ownership=True)


# One case per instantiation of vebpr_hogwild_kernel that vebpr_epoch_hogwild (csrc/vebpr.inc) launches.
SPECS = {
    # unowned, G = 4, 8, 16, 32 with lanes beyond k, then G = 64 at R = 1, 2, 4 with out-of-range lanes in the last pass and
    # the full width k = 256: purpose-built data (_small_data), far below the ownership threshold
    "unowned_k3": _small(3), "unowned_k7": _small(7), "unowned_k12": _small(12), "unowned_k20": _small(20),
    "unowned_k50": _small(50), "unowned_k100": _small(100), "unowned_k200": _small(200, tables_seed=202), "unowned_k256": _small(256),
    # (k = 200: a score is within its float32 bound of 0 once in 10 000 at this width, about two of the 12 000 scores of such
    # an epoch, and the fairness condition allows two ambiguous quadruples: the default tables give five, these none)
    # OWNED, R = 1, 2, 4 (k = 136: 8 live lanes in the third pass, none in the fourth): the flat problem of the owned BPR
    # cases over 300 000 x 600 000 plus a few Zipf views (_large_data).  The grid is 6 workgroups per CU whatever k (6 144
    # waves on an MI355X), so a slice is about 85 samples and every wave's second tile is partial.  No share of such an
    # epoch is asked to be clean (the 2 400 clean quadruples that exist are checked all the same); launch B carries the form.
    # The device test takes the wave count from debug_ownership() and rebuilds the case if it differs.
    "owned_k64": _owned(64), "owned_k100": _owned(100), "owned_k136": _owned(136),
    # the unowned kernel's tile stride: the same data with ownership switched off, 8 192 tiles over at most 6 144 waves, so
    # some waves loop twice.  Launches Z and B only.
    "unowned_stride_k64": dict(form="unowned", data="large", k=64, ownership=False, no_a=True),
}
NAMES = list(SPECS)


def vebpr_grid_waves(cus):
    """the owned form's grid (csrc/vebpr.inc vebpr_epoch_hogwild): 6 workgroups of 4 waves per CU"""
    return cus * 6 * 4


def ownership_applies(nnz, cus):
    """csrc/vebpr.inc vebpr_uses_ownership for 32 < k <= 256: at least one 64-sample tile per wave and epoch"""
    return nnz >= vebpr_grid_waves(cus) * 64


@functools.lru_cache(maxsize=1)
def _small_data():
    """Purpose-built purchase and view matrices over 65 536 items (seeded numpy: Zipf interactions of this size give about
    one skip and no v == i at all):
      5 000 sparse users with ONE purchase each: of every eight, two have two views with the purchase among them (v == i
            half of the time), three have two other views, three have none — the clean quadruples of both kinds;
      1     user who purchased all items but 256: 65 280 samples of the epoch, all but about 255 of them skipped by the
            purchase row (a deep binary search each).  Two users with 2 048 purchases each give the skips as well, but
            their rows then take 2 000 updates of one launch: the drift of such a row between the first and the last
            (8 % at k = 3) times the score tail put C at 0.4 .. 2, where a single update shows on no row at all;
      64    view-dense users with 8 purchases and 16 000 views: skips by the view row alone.  (Few purchases each: where
            alpha d_iv and (1 - alpha) d_vj cancel, a view row's delta is all reg and a few updates of its user move it
            by a large share of that.)
      100   users without purchases."""
    ni = 65_536
    rs = np.random.RandomState(20)
    purchases, views = [], []
    own = rs.choice(ni, 5000, replace=False)
    for usr in range(5000):
        purchases.append([own[usr]])
        if usr % 8 >= 5:
            views.append([])
            continue
        other = rs.choice(ni, 3, replace=False)
        other = other[other != own[usr]]
        views.append(sorted([own[usr], other[0]] if usr % 8 < 2 else other[:2]))
    purchases.append(np.sort(rs.choice(ni, ni - 256, replace=False)))
    views.append([])
    for _ in range(64):
        purchases.append(np.sort(rs.choice(ni, 8, replace=False)))
        views.append(np.sort(rs.choice(ni, 16_000, replace=False)))
    for _ in range(100):
        purchases.append([])
        views.append([])

    def csr(rows):
        indptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
        return indptr, np.concatenate([np.asarray(r, np.int32) for r in rows]).astype(np.int32)

    return len(purchases), ni, csr(purchases), csr(views)


@functools.lru_cache(maxsize=1)
def _large_data():
    """The flat problem of the owned BPR cases (Zipf 0.3 items, log-normal user activity, 524 288 interactions) over 300 000
    users and 600 000 items, plus 6 000 Zipf views among the first 225 000 users.  A whole epoch over the BPR cases' own
    200 000 x 400 000 touches a user row 4.2 times on average, and fewer than half of the touched rows at most twice; and
    with views for most users one view row in a thousand has alpha d_iv u and (1 - alpha) d_vj u cancel down to its reg
    term, where two or three other updates of its user move the delta by 6 % of that path: C = 0.3, at which a single
    update shows on a quarter of the rows.  About 10 000 quadruples with a view remain."""
    nu, ni = 300_000, 600_000
    vu, vi = synth.zipf_interactions(nu * 3 // 4, ni, 6_000, 0.5, 12)
    return nu, ni, bc._data(nu, ni, LARGE_NNZ, 0.3), synth.csr_from_sorted(vu, vi, nu)


def _tables(name, nu, total_items, k, seed=None):
    """normal tables whose scores have unit spread whatever k (x = u.(a - b): variance 2 k s^4 = 1): float32 values, so
    exactly representable on the device"""
    rs = np.random.RandomState(sum(map(ord, name)) + 1000 * k if seed is None else seed)
    s = (0.5 / k) ** 0.25
    return rs.normal(0, s, (nu, k)).astype(np.float32), rs.normal(0, s, (total_items, k)).astype(np.float32)


class Case:
    """the inputs of one case and, computed once and never modified, its quadruples and float64 references"""

    def __init__(self, name, cus=MI355X_CUS, waves=None):
        sp = dict(dict(no_a=False), **SPECS[name])
        self.name, self.spec = name, sp
        for key, v in sp.items():
            setattr(self, key, v)
        self.seed = 0x5EED0000 + self.k
        self.nu, self.ni, (self.indptr, self.indices), (self.v_indptr, self.v_indices) = (
            _small_data() if self.data == "small" else _large_data())
        self.nnz = len(self.indices)
        self.total_items = self.ni + PAD_ROWS
        self.tables = _tables(name, self.nu, self.total_items, self.k, sp.get("tables_seed"))
        self.owned_on_device = self.form == "owned"
        self.own_tables = None
        if self.form == "owned":
            self.own_tables = orc.hogwild_ownership(self.indptr, self.indices, waves or vebpr_grid_waves(cus))
        q = orc.hogwild_quadruples(self.form, self.seed, 0, self.indptr, self.indices, self.v_indptr, self.v_indices, self.ni,
                                   ownership=self.own_tables)
        self.quad = (q["u"], q["i"], q["v"], q["j"])
        self.draws, self.skipped = q["draws"], q["skipped"]
        self.skipped_purchase, self.skipped_view_only, self.shared = q["skipped_purchase"], q["skipped_view_only"], q.get("shared")
        u, i, v, j = self.quad
        self.has_v = v >= 0
        # launch B: the Jacobi sum of every row; launch A: the float64 step of the clean quadruples alone (their rows have
        # no other delta, so no sum is needed); launch Z: the float64 scores (they do not depend on lr)
        self.jac = step.jacobi(self.quad, self.tables, LR_B, REG, ALPHA)
        for tab in "UV":
            for a in self.jac[tab].values():
                a.setflags(write=False)
        self.touches = {tab: self.jac[tab]["touches"] for tab in "UV"}
        tu, tv = self.touches["U"], self.touches["V"]
        # (a quadruple with v == i touches that row twice, so it is never clean)
        self.clean = (tu[u] == 1) & (tv[i] == 1) & (tv[j] == 1) & (~self.has_v | (tv[np.where(self.has_v, v, i)] == 1))
        cq = tuple(a[self.clean] for a in self.quad)
        cu, ci, cv, cj = cq
        cview = cv >= 0
        _, dU, dVi, dVv, dVj = step.deltas(cq, *self.tables, LR_A, REG, ALPHA)
        rows_v = np.concatenate([ci, cj, cv[cview]])
        self.clean_rows = {"U": cu, "V": rows_v}
        self.clean_want = {"U": self.tables[0][cu].astype(np.float64) + dU,
                           "V": self.tables[1][rows_v].astype(np.float64) + np.concatenate([dVi, dVj, dVv[cview]])}
        # the scores that apply to a quadruple: x_ij always, x_iv and x_vj with a view
        self.x = self.jac["x"]
        self.applies = np.stack([np.ones(len(u), bool), self.has_v, self.has_v], axis=1)
        self.x_bound = step.score_error_bound(self.quad, self.tables)

    def quadruples_of(self, table, row):
        u, i, v, j = self.quad
        return np.flatnonzero(u == row if table == "U" else (i == row) | (v == row) | (j == row))

    def describe(self, table, row):
        ids = self.quadruples_of(table, row)
        u, i, v, j = self.quad
        return "%s: table %s row %d, %d touches, quadruples %s" % (
            self.name, table, row, int(self.touches[table][row]),
            ", ".join("#%d (u %d, i %d, v %d, j %d)" % (t, u[t], i[t], v[t], j[t]) for t in ids[:8]) + (" ..." if len(ids) > 8 else ""))


@functools.lru_cache(maxsize=2)
def case(name, cus=MI355X_CUS, waves=None):
    return Case(name, cus, waves)


# ---- the checks: `got` = (U, V) as the device (or a deliberately wrong reference) returns them ----------------------------
def _untouched_identical(c, launch, got):
    for tab, start, g in zip("UV", c.tables, got):
        same = (g == start).all(axis=1) | (c.touches[tab] > 0)
        assert same.all(), "launch %s changed a row no quadruple touches: %s" % (launch, c.describe(tab, int(np.flatnonzero(~same)[0])))


def correct_interval(c):
    """`correct` counts the quadruples whose applicable scores are ALL > 0: in float64, with every score within its float32
    error bound of 0 taken either way (x_iv of a quadruple with v == i is exactly 0 on the device too and its bound is 0: such
    a quadruple is never `correct`)"""
    surely = ((c.x > c.x_bound) | ~c.applies).all(axis=1)
    maybe = ((c.x > -c.x_bound) | ~c.applies).all(axis=1)
    return int(surely.sum()), int(maybe.sum())


def check_z(c, got, correct, skipped):
    for tab, start, g in zip("UV", c.tables, got):
        assert np.array_equal(start, g), "%s: lr = 0 changed table %s" % (c.name, tab)
    assert skipped == c.skipped, "%s: skip counter %d, restatement %d" % (c.name, skipped, c.skipped)
    lo, hi = correct_interval(c)
    assert lo <= correct <= hi, "%s: `correct` = %d, float64 scores give %d..%d" % (c.name, correct, lo, hi)
    return dict(correct=correct, lo=lo, hi=hi)


def check_a(c, got):
    """launch A: clean rows against the float64 step at T_CLEAN, untouched rows bit-identical.  Returns the largest
    clean-row error per table."""
    _untouched_identical(c, "A", got)
    worst = {}
    for tab, g in zip("UV", got):
        rows, want = c.clean_rows[tab], c.clean_want[tab]
        err = np.abs(g[rows].astype(np.float64) - want).max(axis=1) if len(rows) else np.zeros(0)
        worst[tab] = float(err.max()) if len(err) else 0.0
        bad = np.flatnonzero(err > T_CLEAN)
        assert len(bad) == 0, "launch A, clean row off by %.3g > T_CLEAN = %.3g (%d such rows): %s" % (
            err[bad[0]], T_CLEAN, len(bad), c.describe(tab, int(rows[bad[0]])))
    return worst


def tolerance_b(c, tab, coeff=None):
    """per-row tolerance of launch B for one table: C x path + touches x ulp(max |row|) / 2 x sqrt(k)"""
    coeff = C[c.name] if coeff is None else coeff
    j = c.jac[tab]
    start = c.tables["UV".index(tab)].astype(np.float64)
    top = np.maximum(np.abs(start), np.abs(start + j["sum"])).max(axis=1)
    half_ulp = np.spacing(top.astype(np.float32)).astype(np.float64) / 2
    return coeff * j["path"] + j["touches"] * half_ulp * np.sqrt(start.shape[1])


def check_b(c, got, coeff=None):
    """launch B: every touched row against the Jacobi sum.  Returns the largest error / tolerance per table."""
    _untouched_identical(c, "B", got)
    worst = {}
    for tab, start, g in zip("UV", c.tables, got):
        j = c.jac[tab]
        rows = np.flatnonzero(j["touches"] > 0)
        moved = g[rows].astype(np.float64) - start[rows].astype(np.float64)
        err = np.linalg.norm(moved - j["sum"][rows], axis=1)
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
    return float((j["path"][rows] / j["touches"][rows] > 2 * tolerance_b(c, tab, coeff)[rows]).mean())


round_up_1sig = bc.round_up_1sig
