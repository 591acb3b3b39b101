"""The hogwild MF step cases (tests/mf_step_cases.py) are fair tests, their tolerances follow their rules, and their checks
are sharp — all from the CPU restatements of the handle's decisions and the float64 step, without a device."""
import numpy as np
import pytest

import mf_step_cases as mc
from oracle import mf_step_oracle as step

TABLES = mc.TABLES


def _as_device(tables64):
    """what a device holding float32 tables would return for these float64 results"""
    return tuple(np.asarray(t, np.float32) for t in tables64)


def c_measured(c):
    """largest |sequential - jacobi| / path+ over the judged rows of all tables, three orders of application (split rows: on
    the merged row)"""
    n = len(c.rat[0])
    rs = np.random.RandomState(len(c.name))
    worst = dict.fromkeys(TABLES, 0.0)
    for order in (np.arange(n), rs.permutation(n), rs.permutation(n)):
        seq, _ = step.launch(c.rat, c.tables, c.split, c.lr_b, mc.REG, mc.MU, c.use_bias, order)
        for tab, s in zip(TABLES, seq):
            rows, dev = mc.deviation_b(c, tab, s)
            if len(rows):
                worst[tab] = max(worst[tab], float((dev / c.jac[tab]["path"][rows]).max()))
    return worst


_T32 = {}  # per case, filled as the cases go by


def t32_measured(c):
    """largest |float32 step - float64 step| over the clean rows"""
    if c.name not in _T32:
        got = step.step_f32(c.clean_rat, c.tables, mc.LR_A, mc.REG, mc.MU, c.use_bias)[1:]
        errs = [np.abs(g - c.clean_want[tab]) for tab, g in zip(TABLES, got)]
        _T32[c.name] = max([float(e.max()) for e in errs if e.size] + [0.0])
    return _T32[c.name]


def test_restatements_of_the_split_and_the_throttle():
    """split_plan / split_id / step_inflight / align_merge: coverage, copies per item, the figures the cases rely on"""
    assert [step.step_inflight(300, k)[1] for k in (16, 64, 300)] == [1216, 1200, 1200]
    assert step.step_inflight(300, 300, cus=256, blocks_per_cu=1) == (256, 1024)  # (never more than the device holds)
    assert step.step_inflight(10, 3) == (2, 256) and step.step_inflight(30_720, 64)[0] == 2048
    assert step.split_per_copy(60_000, 1216) == 38 == step.split_per_copy(60_000, 1200)
    assert step.split_per_copy(1 << 20) == 1000 and step.split_per_copy((1 << 20) - 1) == 0
    for name, n_split, n_copies, most in (("step_epoch_k16", 3, 6, 2), ("owned_split_k64", 63, 212, 18), ("slice_k16", 0, 0, 0)):
        c = mc.case(name)
        items, ptr = c.split
        w = np.diff(ptr)
        cnt = np.bincount(c.cid, minlength=c.ni)
        print("\n%s: %d split items, %d copies (at most %d per item) holding %.1f %% of the ratings" % (
            name, len(items), ptr[-1], w.max() if len(w) else 0, 100.0 * cnt[items].sum() / c.nnz))
        assert (len(items), int(ptr[-1]), int(w.max()) if len(w) else 0) == (n_split, n_copies, most)
        assert (w >= 1).all() and (w <= 256).all()
        # every rating of a split item names one of ITS copies, every other rating its item; every copy is named
        ext = c.cid_ext
        is_split = np.isin(c.cid, items)
        assert np.array_equal(ext[~is_split], c.cid[~is_split]) and (ext[is_split] >= c.ni).all()
        if len(items):
            v = ext[is_split] - c.ni
            j = np.searchsorted(ptr, v, side="right") - 1
            assert np.array_equal(items[j], c.cid[is_split]) and len(np.unique(v)) == ptr[-1]
            share = np.bincount(v) / np.repeat(cnt[items], w)  # the hash deals a row's ratings evenly over its copies
            assert np.abs(share * np.repeat(w, w) - 1).max() < 0.25, share
    # the align merge: the plain sum for orthogonal deltas, the mean for W equal ones, never beyond the sum
    e = np.eye(4)
    assert np.allclose(step.align_merge(e[:3]), e[:3].sum(0)) and np.allclose(step.align_merge(np.tile(e[0] * 2, (5, 1))), e[0] * 2)
    assert np.allclose(step.align_merge(np.array([0.5, 0.5, 0.5])), 0.5) and step.align_merge(np.zeros((3, 4))).tolist() == [0] * 4
    assert np.allclose(step.align_merge(np.array([1.0, -3.0])), -2.0)


@pytest.mark.parametrize("name", mc.NAMES)
def test_case_is_a_fair_test_and_its_tolerances_follow_their_rules(oracle, name):
    c = mc.case(name)
    n = len(c.rat[0])
    assert n == c.s1 - c.s0 and all(t.dtype == np.float32 for t in c.tables) and c.tables[2].any() and c.tables[3].any()
    if c.n_parts > 1:
        assert n % 64 != 0, "a partial final tile"
    if c.name == "slice_last_k64":
        assert c.s1 == c.nnz
    # real errors on both sides of zero
    e05, e95 = np.quantile(c.err, [0.05, 0.95])
    assert e05 < -1 and e95 > 1 and 1.0 < c.E < 3.0, (e05, e95, c.E)
    n_clean = int(c.clean.sum())
    if c.clean_share:
        assert n_clean >= 300 and 3 * n_clean >= n, (n_clean, n)
    tu, tv = c.touches["U"], c.touches["V"]
    assert (tu == 0).any() and ((tv == 0).any() or c.ni == 300) and tv.max() >= 3, "untouched rows exist, and rows touched often"
    extra = ""
    if c.form == 3:
        assert len(c.split[0]) == 3 and c.n_virtual == 6 and c.inflight[1] in (1216, 1200) and c.per_copy == 38
        assert np.isin(c.items, c.split[0]).mean() > 0.08, "the launch trains the split rows"
        extra = ", in flight %d, a copy per %d, split rows hold %.0f %% of the launch" % (
            c.inflight[1], c.per_copy, 100 * np.isin(c.items, c.split[0]).mean())
    if c.owned:
        assert c.nnz >= mc.MI355X_CUS * 8 * 4 * 64 and c.n_parts == 1 and 32 < c.k <= 256
        own = step.ownership(c.rid, c.cid_ext, c.nu, mc.OWNED_WAVES[c.k])
        wp, ou, oi = own
        # coverage: every rating once, with its user and its (renamed) item
        assert wp[0] == 0 and wp[-1] == c.nnz and (np.diff(wp) >= 0).all()
        key = np.where(ou < 0, ~ou, ou).astype(np.int64) * (c.ni + c.n_virtual) + oi
        assert np.array_equal(np.sort(key), np.sort(c.rid * (c.ni + c.n_virtual) + c.cid_ext))
        # an exclusive user belongs to one wave
        wave = np.searchsorted(wp, np.arange(c.nnz), side="right") - 1
        ex = ou >= 0
        first = np.full(c.nu, -1)
        first[ou[ex]] = wave[ex]
        assert np.array_equal(first[ou[ex]], wave[ex]), "an exclusive user on two waves"
        unr = mc.OWNED_UNR[c.k]
        merges = step.same_user_batches(own, unr)
        extra = ", %d waves, %.0f %% of the ratings on exclusive users, %d batches of %d name one exclusive user twice" % (
            len(wp) - 1, 100 * ex.mean(), merges, unr)
        # (k > 192 runs one rating per wave step: that instantiation has no same-user merge to exercise)
        assert merges >= 100 if unr > 1 else merges == 0, merges
        assert ex.any()
    if c.form == 2:
        hot = mc.blocks_hot(c.cid, c.ni)
        cnt = np.bincount(c.cid, minlength=c.ni)
        assert hot.any() and (~hot & (cnt > 0)).any(), "LDS-resident and hot items both occur"
        extra = ", %d hot items with %.0f %% of the ratings, %d in LDS bins" % (hot.sum(), 100.0 * cnt[hot].sum() / c.nnz, (~hot & (cnt > 0)).sum())
        if c.exempt_split:
            assert 0 < len(c.split[0]) <= 63 and c.exempt["V"].sum() == len(c.split[0])
            extra += ", %d split rows exempt" % len(c.split[0])
    # T_CLEAN covers the float32 step with its 4x margin
    t32 = t32_measured(c)
    assert t32 <= mc.T_CLEAN / 4, (t32, mc.T_CLEAN)
    # C[case]: 4 x measured, rounded up to one significant digit, and <= 0.05 at LR_B, the largest such power of two
    cm = c_measured(c)
    cmax = max(cm.values())
    assert 4 * cmax <= mc.C[name] <= mc.round_up_1sig(4 * cmax * 1.05) and mc.C[name] <= 0.05, (name, cm, mc.round_up_1sig(4 * cmax))
    assert c.lr_b <= 2.0 ** -12 and np.log2(c.lr_b) == round(np.log2(c.lr_b))
    if c.lr_b < 2.0 ** -12:
        twice = max(c_measured(mc.Case(name, 2 * c.lr_b)).values())
        assert mc.round_up_1sig(4 * twice) > 0.05, "LR_B could be twice as large: %g" % twice
        extra += ", at 2 LR_B c = %.3g" % twice
    # launch B: one lost or doubled update shows on nearly every user row
    vis = {tab: mc.visibility(c, tab) for tab in (TABLES if c.use_bias else "UV")}
    print("\n%s: %d ratings, %d clean (%.0f %%), err 5..95 %% = %.2f..%.2f, rms %.2f, max touches U %d V %d, float32 step error "
          "%.3g, LR_B 2^%d, c measured %s -> C = %.3g, single-update visibility %s%s" % (
              name, n, n_clean, 100.0 * n_clean / n, e05, e95, c.E, tu.max(), tv.max(), t32, np.log2(c.lr_b),
              " ".join("%s %.3g" % kv for kv in cm.items()), mc.round_up_1sig(4 * cmax),
              ", ".join("%s %.2f" % kv for kv in vis.items()), extra))
    # A lost update shows on a row of T touches only while 1 / T > 2 C (+ the float32 floor).  The slices and the flat data
    # keep T small: >= 0.9 of the user rows.  A WHOLE epoch over users of log-normal(1) activity (10 to 17 ratings a user in
    # the mean, hundreds on the heaviest, which is the row that sets C and through it LR_B) cannot: a third and more of its
    # users have over 1 / (2 C) ratings, and a smaller step would sink a single update under the floor of its float32 add.
    # Those launches show wrong factors and lost SHARES of a row's updates; measured 0.44 .. 0.76 (header of
    # mf_step_cases.py), asserted >= 0.4.
    heavy_epoch = c.n_parts == 1 and c.data != "flat"
    assert vis["U"] >= (0.4 if heavy_epoch else 0.9), vis


def test_t_clean_follows_its_rule(oracle):
    worst = max(_T32[name] if name in _T32 else t32_measured(mc.case(name)) for name in mc.NAMES)
    print("\nfloat32 step vs float64 step over the clean rows of all cases: %.3g -> T_CLEAN = %.3g" % (worst, mc.round_up_1sig(4 * worst)))
    assert mc.T_CLEAN == mc.round_up_1sig(4 * worst)


# ---- the checks are sharp: a launch with each fault the suite could not see before must fail A or B ---------------------------
MUTANTS = list(step.FAULTS) + ["row_written_to_the_wrong_item", "one_update_lost", "one_update_doubled"]
# k = 7: a lane group of 8 with one lane beyond k; a split case short enough to have clean ratings (launch A) and copies
# whose deltas do not yet agree (the align merge differs from the mean AND, on the bias, from the sum)
MUTATION_CASES = ("slice_k7", "step_short_k64")


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _launches(c, **kw):
    """launch A, then launch B as the device would make them: B's copies are what A left (only a fault looks at them)"""
    a, copies = step.launch(c.rat, c.tables, c.split, mc.LR_A, mc.REG, mc.MU, c.use_bias, copies=None, **kw)
    b, _ = step.launch(c.rat, c.tables, c.split, c.lr_b, mc.REG, mc.MU, c.use_bias, copies=copies, **kw)
    return {"A": a, "B": b}


@pytest.mark.parametrize("name", MUTATION_CASES)
def test_the_unmutated_reference_passes_every_check(oracle, name):
    c = mc.case(name)
    good = _launches(c)
    mc.check_z(c, c.tables, c.sse)
    assert _fails(mc.check_z, c, c.tables, c.sse + 2 * c.sse_bound + 1e-9 * c.sse), "a rating counted twice or not at all shows"
    if name == "slice_k7":  # (a short launch at small k: ONE typical rating left out or counted twice shows in the sum)
        assert c.sse_bound < np.median(c.err ** 2), c.sse_bound
    worst_a = mc.check_a(c, _as_device(good["A"]))
    worst_b = mc.check_b(c, _as_device(good["B"]))
    # the Jacobi sums (C) against the per-rating deltas (numpy): two statements of the same update
    ext = step.extend(c.tables, c.split)
    _, dU, dV, dBu, dBi = step.deltas(c.rat, ext, c.lr_b, mc.REG, mc.MU, True)
    jac = step.jacobi(c.rat, ext, c.lr_b, mc.REG, mc.MU, True)
    for tab, rows, d in (("U", c.rat[0], dU), ("V", c.rat[1], dV), ("Bu", c.rat[0], dBu), ("Bi", c.rat[1], dBi)):
        want = np.zeros(jac[tab]["sum"].shape)
        np.add.at(want, rows, d)
        assert np.abs(want - jac[tab]["sum"]).max() <= 1e-15, tab
    print("\n%s: sequential float64 reference rounded to float32: A %s, B (error / tolerance) %s; sse bound %.3g of %.6g" % (
        name, worst_a, worst_b, c.sse_bound, c.sse))


@pytest.mark.parametrize("mutant", MUTANTS)
@pytest.mark.parametrize("name", MUTATION_CASES)
def test_checks_reject_a_wrong_update(oracle, name, mutant):
    c = mc.case(name)
    if mutant in step.MERGE_FAULTS and not c.n_virtual:
        # (no row of this case is split: the fault has nothing to act on — the split case carries it)
        assert not any(_fails(chk, c, _as_device(t)) for chk, t in zip((mc.check_a, mc.check_b), _launches(c, fault=mutant).values()))
        return
    if mutant in step.FAULTS:
        got = _launches(c, fault=mutant)
    elif mutant == "row_written_to_the_wrong_item":
        got = {key: tuple(t.copy() for t in g) for key, g in _launches(c).items()}
        a, b = np.flatnonzero((c.touches["V"] > 0) & ~np.isin(np.arange(c.ni), c.split[0]))[:2]  # two touched item rows change places on the way back
        for g in got.values():
            g[1][[a, b]] = g[1][[b, a]]
    else:
        tv = np.where(np.isin(np.arange(c.ni), c.split[0]), 0, c.touches["V"])
        row = int(np.flatnonzero(tv == tv[tv >= 2].min())[0])  # an item row touched a few times: not clean, not split
        got = _launches(c, **{"drop" if mutant == "one_update_lost" else "double": ("V", row)})
    out = {launch: _fails(mc.check_a if launch == "A" else mc.check_b, c, _as_device(got[launch])) for launch in "AB"}
    print("\n%s, %s: rejected by %s" % (name, mutant, " and ".join(k for k, v in out.items() if v) or "NOTHING"))
    assert out["A"] or out["B"], mutant
    if mutant.startswith("one_update") or mutant in step.MERGE_FAULTS:
        assert out["B"], "only launch B looks at rows touched more than once"
