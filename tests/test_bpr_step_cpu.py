"""The hogwild BPR step cases (tests/bpr_step_cases.py) are fair tests, their tolerances follow their rules, and their
checks are sharp — all from the CPU restatements of the samplers and the float64 step, without a device."""
import numpy as np
import pytest

import bpr_step_cases as bc
from oracle import bpr_step_oracle as step


def _as_device(tables64):
    """what a device holding float32 tables would return for these float64 results"""
    return tuple(np.asarray(t, np.float32) for t in tables64)


def _c_measured(c):
    """largest |sequential - jacobi| / path over the touched rows of all tables, three orders of application"""
    n = len(c.trip[0])
    rs = np.random.RandomState(len(c.name))
    worst = 0.0
    for order in (np.arange(n), rs.permutation(n), rs.permutation(n)):
        seq = step.sequential(c.trip, c.tables, bc.LR_B, bc.REG, c.use_bias, order)
        for tab, start, s in zip("UVB", c.tables, seq):
            j = c.jac[tab]
            rows = np.flatnonzero(j["touches"] > 0)
            if len(rows):
                dev = np.linalg.norm((s[rows] - start[rows].astype(np.float64) - j["sum"][rows]).reshape(len(rows), -1), axis=1)
                worst = max(worst, float((dev / j["path"][rows]).max()))
    return worst


_T32 = {}  # per case, filled as the cases go by


def _t32_measured(c):
    """largest |float32 step - float64 step| over the clean rows"""
    if c.name in _T32:
        return _T32[c.name]
    trip = tuple(a[c.clean] for a in c.trip)
    _, nu, nvi, nvj, nbi, nbj = step.step_f32(trip, c.tables, bc.LR_A, bc.REG, c.use_bias)
    got = {"U": nu, "V": np.concatenate([nvi, nvj]), "B": np.concatenate([nbi, nbj])}
    errs = [np.abs(got[tab] - c.clean_want[tab]) for tab in "UVB"]
    _T32[c.name] = max([float(e.max()) for e in errs if e.size] + [0.0])
    return _T32[c.name]


@pytest.mark.parametrize("name", bc.NAMES)
def test_case_is_a_fair_test_and_its_tolerances_follow_their_rules(oracle, name):
    c = bc.case(name)
    n_trip = len(c.trip[0])
    draws = n_trip + c.skipped
    if c.form == "fused":
        assert draws == c.n
    elif c.form == "ldsbin":  # every bin rounds its share of the launch down at both ends
        assert abs(draws - c.n) < c.plan["bins"]
    elif c.form == "conveyor":  # the whole epoch of the launched blocks' bins: every interaction of their items, once
        w = c.plan["bpb"] * c.plan["cap"]
        items = np.concatenate([c.slot_item[b * w:(b + 1) * w] for b in c.blocks])
        assert draws == c.draws == np.bincount(c.indices, minlength=c.ni)[items[items >= 0]].sum()
        in_block = c.bin // c.plan["bpb"]
        assert set(in_block.tolist()) == set(c.blocks), "every range of the launch draws"
        first = [int(np.flatnonzero(in_block == b)[0]) for b in c.blocks]
        assert first == sorted(first), "the triplets come range by range, in launch order"
        # every row of a triplet lives in a launched block's buffer, at the slot the layout names
        for rows in c.trip[1:]:  # (both items of a triplet in the bin that drew it)
            assert (c.item_slot[rows] // c.plan["cap"] == c.bin).all() and (c.slot_item[c.item_slot[rows]] == rows).all()
        assert c.epoch != c.layout_epoch and c.seed != c.deal_seed
        if name == "conv_pad_k64":
            assert (items < 0).sum() >= 100, "pad slots in the launched bins"
        if name == "conv_order_k64":
            assert not np.array_equal(c.rank_item, np.argsort(-np.bincount(c.indices, minlength=c.ni), kind="stable"))
    elif c.form == "strata":  # every wave's whole bucket of the phase's partition, for every phase of the launch
        sptr, w = c.strata["buckets"][0], np.arange(c.waves)
        assert draws == sum(int((sptr[8 * w + ((w // 4) % 8 + ph) % 8 + 1] - sptr[8 * w + ((w // 4) % 8 + ph) % 8]).sum())
                            for ph in range(*c.strata["phases"]))
        assert c.strata["phases"] == (c.phase, c.phase + c.phases)
    else:  # one 64-sample tile of every wave's slice
        assert draws == np.minimum(np.diff(c.ownership[0]), 64).sum()
    for start in c.tables:
        assert start.dtype == np.float32
    # real scores: z well away from 0.5 on both sides
    z = c.z
    z05, z95 = np.quantile(z, [0.05, 0.95])
    assert z05 <= 0.25 and z95 >= 0.75, (z05, z95)
    ambiguous = int((np.abs(c.x) < c.x_bound).sum())
    # (a resident-exchange launch is a whole epoch at k up to 256, and the bound grows with k: one triplet in 2 000)
    assert ambiguous <= (n_trip // 2_000 if c.exch else max(2, n_trip // 10_000)), "the float32 score bound decides nearly every sign: %d of %d ambiguous" % (ambiguous, n_trip)
    # launch A: enough clean triplets (LDS bins: enough of them with a hot positive)
    n_clean = int(c.clean.sum())
    n_hot_clean = int((c.clean & c.hot).sum()) if c.hot is not None else None
    if c.form == "conveyor":
        # positives are drawn with replacement from the bin's interactions: at most 1 / e of the triplets can be clean
        if c.kind == "sparse":
            assert c.clean_share and n_clean >= 300 and n_clean >= 0.3 * n_trip, (n_clean, n_trip)
        elif c.kind == "heavy":
            assert c.skipped >= 8 and n_clean >= 300 and c.touches["U"].max() >= 100, (c.skipped, n_clean)
        else:  # popularity negatives: every negative is a positive of the launch too, launch B carries the case
            assert c.kind == "pop" and c.neg_pop and not c.clean_share
            assert (np.bincount(c.indices, minlength=c.ni)[c.trip[2]] > 0).all(), "a negative is the item of an interaction"
    elif c.exch:  # a whole epoch: next to no triplet is clean, launch B carries the family (its conditions: _exch_case_is_fair)
        assert not c.clean_share and c.n == c.nnz and c.s_begin == 0
    elif c.clean_share:
        assert n_clean >= 300 and 3 * n_clean >= n_trip, (n_clean, n_trip)
        if c.form == "ldsbin":
            assert n_hot_clean >= 50, n_hot_clean
    elif not c.only_b:
        assert n_clean >= 300, n_clean  # (what exists is still checked: see the case's comment)
    if c.name == "lds_wide_k64":
        assert np.bincount(c.bin, minlength=c.plan["bins"]).min() >= 8 * 16 * 64, "every bin takes the 64-draw tiles"
    # rows beyond the trained range and untouched rows exist, so "bit-identical" is a real check
    tv = c.touches["V"]
    assert (tv[c.ni:] == 0).all() and ((tv[:c.ni] == 0).any() or c.only_b) and tv.max() >= 3
    # T_CLEAN covers the float32 step with its 4x margin
    t32 = _t32_measured(c)
    assert t32 <= bc.T_CLEAN / 4, (t32, bc.T_CLEAN)
    # C[case]: 4 x measured, rounded up to one significant digit
    # (the "sqrt" twin: its steps are taken on rows displaced by (sqrt(2) - 1) of the rank's own earlier deltas — the share of
    # three host runs of the protocol instead)
    cm = _c_twin_measured(c) if c.exch and c.twin and c.rule == "sqrt" else _c_measured(c)
    assert 4 * cm <= bc.C[name] <= bc.round_up_1sig(4 * cm * 1.05), (name, cm, bc.round_up_1sig(4 * cm))
    # launch B: one lost or doubled update shows on at least half of the touched rows
    vis = {tab: bc.visibility(c, tab) for tab in ("UVB" if c.use_bias else "UV")}
    print("\n%s: %d triplets (%d skipped), %d clean (%.0f %%)%s, z 5..95 %% = %.2f..%.2f, %d ambiguous signs, max touches U %d V %d, "
          "float32 step error %.3g, c measured %.3g -> C = %.3g, single-update visibility %s" % (
              name, n_trip, c.skipped, n_clean, 100.0 * n_clean / n_trip,
              "" if n_hot_clean is None else ", %d with a hot positive" % n_hot_clean, z05, z95, ambiguous,
              c.touches["U"].max(), tv.max(), t32, cm, bc.round_up_1sig(4 * cm),
              ", ".join("%s %.2f" % kv for kv in vis.items())))
    if not c.only_b:  # (the wide-tile case alone may fall below: its comment says why)
        assert min(vis.values()) >= (0.8 if c.exch else 0.5), vis
    if c.exch:
        _exch_case_is_fair(c, n_trip)
    if c.form == "strata":
        _strata_case_is_fair(c, n_trip)
    if c.form == "owned":
        tu = c.touches["U"]
        assert tu[tu > 0].mean() < 4 and tv[tv > 0].mean() < 4, "few touches per row"
        assert c.shared.any() and not c.shared.all(), "exclusive users (plain stores) and shared ones (atomics) both occur"
        assert vis["U"] >= 0.5, vis


_STRATA_SKIPPED = {}  # per strata case, filled as the cases go by


def _repeats_in_a_step(group, row, n_rows):
    """steps (groups) in which one row is named more than once"""
    key, count = np.unique(group * n_rows + row, return_counts=True)
    return len(np.unique(key[count > 1] // n_rows))


def _strata_case_is_fair(c, n_trip):
    """the conditions of a strata case, from the restatement alone: few enough racy rows that the exact rule carries the
    case, enough in-step merges, hot and shared rows that every write path of the kernel is under a rule"""
    t = c.strata
    _STRATA_SKIPPED[c.name] = c.skipped
    touched = int((c.touches["V"] > 0).sum())
    racy = int(c.racy.sum())
    groups = c.racy_groups()
    cold = ~c.ref_hot
    rep_cold = _repeats_in_a_step(c.ref_group[cold], c.ref_row[cold], c.total_items)
    rep_hot = _repeats_in_a_step(c.ref_group[~cold], c.ref_row[~cold], c.total_items)
    excl = ~c.shared
    rep_user = _repeats_in_a_step(c.trip_group[excl], c.trip[0][excl], c.nu)
    steps = int(c.trip_group.max()) + 1
    partial = int((np.bincount(c.trip_group) < t["unr"]).sum())
    vis = bc.racy_visible(c)
    print("\n%s: %d waves, phases %s, %d triplets in %d steps of %d (%d partial, %d in a second tile); n_hot %d, %d hot positives, %d hot "
          "negatives, %d shared-user triplets; steps with a repeated cold item %d, hot item %d, exclusive user %d; racy rows %d of "
          "%d touched = %.1f %% (cap %.0f %%), groups per racy row %s, one lost group visible on %.2f of them" % (
              c.name, c.waves, t["phases"], n_trip, steps, t["unr"], partial, int((t["step"] >= 64).sum()), t["n_hot"],
              int(t["hot_i"].sum()), int(t["hot_j"].sum()), int(c.shared.sum()), rep_cold, rep_hot, rep_user, racy, touched,
              100.0 * racy / touched, 100 * c.racy_cap, {m: len(v[0]) for m, v in sorted(groups.items())},
              vis.mean() if len(vis) else 1.0))
    assert t["unr"] == (4 if c.k <= 64 else 2 if c.k <= 192 else 1)
    assert racy <= c.racy_cap * touched, (racy, touched)
    assert not groups or max(groups) <= bc.MAX_RACY_GROUPS, sorted(groups)
    assert (c.touches["V"][c.racy] >= 2).all() and not c.item_hot[c.racy].any()
    all_hot, no_hot = c.hot_cfg[:2] == (1000, 0), c.hot_cfg[0] == 0
    if all_hot:  # every item hot: no cold row to merge or to race; the atomics carry the repeats
        assert t["n_hot"] == c.ni and t["hot_i"].all() and t["hot_j"].all() and racy == 0
        assert t["unr"] == 1 or (rep_hot >= 1000 and rep_user >= 1000), (rep_hot, rep_user)
    elif t["unr"] > 1:
        assert rep_cold >= 1000 and rep_user >= 1000, (rep_cold, rep_user)
    if no_hot:
        assert t["n_hot"] == 0 and not t["hot_i"].any() and not t["hot_j"].any()
    elif not all_hot:
        assert 0 < t["n_hot"] < c.ni and t["hot_i"].sum() >= 1000 and t["hot_j"].sum() >= 1000
    assert c.shared.any() and not c.shared.all()
    assert (np.bincount(c.trip_group) <= t["unr"]).all()
    if c.name == "strata_partial_k64":  # three partitions hold an item more than the others
        sizes = np.bincount(orc_partitions(c), minlength=8)
        assert c.ni % 8 == 3 and sorted(sizes.tolist()) == [c.ni // 8] * 5 + [c.ni // 8 + 1] * 3
    if c.name == "strata_rehash2_k100":
        from oracle import oracle as orc

        assert t["key"] == orc.strata_key(c.seed, 0) != orc.strata_key(c.seed, 1)
    if c.name == "strata_epoch1_k64":
        from oracle import oracle as orc

        assert t["key"] == orc.strata_key(c.seed, 1) != orc.strata_key(c.seed, 0)


def orc_partitions(c):
    from oracle import oracle as orc

    return orc.strata_partitions(c.strata["key"], c.ni)


def test_the_strata_cases_hold_a_skipped_draw(oracle):
    skipped = {name: _STRATA_SKIPPED[name] if name in _STRATA_SKIPPED else bc.case(name).skipped for name in bc.STRATA_NAMES}
    print("\nskipped draws of the strata cases: %s" % skipped)
    assert sum(skipped.values()) >= 1


def test_t_clean_follows_its_rule(oracle):
    worst = max(_T32[name] if name in _T32 else _t32_measured(bc.case(name)) for name in bc.NAMES)
    print("\nfloat32 step vs float64 step over the clean rows of all cases: %.3g -> T_CLEAN = %.3g" % (worst, bc.round_up_1sig(4 * worst)))
    assert bc.T_CLEAN == bc.round_up_1sig(4 * worst)


# ---- the checks are sharp: a reference with each fault the suite could not see before must fail A or B -------------------
MUTANTS = list(step.FAULTS) + ["row_written_to_the_wrong_item", "one_update_lost", "one_update_doubled"]


def _fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


@pytest.fixture(scope="module")
def mutation_case(oracle):
    c = bc.case("fused_k7")  # k = 7: a lane group of 8 with one lane beyond k
    good = {lr: step.sequential(c.trip, c.tables, lr, bc.REG, True) for lr in (bc.LR_A, bc.LR_B)}
    return c, good


def test_the_unmutated_reference_passes_every_check(mutation_case):
    c, good = mutation_case
    bc.check_z(c, c.tables, int((c.x > 0).sum()), c.skipped)
    worst_a = bc.check_a(c, _as_device(good[bc.LR_A]))
    worst_b = bc.check_b(c, _as_device(good[bc.LR_B]))
    # the Jacobi sums (C) against the per-triplet deltas (numpy): two statements of the same update
    _, _, dU, dVi, dVj, dBi, dBj = step.deltas(c.trip, *c.tables, bc.LR_B, bc.REG, True)
    want_v, want_b = np.zeros(c.tables[1].shape), np.zeros(c.tables[2].shape)
    np.add.at(want_v, np.concatenate(c.trip[1:]), np.concatenate([dVi, dVj]))
    np.add.at(want_b, np.concatenate(c.trip[1:]), np.concatenate([dBi, dBj]))
    assert np.abs(want_v - c.jac["V"]["sum"]).max() <= 1e-15 and np.abs(want_b - c.jac["B"]["sum"]).max() <= 1e-15
    print("\nsequential float64 reference rounded to float32: A %s, B (error / tolerance) %s" % (worst_a, worst_b))


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checks_reject_a_wrong_update(mutation_case, mutant):
    c, good = mutation_case
    out = {}
    for launch, lr in (("A", bc.LR_A), ("B", bc.LR_B)):
        if mutant in step.FAULTS:
            got = step.sequential(c.trip, c.tables, lr, bc.REG, True, fault=mutant)
        elif mutant == "row_written_to_the_wrong_item":
            got = tuple(t.copy() for t in good[lr])
            a, b = c.trip[1][np.flatnonzero(c.clean)[:2]]  # two touched item rows change places on the way back
            got[1][[a, b]] = got[1][[b, a]]
        else:
            tv = c.touches["V"]
            row = int(np.flatnonzero(tv == 3)[0])  # a row touched a few times, so not a clean one
            got = step.sequential(c.trip, c.tables, lr, bc.REG, True, **{"drop" if mutant == "one_update_lost" else "double": ("V", row)})
        check = bc.check_a if launch == "A" else bc.check_b
        out[launch] = _fails(check, c, _as_device(got))
    print("\n%s: rejected by %s" % (mutant, " and ".join(k for k, v in out.items() if v) or "NOTHING"))
    assert out["A"] or out["B"], mutant
    if mutant.startswith("one_update"):
        assert out["B"], "only launch B looks at rows touched more than once"


# ---- the conveyor: the block buffers' layout, and the same mutants against a launch of three ranges ------------------------
def test_pack_and_unpack_are_inverse(oracle):
    c = bc.case("conv_pad_k64")
    bpb, cap = c.plan["bpb"], c.plan["cap"]
    w, blocks = bpb * cap, list(range(c.n_blocks))
    assert len(c.bufs) == c.n_blocks and all(b.shape == (w * c.k + w,) for b in c.bufs)
    # a slot's row and bias sit where csrc/bpr_ldsbin.inc reads them: row s at s k, bias s at bpb cap k + s
    s = int(c.item_slot[12345])
    blk, o = divmod(s, w)
    assert np.array_equal(c.bufs[blk][o * c.k:(o + 1) * c.k], c.tables[1][12345]) and c.bufs[blk][w * c.k + o] == c.tables[2][12345]
    n_pad = sum(int((b == np.float32(bc.PAD)).sum()) for b in c.bufs)
    assert n_pad == (c.slot_item < 0).sum() * (c.k + 1) > 0
    rs = np.random.RandomState(1)
    V0, B0 = rs.normal(size=c.tables[1].shape).astype(np.float32), rs.normal(size=c.tables[2].shape).astype(np.float32)
    V, B = bc.unpack(c.bufs, V0, B0, c.slot_item, blocks, bpb, cap)
    assert np.array_equal(V[:c.ni], c.tables[1][:c.ni]) and np.array_equal(B[:c.ni], c.tables[2][:c.ni])
    assert np.array_equal(V[c.ni:], V0[c.ni:]) and np.array_equal(B[c.ni:], B0[c.ni:])  # (rows beyond n_items are in no buffer)
    again = bc.pack(V, B, c.slot_item, blocks, bpb, cap)
    assert all(np.array_equal(a, b) for a, b in zip(again, c.bufs))
    # into=: only the item slots are written
    into = [np.full_like(b, 3.0) for b in c.bufs[1:3]]
    bc.pack(V, B, c.slot_item, [1, 2], bpb, cap, into=into)
    for buf, blk in zip(into, (1, 2)):
        pad = np.tile(c.slot_item[blk * w:(blk + 1) * w] < 0, c.k + 1)
        pad[:w * c.k] = np.repeat(c.slot_item[blk * w:(blk + 1) * w] < 0, c.k)
        assert (buf[pad] == 3.0).all() and np.array_equal(buf[~pad], c.bufs[blk][~pad])


def _host_conveyor_launch(c, lr, fault=None, bias_at=None, exchange=None, **kw):
    """what a conveyor launch leaves in ALL blocks' buffers, by a host stand-in that finds its rows as the kernel does: range
    r's in d_rows[r], rows at slot x k, biases from bias_at on.  exchange = (r, q): ranges r and q are handed each other's
    buffer.  Returns (bufs, U)."""
    bpb, cap = c.plan["bpb"], c.plan["cap"]
    bufs = [b.copy() for b in c.bufs]
    d_rows = [bufs[b] for b in c.blocks]
    if exchange is not None:
        r, q = exchange
        d_rows[r], d_rows[q] = d_rows[q], d_rows[r]
    V, B = bc.unpack(d_rows, c.tables[1], c.tables[2], c.slot_item, c.blocks, bpb, cap, bias_at=bias_at)
    U, V, B = _as_device(step.sequential(c.trip, (c.tables[0], V, B), lr, bc.REG, c.use_bias, fault=fault, **kw))
    bc.pack(V, B, c.slot_item, c.blocks, bpb, cap, into=d_rows, bias_at=bias_at)
    return bufs, U


@pytest.fixture(scope="module")
def conveyor_mutation_case(oracle):
    return bc.case("conv_ranges3_k100")


def test_the_unmutated_conveyor_launch_passes_every_check(conveyor_mutation_case):
    c = conveyor_mutation_case
    bufs, U = _host_conveyor_launch(c, 0.0)
    bc.check_z(c, bc.conveyor_tables(c, "Z", bufs, U), int((c.x > 0).sum()), c.skipped)
    worst_a = bc.check_a(c, bc.conveyor_tables(c, "A", *_host_conveyor_launch(c, bc.LR_A)))
    worst_b = bc.check_b(c, bc.conveyor_tables(c, "B", *_host_conveyor_launch(c, bc.LR_B)))
    print("\nsequential float64 reference through the block buffers: A %s, B (error / tolerance) %s" % (worst_a, worst_b))


CONVEYOR_MUTANTS = MUTANTS + ["bias_area_at_cap_k", "two_ranges_buffers_exchanged", "unlaunched_block_written"]


@pytest.mark.parametrize("mutant", CONVEYOR_MUTANTS)
def test_checks_reject_a_wrong_conveyor_update(conveyor_mutation_case, mutant):
    c = conveyor_mutation_case
    bpb, cap = c.plan["bpb"], c.plan["cap"]
    out = {}
    for launch, lr in (("A", bc.LR_A), ("B", bc.LR_B)):
        kw = {}
        if mutant in step.FAULTS:
            kw = dict(fault=mutant)
        elif mutant.startswith("one_update"):
            tv = c.touches["V"]
            row = int(np.flatnonzero(tv == 3)[0])  # a row touched a few times, so not a clean one
            kw = {"drop" if mutant == "one_update_lost" else "double": ("V", row)}
        elif mutant == "bias_area_at_cap_k":  # a launched bin's biases sought at cap k instead of bpb cap k
            kw = dict(bias_at=cap * c.k)
        elif mutant == "two_ranges_buffers_exchanged":
            kw = dict(exchange=(0, 2))
        bufs, U = _host_conveyor_launch(c, lr, **kw)
        if mutant == "row_written_to_the_wrong_item":
            a, b = c.item_slot[c.trip[1][np.flatnonzero(c.clean)[:2]]]  # two touched rows change slots on the way back
            (ba, oa), (bb, ob) = divmod(int(a), bpb * cap), divmod(int(b), bpb * cap)
            ra, rb = bufs[ba][oa * c.k:(oa + 1) * c.k].copy(), bufs[bb][ob * c.k:(ob + 1) * c.k].copy()
            bufs[ba][oa * c.k:(oa + 1) * c.k], bufs[bb][ob * c.k:(ob + 1) * c.k] = rb, ra
        elif mutant == "unlaunched_block_written":
            blk = next(b for b in range(c.n_blocks) if b not in c.blocks)
            bufs[blk][5 * c.k + 1] += np.float32(1e-3)

        def run(check):
            check(c, bc.conveyor_tables(c, launch, bufs, U))

        out[launch] = _fails(run, bc.check_a if launch == "A" else bc.check_b)
    print("\n%s: rejected by %s" % (mutant, " and ".join(k for k, v in out.items() if v) or "NOTHING"))
    assert out["A"] or out["B"], mutant
    if mutant.startswith("one_update"):
        assert out["B"], "only launch B looks at rows touched more than once"


def test_checks_reject_a_written_pad_slot(oracle):
    c = bc.case("conv_pad_k64")
    w = c.plan["bpb"] * c.plan["cap"]
    blk = c.blocks[0]
    pad = int(np.flatnonzero(c.slot_item[blk * w:(blk + 1) * w] < 0)[3])
    for at in (pad * c.k + c.k - 1, w * c.k + pad):  # the row's last factor; the bias
        bufs, U = _host_conveyor_launch(c, bc.LR_B)
        bc.check_b(c, bc.conveyor_tables(c, "B", bufs, U))
        bufs[blk][at] = 0.0
        with pytest.raises(AssertionError, match="pad slot"):
            bc.conveyor_tables(c, "B", bufs, U)


# ---- the XCD-strata form: its own ways of being wrong, each built from the float64 step on the case's own triplets ----------
STRATA_MUTANTS = {  # fault -> the case it is shown on
    "lead_of_a_repeated_cold_row_stores_its_own_delta": "strata_k64",
    "every_reference_of_a_repeated_cold_row_adds_the_total": "strata_k64",
    "last_delta_of_a_repeated_exclusive_user_only": "strata_k64",
    "negative_bias_delta_with_the_positive_sign": "strata_k64",
    "hot_rows_written_by_their_last_toucher": "strata_k64",
    "bias_written_one_row_off": "strata_k64",
    "lanes_from_64_of_an_r2_row_left_out": "strata_k100",
}
_MERGE_FAULTS = list(STRATA_MUTANTS)[:3] + ["hot_rows_written_by_their_last_toucher"]  # (they change no clean row: launch B's to find)


def _keep_one_per_key(key, order, which):
    """mask over the references: the first / last one (by `order`) of every key"""
    o = np.lexsort((order, key))
    ks = key[o]
    edge = np.r_[True, ks[1:] != ks[:-1]] if which == "first" else np.r_[ks[1:] != ks[:-1], True]
    keep = np.zeros(len(key), bool)
    keep[o[edge]] = True
    return keep


def _strata_host_launch(c, lr, fault=None):
    """float64 (U, V, B) after the launch as a strata kernel with `fault` would leave them: every triplet's deltas from the
    start tables (the Jacobi sum the checks hold the device to), each reference's delta weighted or moved as the fault says"""
    u, i, j = c.trip
    n = len(u)
    _, z, dU, dVi, dVj, dBi, dBj = step.deltas(c.trip, *c.tables, lr, bc.REG, c.use_bias)
    w_u, w_v = np.ones(n), np.ones(2 * n)  # per triplet; per item reference (the i's, then the j's)
    in_step = 2 * c.ref_trip + c.ref_isj  # the order of the references: triplet by triplet, i before j
    if fault in ("lead_of_a_repeated_cold_row_stores_its_own_delta", "every_reference_of_a_repeated_cold_row_adds_the_total"):
        cold = np.flatnonzero(~c.ref_hot)
        key = c.ref_group[cold] * c.total_items + c.ref_row[cold]  # (step, row)
        if fault.startswith("lead"):
            w_v[cold[~_keep_one_per_key(key, in_step[cold], "first")]] = 0.0
        else:
            _, inv, count = np.unique(key, return_inverse=True, return_counts=True)
            w_v[cold] = count[inv]
    elif fault == "last_delta_of_a_repeated_exclusive_user_only":
        excl = np.flatnonzero(~c.shared)
        w_u[excl[~_keep_one_per_key(c.trip_group[excl] * c.nu + u[excl], excl, "last")]] = 0.0
    elif fault == "hot_rows_written_by_their_last_toucher":
        hot = np.flatnonzero(c.ref_hot)
        w_v[hot[~_keep_one_per_key(c.ref_row[hot], in_step[hot], "last")]] = 0.0
    elif fault == "negative_bias_delta_with_the_positive_sign":
        dBj = lr * (z - bc.REG * c.tables[2][j].astype(np.float64))
    elif fault == "lanes_from_64_of_an_r2_row_left_out":
        assert 64 < c.k <= 128
        dU[:, 64:], dVi[:, 64:], dVj[:, 64:] = 0.0, 0.0, 0.0
    else:
        assert fault in (None, "bias_written_one_row_off"), fault
    U, V, B = (np.array(t, np.float64) for t in c.tables)
    np.add.at(U, u, dU * w_u[:, None])
    np.add.at(V, i, dVi * w_v[:n, None])
    np.add.at(V, j, dVj * w_v[n:, None])
    off = 1 if fault == "bias_written_one_row_off" else 0
    np.add.at(B, i + off, dBi * w_v[:n])
    np.add.at(B, j + off, dBj * w_v[n:])
    return U, V, B


def test_the_unmutated_strata_launch_passes_every_check_and_a_lost_store_passes_the_racy_rule(oracle):
    c = bc.case("strata_k64")
    bc.check_z(c, c.tables, int((c.x > 0).sum()), c.skipped)
    worst_a = bc.check_a(c, _as_device(step.sequential(c.trip, c.tables, bc.LR_A, bc.REG, True)))
    for got in (step.sequential(c.trip, c.tables, bc.LR_B, bc.REG, True), _strata_host_launch(c, bc.LR_B)):
        worst_b = bc.check_b_strata(c, _as_device(got))
        assert worst_b["racy"] == c.racy.sum() == worst_b["whole"] and worst_b["lost"] == 0, worst_b
    # every racy row keeps its LAST group only (each store overwrote the one before): the racy rule accepts, the exact one does not
    U, V, B = _strata_host_launch(c, bc.LR_B)
    for m, (rows, dv, db) in c.racy_groups().items():
        V[rows] = c.tables[1][rows].astype(np.float64) + dv[:, -1]
        B[rows] = c.tables[2][rows].astype(np.float64) + db[:, -1]
    lost = bc.check_b_strata(c, _as_device((U, V, B)))
    assert lost["whole"] == lost["racy"] and lost["lost"] > 0.9 * lost["racy"], lost
    assert _fails(bc.check_b, c, _as_device((U, V, B)))
    print("\nstrata_k64, sequential float64 reference rounded to float32: A %s, B %s; every racy row down to one group: %s" % (
        worst_a, worst_b, lost))


@pytest.mark.parametrize("mutant", list(STRATA_MUTANTS))
def test_checks_reject_a_wrong_strata_update(oracle, mutant):
    c = bc.case(STRATA_MUTANTS[mutant])
    out = {}
    for launch, lr in (("A", bc.LR_A), ("B", bc.LR_B)):
        got = _as_device(_strata_host_launch(c, lr, mutant))
        out[launch] = _fails(bc.check_a if launch == "A" else bc.check_b_strata, c, got)
    print("\n%s, %s: rejected by %s" % (c.name, mutant, " and ".join(k for k, v in out.items() if v) or "NOTHING"))
    assert out["A"] or out["B"], mutant
    if mutant in _MERGE_FAULTS:
        assert out["B"], "only launch B looks at rows touched more than once"


@pytest.mark.parametrize("name", ["strata_k64", "strata_k200"])
@pytest.mark.parametrize("mutant", ["every_group_scaled_by_2", "row_left_at_its_start_value"])
def test_the_racy_rule_rejects_a_wrong_racy_row(oracle, name, mutant):
    """both faults on EVERY racy row at once: the rule must reject at least nine tenths of the rows on which one group shows
    at all (path / groups > 2 x tolerance)"""
    c = bc.case(name)
    U, V, B = _strata_host_launch(c, bc.LR_B)
    rows = np.flatnonzero(c.racy)
    scale = 2.0 if mutant == "every_group_scaled_by_2" else 0.0
    V[rows] = c.tables[1][rows] + scale * c.jac["V"]["sum"][rows]
    B[rows] = c.tables[2][rows] + scale * c.jac["B"]["sum"][rows]
    r = bc.racy_rows(c, _as_device((U, V, B)))
    visible = bc.racy_visible(c)
    assert len(visible) == len(r["ok"]) == len(rows) and np.array_equal(np.sort(r["rows"]), rows)
    rejected = float((~r["ok"][visible]).mean())
    print("\n%s, %s: one group shows on %.3f of the %d racy rows; the racy rule rejects %.3f of those (%.3f of all)" % (
        name, mutant, visible.mean(), len(rows), rejected, (~r["ok"]).mean()))
    assert visible.mean() >= 0.5 and rejected >= 0.9
    assert _fails(bc.check_b_strata, c, _as_device((U, V, B)))


# ---- the resident exchange: a float64 host model of the protocol, the cases' conditions, and the protocol's own ways of being wrong ----
EXCH_FAULTS = ("step_left_out_of_the_published_delta", "delta_published_by_two_exchanges", "row_never_published",
               "correction_applied_by_the_launch_and_by_the_flush", "correction_never_applied",
               "hot_delta_and_base_from_two_reads", "keeps_written_with_the_bucket_value", "weight_left_at_zero")
_TWIN_ONLY = EXCH_FAULTS[3:5] + EXCH_FAULTS[6:7]  # (without a twin every correction is an exact zero and bucket == keep)


def _exch_victim(c, seg):
    """a cold item row that ONE triplet touches, before the first boundary of its bin, on which one update shows: (row, the
    triplet's float64 delta of launch B for [row | bias])"""
    u, i, j = c.trip
    vis = c.jac["V"]["path"] > 2 * bc.tolerance_b(c, "V", extra=c.n_ex)
    hot = np.zeros(c.total_items, bool)
    hot[c.hot_items] = True
    t = int(np.flatnonzero((seg == 0) & (c.touches["V"][i] == 1) & ~hot[i] & vis[i])[0])
    _, _, _, dVi, _, dBi, _ = step.deltas(tuple(a[t:t + 1] for a in c.trip), *c.tables, bc.LR_B, bc.REG, c.use_bias)
    return int(i[t]), np.r_[dVi[0], dBi[0]]


def exch_host_launch(c, lr, n_ex, rule, twin, lag, fault=None):
    """The resident exchange of csrc/bpr_ldsbin.inc and cornac_amd/dist.py in float64 numpy, all bins in step: the triplets
    in the restatement's order, segment by segment (Case.exch_segments: boundary e of a bin at its draw (e + 1) (n_tiles //
    n_ex) tile_w, the last at the end); at boundary e every row publishes d = row - base into bucket e (twice it with a
    twin) and keep e, with the rule's weights, and base = row; an exchange is applied `lag` boundaries after its
    publication (row += c, base += c, c = rule(S) - keep), the rest by the flush.  The hot rows publish their last delta
    BEFORE the last fiftieth of the launch's triplets (their owner bin has finished, other bins step them still): what
    they take afterwards is table - base.  One rank alone has S = d and a weight that makes the factor 1: c is an exact zero
    and is not computed.  Returns `res` as the device test reads it back — U, table and base rounded to float32; the keeps
    and buckets go to the reducer in float64 as they are (a float32 keep is the exact difference of two float32 rows on the
    device, which a rounded float64 difference is not) — and, under "f64", the float64 U, table and P.  fault: one of
    EXCH_FAULTS, on the row of _exch_victim (the hot fault: on the first hot row)."""
    from oracle import oracle as orc

    assert (n_ex, rule, twin) == (c.n_ex, c.rule, c.twin)  # (bc.ExchReducer reads them from the case)
    nt, k = c.total_items, c.k
    nk, width, ranks = nt * k, nt * k + nt, 2.0 if twin else 1.0
    reg = bc.REG if lr else 0.0
    U = c.tables[0].astype(np.float64)
    flat = np.concatenate([c.tables[1].ravel(), c.tables[2]]).astype(np.float64)
    V, B = flat[:nk].reshape(nt, k), flat[nk:]  # (views: the steps go into `flat`)
    base = flat.copy()
    red, pending, ksum = bc.ExchReducer(c), {}, np.zeros(width)
    seg = c.exch_segments(n_ex)
    hot_els = np.concatenate([(c.hot_items[:, None] * k + np.arange(k)[None, :]).ravel(), nk + c.hot_items]).astype(np.int64)
    victim = delta = els = None
    if fault is not None and fault != "hot_delta_and_base_from_two_reads":
        victim, delta = _exch_victim(c, seg)
    elif fault is not None:
        victim = int(c.hot_items[0])
        t = c.triplets_of("V", victim)[-1:]
        _, _, _, dVi, dVj, dBi, dBj = step.deltas(tuple(a[t] for a in c.trip), *c.tables, bc.LR_B, bc.REG, c.use_bias)
        delta = np.r_[dVi[0], dBi[0]] if c.trip[1][t[0]] == victim else np.r_[dVj[0], dBj[0]]
    if fault is not None:
        assert lr == bc.LR_B, "the protocol's faults are launch B's to find"
        els = np.r_[victim * k:(victim + 1) * k, nk + victim]
    published_once = False

    def correction(e):
        K, Bk = pending.pop(e)
        S, wV, wB = Bk[:width], Bk[width:width + nt], Bk[width + nt:]
        if rule == "sqrt":
            fV, fB = 1.0 / np.sqrt(np.maximum(wV, 1.0)), 1.0 / np.sqrt(np.maximum(wB, 1.0))
        else:
            n2V, n2B = (S[:nk].reshape(nt, k) ** 2).sum(axis=1), S[nk:] ** 2
            fV = np.where(n2V > 0, np.minimum(1.0, wV / np.where(n2V > 0, n2V, 1.0)), 1.0)
            fB = np.where(n2B > 0, np.minimum(1.0, wB / np.where(n2B > 0, n2B, 1.0)), 1.0)
        cc = np.empty(width)
        cc[:nk] = (S[:nk].reshape(nt, k) * fV[:, None]).ravel() - K[:nk]
        cc[nk:] = S[nk:] * fB - K[nk:]
        return cc

    def apply(e):
        if not twin:
            return
        cc = correction(e)
        if fault == "correction_never_applied" and e == 0:
            cc[els] = 0.0
        if fault == "correction_applied_by_the_launch_and_by_the_flush" and e == 0:
            cc[els] *= 2.0
        flat[:] += cc
        base[:] += cc

    def publish(e, hot_snapshot=None):
        nonlocal published_once
        cur = flat.copy()
        if hot_snapshot is not None:
            cur[hot_els] = hot_snapshot
        d = cur - base
        hold = None  # elements whose base does not move to `cur`
        if fault == "row_never_published":
            d[els], hold = 0.0, els
        elif victim is not None and not published_once and d[els].any():
            published_once = True
            if fault == "step_left_out_of_the_published_delta":
                d[els] -= delta
            elif fault == "delta_published_by_two_exchanges":
                hold = els
        Bk = np.empty(width + 2 * nt)
        Bk[:width] = ranks * d
        dV, dB = d[:nk].reshape(nt, k), d[nk:]
        if rule == "sqrt":
            Bk[width:width + nt], Bk[width + nt:] = ranks * (dV != 0).any(axis=1), ranks * (dB != 0)
        else:
            Bk[width:width + nt], Bk[width + nt:] = ranks * (dV * dV).sum(axis=1), ranks * dB * dB
        if fault == "weight_left_at_zero" and d[els].any():
            Bk[width + victim] = 0.0
        if fault == "keeps_written_with_the_bucket_value":
            d = Bk[:width].copy()
        red.add(d, Bk)
        ksum[:] += d
        if twin:
            pending[e] = (d, Bk)
        kept = base[hold].copy() if hold is not None else None
        base[:] = cur
        if hold is not None:
            base[hold] = kept
        if fault == "hot_delta_and_base_from_two_reads" and hot_snapshot is not None:
            base[els] += delta  # the base was read a step after the delta

    applied = 0
    for q in range(n_ex):
        ids = np.flatnonzero(seg == q)
        snap = None
        if q == n_ex - 1:
            cut = len(ids) - len(ids) // 50
            orc.bpr_apply_seq_f64(c.trip, ids[:cut], U, V, B, lr, reg, c.use_bias)
            snap, ids = flat[hot_els].copy(), ids[cut:]
        orc.bpr_apply_seq_f64(c.trip, ids, U, V, B, lr, reg, c.use_bias)
        publish(q, snap)
        while applied + lag <= q:
            apply(applied)
            applied += 1
    in_launch = applied
    while applied < n_ex:  # the flush
        apply(applied)
        applied += 1
    signals = np.r_[np.full(n_ex, c.plan["bins"]), np.ones(n_ex, np.int64), 0]
    record = np.zeros(nt, np.int64)
    record[:c.ni] = in_launch
    return dict(U=U.astype(np.float32), flat=flat.astype(np.float32), base=base.astype(np.float32), signals=signals, applied=record,
                red=red.result(), f64=dict(U=U, flat=flat, P=ksum + (flat - base)))


def _c_twin_measured(c):
    """largest |P - jacobi| / path (U: |table - start - jacobi| / path) over the touched rows, float64, over three host runs of
    the protocol that apply an exchange 0, 1 and n_ex boundaries after its publication"""
    worst = 0.0
    for lag in (0, 1, c.n_ex):
        f = exch_host_launch(c, bc.LR_B, c.n_ex, c.rule, c.twin, lag)["f64"]
        moved = {"U": f["U"] - c.tables[0].astype(np.float64)}
        moved["V"], moved["B"] = bc._exch_vb(c, f["P"])
        for tab in "UVB":
            j = c.jac[tab]
            rows = np.flatnonzero(j["touches"] > 0)
            dev = np.linalg.norm((moved[tab][rows] - j["sum"][rows]).reshape(len(rows), -1), axis=1)
            worst = max(worst, float((dev / j["path"][rows]).max()))
    return worst


_EXCH_FACTS = {}  # per exchange case, filled as the cases go by: (neg_pop, triplets with a hot positive, skipped draws)


def _exch_facts(name):
    if name not in _EXCH_FACTS:
        c = bc.case(name)
        _EXCH_FACTS[name] = (c.neg_pop, int(c.hot.sum()), c.skipped)
    return _EXCH_FACTS[name]


def _exch_case_is_fair(c, n_trip):
    """the conditions of a resident-exchange case from the restatement alone, and the unmutated host model, rounded to
    float32, through every check of the device test"""
    _EXCH_FACTS[c.name] = (c.neg_pop, int(c.hot.sum()), c.skipped)
    draws, tile_w, tiles = c.exch_tiles()
    per = tiles // c.n_ex
    tv = c.touches["V"]
    print("\n%s: plan %d bins x %d rows, n_ex %d, rule %s%s; %d..%d tiles of %d draws per bin, %d..%d between two boundaries; %d triplets, "
          "%d skipped, %d with a hot positive (n_hot %d); mean touches of a touched V row %.1f" % (
              c.name, c.plan["bins"], c.plan["cap"], c.n_ex, c.rule, ", twin" if c.twin else "", tiles.min(), tiles.max(), tile_w.max(),
              per.min(), per.max(), n_trip, c.skipped, int(c.hot.sum()), c.n_hot, tv[tv > 0].mean()))
    assert c.n_ex * (c.total_items * c.k + 3 * c.total_items) <= 2.5e8, "buckets and keeps near 1 GB each at the most"
    assert (tile_w == 32).all()
    bins = {"exch_k40": 256, "exch_nobias_k64": 256, "exch_partial_k64": 256, "exch_one_k64": 256, "exch_ex32_k64": 256,
            "exch_twin_sqrt_k64": 256}.get(c.name, 1024)
    assert c.plan["bins"] == bins and not c.plan["passing"], c.plan
    if c.name == "exch_partial_k64":
        assert c.ni % bins == 13 and c.plan["cap"] == 257
    if c.name == "exch_one_k64":
        assert c.n_ex == 1
    elif c.name == "exch_ex32_k64":  # ex_per = 1: one part per boundary, a boundary on every tile
        assert c.n_ex == 32 and (per == 1).all(), (per.min(), per.max())
    elif c.name == "exch_short_k64":  # ex_per = 0: every boundary at the end of the launch
        assert (per == 0).all() and tiles.min() >= 1, (tiles.min(), tiles.max())
    else:
        assert c.n_ex in (4, 8) and per.min() >= 2
    coeff = bc.C[c.name]
    z = exch_host_launch(c, 0.0, c.n_ex, c.rule, c.twin, 1)
    bc.check_z(c, bc.exch_tables(c, z), int((c.x > 0).sum()), c.skipped)
    bc.check_exch_z(c, z)
    a = bc.check_exch_a(c, exch_host_launch(c, bc.LR_A, c.n_ex, c.rule, c.twin, 1))
    for lag in ((0, 1, c.n_ex) if c.twin and c.rule == "sqrt" else (1,)):  # (a correction that is an exact zero has no timing)
        b = bc.check_exch_b(c, exch_host_launch(c, bc.LR_B, c.n_ex, c.rule, c.twin, lag), coeff)
        print("%s, host model, lag %d: A %s; B error / tolerance: table U %.3g V %.3g B %.3g, published deltas V %.3g B %.3g, "
              "identities / floor %.3g, weights %.3g; %d rows apart from their base" % (
                  c.name, lag, {t: "%.3g" % v for t, v in a.items()}, b["U"], b["V"], b["B"], b["PV"], b["PB"], b["floor"], b["w_rel"], b["left"]))
        if c.hot.sum() >= 1000:
            assert b["left"] > 0, "hot rows stepped after their last publication: table - base is part of P"


def test_the_exch_cases_hold_hot_rows_and_a_skipped_draw(oracle):
    facts = {name: _exch_facts(name) for name in bc.EXCH_NAMES}
    print("\nresident-exchange cases, (popularity negatives, triplets with a hot positive, skipped draws): %s" % facts)
    assert max(h for pop, h, _ in facts.values() if not pop) >= 1000 and max(h for pop, h, _ in facts.values() if pop) >= 1000
    assert sum(s for _, _, s in facts.values()) >= 1


@pytest.mark.parametrize("name,fault", [(name, fault) for name in ("exch_k64", "exch_twin_sqrt_k64") for fault in EXCH_FAULTS
                                        if name == "exch_twin_sqrt_k64" or fault not in _TWIN_ONLY])
def test_checks_reject_a_wrong_exchange_protocol(oracle, name, fault):
    c = bc.case(name)
    rejected = []
    for lag in (0, 1, c.n_ex) if c.twin else (1,):
        try:
            bc.check_exch_b(c, exch_host_launch(c, bc.LR_B, c.n_ex, c.rule, c.twin, lag, fault=fault))
            rejected.append(None)
        except AssertionError as err:
            rejected.append(str(err).split(":")[0][:90])
    print("\n%s, %s: rejected by %s" % (c.name, fault, rejected))
    assert all(rejected), (fault, rejected)


@pytest.mark.parametrize("mutant", MUTANTS)
def test_checks_reject_a_wrong_update_in_an_exchange_launch(oracle, mutant):
    """the nine wrong updates on exch_k64: every triplet's (wrong) deltas from the start tables, as _strata_host_launch sums
    them, everything published by the last exchange"""
    c = bc.case("exch_k64")
    nt, k, n = c.total_items, c.k, len(c.trip[0])
    out = {}
    for launch, lr in (("A", bc.LR_A), ("B", bc.LR_B)):
        u, i, j = c.trip
        _, _, dU, dVi, dVj, dBi, dBj = step.deltas(c.trip, *c.tables, lr, bc.REG, c.use_bias, fault=mutant if mutant in step.FAULTS else None)
        w = np.ones(2 * n)
        if mutant.startswith("one_update"):
            row = int(np.flatnonzero(c.touches["V"] == 3)[0])
            t = int(c.triplets_of("V", row)[-1])
            w[t if i[t] == row else n + t] = 0.0 if mutant == "one_update_lost" else 2.0
        U, V, B = (np.array(t, np.float64) for t in c.tables)
        np.add.at(U, u, dU)
        np.add.at(V, i, dVi * w[:n, None])
        np.add.at(V, j, dVj * w[n:, None])
        np.add.at(B, i, dBi * w[:n])
        np.add.at(B, j, dBj * w[n:])
        if mutant == "row_written_to_the_wrong_item":
            a, b = i[np.flatnonzero(c.touches["V"][i] == 1)[:2]]
            V[[a, b]] = V[[b, a]]
        flat = np.concatenate([V.ravel(), B]).astype(np.float32)
        keeps, buckets = np.zeros((c.n_ex, len(flat)), np.float32), np.zeros((c.n_ex, len(flat) + 2 * nt), np.float32)
        keeps[-1] = (flat.astype(np.float64) - np.concatenate([c.tables[1].ravel(), c.tables[2]])).astype(np.float32)
        buckets[-1, :len(flat)] = keeps[-1]
        buckets[-1, len(flat):len(flat) + nt] = (keeps[-1, :nt * k].reshape(nt, k) != 0).any(axis=1)
        buckets[-1, len(flat) + nt:] = keeps[-1, nt * k:] != 0
        res = dict(U=U.astype(np.float32), flat=flat, base=flat.copy(), applied=np.zeros(nt, np.int64),
                   signals=np.r_[np.full(c.n_ex, c.plan["bins"]), np.ones(c.n_ex, np.int64), 0], red=bc.exch_reduce(c, keeps, buckets))
        out[launch] = _fails(bc.check_exch_a if launch == "A" else bc.check_exch_b, c, res)
    print("\nexch_k64, %s: rejected by %s" % (mutant, " and ".join(key for key, v in out.items() if v) or "NOTHING"))
    assert out["A"] or out["B"], mutant
