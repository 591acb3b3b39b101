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
    else:  # one 64-sample tile of every wave's slice
        assert draws == np.minimum(np.diff(c.ownership[0]), 64).sum()
    for start in c.tables:
        assert start.dtype == np.float32
    # real scores: z well away from 0.5 on both sides
    z = c.z
    z05, z95 = np.quantile(z, [0.05, 0.95])
    assert z05 <= 0.25 and z95 >= 0.75, (z05, z95)
    ambiguous = int((np.abs(c.x) < c.x_bound).sum())
    assert ambiguous <= max(2, n_trip // 10_000), "the float32 score bound decides nearly every sign: %d of %d ambiguous" % (ambiguous, n_trip)
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
    cm = _c_measured(c)
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
        assert min(vis.values()) >= 0.5, vis
    if c.form == "owned":
        tu = c.touches["U"]
        assert tu[tu > 0].mean() < 4 and tv[tv > 0].mean() < 4, "few touches per row"
        assert c.shared.any() and not c.shared.all(), "exclusive users (plain stores) and shared ones (atomics) both occur"
        assert vis["U"] >= 0.5, vis


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
