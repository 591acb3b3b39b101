"""The arithmetic of the hogwild BPR kernels against the float64 step, triplet by triplet: every kernel instantiation the
dispatchers return runs one short launch three times (tests/bpr_step_cases.py: Z at lr = 0, A at lr = 0.05 on the rows of
clean triplets, B at lr = 2^-12 on every touched row), and the triplets of that launch are known beforehand from the CPU
restatements of the samplers.  tests/test_bpr_step_cpu.py proves the cases fair and the checks sharp.  The conveyor's
launches (cornac_hip_bpr_conveyor_enqueue: the rows in block buffers) run under the same three rules in a test of their own,
and so do the XCD-strata form's phases, whose launch B holds the cold item rows that two waves touch under a rule of their own,
and the resident exchange's whole epochs, whose launch B also holds what the launch publishes for the other ranks."""
import numpy as np
import pytest

import bpr_step_cases as bc
from cornac_amd import _lib

pytestmark = pytest.mark.gpu


def _launch(tr, c, lr):
    """one launch of the case from its start tables: (tables, correct, skipped)"""
    tr.set_factors(*c.tables)
    tr.seed_hogwild(c.seed)
    args = (c.use_bias, c.neg_population, c.flags)
    if c.s_begin:  # move the sample counter to s_begin without touching anything (launch Z shows that lr = 0 does not)
        tr.hogwild_enqueue(c.s_begin, 0.0, 0.0, *args)
        tr.sync()
    tr.hogwild_enqueue(c.n, lr, bc.REG if lr else 0.0, *args)
    correct, skipped = tr.sync()
    return tr.get_factors(), correct, skipped


@pytest.mark.parametrize("name", [name for name in bc.NAMES if name not in bc.CONVEYOR_NAMES + bc.STRATA_NAMES + bc.EXCH_NAMES])
def test_hogwild_launch_matches_the_float64_step(oracle, name):
    cus = _lib.device_info(0)["compute_units"]
    c = bc.case(name, cus)
    tr = _lib.BprTrainer(c.indptr, c.indices, c.nu, c.ni, c.nu, c.total_items, c.k)
    try:
        if c.form == "ldsbin":
            tr.ldsbin_config(min_candidates=c.min_candidates, max_rounds=c.max_rounds)
            st = tr.ldsbin_stats()
            assert (st["bins"], st["rows_per_bin"], st["block_threads"]) == (
                c.plan["bins"], c.plan["cap"], 512 if c.plan["passing"] else 1024), (st, c.plan)
        if c.form == "owned":
            # the ownership tables exist after the first launch: one sample at lr = 0 builds them
            tr.seed_hogwild(c.seed)
            tr.hogwild_enqueue(1, 0.0, 0.0, c.use_bias, c.neg_population, c.flags)
            tr.sync()
            own = tr.debug_ownership()
            assert own is not None, "%s: expected the owned kernel" % name
            waves = len(own[0]) - 1
            if waves != len(c.ownership[0]) - 1:  # another persistent grid than the case assumed: other triplets
                c = bc.case(name, cus, waves)  # (C[name] was measured for the other launch)
            for mine, dev in zip(c.ownership, own):
                assert np.array_equal(mine, dev), "%s: the ownership tables differ from their restatement" % name
            print("\n%s: %d waves, launch of %d samples" % (name, waves, c.n))
        got, correct, skipped = _launch(tr, c, 0.0)
        if c.form == "fused":
            assert tr.debug_ownership() is None, "%s: expected the unowned kernel" % name
        z = bc.check_z(c, got, correct, skipped)
        a = bc.check_a(c, _launch(tr, c, bc.LR_A)[0])
        b = bc.check_b(c, _launch(tr, c, bc.LR_B)[0])
        if c.form == "ldsbin":
            assert tr.ldsbin_stats()["lock_timeouts"] == 0
    finally:
        tr.close()
    print("\n%s: %d triplets, correct %d in [%d, %d]; A clean-row error U %.3g V %.3g B %.3g (T_CLEAN %.3g); "
          "B error / tolerance U %.3g V %.3g B %.3g (C %.3g)" % (
              name, len(c.trip[0]), z["correct"], z["lo"], z["hi"], a["U"], a["V"], a["B"], bc.T_CLEAN, b["U"], b["V"], b["B"],
              bc.C[name]))


def _strata_launch(tr, c, lr, packed):
    """the launch of a strata case from its start tables: (tables, correct, skipped).  One hogwild_enqueue per phase, no
    sync in between: with packed records (chunk_records) the second phase starts from the records the first left."""
    tr.chunk_records(packed)
    tr.set_factors(*c.tables)
    tr.seed_hogwild(c.seed)
    args = (c.use_bias, c.neg_population, c.flags)
    if c.epoch or c.s_begin:  # the earlier phases at lr = 0 move the sample counter and touch nothing (launch Z shows that)
        tr.hogwild_enqueue(c.epoch * c.nnz + c.s_begin, 0.0, 0.0, *args)
        tr.sync()
    for n in c.launch_ns:
        tr.hogwild_enqueue(n, lr, bc.REG if lr else 0.0, *args)
    correct, skipped = tr.sync()
    return tr.get_factors(), correct, skipped


@pytest.mark.parametrize("name", bc.STRATA_NAMES)
def test_strata_launch_matches_the_float64_step(oracle, name):
    """The XCD-strata form (csrc/bpr_strata.inc) phase by phase.  Before anything is launched the device's hot set, epoch
    key and bucket tables are held against their restatements; then launches Z, A and B, B under two rules
    (bpr_step_cases.check_b_strata: cold item rows that two waves of a phase touch may lose a store, everything else is
    exact)."""
    cus = _lib.device_info(0)["compute_units"]
    c = bc.case(name, cus)
    tr = _lib.BprTrainer(c.indptr, c.indices, c.nu, c.ni, c.nu, c.total_items, c.k)
    try:
        tr.strata_config(*c.hot_cfg)
        tr.seed_hogwild(c.seed)
        if c.flags == 0:  # automatic dispatch: one sample at lr = 0 under flags = 0 must have built buckets for the strata kernel
            assert tr.ldsbin_stats()["bins"] == 0, "%s: an LDS-bin plan exists" % name
            tr.hogwild_enqueue(1, 0.0, 0.0, c.use_bias, c.neg_population, 0)
            tr.sync()
            st = tr.strata_stats()
            assert st["waves"] > 0 and st["bucket_builds"] == 1, "%s: flags = 0 did not take the strata form: %r" % (name, st)
            tr.seed_hogwild(c.seed)
        sptr, rec_u, rec_i, rank_item, key = tr.debug_strata(c.epoch)
        own = tr.debug_ownership()
        assert own is not None, "%s: expected user-row ownership" % name
        waves = len(own[0]) - 1
        if waves != c.waves:  # another persistent grid than the case assumed: other triplets
            c = bc.case(name, cus, waves)  # (C[name] was measured for the other launch)
        for mine, dev in zip(c.ownership, own):
            assert np.array_equal(mine, dev), "%s: the ownership tables differ from their restatement" % name
        st = tr.strata_stats()
        assert st["n_hot"] == c.strata["n_hot"], "%s: n_hot %d, restatement %d" % (name, st["n_hot"], c.strata["n_hot"])
        assert key == c.strata["key"], "%s: the epoch key differs from its restatement" % name
        for what, mine, dev in zip(("sptr", "rec_u", "rec_i", "rank_item"), c.strata["buckets"], (sptr, rec_u, rec_i, rank_item)):
            assert np.array_equal(mine, dev), "%s: %s differs from its restatement" % (name, what)
        builds = st["bucket_builds"]
        got, correct, skipped = _strata_launch(tr, c, 0.0, c.packed)
        z = bc.check_z(c, got, correct, skipped)
        a = bc.check_a(c, _strata_launch(tr, c, bc.LR_A, c.packed)[0])
        b = bc.check_b_strata(c, _strata_launch(tr, c, bc.LR_B, c.packed)[0])
        unpacked = bc.check_b_strata(c, _strata_launch(tr, c, bc.LR_B, False)[0]) if c.packed else None
        st = tr.strata_stats()
        assert st["waves"] == waves and tr.debug_ownership()[0].shape == own[0].shape
        if c.hot_cfg[2] > 1:  # epochs 0 and 1 share a key: the buckets built for the comparison above served every launch
            assert st["bucket_builds"] == builds, (st, builds)
    finally:
        tr.close()
    print("\n%s: %d waves, %d triplets, correct %d in [%d, %d]; A clean-row error U %.3g V %.3g B %.3g (T_CLEAN %.3g); "
          "B error / tolerance, exact rule U %.3g V %.3g B %.3g (C %.3g); racy rows %d, explained whole %d, lost a group %d%s; "
          "misplaced workgroups %d" % (
              name, waves, len(c.trip[0]), z["correct"], z["lo"], z["hi"], a["U"], a["V"], a["B"], bc.T_CLEAN, b["U"], b["V"], b["B"],
              bc.C[name], b["racy"], b["whole"], b["lost"],
              "" if unpacked is None else " (unpacked: V %.3g B %.3g, whole %d, lost %d)" % (
                  unpacked["V"], unpacked["B"], unpacked["whole"], unpacked["lost"]), st["misplaced_workgroups"]))


def test_strata_config_refuses_what_it_cannot_run():
    rs = np.random.RandomState(0)
    indptr = np.arange(0, 4 * 1000 + 1, 4, dtype=np.int32)
    indices = np.sort(rs.randint(0, 8192, (1000, 4)), axis=1).astype(np.int32)
    indices += np.arange(4, dtype=np.int32)  # (strictly ascending within a user)
    tr = _lib.BprTrainer(indptr, indices.ravel(), 1000, 8196, 1000, 8196, 64)
    try:
        for bad, what in (((-1, 200, 1), "hot_permille"), ((1001, 200, 1), "hot_permille"), ((120, -1, 1), "hot_min_mult_x100"),
                          ((120, 200, 0), "rehash_period")):
            with pytest.raises(_lib.HipError, match=what):
                tr.strata_config(*bad)
        tr.strata_config(0, 0, 1)
        tr.strata_config(1000, 200, 3)
    finally:
        tr.close()


def _conveyor_launch(tr, c, lr):
    """one conveyor launch of the case from its start tables and start buffers: ((U, V, B), correct, skipped).  The buffers
    of ALL blocks are on the device; the launch is given those of c.blocks, in that order."""
    import torch

    tr.set_factors(c.tables[0], None, None)
    tr.seed_hogwild(c.seed)
    bufs = [torch.as_tensor(b.copy()).to("cuda:0") for b in c.bufs]
    torch.cuda.synchronize()
    tr.conveyor_enqueue(c.epoch, c.layout_epoch, list(c.blocks), [bufs[b].data_ptr() for b in c.blocks], lr, bc.REG if lr else 0.0,
                        c.use_bias, c.neg_population, c.flags)
    correct, skipped = tr.sync()
    launch = "Z" if lr == 0.0 else "A" if lr == bc.LR_A else "B"
    return bc.conveyor_tables(c, launch, [b.cpu().numpy() for b in bufs], tr.get_user_factors()), correct, skipped


@pytest.mark.parametrize("name", bc.CONVEYOR_NAMES)
def test_conveyor_launch_matches_the_float64_step(oracle, name):
    import torch

    cus = _lib.device_info(0)["compute_units"]
    c = bc.case(name, cus)
    tr = _lib.BprTrainer(c.indptr, c.indices, c.nu, c.ni, c.nu, c.ni, c.k)
    try:
        got = tr.conveyor_setup(c.n_blocks, c.rank_item, c.deal_seed)
        assert got == (c.plan["bins"], c.plan["bpb"], c.plan["cap"]), (got, c.plan)
        # the device's layout of (deal_seed, layout_epoch) against the oracle's, from which the buffers are filled
        slot_item = torch.full((len(c.slot_item),), -2, dtype=torch.int32, device="cuda:0")
        item_slot = torch.full((c.ni,), -2, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        tr.conveyor_layout(c.layout_epoch, slot_item.data_ptr(), item_slot.data_ptr())
        tr.sync()
        assert np.array_equal(slot_item.cpu().numpy(), c.slot_item), "%s: slot_item differs from its restatement" % name
        assert np.array_equal(item_slot.cpu().numpy(), c.item_slot), "%s: item_slot differs from its restatement" % name
        tables, correct, skipped = _conveyor_launch(tr, c, 0.0)
        z = bc.check_z(c, tables, correct, skipped)
        a = bc.check_a(c, _conveyor_launch(tr, c, bc.LR_A)[0])
        b = bc.check_b(c, _conveyor_launch(tr, c, bc.LR_B)[0])
        assert tr.ldsbin_stats()["lock_timeouts"] == 0
    finally:
        tr.close()
    print("\n%s: %d bins, %d per block, %d rows per bin, blocks %s; %d triplets (%d skipped), correct %d in [%d, %d]; A clean-row "
          "error U %.3g V %.3g B %.3g (T_CLEAN %.3g); B error / tolerance U %.3g V %.3g B %.3g (C %.3g)" % (
              name, got[0], got[1], got[2], list(c.blocks), len(c.trip[0]), c.skipped, z["correct"], z["lo"], z["hi"], a["U"], a["V"],
              a["B"], bc.T_CLEAN, b["U"], b["V"], b["B"], bc.C[name]))


def _exchange_launch(sh, tr, c, lr):
    """one resident-exchange epoch of the case from its start tables, through the production driver: `res` as
    bpr_step_cases.check_exch_* take it (table and base read BEFORE finish(), whose closing exchange makes base = table on a
    rank without a process group), with the launch's counters"""
    import torch

    tr.set_factors(c.tables[0], None, None)
    tr.seed_hogwild(c.seed)
    sh.load_items(c.tables[1], c.tables[2])  # (base = table)
    if sh._resident is not None:  # what the launch before left in the buffers says nothing about this one
        with sh._on_stream():
            for key in ("buckets", "keeps", "applied"):
                sh._resident[key].zero_()
        sh.stream.synchronize()
    sh.run_epoch(c.nnz, c.n_ex, lr, bc.REG if lr else 0.0, c.use_bias, c.neg_population, c.flags, resident=True)
    sh.stream.synchronize()
    st = sh._resident
    st["comm"].synchronize()
    res = dict(flat=sh.table.flat.cpu().numpy(), base=sh.table.base.cpu().numpy(), signals=st["signals"].cpu().numpy(),
               applied=st["applied"].cpu().numpy(), red=bc.exch_reduce(c, st["keeps"], st["buckets"]))
    torch.cuda.synchronize()
    res["correct"], res["skipped"] = sh.finish()
    res["U"] = tr.get_user_factors()
    assert np.array_equal(sh.table.flat.cpu().numpy(), res["flat"]) and np.array_equal(sh.table.base.cpu().numpy(), res["flat"]), (
        "%s: one rank's closing exchange is the identity and leaves base = table" % c.name)
    return res


@pytest.mark.parametrize("name", bc.EXCH_NAMES)
def test_resident_exchange_epoch_matches_the_float64_step(oracle, name):
    """The resident exchange (csrc/bpr_ldsbin.inc, EXCH instantiations) through cornac_amd.dist.ShardedBprTrainer on ONE rank
    without a process group: a whole epoch per launch, Z, A and B, and in launch B what the launch publishes (keeps, buckets,
    base) beside the table — bpr_step_cases.check_exch_b.  A twin case plays a second rank with the same deltas on the
    communication stream."""
    import torch

    from cornac_amd.dist import ShardedBprTrainer

    cus = _lib.device_info(0)["compute_units"]
    c = bc.case(name, cus)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    tr = _lib.BprTrainer(c.indptr, c.indices, c.nu, c.ni, c.nu, c.total_items, c.k)
    try:
        tr.ldsbin_config(min_candidates=c.min_candidates, max_rounds=c.max_rounds)
        tr.seed_hogwild(c.seed)
        st = tr.ldsbin_stats()
        assert (st["bins"], st["rows_per_bin"], st["block_threads"]) == (c.plan["bins"], c.plan["cap"], 1024), (st, c.plan)
        sh = ShardedBprTrainer(tr, c.total_items, c.k, dev, sync_every=c.nnz, rule=c.rule)
        sh.load_items(c.tables[1], c.tables[2])
        assert sh.resident_bins(c.neg_population, c.flags) == c.plan["bins"]
        if c.twin:
            sh.resident_bucket_hook = lambda e, b: b.mul_(2.0)
        rz = _exchange_launch(sh, tr, c, 0.0)
        assert tr.ldsbin_stats()["n_hot"] == c.n_hot, "%s: n_hot %d, restatement %d" % (name, tr.ldsbin_stats()["n_hot"], c.n_hot)
        z = bc.check_z(c, bc.exch_tables(c, rz), rz["correct"], rz["skipped"])
        bc.check_exch_z(c, rz)
        a = bc.check_exch_a(c, _exchange_launch(sh, tr, c, bc.LR_A))
        rb = _exchange_launch(sh, tr, c, bc.LR_B)
        lock_timeouts = tr.ldsbin_stats()["lock_timeouts"]
        assert sh.table.exchanges.get("resident") == 3 * c.n_ex, sh.table.exchanges
    finally:
        tr.close()
    acc = c.twin and c.rule == "sqrt"
    apart_v, apart_b = bc._exch_vb(c, rb["flat"] != rb["base"])
    print("\n%s: %d bins x %d rows, n_ex %d, rule %s%s; %d triplets (%d skipped), correct %d in [%d, %d]; A clean-row error U %.3g V %.3g "
          "B %.3g (T_CLEAN %.3g); B: applied in the launch %d..%d of %d, %d rows apart from their base (n_hot %d), largest |sum c| %.3g" % (
              name, c.plan["bins"], c.plan["cap"], c.n_ex, c.rule, ", twin" if c.twin else "", len(c.trip[0]), c.skipped, z["correct"],
              z["lo"], z["hi"], a["U"], a["V"], a["B"], bc.T_CLEAN, rb["applied"][:c.ni].min(), rb["applied"][:c.ni].max(), c.n_ex,
              int((apart_v.any(axis=1) | apart_b).sum()), c.n_hot, np.abs(rb["red"]["csum"]).max()))
    b = bc.check_exch_b(c, rb, lock_timeouts=lock_timeouts)
    print("%s: B error / tolerance: table rule U %.3g%s, published-delta rule V %.3g B %.3g (C %.3g); %s / floor %.3g; "
          "weights / tolerance %.3g" % (
              name, b["U"], "" if acc else " V %.3g B %.3g" % (b["V"], b["B"]), b["PV"], b["PB"], bc.C[name],
              "twin accounting residual" if acc else "base - start - sum of keeps", b["floor"], b["w_rel"]))


def test_conveyor_setup_refuses_k_above_256():
    rs = np.random.RandomState(0)
    indptr = np.arange(0, 4 * 1000 + 1, 4, dtype=np.int32)
    indices = np.sort(rs.randint(0, 8192, (1000, 4)), axis=1).astype(np.int32)
    indices += np.arange(4, dtype=np.int32)  # (strictly ascending within a user)
    tr = _lib.BprTrainer(indptr, indices.ravel(), 1000, 8196, 1000, 8196, 257)
    try:
        with pytest.raises(_lib.HipError, match="no conveyor layout"):
            tr.conveyor_setup(4, None, 1)
    finally:
        tr.close()
