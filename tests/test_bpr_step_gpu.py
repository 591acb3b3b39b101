"""The arithmetic of the hogwild BPR kernels against the float64 step, triplet by triplet: every kernel instantiation the
dispatchers return runs one short launch three times (tests/bpr_step_cases.py: Z at lr = 0, A at lr = 0.05 on the rows of
clean triplets, B at lr = 2^-12 on every touched row), and the triplets of that launch are known beforehand from the CPU
restatements of the samplers.  tests/test_bpr_step_cpu.py proves the cases fair and the checks sharp."""
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


@pytest.mark.parametrize("name", bc.NAMES)
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
