"""The arithmetic of the hogwild MF kernels against the float64 step, rating by rating: every kernel instantiation the
dispatchers return runs one launch three times (tests/mf_step_cases.py: Z at lr = 0, A at lr = 0.01 on the rows of clean
ratings, B at a small lr on every touched row), and the ratings of that launch — with the copies the split rows' ratings
name — are known beforehand from the inputs.  tests/test_mf_step_cpu.py proves the cases fair and the checks sharp."""
import warnings

import numpy as np
import pytest

import mf_step_cases as mc
from cornac_amd import _lib
from oracle import mf_step_oracle as step

pytestmark = pytest.mark.gpu


def _launch(tr, c, lr, set_tables=True):
    """one launch of the case from its start tables: (tables, sum of squared errors)"""
    if set_tables:
        tr.set_factors(*c.tables)
    tr.epoch_enqueue(c.part, c.n_parts, lr, mc.REG, mc.MU, c.use_bias)
    sse = tr.sync()
    return tr.get_factors(), sse


@pytest.mark.parametrize("name", mc.NAMES)
def test_hogwild_launch_matches_the_float64_step(oracle, name):
    cus = _lib.device_info(0)["compute_units"]
    c = mc.case(name)
    if c.owned and c.nnz < cus * 8 * 4 * 64:
        pytest.skip("%s: the owned kernel needs %d ratings on this device (%d CUs), the case has %d" % (name, cus * 8 * 4 * 64, cus, c.nnz))
    tr = _lib.MfTrainer(c.rid, c.cid, c.val, c.nu, c.ni, c.k)
    try:
        if c.form:
            tr.hogwild_form(c.form)
        got, sse = _launch(tr, c, 0.0)
        # what the handle decided against the restatements, before the case is trusted
        st = tr.hogwild_stats()
        if c.form == 2:
            assert st["form_used"] == (1 if st["gave_up"] else 2), st
            if st["gave_up"]:
                warnings.warn("MF block rotation gave up on this box (workgroup placement): %r — the fused kernel ran" % (st,))
        else:
            assert st["form_used"] == 1, st
        items, ptr = tr.debug_split()
        assert np.array_equal(items, c.split[0]) and np.array_equal(ptr, c.split[1]), "%s: the device's split differs from its restatement: %r %r, %r" % (
            name, items, ptr, c.split)
        own = tr.debug_ownership()
        extra = ""
        if c.owned or (c.form == 2 and st["gave_up"] and c.nnz >= cus * 8 * 4 * 64):
            assert own is not None, "%s: expected the owned kernel" % name
            mine = step.ownership(c.rid, c.cid_ext, c.nu, len(own[0]) - 1)
            for a, b, what in zip(mine, own, ("wave_ptr", "own_u", "own_i")):
                assert np.array_equal(a, b), "%s: the ownership table %s differs from its restatement" % (name, what)
            unr = 4 if c.k <= 64 else 2 if c.k <= 192 else 1
            extra = "; %d waves, %d batches of %d name one exclusive user twice" % (len(own[0]) - 1, step.same_user_batches(own, unr), unr)
        else:
            assert own is None, "%s: expected an unowned launch" % name
        z = mc.check_z(c, got, sse)
        a = mc.check_a(c, _launch(tr, c, mc.LR_A)[0])
        got_b = _launch(tr, c, c.lr_b)[0]
        b = mc.check_b(c, got_b)
        if c.n_virtual:
            # every copy ended launch B equal to its merged row: a launch at lr = 0 on top of B's tables moves nothing
            again, _ = _launch(tr, c, 0.0, set_tables=False)
            for tab, x, y in zip(mc.TABLES, got_b, again):
                assert np.array_equal(x, y), "%s: lr = 0 after launch B changed table %s" % (name, tab)
    finally:
        tr.close()
    print("\n%s: %d ratings, form %d%s; Z sse off by %.3g (bound %.3g); A clean-row error %s (T_CLEAN %.3g); B error / tolerance %s "
          "(LR_B 2^%d, C %.3g)" % (name, len(c.rat[0]), st["form_used"], extra, z["sse_err"], z["sse_bound"],
                                  " ".join("%s %.3g" % kv for kv in a.items()), mc.T_CLEAN,
                                  " ".join("%s %.3g" % kv for kv in b.items()), np.log2(c.lr_b), mc.C[name]))
