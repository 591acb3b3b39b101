"""The arithmetic of the hogwild VEBPR kernel against the float64 step, quadruple by quadruple: every instantiation of
vebpr_hogwild_kernel that the dispatcher launches runs one epoch three times (tests/vebpr_step_cases.py: Z at lr = 0, A at
lr = 0.05 on the rows of clean quadruples, B at lr = 2^-12 on every touched row), and the quadruples of that epoch are
known beforehand from the CPU restatement of the sampler.  tests/test_vebpr_step_cpu.py proves the cases fair and the
checks sharp."""
import numpy as np
import pytest

import vebpr_step_cases as vc
from cornac_amd import _lib

pytestmark = pytest.mark.gpu


def _trainer(c, k=None):
    tr = _lib.BprTrainer(c.indptr, c.indices, c.nu, c.ni, c.nu, c.total_items, k or c.k)
    tr.set_views(c.v_indptr, c.v_indices)
    return tr


def _launch(tr, c, lr):
    """one epoch of the case from its start tables: ((U, V), correct, skipped)"""
    tr.set_factors(c.tables[0], c.tables[1], None)
    tr.seed_hogwild(c.seed)  # (resets the epoch counter: every launch is epoch 0)
    correct, skipped = tr.fit_epochs_vebpr(1, lr, vc.REG if lr else 0.0, vc.ALPHA, _lib.MODE_HOGWILD, ownership=c.ownership)
    return tr.get_factors()[:2], correct, skipped


@pytest.mark.parametrize("name", vc.NAMES)
def test_hogwild_epoch_matches_the_float64_step(oracle, name):
    cus = _lib.device_info(0)["compute_units"]
    if vc.SPECS[name]["form"] == "owned" and not vc.ownership_applies(vc.LARGE_NNZ, cus):
        pytest.skip("too few interactions per wave for user-row ownership on this device: %d < %d CUs x 6 x 4 x 64" % (vc.LARGE_NNZ, cus))
    c = vc.case(name, cus)
    tr = _trainer(c)
    try:
        got, correct, skipped = _launch(tr, c, 0.0)
        assert tr.vebpr_hogwild_owned() == c.owned_on_device, "%s: expected the %s kernel" % (name, c.form)
        if c.form == "owned":
            # the ownership tables exist after the first launch
            own = tr.debug_ownership()
            assert own is not None, "%s: no ownership tables" % name
            waves = len(own[0]) - 1
            if waves != len(c.own_tables[0]) - 1:  # another grid than the case assumed: other quadruples
                c = vc.case(name, cus, waves)  # (C[name] was measured for the other launch)
            for mine, dev in zip(c.own_tables, own):
                assert np.array_equal(mine, dev), "%s: the ownership tables differ from their restatement" % name
            print("\n%s: %d waves, vebpr_hogwild_owned() == %s, ownership tables equal to their restatement" % (
                name, waves, tr.vebpr_hogwild_owned()))
        z = vc.check_z(c, got, correct, skipped)
        a = {"U": float("nan"), "V": float("nan")} if c.no_a else vc.check_a(c, _launch(tr, c, vc.LR_A)[0])
        b = vc.check_b(c, _launch(tr, c, vc.LR_B)[0])
        assert tr.vebpr_hogwild_owned() == c.owned_on_device
    finally:
        tr.close()
    print("\n%s: %d quadruples, %d skipped, correct %d in [%d, %d]; A clean-row error U %.3g V %.3g (T_CLEAN %.3g); "
          "B error / tolerance U %.3g V %.3g (C %.3g)" % (
              name, len(c.quad[0]), c.skipped, z["correct"], z["lo"], z["hi"], a["U"], a["V"], vc.T_CLEAN, b["U"], b["V"], vc.C[name]))


def test_k_257_is_refused_and_leaves_the_tables_alone(oracle):
    c = vc.case("unowned_k3")
    k = 257
    rs = np.random.RandomState(257)
    U, V = rs.normal(0, 0.2, (c.nu, k)).astype(np.float32), rs.normal(0, 0.2, (c.total_items, k)).astype(np.float32)
    tr = _trainer(c, k)
    try:
        tr.set_factors(U, V, None)
        tr.seed_hogwild(1)
        with pytest.raises(_lib.HipError):
            tr.fit_epochs_vebpr(1, vc.LR_A, vc.REG, vc.ALPHA, _lib.MODE_HOGWILD)
        got = tr.get_factors()
        assert np.array_equal(got[0], U) and np.array_equal(got[1], V)
    finally:
        tr.close()
