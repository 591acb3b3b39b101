"""The deterministic MF dataflow launch (csrc/mf.hip, mf_det_chain_kernel<R, OWN_USER> on the driver of csrc/chain.h)
against the sequential loop, at its smallest shapes: every register slice R = 1..4, both owned sides, all three stored
orders, the size and factor-count thresholds, biases off, epochs chained across calls.

Acceptance (tests/mf_chain_cases.py): U, V, Bu and Bi equal oracle_mf_fit BIT FOR BIT — one expression tree, contraction
off on both sides, every row updated in stored order — and loss_per_epoch to rtol 2e-4.  Which form ran, and which side
the waves owned, is asserted with MfTrainer.det_form everywhere: a refused cooperative launch must not turn these into
level-schedule tests unnoticed.
"""
import numpy as np
import pytest

import mf_chain_cases as mc
from cornac_amd import _lib

pytestmark = pytest.mark.gpu


def trainer_for(c):
    tr = _lib.MfTrainer(c["uid"], c["iid"], c["stars"], c["nu"], c["ni"], c["k"])
    tr.set_factors(c["U"], c["V"], np.zeros(c["nu"], np.float32), np.zeros(c["ni"], np.float32))
    return tr


def fit(tr, c, epochs=mc.EPOCHS, use_bias=True):
    loss, ran = tr.fit(epochs, mc.LR, mc.REG, c["mu"], use_bias, False, _lib.MODE_DETERMINISTIC)
    assert ran == epochs
    return loss


def compare(what, got, want, c):
    """got / want: (U, V, Bu, Bi, loss)"""
    names = ("U", "V", "Bu", "Bi")
    rel = float(np.max(np.abs(got[4] - want[4]) / np.abs(want[4])))
    print("%s: %s, loss rel err %.3g" % (what, ", ".join("max |d%s| %.3g" % (n, mc.max_abs_diff(g, w))
                                                         for n, g, w in zip(names, got, want)), rel))
    assert all(np.isfinite(a).all() for a in got), what
    assert np.abs(want[0] - c["U"]).max() > 1e-3 and np.abs(got[0] - c["U"]).max() > 1e-3, what + ": the run did not move the factors"
    for n, g, w in zip(names, got, want):
        assert mc.bits_equal(g, w), "%s: %s differs, max |diff| %g" % (what, n, mc.max_abs_diff(g, w))
    assert rel <= mc.LOSS_RTOL, "%s: loss %r against %r" % (what, got[4], want[4])


def check(kind, k, form, use_bias=True, own_user=None):
    c = mc.case(kind, k)
    want = mc.reference(kind, k, use_bias)
    tr = trainer_for(c)
    try:
        assert tr.det_form() == (mc.FORM_NONE, 0)
        loss = fit(tr, c, use_bias=use_bias)
        got = tr.get_factors() + (loss,)
        got_form, got_own = tr.det_form()
    finally:
        tr.close()
    what = "%s k=%d%s" % (kind, k, "" if use_bias else " no bias")
    print("%s: form %d, users owned %d" % (what, got_form, got_own))
    assert got_form == form, what
    if form == mc.FORM_CHAIN:
        assert got_own == int(mc.owns_users(c["uid"], c["iid"])), what
        if own_user is not None:
            assert got_own == own_user, what
    compare(what, got, want, c)
    return got


@pytest.mark.parametrize("k", mc.K_CHAIN)
def test_factor_counts_on_the_dataflow_launch(k):
    check("edge", k, mc.FORM_CHAIN)


def test_k_257_takes_the_level_schedule():
    check("edge", mc.K_LEVELS, mc.FORM_LEVELS)


def test_no_bias_leaves_the_biases_zero():
    U, V, Bu, Bi, _ = check("edge", 10, mc.FORM_CHAIN, use_bias=False)
    assert not Bu.any() and not Bi.any()


@pytest.mark.parametrize("nnz,form", [(4095, mc.FORM_LEVELS), (4096, mc.FORM_CHAIN)])
def test_size_threshold(nnz, form):
    check("nnz%d" % nnz, 5, form)


@pytest.mark.parametrize("k", mc.ORDER_K)
@pytest.mark.parametrize("order", mc.ORDERS)
def test_stored_orders(order, k):
    """sorted by user (users owned), by item (items owned), shuffled; a 1 000-rating item, a single-rating user, repeated
    (u, i) pairs — one register slice (k = 10) and three (k = 130)"""
    check("order_" + order, k, mc.FORM_CHAIN, own_user=mc.OWN_USER.get(order))


def test_epochs_chain_across_calls():
    c = mc.case("edge", 10)
    want = mc.reference("edge", 10, True)
    one, two = trainer_for(c), trainer_for(c)
    try:
        l2 = fit(two, c, 2)
        l1a, l1b = fit(one, c, 1), fit(one, c, 1)
        got2, got11 = two.get_factors(), one.get_factors()
        assert one.det_form()[0] == two.det_form()[0] == mc.FORM_CHAIN
    finally:
        one.close()
        two.close()
    for n, a, b in zip(("U", "V", "Bu", "Bi"), got11, got2):
        assert mc.bits_equal(a, b), "1 + 1 epochs in two calls differ from 2 in one: " + n
    compare("edge k=10, 1 + 1 epochs", got11 + (np.concatenate([l1a, l1b]),), want, c)
    compare("edge k=10, 2 epochs", got2 + (l2,), want, c)
