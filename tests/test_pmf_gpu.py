"""PMF on the device against the restatement of the reference's loops (tests/pmf_cases.pmf_fit, itself held bit for bit
against the reference's compiled loop by tests/test_pmf_cpu.py), through the C ABI and through cornac_amd.PMF.

Acceptance: U and V equal the restatement BIT FOR BIT under both variants — every operation is a correctly rounded IEEE
double + - * / sqrt in a pinned order with contraction off, and the sigmoid's expf is evaluated operation for operation
as the host's libm evaluates it (csrc/pmf.inc, pmf_expf) — so a mismatch is a bug in the expression tree or in the
hand-over, not noise.  loss_per_epoch: relative error <= 1e-12 (a sum of at most 5 000 non-negative per-rating terms in
another order: n 2^-53 ~ 6e-13).

The base case (48 users x 32 items x 256 ratings, k = 5, 3 epochs) is below the dataflow kernel's size threshold and runs
the level schedule; every factor count is therefore checked there AND on 64 users x 48 items x 4 096 ratings, the
smallest shape that takes the dataflow launch (where the lane-group sizes 8 / 16 / 32, the switch to one rating per wave
at 32 | 33 and the register slices R = 1..4 live).  Which form ran is asserted with pmf_form everywhere.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pmf_cases as pc
from cornac_amd import PMF, Dataset, _lib

pytestmark = pytest.mark.gpu

K_EDGES = (1, 5, 8, 9, 16, 17, 32, 33, 64, 65, 130, 256)
FORM_CHAIN, FORM_LEVELS = 1, 2


def ratings_per_pass(k):
    """of the dataflow kernel: lane groups of pow2 >= k lanes up to 32, else the whole wave"""
    return 8 if k <= 8 else 4 if k <= 16 else 2 if k <= 32 else 1


@functools.lru_cache(maxsize=None)
def case(kind, k=5):
    if kind == "base":
        return pc.base_case(k)
    if kind == "chain":
        return pc.random_case(64, 48, 4096, k, epochs=2, seed=5)
    if kind.startswith("nnz"):
        return pc.threshold_case(int(kind[3:]))
    if kind.startswith("order_"):
        return pc.order_case(kind[6:], k)
    assert kind == "saturation"
    return pc.saturation_case()


@functools.lru_cache(maxsize=None)
def reference(kind, k, variant):
    c = case(kind, k)
    U, V, loss, _ = pc.run_reference(c, variant, rat=c["rat01"] if kind == "saturation" else None)
    for a in (U, V, loss):
        a.setflags(write=False)
    return U, V, loss


def trainer_for(c, rat):
    return _lib.MfTrainer(c["uid"], c["iid"], rat, c["nu"], c["ni"], c["k"])


def fit(tr, c, variant, epochs=None):
    return tr.pmf_fit(c["epochs"] if epochs is None else epochs, c["learning_rate"], c["lambda_reg"], c["gamma"], variant)


def check(kind, k, variant, form):
    c = case(kind, k)
    rat = c["rat01"] if kind == "saturation" else pc.ratings_for(variant, c["stars"])
    want_U, want_V, want_loss = reference(kind, k, variant)
    tr = trainer_for(c, rat)
    try:
        assert tr.pmf_form() == (0, 0)
        tr.pmf_set_factors(c["U"], c["V"])
        loss = fit(tr, c, variant)
        U, V = tr.pmf_get_factors()
        got_form, group = tr.pmf_form()
    finally:
        tr.close()
    what = "%s k=%d %s" % (kind, k, variant)
    rel = float(np.max(np.abs(loss - want_loss) / want_loss))
    print("%s: form %d group %d, max |dU| %.3g, max |dV| %.3g, loss rel err %.3g" % (
        what, got_form, group, pc.max_abs_diff(U, want_U), pc.max_abs_diff(V, want_V), rel))
    assert got_form == form, what
    if form == FORM_CHAIN:
        assert group == ratings_per_pass(k), what
    assert np.abs(want_U - c["U"]).max() > 1e-3, what + ": the run did not move the factors"
    assert pc.bits_equal(U, want_U), "%s: U differs, max |diff| %g" % (what, pc.max_abs_diff(U, want_U))
    assert pc.bits_equal(V, want_V), "%s: V differs, max |diff| %g" % (what, pc.max_abs_diff(V, want_V))
    assert rel <= 1e-12, "%s: loss %r against %r" % (what, loss, want_loss)


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("k", K_EDGES + (257,))
def test_factor_counts_on_the_level_schedule(k, variant):
    check("base", k, variant, FORM_LEVELS)


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("k", K_EDGES)
def test_factor_counts_on_the_dataflow_launch(k, variant):
    check("chain", k, variant, FORM_CHAIN)


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_k_257_takes_the_level_schedule_at_any_size(variant):
    check("chain", 257, variant, FORM_LEVELS)


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("nnz,form", [(4095, FORM_LEVELS), (4096, FORM_CHAIN)])
def test_size_threshold(nnz, form, variant):
    check("nnz%d" % nnz, 5, variant, form)


@pytest.mark.parametrize("variant", pc.VARIANTS)
@pytest.mark.parametrize("k", (10, 40))
@pytest.mark.parametrize("order", ("user", "item", "shuffled"))
def test_stored_orders(order, k, variant):
    """sorted by user (users owned), by item (items owned), shuffled; a 1 000-rating row, a single-rating user, repeated
    (u, i) pairs — grouped (k = 10) and one rating per wave (k = 40)"""
    check("order_" + order, k, variant, FORM_CHAIN)


def test_sigmoid_saturation():
    check("saturation", 5, "non_linear", FORM_LEVELS)


@pytest.mark.parametrize("kind,form", [("base", FORM_LEVELS), ("chain", FORM_CHAIN)])
def test_epochs_chain_across_calls_and_set_factors_resets_the_caches(kind, form):
    c = case(kind, 5)
    variant = "non_linear"
    rat = pc.ratings_for(variant, c["stars"])
    U3, V3, loss3, _ = pc.run_reference(c, variant, epochs=3)
    U1, V1, _, _ = pc.run_reference(c, variant, epochs=1)
    Ur, Vr, _, _ = pc.run_reference(c, variant, epochs=2, U=U1, V=V1)     # fresh caches after the first epoch
    tr = trainer_for(c, rat)
    try:
        tr.pmf_set_factors(c["U"], c["V"])
        l1 = fit(tr, c, variant, epochs=1)
        l2 = fit(tr, c, variant, epochs=2)
        U, V = tr.pmf_get_factors()
        assert tr.pmf_form()[0] == form
        assert pc.bits_equal(U, U3) and pc.bits_equal(V, V3), "1 + 2 epochs in two calls differ from 3 in one"
        assert np.max(np.abs(np.concatenate([l1, l2]) - loss3) / loss3) <= 1e-12
        assert len(fit(tr, c, variant, epochs=0)) == 0
        assert all(pc.bits_equal(a, b) for a, b in zip(tr.pmf_get_factors(), (U3, V3))), "0 epochs moved the factors"
        tr.pmf_set_factors(U1, V1)
        fit(tr, c, variant, epochs=2)
        U, V = tr.pmf_get_factors()
        assert pc.bits_equal(U, Ur) and pc.bits_equal(V, Vr), "set_factors did not zero the caches"
        assert not pc.bits_equal(Ur, U3)
    finally:
        tr.close()


def test_pmf_leaves_the_mf_state_alone_and_mf_still_fits():
    c = case("chain", 5)
    rs = np.random.RandomState(3)
    mfU, mfV = rs.normal(0, 0.1, (c["nu"], 5)).astype(np.float32), rs.normal(0, 0.1, (c["ni"], 5)).astype(np.float32)
    Bu, Bi = rs.normal(0, 0.1, c["nu"]).astype(np.float32), rs.normal(0, 0.1, c["ni"]).astype(np.float32)
    tr = trainer_for(c, c["stars"])
    other = trainer_for(c, c["stars"])
    try:
        tr.set_factors(mfU, mfV, Bu, Bi)
        tr.pmf_set_factors(c["U"], c["V"])
        fit(tr, c, "linear")
        assert all(np.array_equal(a, b) for a, b in zip(tr.get_factors(), (mfU, mfV, Bu, Bi))), "a PMF fit touched the MF tables"
        U, V = tr.pmf_get_factors()
        want_U, want_V, _ = reference("chain", 5, "linear")
        assert pc.bits_equal(U, want_U) and pc.bits_equal(V, want_V)
        # the deterministic MF fit of a handle that has run PMF equals that of a fresh handle, and leaves PMF's tables
        other.set_factors(mfU, mfV, Bu, Bi)
        args = (2, 0.01, 0.02, 3.0, True, False, _lib.MODE_DETERMINISTIC)
        tr.fit(*args)
        other.fit(*args)
        assert all(np.array_equal(a, b) for a, b in zip(tr.get_factors(), other.get_factors()))
        assert not np.array_equal(tr.get_factors()[0], mfU)
        assert all(pc.bits_equal(a, b) for a, b in zip(tr.pmf_get_factors(), (U, V)))
    finally:
        tr.close()
        other.close()


def test_argument_checks():
    c = case("base", 5)
    tr = trainer_for(c, c["stars"])
    L = _lib.lib()
    try:
        assert L.cornac_hip_mf_pmf_fit(tr.h, 1, 0.1, 0.1, 0.9, 0, None) == 1, "pmf_fit before pmf_set_factors"
        assert b"pmf_set_factors" in L.cornac_hip_last_error()
        assert L.cornac_hip_mf_pmf_get_factors(tr.h, None, None) == 1
        assert L.cornac_hip_mf_pmf_set_factors(tr.h, None, None) == 1
        tr.pmf_set_factors(c["U"], c["V"])
        assert L.cornac_hip_mf_pmf_fit(tr.h, 1, 0.1, 0.1, 0.9, 2, None) == 1 and b"variant" in L.cornac_hip_last_error()
        assert L.cornac_hip_mf_pmf_fit(tr.h, -1, 0.1, 0.1, 0.9, 0, None) == 1 and b"n_epochs" in L.cornac_hip_last_error()
        assert L.cornac_hip_mf_pmf_fit(tr.h, 1, 0.005, 0.01, 0.9, 0, None) == 0, "loss_per_epoch may be NULL"
        form = C.c_int()
        assert L.cornac_hip_mf_pmf_form(tr.h, C.byref(form), None) == 0 and form.value == FORM_LEVELS
        U, _ = tr.pmf_get_factors()
        assert np.isfinite(U).all() and not np.array_equal(U, c["U"])
    finally:
        tr.close()


@pytest.mark.parametrize("variant", pc.VARIANTS)
def test_model_fit_score_rank(variant):
    """PMF(seed=123).fit(ds) == the restatement started from the same RandomState draws; score(u) and score(u, i) to 1e-12
    relative, rank(u, k=10) in the order of the restatement's scores"""
    c = pc.order_case("shuffled")
    ds = Dataset.from_uir([(int(u), int(i), float(r)) for u, i, r in zip(c["uid"], c["iid"], c["stars"])], seed=123)
    kw = dict(k=10, max_iter=2, learning_rate=0.005, lambda_reg=0.01, variant=variant, seed=123)
    m = PMF(**kw).fit(ds)
    rs = np.random.RandomState(123)
    U0, V0 = rs.normal(0.0, 0.001, (ds.num_users, 10)), rs.normal(0.0, 0.001, (ds.num_items, 10))
    uid, iid, val = ds.uir_tuple
    rat = pc.ratings_for(variant, val)
    U, V, loss, _ = pc.pmf_fit(uid, iid, rat, U0, V0, 2, 0.01, 0.005, 0.9, variant)
    assert pc.bits_equal(m.U, U) and pc.bits_equal(m.V, V), (pc.max_abs_diff(m.U, U), pc.max_abs_diff(m.V, V))
    assert np.max(np.abs(m.loss_history - loss) / loss) <= 1e-12
    for u in (0, 17, ds.num_users - 1):
        want = V @ U[u]
        got = m.score(u)
        assert got.dtype == np.float64 and np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
        for i in (0, 3, ds.num_items - 1):
            one = V[i].dot(U[u])
            if variant == "non_linear":
                one = 1.0 / (1.0 + np.exp(-one)) * (ds.max_rating - ds.min_rating) + ds.min_rating
            assert abs(m.score(u, i) - one) <= 1e-12 * abs(one)
        ranked, scores = m.rank(u, k=10)
        assert np.array_equal(scores, got) and len(ranked) == ds.num_items
        order = np.lexsort((np.arange(ds.num_items), want))[::-1]
        assert np.array_equal(ranked[:10], order[:10])
