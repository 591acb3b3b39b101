"""NMF on the device against the restatement of the reference's loop (tests/nmf_cases.nmf_fit, itself held bit for bit against
the reference's compiled loop by tests/test_nmf_cpu.py), through the C ABI and through cornac_amd.NMF.

Deterministic mode: U, V, Bu, Bi equal the float32 restatement BIT FOR BIT — every operation is a correctly rounded IEEE
float + - * / in a pinned order with contraction off, so a mismatch is a bug in the expression tree, in a row sum's order
or in the bias hand-over, not noise.  loss_per_epoch: relative error <= 1e-12 (at most ~25 000 non-negative float32 terms
summed in double in another order: n 2^-53 ~ 3e-12 worst case, sqrt(n) 2^-53 ~ 2e-14 typical).

Free-order (hogwild) mode, one epoch against the float64 run of the same restatement: every element with a nonzero
float64 value within (2 deg + 2 k + 16) 2^-24 relative (deg: its row's rating count) — the first-order bound of two
deg-term sums of non-negative terms that each carry r_pred's own (k + 2)-term error, plus the final multiply and divide;
tests/test_nmf_cpu.py shows the float32 run in the reference's own order at < 0.1 of it.  The loss within
2 (k + 3) 2^-24 sum |e| (r + r_pred) plus the same relative factor on the regulariser.  Every case is held to these two
bounds as they stand, with one exception among the element bounds: long rows at k = 257 WITH biases.  There the
uniform(0, 1) start predicts about 67 for ratings 1..5, the biases fall to -40 / -64 within the epoch and r_pred cancels
(its minimum is -1.89 out of terms of magnitude 130), so r_pred's (k + 2)-term error is relative to the sum of its terms'
magnitudes, not to r_pred.  On that case the reference's own sequential float32 loop stands at 8.04 of the plain bound —
its worst element belongs to a single-rating user, where no order exists to choose — and
tests/test_nmf_cpu.py::test_with_biases_the_bound_carries_the_conditioning_of_r_pred asserts it.  For that case alone each
element's bound is multiplied by (its denominator summed over those magnitudes) / |its denominator| >= 1 from the
float64 run (nmf_cases.free_order_condition); its loss bound is the plain one.

Every check prints the forms taken (nmf_form) and the measured distance to its bound.
"""
import functools

import numpy as np
import pytest

import nmf_cases as nc
from cornac_amd import NMF, Dataset, _lib
from cornac_amd import eval as ev
from cornac_amd import metrics as mm

pytestmark = pytest.mark.gpu

K_EDGES = (1, 5, 15, 16, 17, 32, 33, 64, 65, 256, 257)   # 257: past the register-resident sums
DET, HOG = _lib.MODE_DETERMINISTIC, _lib.MODE_HOGWILD
SUM_ORDERED, SUM_FREE = 1, 2
BIAS_NONE, BIAS_CHAIN, BIAS_LEVELS = 0, 1, 2


@functools.lru_cache(maxsize=None)
def case(kind, k=15):
    if kind == "base":
        return nc.base_case(k)
    if kind == "chain":
        return nc.chain_case(k)
    if kind == "long":
        return nc.long_rows_case(k)
    assert kind.startswith("nnz")
    return nc.threshold_case(int(kind[3:]), k)


@functools.lru_cache(maxsize=None)
def reference(kind, k, use_bias, epochs=None, dtype=np.float32):
    out = nc.run_reference(case(kind, k), use_bias, epochs=epochs, dtype=dtype, details=True)
    for a in out[:5]:
        a.setflags(write=False)
    return out


def expected_bias_form(c, use_bias):
    return BIAS_NONE if not use_bias else BIAS_CHAIN if len(c["val"]) >= 4096 else BIAS_LEVELS


def trainer_for(c):
    return _lib.MfTrainer(c["rid"], c["cid"], c["val"], c["nu"], c["ni"], c["k"])


def fit(tr, c, use_bias, mode, epochs=None):
    return tr.nmf_fit(c["epochs"] if epochs is None else epochs, c["lr"], c["lambda_u"], c["lambda_v"], c["lambda_bu"],
                      c["lambda_bi"], c["mu"] if use_bias else 0.0, use_bias, mode)


def run(c, use_bias, mode, epochs=None):
    tr = trainer_for(c)
    try:
        assert tr.nmf_form() == (0, 0, 0)
        tr.nmf_set_factors(c["U"], c["V"])
        loss = fit(tr, c, use_bias, mode, epochs)
        return tr.nmf_get_factors(), loss, tr.nmf_form()
    finally:
        tr.close()


def check_deterministic(kind, k, use_bias):
    c = case(kind, k)
    *want, want_loss, _ = reference(kind, k, use_bias)
    got, loss, form = run(c, use_bias, DET)
    what = "%s k=%d %s" % (kind, k, "bias" if use_bias else "plain")
    rel = float(np.max(np.abs(loss - want_loss) / want_loss))
    print("%s: forms (sum, bias, split) %r, max |d| U %.3g V %.3g Bu %.3g Bi %.3g, loss rel err %.3g (bound 1e-12)" % (
        (what, form) + tuple(nc.max_abs_diff(a, b) for a, b in zip(got, want)) + (rel,)))
    assert form == (SUM_ORDERED, expected_bias_form(c, use_bias), 0), what
    assert np.abs(want[0] - c["U"]).max() > 1e-2 and np.abs(want[1] - c["V"]).max() > 1e-2, what + ": the run did not move the factors"
    assert (np.abs(want[2]).max() > 1e-4) == use_bias, what
    for a, b, name in zip(got, want, ("U", "V", "Bu", "Bi")):
        assert nc.bits_equal(a, b), "%s: %s differs, max |diff| %g" % (what, name, nc.max_abs_diff(a, b))
    assert rel <= 1e-12, "%s: loss %r against %r" % (what, loss, want_loss)


@pytest.mark.parametrize("use_bias", (False, True))
@pytest.mark.parametrize("k", K_EDGES)
def test_deterministic_factor_counts_below_the_dataflow_threshold(k, use_bias):
    check_deterministic("base", k, use_bias)


@pytest.mark.parametrize("use_bias", (False, True))
@pytest.mark.parametrize("k", K_EDGES)
def test_deterministic_factor_counts_from_the_dataflow_threshold(k, use_bias):
    check_deterministic("chain", k, use_bias)


@pytest.mark.parametrize("nnz", (4095, 4096))
def test_deterministic_size_threshold_of_the_bias_pass(nnz):
    assert expected_bias_form(case("nnz%d" % nnz, 5), True) == (BIAS_LEVELS if nnz == 4095 else BIAS_CHAIN)
    check_deterministic("nnz%d" % nnz, 5, True)


@pytest.mark.parametrize("use_bias", (False, True))
@pytest.mark.parametrize("k", (15, 40))
def test_deterministic_long_rows(k, use_bias):
    """a 1000-rating item, a 199-rating user, a single-rating user, a user and an item without ratings (exactly zero)"""
    check_deterministic("long", k, use_bias)
    want_U, want_V = reference("long", k, use_bias)[:2]
    assert not want_U[7].any() and not want_V[11].any() and want_U[0].all()


def check_free_order(kind, k, use_bias, conditioned=False):
    c = case(kind, k)
    U64, V64, Bu64, Bi64, loss64, info = reference(kind, k, use_bias, 1, np.float64)
    (U, V, Bu, Bi), loss, form = run(c, use_bias, HOG, epochs=1)
    again, _, form2 = run(c, use_bias, HOG, epochs=1)
    what = "%s k=%d %s" % (kind, k, "bias" if use_bias else "plain")
    du, di = np.bincount(c["rid"], minlength=c["nu"]), np.bincount(c["cid"], minlength=c["ni"])
    cond_u, cond_i = nc.free_order_condition(c, info) if conditioned else (np.ones_like(U64), np.ones_like(V64))
    eu, nu_checked = nc.free_order_excess(U, U64, du, k, cond_u)
    ei, ni_checked = nc.free_order_excess(V, V64, di, k, cond_i)
    loss_bound = nc.free_order_loss_bound(c, k, info, c["U"], c["V"])
    print("%s: forms (sum, bias, split) %r, U at %.3f of its bound (%d elements), V at %.3f (%d), loss off by %.3g (bound %.3g); "
          "largest condition factor %.3g" % (what, form, eu, nu_checked, ei, ni_checked, abs(loss[0] - loss64[0]), loss_bound,
                                             max(cond_u.max(), cond_i.max())))
    assert form[:2] == (SUM_FREE, expected_bias_form(c, use_bias)) and form2 == form, what
    assert nu_checked == (U64 != 0).sum() and ni_checked == (V64 != 0).sum(), "no element may be left out"
    assert nu_checked >= (du > 0).sum() * k - 2 and ni_checked >= (di > 0).sum() * k - 2
    assert eu <= 1.0 and ei <= 1.0, what
    assert not U[du == 0].any() and not V[di == 0].any(), what + ": a row without ratings becomes exactly zero"
    assert np.all(U[U64 == 0] == 0) and np.all(V[V64 == 0] == 0)
    assert abs(loss[0] - loss64[0]) <= loss_bound, what
    for a, b, name in zip((U, V, Bu, Bi), again, ("U", "V", "Bu", "Bi")):
        assert nc.bits_equal(a, b), "%s: %s differs between two runs" % (what, name)
    if use_bias:   # the bias pass is sequential-exact in both modes
        _, _, Bu32, Bi32, _, _ = reference(kind, k, True, 1)
        assert nc.bits_equal(Bu, Bu32) and nc.bits_equal(Bi, Bi32), what + ": biases differ from deterministic mode's"
    else:
        assert not Bu.any() and not Bi.any()
    return form


@pytest.mark.parametrize("use_bias", (False, True))
@pytest.mark.parametrize("kind,k", [("base", 1), ("base", 15), ("base", 33), ("base", 65), ("base", 130), ("base", 257),
                                    ("chain", 15), ("chain", 64)])
def test_free_order_against_the_float64_run(kind, k, use_bias):
    assert check_free_order(kind, k, use_bias)[2] == 0


@pytest.mark.parametrize("use_bias", (False, True))
@pytest.mark.parametrize("k", (15, 40, 257))
def test_free_order_long_rows_are_split_and_combined_in_order(k, use_bias):
    # the one case whose element bounds carry the condition factor (module docstring): k = 257 with biases
    form = check_free_order("long", k, use_bias, conditioned=(k == 257 and use_bias))
    assert form[2] >= 1, "item 3 (1000 ratings) is summed in pieces"


@pytest.mark.parametrize("mode", (DET, HOG))
@pytest.mark.parametrize("kind", ("base", "chain"))
def test_epochs_chain_across_calls_and_zero_epochs_move_nothing(kind, mode):
    c = case(kind, 15)
    tr, one = trainer_for(c), trainer_for(c)
    try:
        tr.nmf_set_factors(c["U"], c["V"])
        one.nmf_set_factors(c["U"], c["V"])
        l1 = fit(tr, c, True, mode, epochs=1)
        l2 = fit(tr, c, True, mode, epochs=2)
        l3 = fit(one, c, True, mode, epochs=3)
        got, want = tr.nmf_get_factors(), one.nmf_get_factors()
        assert all(nc.bits_equal(a, b) for a, b in zip(got, want)), "1 + 2 epochs in two calls differ from 3 in one"
        assert np.max(np.abs(np.concatenate([l1, l2]) - l3) / l3) <= 1e-12
        if mode == DET:
            assert all(nc.bits_equal(a, b) for a, b in zip(got, reference(kind, 15, True, 3)[:4]))
        assert len(fit(tr, c, True, mode, epochs=0)) == 0
        assert all(nc.bits_equal(a, b) for a, b in zip(tr.nmf_get_factors(), want)), "0 epochs moved the tables"
    finally:
        tr.close()
        one.close()


def test_nmf_leaves_the_mf_and_pmf_state_alone_and_they_leave_nmf_alone():
    c = case("chain", 5)
    rs = np.random.RandomState(3)
    mfU, mfV = rs.normal(0, 0.1, (c["nu"], 5)).astype(np.float32), rs.normal(0, 0.1, (c["ni"], 5)).astype(np.float32)
    Bu, Bi = rs.normal(0, 0.1, c["nu"]).astype(np.float32), rs.normal(0, 0.1, c["ni"]).astype(np.float32)
    pU, pV = rs.normal(0, 0.3, (c["nu"], 5)), rs.normal(0, 0.3, (c["ni"], 5))
    tr, other = trainer_for(c), trainer_for(c)
    try:
        tr.set_factors(mfU, mfV, Bu, Bi)
        tr.pmf_set_factors(pU, pV)
        tr.nmf_set_factors(c["U"], c["V"])
        for mode in (DET, HOG):
            fit(tr, c, True, mode)
        assert all(np.array_equal(a, b) for a, b in zip(tr.get_factors(), (mfU, mfV, Bu, Bi))), "an NMF fit touched the MF tables"
        assert all(np.array_equal(a, b) for a, b in zip(tr.pmf_get_factors(), (pU, pV))), "an NMF fit touched the PMF tables"
        nmf = tr.nmf_get_factors()
        assert not np.array_equal(nmf[0], c["U"]) and np.abs(nmf[2]).max() > 0
        # a deterministic MF fit and a PMF fit of the handle that has run NMF equal a fresh handle's, and leave NMF's tables
        other.set_factors(mfU, mfV, Bu, Bi)
        other.pmf_set_factors(pU, pV)
        args = (2, 0.01, 0.02, 3.0, True, False, DET)
        tr.fit(*args)
        other.fit(*args)
        assert all(np.array_equal(a, b) for a, b in zip(tr.get_factors(), other.get_factors()))
        assert not np.array_equal(tr.get_factors()[0], mfU)
        for t in (tr, other):
            t.pmf_fit(1, 0.005, 0.01, 0.9, "linear")
        assert all(np.array_equal(a, b) for a, b in zip(tr.pmf_get_factors(), other.pmf_get_factors()))
        assert all(nc.bits_equal(a, b) for a, b in zip(tr.nmf_get_factors(), nmf)), "an MF or PMF fit touched the NMF tables"
    finally:
        tr.close()
        other.close()


def test_argument_checks():
    c = case("base", 5)
    L = _lib.lib()
    args = (0.005, 0.06, 0.06, 0.02, 0.02, 0.0, 0)
    tr = trainer_for(c)
    p = np.random.RandomState(0).permutation(len(c["val"]))
    shuffled = _lib.MfTrainer(c["rid"][p], c["cid"][p], c["val"][p], c["nu"], c["ni"], c["k"])
    try:
        assert L.cornac_hip_mf_nmf_fit(tr.h, 1, *args, DET, None) == 1, "nmf_fit before nmf_set_factors"
        assert b"nmf_set_factors" in L.cornac_hip_last_error()
        assert L.cornac_hip_mf_nmf_get_factors(tr.h, None, None, None, None) == 1
        assert L.cornac_hip_mf_nmf_set_factors(tr.h, None, None, None, None) == 1
        tr.nmf_set_factors(c["U"], c["V"])
        assert L.cornac_hip_mf_nmf_fit(tr.h, -1, *args, DET, None) == 1 and b"n_epochs" in L.cornac_hip_last_error()
        assert L.cornac_hip_mf_nmf_fit(tr.h, 1, *args, 2, None) == 1 and b"mode" in L.cornac_hip_last_error()
        shuffled.nmf_set_factors(c["U"], c["V"])
        assert L.cornac_hip_mf_nmf_fit(shuffled.h, 1, *args, DET, None) == 1 and b"stored by user" in L.cornac_hip_last_error()
        assert all(nc.bits_equal(a, b) for a, b in zip(shuffled.nmf_get_factors()[:2], (c["U"], c["V"])))
        assert L.cornac_hip_mf_nmf_fit(tr.h, 1, *args, HOG, None) == 0, "loss_per_epoch may be NULL"
        assert tr.nmf_form() == (SUM_FREE, BIAS_NONE, 0)
        U, V, Bu, Bi = tr.nmf_get_factors()
        assert np.isfinite(U).all() and not np.array_equal(U, c["U"]) and not Bu.any() and not Bi.any()
        # given biases are taken; without use_bias they enter r_pred and stay as they are
        B = np.full(c["nu"], 0.25, np.float32)
        tr.nmf_set_factors(c["U"], c["V"], B, None)
        fit(tr, c, False, DET, epochs=1)
        want = nc.run_reference(c, False, epochs=1, Bu=B)
        assert all(nc.bits_equal(a, b) for a, b in zip(tr.nmf_get_factors(), want[:4])) and np.all(want[2] == 0.25)
    finally:
        tr.close()
        shuffled.close()


@pytest.mark.parametrize("use_bias", (False, True))
def test_model_fit_score_rank_and_batched_evaluation(use_bias):
    """NMF(seed=123).fit(ds) == the restatement started from the same RandomState draws over the CSR of ds.matrix;
    score / rank / ranking_eval / rating_eval through the batched scorer agree with the per-user flow"""
    c = case("long", 15)
    ds = Dataset.from_uir([(int(u), int(i), float(r)) for u, i, r in zip(c["rid"], c["cid"], c["val"])], seed=123)
    m = NMF(k=15, max_iter=2, use_bias=use_bias, seed=123).fit(ds)
    assert m.effective_mode == "deterministic"
    rs = np.random.RandomState(123)
    U0 = rs.uniform(0, 1, (ds.num_users, 15)).astype(np.float32)
    V0 = rs.uniform(0, 1, (ds.num_items, 15)).astype(np.float32)
    X = ds.matrix
    rid = np.repeat(np.arange(ds.num_users), np.diff(X.indptr))
    mu = ds.global_mean if use_bias else 0.0
    U, V, Bu, Bi, loss = nc.nmf_fit(rid, X.indices, X.data.astype(np.float32), U0, V0, None, None, 2, mu=mu, use_bias=use_bias)
    for a, b, name in zip((m.u_factors, m.i_factors, m.u_biases, m.i_biases), (U, V, Bu, Bi), ("U", "V", "Bu", "Bi")):
        assert nc.bits_equal(a, b), "%s: max |diff| %g" % (name, nc.max_abs_diff(a, b))
    assert np.max(np.abs(m.loss_history - loss) / loss) <= 1e-12 and m.global_mean == mu
    assert m._scorer_row_count() == ds.num_users, "the float32 tables are served by the batched kernels"
    for u in (0, 17, ds.num_users - 1):
        want = (np.float64(mu) + Bi + Bu[u] + V.astype(np.float64) @ U[u].astype(np.float64))
        got = m.score(u)
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-5, atol=0)
        for i in (0, 3, ds.num_items - 1):
            assert m.score(u, i) == pytest.approx(want[i], rel=1e-5)
        ranked, scores = m.rank(u, k=10)
        assert np.array_equal(scores, got) and len(ranked) == ds.num_items
        assert np.array_equal(ranked[:10], np.lexsort((np.arange(ds.num_items), got))[::-1][:10])
    users, items = ds.user_ids, ds.item_ids
    test = Dataset.build([(users[u], items[i], float(1 + (u + i) % 5)) for u in range(0, ds.num_users, 7) for i in (5, 20, 60)],
                         global_uid_map=ds.uid_map, global_iid_map=ds.iid_map, seed=1)
    metrics = lambda: [mm.Recall(k=20), mm.NDCG(k=20), mm.AUC()]  # noqa: E731
    avg, _ = ev.ranking_eval(m, metrics(), ds, test, rating_threshold=4.0)
    plain = type("PlainModel", (), {"rank": lambda self, **kw: m.rank(**kw)})()
    avg2, _ = ev.ranking_eval(plain, metrics(), ds, test, rating_threshold=4.0)
    assert np.allclose(avg, avg2, atol=1e-9) and all(np.isfinite(avg))
    (rmse,), _ = ev.rating_eval(m, [mm.RMSE()], test)
    per_pair = [m.rate(int(u), int(i)) for u, i in zip(*test.uir_tuple[:2])]
    # the batched kernel's fma chain against score()'s float32 dot: k 2^-24 ~ 1e-6 relative per prediction
    assert rmse == pytest.approx(float(np.sqrt(np.mean((np.asarray(per_pair) - test.uir_tuple[2]) ** 2))), rel=1e-5)
