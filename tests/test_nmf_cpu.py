"""NMF without a GPU: (1) the restatement of the reference's loop (tests/nmf_cases.nmf_fit) reproduces, bit for bit, what the
reference's own compiled loop wrote into tests/golden/nmf_ref.npz, and the inputs hold what their docstrings promise;
(2) the host logic of cornac_amd.NMF, run through a device double that calls the restatement; (3) the four ABI entry
points are declared and bound."""
import os
import pickle
import re

import numpy as np
import pytest

import fake_device
import nmf_cases as nc
from conftest import ROOT, load_golden, synth_dataset
from cornac_amd import MF, NMF, Experiment, RatioSplit, Recommender, ScoreException, _lib
from cornac_amd import metrics as mm


# ---- (1) restatement == the reference's compiled loop --------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("nmf_ref")


@pytest.mark.parametrize("name", ["plain_k5", "bias_k5", "plain_k15", "bias_k15"])
def test_restatement_reproduces_the_reference_bit_for_bit(golden, name):
    assert name in list(golden["cases"])
    g = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    assert len(g["val"]) == 600 and g["U0"].shape[0] == 60 and g["V0"].shape[0] == 40
    assert bool(g["use_bias"]) == name.startswith("bias") and g["U0"].shape[1] == int(name.split("_k")[1])
    lr, lu, lv, lbu, lbi, mu = g["hyper"]
    assert (mu != 0.0) == bool(g["use_bias"])
    U, V, Bu, Bi, _ = nc.nmf_fit(g["rid"], g["cid"], g["val"], g["U0"], g["V0"], None, None, int(g["epochs"]), lr, lu, lv, lbu,
                                 lbi, mu, bool(g["use_bias"]))
    assert np.abs(g["U"] - g["U0"]).max() > 1e-2, "the golden run did not move the factors"
    assert g["Bu"].any() == bool(g["use_bias"]) and g["Bi"].any() == bool(g["use_bias"])
    for mine, ref, what in ((U, g["U"], "U"), (V, g["V"], "V"), (Bu, g["Bu"], "Bu"), (Bi, g["Bi"], "Bi")):
        assert nc.bits_equal(mine, ref), "%s: max |diff| %g" % (what, nc.max_abs_diff(mine, ref))


def test_restatement_epochs_chain_across_calls():
    """what the device tests lean on: no state but the tables — 1 + 2 epochs = 3 epochs"""
    c = nc.base_case(5)
    for use_bias in (False, True):
        U3, V3, Bu3, Bi3, loss3 = nc.run_reference(c, use_bias, epochs=3)
        U1, V1, Bu1, Bi1, l1 = nc.run_reference(c, use_bias, epochs=1)
        U, V, Bu, Bi, l2 = nc.run_reference(c, use_bias, epochs=2, U=U1, V=V1, Bu=Bu1, Bi=Bi1)
        assert all(nc.bits_equal(a, b) for a, b in zip((U, V, Bu, Bi), (U3, V3, Bu3, Bi3)))
        assert np.array_equal(np.concatenate([l1, l2]), loss3)


def test_cases_hold_what_their_docstrings_promise():
    for c, shape in ((nc.base_case(), (48, 32, 256)), (nc.chain_case(), (128, 48, 4096)), (nc.wide_case(), (300, 200, 5000)),
                     (nc.threshold_case(4095), (200, 150, 4095)), (nc.threshold_case(4096), (200, 150, 4096)),
                     (nc.long_rows_case(), (1200, 200, 6000))):
        assert (c["nu"], c["ni"], len(c["val"])) == shape
        assert c["U"].shape == (c["nu"], c["k"]) and c["V"].shape == (c["ni"], c["k"]) and c["U"].dtype == np.float32
        cells = c["rid"].astype(np.int64) * c["ni"] + c["cid"]
        assert (np.diff(cells) > 0).all(), "unique cells in CSR order"
        assert set(np.unique(c["val"])) <= {1.0, 2.0, 3.0, 4.0, 5.0} and c["U"].min() >= 0 and c["U"].max() < 1
        assert (c["lambda_u"], c["lambda_v"], c["lambda_bu"], c["lambda_bi"]) == (0.06, 0.06, 0.02, 0.02)
    assert len(nc.chain_case()["val"]) >= 4096
    c = nc.long_rows_case()
    cu, ci = np.bincount(c["rid"], minlength=1200), np.bincount(c["cid"], minlength=200)
    assert ci[3] == 1000 and cu[1199] == 1 and cu[7] == 0 and ci[11] == 0
    assert cu[0] == 199 == (ci > 0).sum(), "user 0 rates every item that has ratings"
    assert ci[3] > 3 * 256, "item 3's row spans at least four pieces of the free-order plan"


@pytest.mark.parametrize("case", ["base", "wide"])
def test_sequential_float32_run_sits_well_inside_the_free_order_bound(case):
    """the bound of the device's free-order check is not tuned to the device: the float32 run in the REFERENCE's order
    stays below 0.1 of it (against the float64 run of the same restatement), and no element is left out of the check.
    Of the deg-free (k + 16) form it stands at 0.14 / 0.16 on base and at 0.22 on wide (printed, not a bound: that form
    ignores the length of the sums)."""
    c = nc.base_case() if case == "base" else nc.wide_case()
    k = c["k"]
    U32, V32, _, _, loss32 = nc.run_reference(c, epochs=1)
    U64, V64, _, _, loss64, info = nc.run_reference(c, epochs=1, dtype=np.float64, details=True)
    du, di = np.bincount(c["rid"], minlength=c["nu"]), np.bincount(c["cid"], minlength=c["ni"])
    for got, want, deg in ((U32, U64, du), (V32, V64, di)):
        excess, checked = nc.free_order_excess(got, want, deg, k)
        tight, _ = nc.free_order_excess(got, want, np.full(len(deg), -k / 2.0), k)      # the deg-free (k + 16) form
        print("%s: %.3f of the bound, %.3f of its k + 16 form, %d elements" % (case, excess, tight, checked))
        assert checked == (deg > 0).sum() * k and excess <= 0.1 and excess <= tight
        assert (got[deg == 0] == 0).all() and (want[deg == 0] == 0).all()
    assert abs(loss32[0] - loss64[0]) <= nc.free_order_loss_bound(c, k, info, c["U"], c["V"])


BIAS_CASES = [("base", k) for k in (1, 15, 33, 65, 130, 257)] + [("chain", 15), ("chain", 64), ("long", 15), ("long", 40)]


@pytest.mark.parametrize("kind,k", BIAS_CASES)
def test_with_biases_the_plain_bound_is_within_reach_on_every_case_but_one(kind, k):
    """every bias case of the device's free-order check except long rows at k = 257: the sequential float32 run meets the
    plain element bound (at most 0.32 of it, long rows at k = 40) and the plain loss bound, so the device is held to both"""
    c = {"base": nc.base_case, "chain": nc.chain_case, "long": nc.long_rows_case}[kind](k)
    U32, V32, _, _, loss32 = nc.run_reference(c, True, epochs=1)
    U64, V64, _, _, loss64, info = nc.run_reference(c, True, epochs=1, dtype=np.float64, details=True)
    du, di = np.bincount(c["rid"], minlength=c["nu"]), np.bincount(c["cid"], minlength=c["ni"])
    eu, ei = nc.free_order_excess(U32, U64, du, k)[0], nc.free_order_excess(V32, V64, di, k)[0]
    print("%s k=%d bias: sequential float32 run at %.3f / %.3f (U / V) of the plain bound" % (kind, k, eu, ei))
    assert eu <= 1.0 and ei <= 1.0
    assert abs(loss32[0] - loss64[0]) <= nc.free_order_loss_bound(c, k, info, c["U"], c["V"])


def test_with_biases_the_bound_carries_the_conditioning_of_r_pred():
    """long rows, k = 257, use_bias — the ONE case whose element bounds carry the condition factor: the biases fall to
    -40 / -64 against dot products of 64, r_pred cancels (minimum -1.89 out of terms of magnitude 130; the worst element's
    row, a single-rating user, has -0.70) and the reference's own sequential float32 run stands at 8.04 of the plain
    bound — no summation order can do better on a row of one rating.  With the condition factor (exactly 1 where nothing
    cancels: every case without biases) it stands at 0.02.  The plain LOSS bound holds here too."""
    c = nc.long_rows_case(257)
    U32, V32, _, _, loss32 = nc.run_reference(c, True, epochs=1)
    U64, V64, _, _, loss64, info = nc.run_reference(c, True, epochs=1, dtype=np.float64, details=True)
    du, di = np.bincount(c["rid"], minlength=c["nu"]), np.bincount(c["cid"], minlength=c["ni"])
    cond_u, cond_i = nc.free_order_condition(c, info)
    plain = nc.free_order_excess(U32, U64, du, 257)[0]
    print("sequential float32 run: %.3f of the plain bound, %.3f / %.3f (U / V) of the conditioned one; r_pred min %.3g" % (
        plain, nc.free_order_excess(U32, U64, du, 257, cond_u)[0], nc.free_order_excess(V32, V64, di, 257, cond_i)[0],
        info["r_pred"].min()))
    assert plain > 1.0 and info["r_pred"].min() < 0 and cond_u.min() >= 1.0 and cond_i.min() >= 1.0
    assert nc.free_order_excess(U32, U64, du, 257, cond_u)[0] <= 1.0 and nc.free_order_excess(V32, V64, di, 257, cond_i)[0] <= 1.0
    assert abs(loss32[0] - loss64[0]) <= nc.free_order_loss_bound(c, 257, info, c["U"], c["V"])
    # without biases nothing is negative: the factor is exactly 1 and the bound is the plain one
    _, _, _, _, _, info = nc.run_reference(c, False, epochs=1, dtype=np.float64, details=True)
    assert all((x == 1).all() for x in nc.free_order_condition(c, info))


# ---- (2) host logic of the NMF class over a device double ----------------------------------------------------------
class FakeNmfTrainer(fake_device.FakeMfTrainer):
    """the MF double plus the NMF calls, served by the restatement; records what the model handed over"""
    last = None

    def __init__(self, rid, cid, val, n_users, n_items, k, device=0):
        super().__init__(rid, cid, val, n_users, n_items, k, device)
        self.raw = (rid, cid, val)
        self.shape = (int(n_users), int(n_items), int(k))
        FakeNmfTrainer.last = self

    def nmf_set_factors(self, U, V, Bu=None, Bi=None):
        assert all(a.dtype == np.float32 for a in (U, V, Bu, Bi))
        assert U.shape == (self.shape[0], self.shape[2]) and V.shape == (self.shape[1], self.shape[2])
        self.start = tuple(a.copy() for a in (U, V, Bu, Bi))
        self.tables = self.start

    def nmf_fit(self, n_epochs, lr, lambda_u, lambda_v, lambda_bu, lambda_bi, mu, use_bias=False, mode=_lib.MODE_HOGWILD):
        self.call = dict(n_epochs=n_epochs, lr=lr, lambda_u=lambda_u, lambda_v=lambda_v, lambda_bu=lambda_bu,
                         lambda_bi=lambda_bi, mu=mu, use_bias=use_bias, mode=mode)
        *self.tables, loss = nc.nmf_fit(self.rid, self.cid, self.val, *self.tables, n_epochs, lr, lambda_u, lambda_v, lambda_bu,
                                        lambda_bi, mu, use_bias)
        return loss

    def nmf_get_factors(self):
        return tuple(a.copy() for a in self.tables)


@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "MfTrainer", FakeNmfTrainer)
    monkeypatch.chdir(tmp_path)


@pytest.fixture(scope="module")
def ds():
    return synth_dataset(60, 40, 700, seed=4)


KW = dict(k=5, max_iter=2, seed=123)


def test_constructor_is_the_references():
    m = NMF()
    assert (m.name, m.k, m.max_iter, m.learning_rate, m.lambda_reg, m.lambda_u, m.lambda_v, m.lambda_bu, m.lambda_bi, m.use_bias,
            m.trainable, m.verbose, m.seed, m.mode, m.device) == \
        ("NMF", 15, 50, 0.005, 0.0, 0.06, 0.06, 0.02, 0.02, False, True, False, None, None, 0)
    import inspect

    assert list(inspect.signature(NMF.__init__).parameters)[1:] == [
        "name", "k", "max_iter", "learning_rate", "lambda_reg", "lambda_u", "lambda_v", "lambda_bu", "lambda_bi", "use_bias",
        "num_threads", "trainable", "verbose", "init_params", "seed", "mode", "device"]
    assert m.u_factors is None and m.i_biases is None and m.global_mean is None and m.init_params == {}
    assert isinstance(m, Recommender) and NMF(seed=3).num_threads == 1
    assert m.effective_mode == "hogwild" and NMF(seed=3).effective_mode == "deterministic"
    assert NMF(seed=3, mode="hogwild").effective_mode == "hogwild"
    with pytest.raises(ValueError):
        NMF(mode="racy")
    o = NMF(lambda_reg=0.3)
    assert (o.lambda_u, o.lambda_v, o.lambda_bu, o.lambda_bi) == (0.3, 0.3, 0.3, 0.3)


def test_hand_over_csr_order_init_and_in_place_refresh(device_double, ds):
    m = NMF(**KW).fit(ds)
    t = FakeNmfTrainer.last
    X = ds.matrix
    # the CSR of train_set.matrix, not uir_tuple (which is in shuffled insertion order here)
    assert np.array_equal(t.rid, np.repeat(np.arange(ds.num_users), np.diff(X.indptr))) and (np.diff(t.rid) >= 0).all()
    assert np.array_equal(t.cid, X.indices) and np.array_equal(t.val, X.data.astype(np.float32))
    assert t.raw[2].dtype == np.float32 and t.raw[0].dtype == X.indices.dtype
    assert not np.array_equal(t.rid, ds.uir_tuple[0])
    rs = np.random.RandomState(123)
    U0 = rs.uniform(0, 1, (ds.num_users, 5)).astype(np.float32)
    V0 = rs.uniform(0, 1, (ds.num_items, 5)).astype(np.float32)
    assert np.array_equal(t.start[0], U0) and np.array_equal(t.start[1], V0)
    assert not t.start[2].any() and not t.start[3].any()
    assert t.call == dict(n_epochs=2, lr=0.005, lambda_u=0.06, lambda_v=0.06, lambda_bu=0.02, lambda_bi=0.02, mu=0.0,
                          use_bias=False, mode=_lib.MODE_DETERMINISTIC)
    assert m.global_mean == 0.0 and len(m.loss_history) == 2 and m.u_factors.dtype == np.float32
    assert all(np.array_equal(a, b) for a, b in zip((m.u_factors, m.i_factors, m.u_biases, m.i_biases), t.tables))
    # mu and the lambda override; unseeded: hogwild
    NMF(k=5, max_iter=1, use_bias=True, lambda_reg=0.1).fit(ds)
    c = FakeNmfTrainer.last.call
    assert c["mu"] == pytest.approx(ds.global_mean) and c["use_bias"] is True and c["mode"] == _lib.MODE_HOGWILD
    assert (c["lambda_u"], c["lambda_v"], c["lambda_bu"], c["lambda_bi"]) == (0.1, 0.1, 0.1, 0.1)
    # given tables are used and refreshed IN PLACE; the missing one takes the generator's first draw
    Ug = np.full((ds.num_users, 5), 0.5, np.float32)
    Bg = np.full(ds.num_items, 0.25, np.float32)
    m2 = NMF(init_params={"U": Ug, "Bi": Bg, "mu": 9.0}, use_bias=True, **KW).fit(ds)
    t = FakeNmfTrainer.last
    assert np.all(t.start[0] == 0.5) and np.all(t.start[3] == 0.25)
    assert np.array_equal(t.start[1], np.random.RandomState(123).uniform(0, 1, (ds.num_items, 5)).astype(np.float32))
    assert m2.u_factors is Ug and m2.i_biases is Bg and not np.all(Ug == 0.5) and not np.all(Bg == 0.25)
    assert m2.global_mean == ds.global_mean, "the train set's mean, whatever init_params said"


def test_float64_tables_raise_type_error(device_double, ds):
    for key, shape in (("U", (ds.num_users, 5)), ("V", (ds.num_items, 5)), ("Bu", (ds.num_users,)), ("Bi", (ds.num_items,))):
        with pytest.raises(TypeError, match="float32"):
            NMF(init_params={key: np.full(shape, 0.5)}, **KW).fit(ds)


def test_trainable_false_initialises_but_does_not_train(device_double, ds):
    FakeNmfTrainer.last = None
    U = np.full((ds.num_users, 5), 0.5, np.float32)
    m = NMF(trainable=False, init_params={"U": U}, **KW).fit(ds)
    assert FakeNmfTrainer.last is None and np.all(m.u_factors == 0.5)
    assert m.i_factors.shape == (ds.num_items, 5) and not m.u_biases.any() and m.global_mean == 0.0   # _init ran


def test_score_branches_and_vectors(device_double, ds):
    for use_bias in (False, True):
        m = NMF(use_bias=use_bias, **KW).fit(ds)
        mu = m.global_mean
        assert (mu != 0.0) == use_bias
        want = mu + m.i_biases + m.u_biases[7] + m.i_factors @ m.u_factors[7]
        got = m.score(7)
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-5, atol=0)
        assert m.score(7, 11) == pytest.approx(float(want[11]), rel=1e-5)
        for unknown in (ds.num_users, -1, None):
            assert np.array_equal(m.score(unknown), mu + m.i_biases)
            assert m.score(unknown, 3) == mu + m.i_biases[3]
        for bad in (ds.num_items, -1):
            with pytest.raises(ScoreException):
                m.score(0, bad)
        ranked, scores = m.rank(7, k=10)
        assert np.array_equal(scores, got) and set(ranked[:10]) == set(np.argsort(-want.astype(np.float64), kind="stable")[:10])
        uv, iv = m.get_user_vectors(), m.get_item_vectors()
        assert m.get_vector_measure() == "dot"
        if use_bias:
            assert uv.shape == (ds.num_users, 6) and np.all(uv[:, 5] == 1) and np.array_equal(iv[:, 5], m.i_biases)
        else:
            assert uv is m.u_factors and iv is m.i_factors


def test_clone_save_load_pickle(device_double, ds, tmp_path):
    m = NMF(use_bias=True, lambda_u=0.1, mode="hogwild", **KW).fit(ds)
    c = m.clone()
    assert (c.k, c.lambda_u, c.use_bias, c.seed, c.max_iter, c.mode) == (5, 0.1, True, 123, 2, "hogwild")
    assert c.u_factors is None and not c.is_fitted and m.clone({"k": 7}).k == 7
    back = NMF.load(m.save(str(tmp_path)))
    assert all(np.array_equal(getattr(back, a), getattr(m, a)) for a in ("u_factors", "i_factors", "u_biases", "i_biases"))
    assert back.trainable is False and back.global_mean == m.global_mean and np.array_equal(back.score(3), m.score(3))
    again = pickle.loads(pickle.dumps(m))
    assert np.array_equal(again.i_factors, m.i_factors) and not hasattr(again, "train_set")


def test_experiment_over_mf_and_nmf(device_double, capsys):
    rs = np.random.RandomState(8)
    keys = rs.permutation(70 * 50)[:1500]
    data = [("u%d" % (k // 50), "i%d" % (k % 50), float(rs.randint(1, 6))) for k in keys]
    split = RatioSplit(data, test_size=0.2, rating_threshold=4.0, seed=123)
    models = [MF(k=10, max_iter=5, learning_rate=0.01, lambda_reg=0.02, use_bias=True, seed=123),
              NMF(k=15, max_iter=20, seed=123)]
    ex = Experiment(split, models, [mm.RMSE(), mm.Recall(k=20)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["MF", "NMF"]
    row = ex.result[1].metric_avg_results
    assert {"RMSE", "Recall@20"} <= set(row) and all(np.isfinite(v) for v in row.values())
    assert 0.0 < row["RMSE"] < 4.0 and 0.0 <= row["Recall@20"] <= 1.0
    capsys.readouterr()


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_nmf_entry_points():
    names = ["cornac_hip_mf_nmf_set_factors", "cornac_hip_mf_nmf_get_factors", "cornac_hip_mf_nmf_fit", "cornac_hip_mf_nmf_form"]
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in names:
        assert re.search(r"\bint %s\s*\(cornac_hip_mf_t h" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
        assert all(hasattr(_lib.MfTrainer, n) for n in ("nmf_set_factors", "nmf_get_factors", "nmf_fit", "nmf_form"))
    assert "recom_nmf.pyx" in header
    # argument checks need no device: a NULL handle is refused with the invalid-argument status
    assert _lib.lib().cornac_hip_mf_nmf_fit(None, 1, 0.1, 0.1, 0.1, 0.1, 0.1, 0.0, 0, 0, None) == 1
    assert _lib.lib().cornac_hip_mf_nmf_form(None, None, None, None) == 1
