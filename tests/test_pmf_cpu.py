"""PMF without a GPU: (1) the restatement of the reference's two loops (tests/pmf_cases.pmf_fit) reproduces, bit for bit, what
the reference's own compiled loop wrote into tests/golden/pmf_ref.npz; (2) the host logic of cornac_amd.PMF, run through a
device double that calls the restatement; (3) the four ABI entry points are declared and bound."""
import os
import pickle
import re

import numpy as np
import pytest

import fake_device
import pmf_cases as pc
from conftest import ROOT, load_golden, synth_dataset
from cornac_amd import BPR, MF, PMF, Experiment, RatioSplit, Recommender, ScoreException, _lib
from cornac_amd import metrics as mm


# ---- (1) restatement == the reference's compiled loop --------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return load_golden("pmf_ref")


@pytest.mark.parametrize("name", ["linear_k5", "linear_k10", "non_linear_k5", "non_linear_k10"])
def test_restatement_reproduces_the_reference_bit_for_bit(golden, name):
    assert name in list(golden["cases"])
    g = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    variant = "non_linear" if name.startswith("non_linear") else "linear"
    assert len(g["rat"]) == 600 and g["U0"].shape[0] == 60 and g["V0"].shape[0] == 40
    reg, lr, gamma = g["hyper"]
    U, V, loss, _ = pc.pmf_fit(g["uid"], g["iid"], g["rat"], g["U0"], g["V0"], int(g["epochs"]), reg, lr, gamma, variant)
    assert np.abs(g["U"] - g["U0"]).max() > 1e-3, "the golden run did not move the factors"
    assert pc.bits_equal(U, g["U"]), "U: max |diff| %g" % pc.max_abs_diff(U, g["U"])
    assert pc.bits_equal(V, g["V"]), "V: max |diff| %g" % pc.max_abs_diff(V, g["V"])
    assert pc.bits_equal(loss, g["loss"]), (loss, g["loss"])


def test_restatement_caches_chain_across_calls():
    """what the device tests lean on: 1 + 2 epochs with the caches handed on = 3 epochs; from zero caches it is not"""
    c = pc.base_case()
    U3, V3, _, _ = pc.run_reference(c, "linear", epochs=3)
    U1, V1, _, caches = pc.run_reference(c, "linear", epochs=1)
    U, V, _, _ = pc.run_reference(c, "linear", epochs=2, caches=caches, U=U1, V=V1)
    assert pc.bits_equal(U, U3) and pc.bits_equal(V, V3)
    U, V, _, _ = pc.run_reference(c, "linear", epochs=2, U=U1, V=V1)
    assert not pc.bits_equal(U, U3)


def test_cases_hold_what_their_docstrings_promise():
    for order in ("user", "item", "shuffled"):
        c = pc.order_case(order)
        assert len(c["stars"]) == 5000 and (c["iid"] == 3).mean() >= 0.2 and (c["uid"] == 299).sum() == 1
        side = c["uid"] if order == "user" else c["iid"]
        assert (np.diff(side) >= 0).all() == (order != "shuffled")
    c = pc.saturation_case()
    assert set(np.unique(c["rat01"])) == {0.0, 1.0}
    assert len(pc.threshold_case(4095)["stars"]) == 4095


# ---- (2) host logic of the PMF class over a device double ----------------------------------------------------------
class FakePmfTrainer(fake_device.FakeMfTrainer):
    """the MF double plus the four PMF calls, served by the restatement; records what the model handed over"""
    last = None

    def __init__(self, rid, cid, val, n_users, n_items, k, device=0):
        super().__init__(rid, cid, val, n_users, n_items, k, device)
        self.shape = (int(n_users), int(n_items), int(k))
        FakePmfTrainer.last = self

    def pmf_set_factors(self, U, V):
        assert U.dtype == np.float64 and V.dtype == np.float64
        assert U.shape == (self.shape[0], self.shape[2]) and V.shape == (self.shape[1], self.shape[2])
        self.pU, self.pV, self.caches = U.copy(), V.copy(), None
        self.U0, self.V0 = U.copy(), V.copy()

    def pmf_fit(self, n_epochs, lr, reg, gamma, variant):
        self.pU, self.pV, loss, self.caches = pc.pmf_fit(self.rid, self.cid, self.val, self.pU, self.pV, n_epochs, reg, lr,
                                                         gamma, variant, caches=self.caches)
        self.call = dict(n_epochs=n_epochs, lr=lr, reg=reg, gamma=gamma, variant=variant)
        return loss

    def pmf_get_factors(self):
        return self.pU.copy(), self.pV.copy()


@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "MfTrainer", FakePmfTrainer)
    monkeypatch.chdir(tmp_path)


@pytest.fixture(scope="module")
def ds():
    return synth_dataset(60, 40, 700, seed=4)


KW = dict(k=5, max_iter=2, learning_rate=0.005, lambda_reg=0.01, seed=123)


def test_constructor_defaults_are_the_references():
    m = PMF()
    assert (m.k, m.max_iter, m.learning_rate, m.gamma, m.lambda_reg, m.name, m.variant, m.trainable, m.verbose, m.seed) == \
        (5, 100, 0.001, 0.9, 0.001, "PMF", "non_linear", True, False, None)
    assert m.U is None and m.V is None and m.init_params == {}
    assert isinstance(m, Recommender)


def test_init_draws_U_then_V_in_double_from_one_generator(device_double, ds):
    m = PMF(**KW).fit(ds)
    rs = np.random.RandomState(123)
    U0 = rs.normal(0.0, 0.001, (ds.num_users, 5))
    V0 = rs.normal(0.0, 0.001, (ds.num_items, 5))
    t = FakePmfTrainer.last
    assert np.array_equal(t.U0, U0) and np.array_equal(t.V0, V0) and t.U0.dtype == np.float64
    assert t.call == dict(n_epochs=2, lr=0.005, reg=0.01, gamma=0.9, variant="non_linear")
    assert m.U.dtype == np.float64 and m.U.shape == (ds.num_users, 5) and m.V.shape == (ds.num_items, 5)
    assert len(m.loss_history) == 2
    # init_params: the given table is used, only the missing one is drawn (first draw of the generator)
    Ugiven = np.full((ds.num_users, 5), 0.01)
    PMF(init_params={"U": Ugiven}, **KW).fit(ds)
    t = FakePmfTrainer.last
    assert np.array_equal(t.U0, Ugiven)
    assert np.array_equal(t.V0, np.random.RandomState(123).normal(0.0, 0.001, (ds.num_items, 5)))


def test_ratings_are_rescaled_for_the_non_linear_variant_only(device_double, ds):
    raw = np.asarray(ds.uir_tuple[2], np.float32)
    assert [ds.min_rating, ds.max_rating] == [1, 5]
    PMF(variant="linear", **KW).fit(ds)
    assert np.array_equal(FakePmfTrainer.last.val, raw) and FakePmfTrainer.last.val.dtype == np.float32
    PMF(variant="non_linear", **KW).fit(ds)
    assert np.array_equal(FakePmfTrainer.last.val, ((raw - 1.0) / 4.0).astype(np.float32))
    assert np.array_equal(FakePmfTrainer.last.rid, ds.uir_tuple[0]) and np.array_equal(FakePmfTrainer.last.cid, ds.uir_tuple[1])
    # a [0, 1] range is handed over as it is
    from cornac_amd import Dataset

    u, i, r = ds.uir_tuple
    ds01 = Dataset.from_uir([(int(a), int(b), float(c > 3)) for a, b, c in zip(u, i, r)], seed=1)
    assert [ds01.min_rating, ds01.max_rating] == [0, 1]
    PMF(variant="non_linear", **KW).fit(ds01)
    assert set(np.unique(FakePmfTrainer.last.val)) == {0.0, 1.0}


def test_unknown_variant_raises_in_fit(device_double, ds):
    with pytest.raises(ValueError, match="variant must be one of"):
        PMF(variant="cubic", **KW).fit(ds)


def test_score_branches_and_exceptions(device_double, ds):
    for variant in pc.VARIANTS:
        m = PMF(variant=variant, **dict(KW, max_iter=3)).fit(ds)
        raw = m.V @ m.U[7]
        assert np.allclose(m.score(7), raw, rtol=1e-12, atol=0) and m.score(7).dtype == np.float64
        one = m.score(7, 11)
        if variant == "linear":
            assert one == m.V[11].dot(m.U[7])
        else:   # the asymmetry of recom_pmf.py:215-222: sigmoid, then mapped back to the rating range
            want = 1.0 / (1.0 + np.exp(-m.V[11].dot(m.U[7]))) * (5.0 - 1.0) + 1.0
            assert one == pytest.approx(want, rel=1e-15) and 1.0 <= one <= 5.0
        for bad in ((ds.num_users, None), (-1, None), (0, ds.num_items), (0, -1)):
            with pytest.raises(ScoreException):
                m.score(*bad)
        ranked, scores = m.rank(7, k=10)
        assert np.array_equal(scores, m.score(7)) and len(ranked) == ds.num_items
        assert np.array_equal(ranked, np.lexsort((np.arange(ds.num_items), raw))[::-1])
        assert m.get_vector_measure() == "dot" and m.get_user_vectors() is m.U and m.get_item_vectors() is m.V


def test_clone_pickle_and_pretrained(device_double, ds, tmp_path):
    m = PMF(variant="linear", gamma=0.8, **KW).fit(ds)
    c = m.clone()
    assert (c.k, c.gamma, c.variant, c.seed, c.max_iter) == (5, 0.8, "linear", 123, 2) and c.U is None and not c.is_fitted
    assert m.clone({"k": 7}).k == 7
    path = m.save(str(tmp_path))
    back = PMF.load(path)
    assert np.array_equal(back.U, m.U) and np.array_equal(back.V, m.V) and back.trainable is False
    assert np.array_equal(back.score(3), m.score(3))
    again = pickle.loads(pickle.dumps(m))
    assert np.array_equal(again.V, m.V) and not hasattr(again, "train_set")
    # trainable=False: the given tables serve as they are, nothing reaches the device
    FakePmfTrainer.last = None
    pre = PMF(trainable=False, init_params={"U": m.U.copy(), "V": m.V.copy()}, **KW).fit(ds)
    assert FakePmfTrainer.last is None and np.array_equal(pre.U, m.U) and np.array_equal(pre.score(3), m.score(3))
    # a refit continues from the learned tables (recom_pmf.py:141) with fresh caches
    m2 = PMF(variant="linear", **KW).fit(ds)
    U1 = m2.U.copy()
    with pytest.warns(UserWarning):
        m2.fit(ds)
    assert np.array_equal(FakePmfTrainer.last.U0, U1)


def test_first_example_wiring_mf_pmf_bpr(device_double, capsys):
    """the reference's first README example: RatioSplit + Experiment over [MF, PMF, BPR]"""
    rs = np.random.RandomState(8)
    keys = rs.permutation(70 * 50)[:1500]
    data = [("u%d" % (k // 50), "i%d" % (k % 50), float(rs.randint(1, 6))) for k in keys]
    split = RatioSplit(data, test_size=0.2, rating_threshold=4.0, seed=123)
    models = [MF(k=10, max_iter=5, learning_rate=0.01, lambda_reg=0.02, use_bias=True, seed=123),
              PMF(k=10, max_iter=5, learning_rate=0.001, lambda_reg=0.001, seed=123),
              BPR(k=10, max_iter=5, learning_rate=0.001, lambda_reg=0.01, seed=123)]
    ex = Experiment(split, models, [mm.MAE(), mm.RMSE(), mm.Recall(k=20), mm.Precision(k=20)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["MF", "PMF", "BPR"]
    row = ex.result[1].metric_avg_results
    assert {"MAE", "RMSE", "Recall@20", "Precision@20"} <= set(row) and all(np.isfinite(v) for v in row.values())
    assert 0.0 < row["RMSE"] < 4.0 and 0.0 <= row["Recall@20"] <= 1.0
    capsys.readouterr()


def test_adopts_the_reference_base_class_where_it_is_loaded(device_double):
    from oracle import ref_loader

    if not ref_loader.available():
        pytest.skip("reference not available / oracle/_ref not built")
    import cornac_amd as ca

    ns = ref_loader.load()
    assert ca.adopt_reference_classes()
    assert isinstance(PMF(), ns.Recommender)


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_pmf_entry_points():
    names = ["cornac_hip_mf_pmf_set_factors", "cornac_hip_mf_pmf_get_factors", "cornac_hip_mf_pmf_fit", "cornac_hip_mf_pmf_form"]
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in names:
        assert re.search(r"\bint %s\s*\(cornac_hip_mf_t h" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    assert "#define CORNAC_HIP_PMF_LINEAR 0" in header and "#define CORNAC_HIP_PMF_NON_LINEAR 1" in header
    assert _lib.MfTrainer.PMF_VARIANTS == {"linear": 0, "non_linear": 1}
    # argument checks need no device: a NULL handle is refused with the invalid-argument status
    assert _lib.lib().cornac_hip_mf_pmf_fit(None, 1, 0.1, 0.1, 0.9, 0, None) == 1
