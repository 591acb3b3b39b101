"""VAECF without a GPU: (1) the float64 restatement (tests/vaecf_cases.py) against what the reference's own VAE / learn wrote
into tests/golden/vaecf_ref.npz; (2) the host logic of cornac_amd.VAECF through a device double that calls the restatement;
(3) the ABI entry points are declared and bound.

(1) Bound: twice the distance recorded in vaecf_cases.RESTATEMENT_VS_REFERENCE.  Measured here, max over the ten tables of
|restatement - reference float32|: i257 6.54e-08, al/tanh/mult 8.81e-08, sat 4.65e-07 (the tables moved 5.5e-3 to 9e-3);
Adam's exp_avg within 4.2e-07 and exp_avg_sq within 5.7e-08 of the reference's (both in the saturated case; 3.5e-08 and
4.1e-10 otherwise); per-step losses within 1.3e-07 relative (bound 2e-5: a float32 sum of n_items <= 257 terms,
257 * 2^-24); the reference's scores within 5.6e-07 relative of the restatement's at the reference's tables (bound
64 * 2^-24 * (1 + max|logit|), the device's own)."""
import inspect
import os
import pickle
import re
import warnings

import numpy as np
import pytest

import fake_device
import vaecf_cases as vc
from conftest import ROOT, load_golden
from cornac_amd import VAECF, Experiment, RatioSplit, Recommender, ScoreException, _lib
from cornac_amd import metrics as mm


@pytest.fixture(scope="module")
def golden():
    return load_golden("vaecf_ref")


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases_the_issue_counts(golden):
    assert sorted(golden["cases"]) == sorted(vc.CASES)
    C = vc.CASES.values()
    assert {1, 63, 64, 65, 257, 1031} <= {c["ni"] for c in C} and {1, 20, 64, 65} <= {c["h"] for c in C}
    assert {1, 10, 33} <= {c["k"] for c in C} and {1, 16, 100} <= {c["bs"] for c in C}
    assert {(c["act"], c["lik"]) for n, c in vc.CASES.items() if n.startswith("al/")} == {(a, l) for a in vc.ACTS for l in vc.LIKELIHOODS}
    assert max(c["ni"] for c in C) <= 1100
    for name, c in vc.CASES.items():
        assert vc.n_steps(c) >= 3 and c["epochs"] >= 2 and (c["bs"] == 1 or c["nu"] % c["bs"] != 0), name
        for kind in ("d_ref", "d_ref_m", "d_ref_v", "move", "max", "max_m", "max_v"):
            assert golden["%s/%s" % (name, kind)].shape == (10,) and np.isfinite(golden["%s/%s" % (name, kind)]).all()
        share = vc.check_condition(golden, name)
        print("%s: the device's tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
        X = vc.case_matrix(c)
        if c["ni"] >= 8:
            T = X.tocsc()
            assert T[:, 1].nnz == 0 and sorted(T[:, 2].indices) == [0, 1] and X[3].nnz == 1 and (X.data == 0).sum() == 1
    M = vc.dataset("i257").matrix
    assert M.nnz == vc.case_matrix(vc.CASES["i257"]).nnz and (M.data == 0).sum() == 1, "the Dataset keeps the stored zero stored"
    for name in vc.FULL_CASES:
        c = vc.CASES[name]
        assert golden[name + "/scores"].shape == (len(vc.score_users(c)), c["ni"]) and golden[name + "/losses"].shape == (vc.n_steps(c),)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vaecf_ref.npz")) < 300 * 1024
    c = vc.CASES["sat"]
    r = vc.Restatement(vc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"], vc.case_params(c))
    p = r.forward(r.B, vc.case_noise(c)[0])["p"]
    assert (p[r.B > 0] < 1e-6).any() and p[r.B > 0].min() > 1e-12, "saturated: EPS = 1e-10 shows next to some held item's p"


@pytest.mark.parametrize("name", vc.FULL_CASES)
def test_restatement_against_the_references_tables(golden, name):
    c = vc.CASES[name]
    r, losses, init = vc.run_case(name)
    recorded = vc.RESTATEMENT_VS_REFERENCE[name]
    worst = {}
    for kind, mine in (("P", r.P), ("M", r.M), ("V", r.V)):
        worst[kind] = max(float(np.abs(golden["%s/%s/%s" % (name, kind, vc.SHORT[n])].astype(np.float64) - mine[n]).max()) for n in vc.NAMES)
    move = min(float(np.abs(r.P[n] - init[n]).max()) for n in vc.NAMES)
    rel = float(np.max(np.abs(losses - golden[name + "/losses"]) / np.abs(losses)))
    print("%s: max|restatement - reference| tables %.3g (recorded %.3g, bound twice that), exp_avg %.3g, exp_avg_sq %.3g; the tables "
          "moved at least %.3g; losses %.3g relative (bound 2e-5)" % (name, worst["P"], recorded, worst["M"], worst["V"], move, rel))
    assert worst["P"] <= 2 * recorded and worst["P"] < 1e-3 * move
    assert np.allclose(golden[name + "/d_ref"], [np.abs(golden["%s/P/%s" % (name, vc.SHORT[n])].astype(np.float64) - r.P[n]).max()
                                                for n in vc.NAMES], rtol=1e-3, atol=1e-12)
    assert worst["M"] <= 2 * golden[name + "/d_ref_m"].max() + 1e-12 and worst["V"] <= 2 * golden[name + "/d_ref_v"].max() + 1e-14
    assert rel <= 2e-5
    # the reference's own score() at its own tables
    ref = vc.Restatement(vc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"],
                         {n: golden["%s/P/%s" % (name, vc.SHORT[n])] for n in vc.NAMES})
    users, (pu, pi) = vc.score_users(c), vc.score_pairs(c)
    want = ref.scores(users)
    srel = float(np.max(np.abs(golden[name + "/scores"] - want) / want))
    print("%s: the reference's scores vs the restatement's at the same tables: %.3g relative (bound 64 * 2^-24 * (1 + max|logit|) = %.3g)" % (
        name, srel, 64 * 2.0 ** -24 * (1 + np.abs(ref.logits(users)).max())))
    assert srel <= 64 * 2.0 ** -24 * (1 + np.abs(ref.logits(users)).max())
    assert np.allclose(golden[name + "/pair_scores"], ref.scores(pu)[np.arange(len(pu)), pi], rtol=1e-4, atol=0)


def test_restatement_gradients_are_the_loss_slopes():
    """the hand-written backward against central differences of the restatement's own loss, all likelihoods"""
    for lik in vc.LIKELIHOODS:
        c = vc.CASES["al/elu/" + lik]
        X, eps = vc.case_matrix(c), vc.case_noise(c)[0][:c["bs"]]
        base = vc.Restatement(X, c["k"], c["h"], c["act"], lik, vc.case_params(c))

        def loss(params):
            r = vc.Restatement(X, c["k"], c["h"], c["act"], lik, params)
            return r.step(0, c["bs"], eps, 0.0, c["beta"])

        one = vc.Restatement(X, c["k"], c["h"], c["act"], lik, vc.case_params(c))
        one.step(0, c["bs"], eps, 0.0, c["beta"])
        rs = np.random.RandomState(4)
        for n in vc.NAMES:
            idx = tuple(rs.randint(s) for s in base.P[n].shape)
            if n == vc.NAMES[0]:
                idx = (idx[0], 5)   # an item somebody of the batch may hold
            up, dn = ({m: a.copy() for m, a in base.P.items()} for _ in range(2))
            up[n][idx] += 1e-6
            dn[n][idx] -= 1e-6
            slope, g = (loss(up) - loss(dn)) / 2e-6, one.M[n][idx] / 0.1   # (m after one step is 0.1 g)
            assert abs(slope - g) <= 1e-6 * max(1.0, abs(g)) + 1e-8, (lik, n, slope, g)


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "VaecfModel", vc.FakeVaecfModel)
    monkeypatch.chdir(tmp_path)
    vc.FakeVaecfModel.built, vc.FakeVaecfModel.last = 0, None


KW = dict(k=5, autoencoder_structure=[7], n_epochs=2, batch_size=16, seed=9)


def test_constructor_is_the_references():
    m = VAECF()
    assert (m.name, m.k, m.autoencoder_structure, m.act_fn, m.likelihood, m.n_epochs, m.batch_size, m.learning_rate, m.beta,
            m.trainable, m.verbose, m.seed, m.use_gpu, m.device) == ("VAECF", 10, [20], "tanh", "mult", 100, 100, 0.001, 1.0, True,
                                                                      False, None, False, 0)
    assert list(inspect.signature(VAECF.__init__).parameters)[1:] == [
        "name", "k", "autoencoder_structure", "act_fn", "likelihood", "n_epochs", "batch_size", "learning_rate", "beta", "trainable",
        "verbose", "seed", "use_gpu", "device"]
    assert isinstance(m, Recommender) and not m.is_fitted and not hasattr(m, "vae")
    c = VAECF(use_gpu=True, **KW).clone({"k": 3})
    assert (c.k, c.autoencoder_structure, c.seed, c.use_gpu, c.n_epochs) == (3, [7], 9, True, 2) and not c.is_fitted


def test_seeded_init_is_five_seeded_linear_layers_and_noise_is_randn_per_batch(device_double):
    import torch

    ds = vc.dataset("al/tanh/mult")
    m = VAECF(**KW).fit(ds)
    fake = vc.FakeVaecfModel.last
    torch.manual_seed(9)
    layers = [torch.nn.Linear(*io) for io in ((131, 7), (7, 5), (7, 5), (5, 7), (7, 131))]
    want_noise = [np.concatenate([torch.randn(b, 5).numpy() for b in (16, 16, 5)]) for _ in range(2)]
    init = {}
    for q, layer in enumerate(layers):
        init[vc.NAMES[2 * q]], init[vc.NAMES[2 * q + 1]] = layer.weight.detach().numpy(), layer.bias.detach().numpy()
    assert fake.epochs == 2 and all(np.array_equal(a, b) for a, b in zip(fake.noise, want_noise))
    r = vc.Restatement(ds.matrix, 5, 7, "tanh", "mult", init)
    losses = [r.fit_epoch(16, 0.001, 1.0, e).sum() / 37 for e in want_noise]
    assert list(m.vae) == list(vc.NAMES) and all(a.dtype == np.float32 for a in m.vae.values())
    assert all(np.array_equal(m.vae[n], r.P[n].astype(np.float32)) for n in vc.NAMES)
    assert np.allclose(m.loss_history, losses, rtol=1e-12)
    again = VAECF(**KW).fit(ds)
    assert all(np.array_equal(m.vae[n], again.vae[n]) for n in vc.NAMES), "a seeded fit repeats itself"
    # without a seed: the device generator, a seed of its own per fit, no host noise
    free = VAECF(**dict(KW, seed=None)).fit(ds)
    assert vc.FakeVaecfModel.last.epochs == 2 and np.isfinite(free.vae[vc.NAMES[0]]).all()


def test_refit_continues_and_trainable_false_trains_nothing(device_double):
    ds = vc.dataset("al/tanh/mult")
    m = VAECF(**KW).fit(ds)
    first = {n: a.copy() for n, a in m.vae.items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(ds)
    fake = vc.FakeVaecfModel.last
    assert fake.r.t == 6, "a new Adam per fit, as learn() builds one"
    r = vc.Restatement(ds.matrix, 5, 7, "tanh", "mult", first)
    for e in fake.noise:
        r.fit_epoch(16, 0.001, 1.0, e)
    assert all(np.array_equal(m.vae[n], r.P[n].astype(np.float32)) for n in vc.NAMES), "the second fit starts from the first's weights"
    assert not np.array_equal(m.vae[vc.NAMES[0]], first[vc.NAMES[0]])
    built = vc.FakeVaecfModel.built
    frozen = VAECF(trainable=False, **KW)
    frozen.load_state_dict(m.state_dict())
    frozen.r_mat = ds.matrix
    frozen.fit(ds)
    assert vc.FakeVaecfModel.built == built and all(np.array_equal(frozen.vae[n], m.vae[n]) for n in vc.NAMES)
    assert np.array_equal(frozen.score(4), m.score(4))


def test_refusals(device_double):
    ds = vc.dataset("al/tanh/mult")
    for structure in ([], [20, 10]):
        with pytest.raises(NotImplementedError, match="length 1"):
            VAECF(autoencoder_structure=structure).fit(ds)
    with pytest.raises(ValueError, match="act_fn"):
        VAECF(act_fn="gelu").fit(ds)
    with pytest.raises(ValueError, match="likelihoods"):
        VAECF(likelihood="zinb").fit(ds)
    assert vc.FakeVaecfModel.built == 0, "refused before anything reaches the device"
    m = VAECF(**KW).fit(ds)
    for bad in (37, -1):
        with pytest.raises(ScoreException, match="user"):
            m.score(bad)
        with pytest.raises(ScoreException, match="user"):
            m.score(bad, 3)
        with pytest.raises(ScoreException):
            m.score_batch([0, bad])
    for bad in (131, -1):
        with pytest.raises(ScoreException, match="item"):
            m.score(0, bad)
    assert m.rate(37, 0) == m.default_score()
    got = m.rate_batch(np.array([0, 37, 2]), np.array([1, 2, 131]), clipping=False)
    assert got[0] == m.score(0, 1) and got[1] == got[2] == m.default_score()
    with pytest.raises(KeyError):
        m.load_state_dict({"encoder.fc0.weight": np.zeros((7, 131))})
    bad = m.state_dict()
    bad[vc.NAMES[8]] = np.zeros((130, 7), np.float32)
    with pytest.raises(ValueError, match="decoder.fc1.weight"):
        m.load_state_dict(bad)


def test_state_dict_round_trip_save_load_pickle(device_double, tmp_path):
    import torch

    ds = vc.dataset("al/tanh/mult")
    m = VAECF(**KW).fit(ds)
    sd = m.state_dict()
    assert list(sd) == list(vc.NAMES) and all(sd[n].shape == vc.shapes(131, 5, 7)[n] and sd[n] is not m.vae[n] for n in vc.NAMES)
    s4 = m.score(4)
    assert s4.dtype == np.float32 and s4.shape == (131,) and abs(float(s4.sum()) - 1.0) < 1e-5
    assert s4[9] == m.score(4, 9) == m.score_batch([4])[0][9]
    built = vc.FakeVaecfModel.built
    other = VAECF(**KW)
    other.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})   # tensors, as the reference's state_dict holds
    other.fit.__func__   # (not fitted: scoring needs r_mat and the dataset facts)
    other.r_mat, other.num_users, other.num_items = ds.matrix, 37, 131
    assert np.array_equal(other.score(4), s4) and vc.FakeVaecfModel.built == built + 1
    again = pickle.loads(pickle.dumps(m))
    assert "_vae_handle" not in again.__dict__ and not hasattr(again, "train_set") and np.array_equal(again.score(4), s4)
    back = VAECF.load(m.save(str(tmp_path)))
    assert back.trainable is False and "_vae_handle" not in back.__dict__ and "_scorer" not in back.__dict__
    assert all(np.array_equal(back.vae[n], m.vae[n]) for n in vc.NAMES) and np.array_equal(back.score_batch([4, 5]), m.score_batch([4, 5]))
    # an edited table reaches the device
    m.vae[vc.NAMES[9]] = m.vae[vc.NAMES[9]] + np.float32(1.0) * (np.arange(131) % 2).astype(np.float32)
    assert not np.array_equal(m.score(4), s4)
    from oracle import ref_loader

    if ref_loader.available():   # the arrays load into the reference's VAE and back
        import importlib

        ref_loader.load()
        vae = importlib.import_module("cornac.models.vaecf.vaecf").VAE(5, [131, 7], "tanh", "mult")
        vae.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})
        fresh = VAECF(**KW)
        fresh.load_state_dict(vae.state_dict())
        assert all(np.array_equal(fresh.vae[n], sd[n]) for n in vc.NAMES)


def test_scoring_tables_order_items_as_score_does(device_double):
    ds = vc.dataset("i257")
    m = VAECF(k=10, autoencoder_structure=[20], n_epochs=1, batch_size=100, seed=2).fit(ds)
    U, V, ib, ub = m._scoring_tables()
    assert U.shape == (250, 20) and V is m.vae[vc.NAMES[8]] and ib is m.vae[vc.NAMES[9]] and (ub == 0).all()
    assert m._scoring_tables()[0] is U, "cached: the fused scorer is not rebuilt per call"
    for u in (0, 3, 249):
        s = m.score(u).astype(np.float64)
        logits = V.astype(np.float64) @ U[u] + ib
        assert np.array_equal(np.argsort(-logits, kind="stable"), np.argsort(-s, kind="stable")) or len(np.unique(s)) < len(s)
        ranked, scores = m.rank(u)
        assert np.array_equal(scores, m.score(u)) and np.array_equal(ranked[:10], np.argsort(-logits, kind="stable")[:10])
    items, _ = m.rank_batch([0, 3, 249], k=10)
    assert all(np.array_equal(items[r], m.rank(u)[0][:10]) for r, u in enumerate((0, 3, 249)))


def _feedback(seed=8):
    rs = np.random.RandomState(seed)
    keys = rs.permutation(50 * 30)[:600]
    return [("u%d" % (k // 30), "i%d" % (k % 30), float(rs.randint(1, 6))) for k in keys]


def test_experiment_with_ratio_split(device_double, capsys):
    split = RatioSplit(_feedback(), test_size=0.2, exclude_unknowns=True, seed=123, verbose=False)
    models = [VAECF(k=4, autoencoder_structure=[6], n_epochs=3, batch_size=16, seed=1),
              VAECF(k=4, autoencoder_structure=[6], n_epochs=3, batch_size=16, seed=1, likelihood="bern", act_fn="relu", name="VAECF-bern")]
    ex = Experiment(split, models, [mm.Recall(k=10), mm.NDCG(k=10)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["VAECF", "VAECF-bern"]
    for r in ex.result:
        assert 0.0 < r.metric_avg_results["Recall@10"] <= 1.0
    capsys.readouterr()


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------------
VAECF_SYMBOLS = ["cornac_hip_vaecf_create", "cornac_hip_vaecf_destroy", "cornac_hip_vaecf_set_params", "cornac_hip_vaecf_get_params",
                 "cornac_hip_vaecf_get_state", "cornac_hip_vaecf_reset_optimizer", "cornac_hip_vaecf_fit_epoch",
                 "cornac_hip_vaecf_encode_users", "cornac_hip_vaecf_score_users", "cornac_hip_vaecf_score_pairs"]


def test_abi_declares_and_binds_the_vaecf_entry_points():
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in VAECF_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    section = header[header.index("VAECF (Liang et al. 2018"):]
    assert "vaecf.py" in section and "recom_vaecf.py" in section
    assert "vaecf.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    # argument checks need no device: NULL handles are refused with the invalid-argument status
    L = _lib.lib()
    assert L.cornac_hip_vaecf_set_params(None, None) == 1 and L.cornac_hip_vaecf_get_params(None, None) == 1
    assert L.cornac_hip_vaecf_get_state(None, None, None, None) == 1 and L.cornac_hip_vaecf_reset_optimizer(None) == 1
    assert L.cornac_hip_vaecf_fit_epoch(None, 1, 0.1, 1.0, None, 0, None, None) == 1
    assert L.cornac_hip_vaecf_encode_users(None, None, 0, None) == 1 and L.cornac_hip_vaecf_score_users(None, None, 0, None) == 1
    assert L.cornac_hip_vaecf_score_pairs(None, None, None, 0, None) == 1 and L.cornac_hip_vaecf_destroy(None) == 0
    X = vc.case_matrix(vc.CASES["b1"])
    for kw, text in ((dict(k=257, h=4), "1 <= k <= 256"), (dict(k=4, h=1025), "1 <= h <= 1024")):
        with pytest.raises(_lib.HipError, match=text):
            _lib.VaecfModel(X, **kw)
    bad = X.copy()
    bad.indices[:2] = bad.indices[:2][::-1].copy()
    if X.indptr[1] >= 2:
        bad.has_sorted_indices = True
        with pytest.raises(_lib.HipError, match="sorted indices"):
            _lib.VaecfModel(bad, 2, 3)
