"""BiVAECF without a GPU: (1) the float64 restatement (tests/bivae_cases.py) against what the reference's own BiVAE / learn
wrote into tests/golden/bivae_ref.npz; (2) the host logic of cornac_amd.BiVAECF through a device double that calls the
restatement; (3) the ABI entry points are declared and bound.

(1) Bound: twice the distance recorded in bivae_cases.RESTATEMENT_VS_REFERENCE.  Measured here, max over the 12 tables of
|restatement - reference float32|: i257 3.25e-08, al/tanh/pois 1.02e-07, sat 9.63e-08 (the tables moved at least 5.3e-3); the
factor tables within 2.5e-07, Adam's exp_avg within 4.1e-07 and exp_avg_sq within 1.1e-07 of the reference's; per-step losses
within 1.5e-07 relative (bound 2e-5: a float32 sum of at most 257 terms per row, 257 * 2^-24); the reference's scores are
held to 64 * 2^-24 * (1 + max|logit|) relative of the restatement's at the reference's tables, the device's own bound.

The golden's batches are consecutive ranges over ALL ids, the case's item that nobody holds included (the reference's
iterators walk only the ids that occur in the training triplets; on a real split these are all ids of the matrix)."""
import inspect
import os
import pickle
import re
import warnings

import numpy as np
import pytest

import bivae_cases as bc
import fake_device
from conftest import ROOT, load_golden
from cornac_amd import BiVAECF, Experiment, RatioSplit, Recommender, ScoreException, _lib
from cornac_amd import metrics as mm
from cornac_amd.bivaecf import BiVAETables


@pytest.fixture(scope="module")
def golden():
    return load_golden("bivae_ref")


def restatement(c, params=None, factors=None):
    return bc.Restatement(bc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"], bc.case_params(c) if params is None else params,
                          bc.case_factors(c) if factors is None else factors)


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases_the_issue_counts(golden):
    assert sorted(golden["cases"]) == sorted(bc.CASES)
    C = bc.CASES.values()
    for side in ("ni", "nu"):   # the other side's table length, on each side
        assert {1, 63, 64, 65, 257, 1031} <= {c[side] for c in C}
    assert any(c["nu"] != c["ni"] for c in C) and {1, 10, 33} <= {c["k"] for c in C} and {64, 65} & {c["k"] for c in C}
    assert {1, 20, 65} <= {c["h"] for c in C} and {1, 16, 100} <= {c["bs"] for c in C}
    assert {(c["act"], c["lik"]) for n, c in bc.CASES.items() if n.startswith("al/")} == {(a, l) for a in bc.ACTS for l in bc.LIKELIHOODS}
    assert max(max(c["ni"], c["nu"]) for c in C) <= 1100
    # the dense pass splits the other side's table into ranges: some case has two ranges or more, on each side
    assert _lib.BIVAE_RANGE == _lib.BivaeModel.RANGE
    assert any(c["nu"] > _lib.BIVAE_RANGE for c in C) and any(c["ni"] > _lib.BIVAE_RANGE for c in C)
    for name, c in bc.CASES.items():
        assert c["epochs"] >= 2 and (c["bs"] == 1 or (c["nu"] % c["bs"] != 0 and c["ni"] % c["bs"] != 0)), name
        for kind, n in (("d_ref", 16), ("d_ref_m", 12), ("d_ref_v", 12), ("move", 12), ("max", 16), ("max_m", 12), ("max_v", 12)):
            assert golden["%s/%s" % (name, kind)].shape == (n,) and np.isfinite(golden["%s/%s" % (name, kind)]).all()
        share = bc.check_condition(golden, name)
        print("%s: the device's tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
        X = bc.case_matrix(c)
        if c["ni"] >= 8:
            T = X.tocsc()
            assert T[:, 1].nnz == 0 and sorted(T[:, 2].indices) == [0, 1] and X[3].nnz == 1 and (X.data == 0).sum() == 1
    M = bc.dataset("i257").matrix
    assert M.nnz == bc.case_matrix(bc.CASES["i257"]).nnz and (M.data == 0).sum() == 1, "the Dataset keeps the stored zero stored"
    for name in bc.FULL_CASES:
        c = bc.CASES[name]
        assert golden[name + "/scores"].shape == (len(bc.score_users(c)), c["ni"]) and golden[name + "/losses"].shape == (sum(bc.n_steps(c)),)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "bivae_ref.npz")) < 300 * 1024
    # saturated: in the first item pass some held entry has p < 1e-6, so EPS = 1e-10 shows next to it
    c = bc.CASES["sat"]
    r = restatement(c)
    p = r.loss_and_gradients("item", 0, c["ni"], bc.case_noise(c)[0][0, 0].astype(np.float64), c["beta"])[2]
    held = r.rows("item") > 0
    print("sat: the smallest p of a held entry in the first item pass is %.3g" % p[held].min())
    assert (p[held] < 1e-6).any() and p[held].min() > 1e-12


@pytest.mark.parametrize("name", bc.FULL_CASES)
def test_restatement_against_the_references_tables(golden, name):
    c = bc.CASES[name]
    r, losses, init = bc.run_case(name)
    recorded = bc.RESTATEMENT_VS_REFERENCE[name]
    worst = {}
    for kind, mine in (("P", r.P), ("M", r.M), ("V", r.V)):
        worst[kind] = max(float(np.abs(golden["%s/%s/%s" % (name, kind, bc.SHORT[n])].astype(np.float64) - mine[n]).max()) for n in bc.NAMES)
    worst["F"] = max(float(np.abs(golden["%s/F/%s" % (name, n)].astype(np.float64) - r.F[n]).max()) for n in bc.FACTORS)
    move = min(float(np.abs(r.P[n] - init[n]).max()) for n in bc.NAMES)
    rel = float(np.max(np.abs(losses - golden[name + "/losses"]) / np.abs(losses)))
    print("%s: max|restatement - reference| tables %.3g (recorded %.3g, bound twice that), factor tables %.3g, exp_avg %.3g, exp_avg_sq "
          "%.3g; the tables moved at least %.3g; losses %.3g relative (bound 2e-5)" % (name, worst["P"], recorded, worst["F"], worst["M"],
                                                                                      worst["V"], move, rel))
    assert worst["P"] <= 2 * recorded and worst["P"] < 1e-3 * move
    mine = [np.abs(golden["%s/P/%s" % (name, bc.SHORT[n])].astype(np.float64) - r.P[n]).max() for n in bc.NAMES] + [
        np.abs(golden["%s/F/%s" % (name, n)].astype(np.float64) - r.F[n]).max() for n in bc.FACTORS]
    assert np.allclose(golden[name + "/d_ref"], mine, rtol=1e-3, atol=1e-12)
    assert worst["M"] <= 2 * golden[name + "/d_ref_m"].max() + 1e-12 and worst["V"] <= 2 * golden[name + "/d_ref_v"].max() + 1e-14
    assert rel <= 2e-5
    assert (r.t["item"], r.t["user"]) == bc.n_steps(c)
    # the reference's own score() at its own tables
    ref = restatement(c, {}, {n: golden["%s/F/%s" % (name, n)] for n in bc.FACTORS})
    users, (pu, pi) = bc.score_users(c), bc.score_pairs(c)
    want = ref.scores(users)
    bound = 64 * 2.0 ** -24 * (1 + np.abs(ref.logits(users)).max())
    srel = float(np.max(np.abs(golden[name + "/scores"] - want) / want))
    print("%s: the reference's scores vs the restatement's at the same tables: %.3g relative (bound %.3g)" % (name, srel, bound))
    assert srel <= bound
    lo, hi = bc.dataset(name).min_rating, bc.dataset(name).max_rating
    assert np.allclose(golden[name + "/pair_scores"], ref.scores(pu)[np.arange(len(pu)), pi] * (hi - lo) + lo, rtol=1e-4, atol=0)


def test_restatement_gradients_are_the_loss_slopes():
    """the hand-written backward against central differences of the restatement's own loss: all likelihoods, both sides"""
    for lik in bc.LIKELIHOODS:
        c = bc.CASES["al/elu/" + lik]
        for side, noise in zip(("item", "user"), bc.case_noise(c)):
            eps = noise[0, 0, :c["bs"]].astype(np.float64)
            base = restatement(c)
            _, G, _ = base.loss_and_gradients(side, 0, c["bs"], eps, c["beta"])
            rs = np.random.RandomState(4)
            for n, g in G.items():
                idx = tuple(rs.randint(s) for s in base.P[n].shape)
                if n.endswith("fc0.weight"):
                    idx = (idx[0], int(np.flatnonzero(base.rows(side)[:c["bs"]].sum(axis=0))[0]))   # a column somebody of the batch holds
                slopes = []
                for sign in (1.0, -1.0):
                    moved = {m: a.copy() for m, a in base.P.items()}
                    moved[n][idx] += sign * 1e-6
                    slopes.append(restatement(c, moved).loss_and_gradients(side, 0, c["bs"], eps, c["beta"])[0])
                slope = (slopes[0] - slopes[1]) / 2e-6
                assert abs(slope - g[idx]) <= 1e-6 * max(1.0, abs(g[idx])) + 1e-8, (lik, side, n, slope, g[idx])
            other = [n for n in bc.NAMES if n not in G]
            assert len(G) == 6 and len(other) == 6, "a step has gradients for its own side's tables only"


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "BivaeModel", bc.FakeBivaeModel)
    monkeypatch.chdir(tmp_path)
    bc.FakeBivaeModel.built, bc.FakeBivaeModel.last = 0, None


KW = dict(k=5, encoder_structure=[7], n_epochs=2, batch_size=16, seed=9)
CASE = "al/tanh/pois"   # 37 users x 131 items


def test_constructor_is_the_references():
    m = BiVAECF()
    assert (m.name, m.k, m.encoder_structure, m.act_fn, m.likelihood, m.n_epochs, m.batch_size, m.learning_rate, m.beta_kl, m.cap_priors,
            m.trainable, m.verbose, m.seed, m.use_gpu, m.device) == ("BiVAECF", 10, [20], "tanh", "pois", 100, 100, 0.001, 1.0,
                                                                      {"user": False, "item": False}, True, False, None, True, 0)
    assert list(inspect.signature(BiVAECF.__init__).parameters)[1:] == [
        "name", "k", "encoder_structure", "act_fn", "likelihood", "n_epochs", "batch_size", "learning_rate", "beta_kl", "cap_priors",
        "trainable", "verbose", "seed", "use_gpu", "device"]
    assert isinstance(m, Recommender) and not m.is_fitted and not hasattr(m, "bivae")
    c = BiVAECF(use_gpu=False, **KW).clone({"k": 3})
    assert (c.k, c.encoder_structure, c.seed, c.use_gpu, c.n_epochs) == (3, [7], 9, False, 2) and not c.is_fitted


def test_seeded_init_is_the_references_construction_order_and_noise_is_two_randn_per_batch(device_double):
    import torch

    ds = bc.dataset(CASE)
    m = BiVAECF(**KW).fit(ds)
    fake = bc.FakeBivaeModel.last
    torch.manual_seed(9)
    theta = torch.randn(37, 5) * 0.01
    beta = torch.randn(131, 5) * 0.01
    torch.nn.init.kaiming_uniform_(theta, a=np.sqrt(5))
    layers = [torch.nn.Linear(*io) for io in ((131, 7), (7, 5), (7, 5), (37, 7), (7, 5), (7, 5))]
    want_noise = []
    for _ in range(2):
        epoch = []
        for n in (131, 37):   # items first
            eps = np.empty((2, n, 5), np.float32)
            for r0 in range(0, n, 16):
                for draw in range(2):   # the training forward's first
                    eps[draw, r0:r0 + 16] = torch.randn(min(16, n - r0), 5).numpy()
            epoch.append(eps)
        want_noise.append(epoch)
    init = {}
    for q, layer in enumerate(layers):
        init[bc.NAMES[2 * q]], init[bc.NAMES[2 * q + 1]] = layer.weight.detach().numpy(), layer.bias.detach().numpy()
    assert np.abs(theta.numpy()).max() <= 1 / np.sqrt(5) and np.abs(theta.numpy()).max() > 0.3, "theta is kaiming-uniform, not 0.01 x normal"
    assert fake.epochs == 2 and fake.inferred == 1
    assert all(np.array_equal(a, b) for got, want in zip(fake.noise, want_noise) for a, b in zip(got, want))
    r = bc.Restatement(ds.matrix, 5, 7, "tanh", "pois", init, dict(theta=theta.numpy(), beta=beta.numpy()))
    history = []
    for ei, eu in want_noise:
        steps = r.fit_epoch(16, 0.001, 1.0, ei, eu)
        history.append((steps[:9].sum() / 131, steps[9:].sum() / 37))
    r.infer_means()
    assert list(m.bivae.tables) == list(bc.NAMES) and all(a.dtype == np.float32 for a in m.bivae.tables.values())
    assert all(np.array_equal(m.bivae.tables[n], r.P[n].astype(np.float32)) for n in bc.NAMES)
    assert all(np.array_equal(getattr(m.bivae, n), r.F[n].astype(np.float32)) and getattr(m.bivae, n).dtype == np.float32 for n in bc.FACTORS)
    assert np.allclose(m.loss_history, history, rtol=1e-12) and np.shape(m.loss_history) == (2, 2)
    assert m.get_user_vectors() is m.bivae.mu_theta and m.get_item_vectors() is m.bivae.mu_beta
    again = BiVAECF(**KW).fit(ds)
    assert all(np.array_equal(m.bivae.tables[n], again.bivae.tables[n]) for n in bc.NAMES), "a seeded fit repeats itself"
    # without a seed: the device generator, a seed of its own per fit, no host noise
    free = BiVAECF(**dict(KW, seed=None)).fit(ds)
    assert bc.FakeBivaeModel.last.noise == [(None, None)] * 2 and np.isfinite(free.bivae.mu_theta).all()


def test_refit_continues_and_trainable_false_trains_nothing(device_double):
    ds = bc.dataset(CASE)
    m = BiVAECF(**KW).fit(ds)
    first = m.bivae
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(ds)
    fake = bc.FakeBivaeModel.last
    assert (fake.r.t["item"], fake.r.t["user"]) == (18, 6), "two new Adam per fit, as learn() builds them"
    r = bc.Restatement(ds.matrix, 5, 7, "tanh", "pois", first.tables, {n: getattr(first, n) for n in bc.FACTORS})
    for ei, eu in fake.noise:
        r.fit_epoch(16, 0.001, 1.0, ei, eu)
    assert all(np.array_equal(m.bivae.tables[n], r.P[n].astype(np.float32)) for n in bc.NAMES), "the second fit starts from the first's tables"
    assert np.array_equal(m.bivae.theta, r.F["theta"].astype(np.float32)), "... and from its factor tables"
    assert not np.array_equal(m.bivae.tables[bc.NAMES[0]], first.tables[bc.NAMES[0]])
    built = bc.FakeBivaeModel.built
    frozen = BiVAECF(trainable=False, **KW)
    frozen.bivae = pickle.loads(pickle.dumps(m.bivae))
    frozen.r_mat = ds.matrix
    frozen.fit(ds)
    assert bc.FakeBivaeModel.built == built and all(np.array_equal(frozen.bivae.tables[n], m.bivae.tables[n]) for n in bc.NAMES)
    assert np.array_equal(frozen.score(4), m.score(4))


def test_refusals(device_double):
    ds = bc.dataset(CASE)
    for structure in ([], [20, 10]):
        with pytest.raises(NotImplementedError, match="length 1"):
            BiVAECF(encoder_structure=structure).fit(ds)
    for priors in ({"user": True, "item": False}, {"user": False, "item": True}, {"user": True, "item": True}):
        with pytest.raises(NotImplementedError, match="standard normal prior"):
            BiVAECF(cap_priors=priors).fit(ds)
    with pytest.raises(ValueError, match="act_fn"):
        BiVAECF(act_fn="gelu").fit(ds)
    with pytest.raises(ValueError, match="likelihoods"):
        BiVAECF(likelihood="mult").fit(ds)
    assert bc.FakeBivaeModel.built == 0, "refused before anything reaches the device"
    m = BiVAECF(**KW).fit(ds)
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
        m.bivae.load_state_dict({"user_encoder.fc0.weight": np.zeros((7, 131))})
    bad = m.bivae.state_dict()
    bad[bc.NAMES[8]] = np.zeros((4, 7), np.float32)
    with pytest.raises(ValueError, match="item_mu.weight"):
        m.bivae.load_state_dict(bad)
    assert m.bivae.tables[bc.NAMES[8]].shape == (5, 7), "a refused state_dict leaves the tables as they were"


def test_state_dict_round_trip_save_load_pickle(device_double, tmp_path):
    import torch

    ds = bc.dataset(CASE)
    m = BiVAECF(**KW).fit(ds)
    sd = m.bivae.state_dict()
    assert list(sd) == list(bc.NAMES) and all(sd[n].shape == bc.shapes(37, 131, 5, 7)[n] and sd[n] is not m.bivae.tables[n] for n in bc.NAMES)
    s4 = m.score(4)
    lo, hi = m.min_rating, m.max_rating
    assert s4.dtype == np.float32 and s4.shape == (131,) and (s4 > 0).all() and (s4 < 1).all()
    assert s4[9] == m.score_batch([4])[0][9] and m.score(4, 9) == np.float64(s4[9]) * (hi - lo) + lo, "a pair goes through the scaling"
    assert lo < hi and lo <= m.score(4, 9) <= hi
    built = bc.FakeBivaeModel.built
    other = BiVAECF(**KW)
    other.bivae = pickle.loads(pickle.dumps(m.bivae))
    other.bivae.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})   # tensors, as the reference's state_dict holds
    other.r_mat, other.num_users, other.num_items = ds.matrix, 37, 131
    assert np.array_equal(other.score(4), s4) and bc.FakeBivaeModel.built == built + 1
    blob = pickle.dumps(m)
    assert b"torch" not in blob and b"FakeBivaeModel" not in blob and b"BivaeModel" not in blob, "no torch object and no handle in the pickle"
    again = pickle.loads(blob)
    assert "_bivae_handle" not in again.__dict__ and not hasattr(again, "train_set") and np.array_equal(again.score(4), s4)
    assert isinstance(again.bivae, BiVAETables) and again.bivae.dims == (37, 131, 5, 7)
    back = BiVAECF.load(m.save(str(tmp_path)))
    assert back.trainable is False and "_bivae_handle" not in back.__dict__ and "_scorer" not in back.__dict__
    assert all(np.array_equal(back.bivae.tables[n], m.bivae.tables[n]) for n in bc.NAMES)
    assert np.array_equal(back.score_batch([4, 5]), m.score_batch([4, 5]))
    # an edited table reaches the device
    m.bivae.mu_beta = m.bivae.mu_beta + np.float32(1.0) * (np.arange(131) % 2).astype(np.float32)[:, None]
    assert not np.array_equal(m.score(4), s4)
    from oracle import ref_loader

    if ref_loader.available():   # the arrays load into the reference's BiVAE and back
        import importlib

        ref_loader.load()
        net = importlib.import_module("cornac.models.bivaecf.bivae").BiVAE(
            k=5, user_encoder_structure=[131, 7], item_encoder_structure=[37, 7], act_fn="tanh", likelihood="pois",
            cap_priors={"user": False, "item": False}, feature_dim={"user": None, "item": None}, batch_size=16)
        net.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})
        assert list(net.state_dict()) == list(bc.NAMES)
        fresh = pickle.loads(pickle.dumps(back.bivae))
        fresh.load_state_dict(net.state_dict())
        assert all(np.array_equal(fresh.tables[n], sd[n]) for n in bc.NAMES)


def test_scoring_tables_order_items_as_score_does(device_double):
    ds = bc.dataset("i257")
    m = BiVAECF(k=10, encoder_structure=[20], n_epochs=1, batch_size=100, seed=2).fit(ds)
    U, V, ib, ub = m._scoring_tables()
    assert U is m.bivae.mu_theta and V is m.bivae.mu_beta and U.shape == (250, 10) and V.shape == (257, 10) and (ib == 0).all() and (ub == 0).all()
    assert m._scoring_tables()[2] is ib, "cached: the fused scorer is not rebuilt per call"
    for u in (0, 3, 249):
        s = m.score(u).astype(np.float64)
        logits = V.astype(np.float64) @ U[u]
        assert np.array_equal(np.argsort(-logits, kind="stable"), np.argsort(-s, kind="stable")) or len(np.unique(s)) < len(s)
        ranked, scores = m.rank(u)
        assert np.array_equal(scores, m.score(u)) and np.array_equal(ranked[:10], np.argsort(-logits, kind="stable")[:10])
    items, _ = m.rank_batch([0, 3, 249], k=10)
    assert all(np.array_equal(items[r], m.rank(u)[0][:10]) for r, u in enumerate((0, 3, 249)))


def test_rank_case_has_distinct_top_probabilities(golden):
    """the case test_bivaecf_gpu.py ranks on: at the reference's tables at least 90 % of the users have 21 distinct top
    float32 probabilities"""
    name = "i257"
    c = bc.CASES[name]
    r = restatement(c, {}, {n: golden["%s/F/%s" % (name, n)] for n in bc.FACTORS})
    S = r.scores(np.arange(c["nu"])).astype(np.float32)
    top = -np.sort(-S.astype(np.float64), axis=1)[:, :21]
    clear = (np.diff(top, axis=1) < 0).all(axis=1)
    print("%d of %d users have 21 distinct top probabilities" % (clear.sum(), len(clear)))
    assert clear.sum() >= 0.9 * c["nu"]


def _feedback(seed=8):
    rs = np.random.RandomState(seed)
    keys = rs.permutation(50 * 30)[:600]
    return [("u%d" % (k // 30), "i%d" % (k % 30), float(rs.randint(1, 6))) for k in keys]


def test_experiment_with_ratio_split(device_double, capsys):
    split = RatioSplit(_feedback(), test_size=0.2, exclude_unknowns=True, seed=123, verbose=False)
    models = [BiVAECF(k=4, encoder_structure=[6], n_epochs=3, batch_size=16, seed=1),
              BiVAECF(k=4, encoder_structure=[6], n_epochs=3, batch_size=16, seed=1, likelihood="bern", act_fn="relu", name="BiVAECF-bern")]
    ex = Experiment(split, models, [mm.Recall(k=10), mm.NDCG(k=10), mm.RMSE()], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["BiVAECF", "BiVAECF-bern"]
    for r in ex.result:
        assert 0.0 < r.metric_avg_results["Recall@10"] <= 1.0 and np.isfinite(r.metric_avg_results["RMSE"])
    capsys.readouterr()


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------------
BIVAE_SYMBOLS = ["cornac_hip_bivae_create", "cornac_hip_bivae_destroy", "cornac_hip_bivae_set_params", "cornac_hip_bivae_get_params",
                 "cornac_hip_bivae_set_factors", "cornac_hip_bivae_get_factors", "cornac_hip_bivae_get_state",
                 "cornac_hip_bivae_reset_optimizer", "cornac_hip_bivae_fit_epoch", "cornac_hip_bivae_last_timing", "cornac_hip_bivae_infer_means",
                 "cornac_hip_bivae_score_users", "cornac_hip_bivae_score_pairs"]


def test_abi_declares_and_binds_the_bivae_entry_points():
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in BIVAE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    assert sorted(s for s in _lib.SYMBOLS if s.startswith("cornac_hip_bivae_")) == sorted(BIVAE_SYMBOLS)
    section = header[header.index("BiVAECF (Truong"):]
    assert "bivae.py" in section and "recom_bivaecf.py" in section
    assert int(re.search(r"#define CORNAC_HIP_BIVAE_RANGE (\d+)", header).group(1)) == _lib.BIVAE_RANGE
    assert "bivae.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    assert _lib.BivaeModel.NAMES == bc.NAMES and _lib.BivaeModel.FACTORS == bc.FACTORS
    assert _lib.BivaeModel.ACTS == bc.ACTS and _lib.BivaeModel.LIKELIHOODS == bc.LIKELIHOODS
    assert _lib.BivaeModel.shapes(37, 131, 5, 7) == bc.shapes(37, 131, 5, 7)
    # argument checks need no device: NULL handles are refused with the invalid-argument status
    L = _lib.lib()
    assert L.cornac_hip_bivae_set_params(None, None) == 1 and L.cornac_hip_bivae_get_params(None, None) == 1
    assert L.cornac_hip_bivae_set_factors(None, None, None, None, None) == 1 and L.cornac_hip_bivae_get_factors(None, None, None, None, None) == 1
    assert L.cornac_hip_bivae_get_state(None, None, None, None, None) == 1 and L.cornac_hip_bivae_reset_optimizer(None) == 1
    assert L.cornac_hip_bivae_fit_epoch(None, 1, 0.1, 1.0, None, None, 0, None, None, None) == 1 and L.cornac_hip_bivae_infer_means(None) == 1
    assert L.cornac_hip_bivae_last_timing(None, None, None) == 1
    assert L.cornac_hip_bivae_score_users(None, None, 0, None) == 1 and L.cornac_hip_bivae_score_pairs(None, None, None, 0, None) == 1
    assert L.cornac_hip_bivae_destroy(None) == 0
    X = bc.case_matrix(bc.CASES["b1"])
    for kw, text in ((dict(k=257, h=4), "1 <= k <= 256"), (dict(k=4, h=1025), "1 <= h <= 1024")):
        with pytest.raises(_lib.HipError, match=text):
            _lib.BivaeModel(X, **kw)
    bad = X.copy()
    bad.indices[:2] = bad.indices[:2][::-1].copy()
    if X.indptr[1] >= 2:
        bad.has_sorted_indices = True
        with pytest.raises(_lib.HipError, match="sorted indices"):
            _lib.BivaeModel(bad, 2, 3)
