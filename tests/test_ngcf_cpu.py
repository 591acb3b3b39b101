"""NGCF without a GPU: (1) the float64 restatement of tests/ngcf_cases.py against the golden that the reference's own ngcf.Model,
construct_graph and NGCF.fit wrote (parameters, Adam's state, losses, eval-mode embeddings, scores), the tolerance rule's
condition and the cases' own conditions; (2) the model class's host logic over a device double served by the restatement: the
seeded fit with dropout 0 against the reference's own seeded fit, the draw order, state_dict, save / load, a refit, unknown
ids, early stopping; (3) the ABI and its refusals."""
import ctypes
import inspect
import os
import pickle
import re

import numpy as np
import pytest
import scipy.sparse as sp

import fake_device
import ngcf_cases as nc
from conftest import ROOT, load_golden
from cornac_amd import NGCF, Dataset, Recommender, ScoreException, _lib

STATS = ("d_ref", "d_ref_m", "d_ref_v", "move", "max", "max_m", "max_v")
NAMES_2 = ["layers.0.W1.weight", "layers.0.W1.bias", "layers.0.W2.weight", "layers.0.W2.bias", "layers.1.W1.weight", "layers.1.W1.bias",
           "layers.1.W2.weight", "layers.1.W2.bias", "feature_dict.item", "feature_dict.user"]


@pytest.fixture(scope="module")
def golden():
    return load_golden("ngcf_ref")


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases(golden):
    assert sorted(golden["cases"]) == sorted(list(nc.CASES) + list(nc.SEEDED))
    assert set(nc.CASES) == {"w1", "mixed", "d33", "d64", "d256", "cross", "big", "chunks", "hub", "zero", "l4reg", "lam0"}
    for name, c in nc.CASES.items():
        n_tables = 4 * len(c["layers"]) + 2
        for kind in STATS:
            assert golden["%s/%s" % (name, kind)].shape == (n_tables,) and np.isfinite(golden["%s/%s" % (name, kind)]).all()
        assert int(golden[name + "/finite"]) == 1
        X, batches = nc.case_graph(c), nc.case_batches(c)
        tu, ti = nc.totals(c)
        assert X.shape == (tu, ti) and X.has_sorted_indices and len(batches) == 3 and [len(b[0]) for b in batches] == list(c["steps"])
        deg_u, deg_i = np.diff(X.indptr), np.bincount(X.indices, minlength=ti)
        assert (deg_u[:c["nu"]] > 0).all() and (deg_i[:c["ni"]] > 0).all() and not deg_u[c["nu"]:].any() and not deg_i[c["ni"]:].any()
        later = np.concatenate([b[0] for b in batches[1:]])
        assert batches[0][0][0] == 0 and 0 not in later, "user 0: the first step only"
        assert all((b[1] == 1).sum() * 3 >= len(b[1]) for b in batches if len(b[1]) >= 5), "a third of the positives are item 1"
        assert all(len(np.intersect1d(b[1], b[2])) > 0 for b in batches if len(b[1]) >= 2), "an item is positive and negative in one step"
        assert all(any(abs(a).max() > 0 for n, a in nc.case_params(c).items() if n.endswith("bias")) for _ in (0,)), "non-zero biases"
    c = nc.CASES["mixed"]
    assert (c["emb"], c["layers"], c["drop"], c["iso_u"], c["iso_i"]) == (8, (16, 4, 7), (.1, 0, .5), 2, 1)
    assert (nc.CASES["d64"]["emb"], nc.CASES["d64"]["layers"], nc.CASES["d64"]["drop"]) == (64, (64, 64, 64), (.1, .1, .1))
    assert nc.CASES["cross"]["layers"] == (130, 2) and nc.CASES["d256"]["layers"] == (256,) and nc.CASES["d33"]["layers"] == (65, 33)
    assert nc.CASES["l4reg"]["lam"] == 1e-2 and len(nc.CASES["l4reg"]["layers"]) == 4 and nc.CASES["lam0"]["lam"] == 0.0
    assert nc.CASES["zero"]["layers"] == (1, 8) and nc.CASES["zero"]["drop"] == (.5, 0) and nc.CASES["w1"]["layers"] == (1,)
    print("seeded: %.3g of a table's movement" % nc.check_condition(golden, "seeded"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ngcf_ref.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "lightgcn_ref.npz"))


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_tolerance_stays_under_one_percent_of_the_tables_movement(golden, name):
    share = nc.check_condition(golden, name)
    print("%s: the device's tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))


def test_chunks_and_hub_span_three():
    assert nc.PIECE == _lib.NgcfModel.PIECE == _lib.LightGcnModel.PIECE and nc.WGRAD_ROWS == _lib.NgcfModel.WGRAD_ROWS
    tu, ti = nc.totals(nc.CASES["chunks"])
    assert tu + ti >= 2 * _lib.NgcfModel.WGRAD_ROWS + 1 and (tu + ti) % _lib.NgcfModel.WGRAD_ROWS != 0, "three chunks, the last partial"
    X = nc.case_graph(nc.CASES["hub"])
    hub = int(np.bincount(X.indices)[0])
    assert hub == nc.CASES["hub"]["nu"] and -(-hub // _lib.NgcfModel.PIECE) >= 3
    assert np.diff(X.indptr).max() <= _lib.NgcfModel.PIECE   # (and nothing else is split)


def test_dropout_mask_is_philox():
    """the known answers of Philox4x32-10 (Random123's kat_vectors), then the mask's own properties"""
    got = [int(x) for x in nc.philox4x32_10(0, 0, 0, 0, 0, 0)]
    assert got == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    got = [int(x) for x in nc.philox4x32_10(0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff)]
    assert got == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    a = nc.dropout_mask(nc.KEY, 1, 0, 200, 7, 0.5)
    assert a.shape == (200, 7) and 0.4 < a.mean() < 0.6
    assert np.array_equal(a, nc.dropout_mask(nc.KEY, 1, 0, 200, 7, 0.5))
    assert all(not np.array_equal(a, nc.dropout_mask(*args)) for args in ((nc.KEY + 1, 1, 0, 200, 7, 0.5), (nc.KEY, 2, 0, 200, 7, 0.5),
                                                                         (nc.KEY, 1, 1, 200, 7, 0.5)))
    assert nc.dropout_mask(nc.KEY, 1, 0, 50, 4, 0.0).all() and nc.dropout_mask(nc.KEY, 1, 0, 5000, 4, 0.1).mean() > 0.88
    assert nc.keep_multiplier(0.5) == 2.0 and nc.keep_multiplier(0.1) == float(np.float32(1) / np.float32(0.9))


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_restatement_against_the_reference(golden, name):
    run = nc.run_case(name)
    r = run["r"]
    assert np.isfinite(run["losses"]).all() and r.t == 3 and all(np.isfinite(a).all() for a in r.W.values())
    assert float(golden[name + "/d_ref"][-2:].max()) <= 2e-6
    assert float(golden[name + "/d_ref_loss"]) <= 1e-4
    if name not in nc.FULL_CASES:
        return
    for q, n in enumerate(r.W):
        for kind, mine, stat in (("P", r.W, "d_ref"), ("M", r.M, "d_ref_m"), ("V", r.V, "d_ref_v")):
            d = np.abs(golden["%s/%s/%s" % (name, kind, n)].astype(np.float64) - mine[n]).max()
            assert d == golden["%s/%s" % (name, stat)][q], (name, kind, n, d)
    assert np.abs(golden[name + "/losses"] - run["losses"]).max() == float(golden[name + "/d_ref_loss"])
    E = r.final()
    users = nc.score_users(nc.CASES[name])
    if name == "zero":
        # the one-column layer's weights have a zero gradient by construction (y = +-1); the reference moves them by its own
        # rounding noise (d_ref 2.4e-3), and its layers' outputs follow its weights.  What does not depend on them is held: the
        # X_0 slice of the embeddings, which is the tables themselves
        emb = nc.CASES[name]["emb"]
        for q, n in enumerate(("user", "item")):
            d = np.abs(golden[name + "/E/" + n][:, :emb].astype(np.float64) - E[q][:, :emb]).max()
            assert d <= float(golden[name + "/d_ref"][-2:].max()), (n, d)
        return
    assert max(np.abs(golden[name + "/E/" + n].astype(np.float64) - E[q]).max() for q, n in enumerate(("user", "item"))) <= 1e-4
    assert np.abs(golden[name + "/scores"] - E[0][users] @ E[1].T).max() <= 1e-3


def test_one_column_layers_have_a_zero_gradient():
    """ngcf_cases.one_column: the parameters that check_condition leaves out, and whose comparison on the device is vacuous where
    the reference moved them by noise (zero: tolerance 16 d_ref above their movement).  The restated gradient of every one of
    them is exactly zero at every step, so the restatement leaves them, m and v in place, bit for bit"""
    assert nc.one_column(nc.CASES["w1"]) == ["layers.0.W1.weight", "layers.0.W1.bias", "layers.0.W2.weight", "layers.0.W2.bias"]
    assert nc.one_column(nc.CASES["zero"]) == nc.one_column(nc.CASES["w1"])
    assert [n for c in nc.CASES.values() for n in nc.one_column(c)] == 2 * nc.one_column(nc.CASES["w1"]), "no other case has such a layer"
    for name in ("w1", "zero"):
        c = nc.CASES[name]
        init = nc.case_params(c)
        r = nc.new_restatement(c, init)
        for t, (u, i, j) in enumerate(nc.case_batches(c), 1):
            E, caches = r.forward(t=t)
            g = r.backward(r.gradient_at_E(E, u, i, j, c["lam"]), caches)
            assert all(not g[n].any() for n in nc.one_column(c)), (name, t)
            r.step(u, i, j, c["lr"], c["lam"])
        for n in nc.one_column(c):
            assert np.array_equal(r.W[n], init[n].astype(np.float64)) and not r.M[n].any() and not r.V[n].any()


def test_zero_holds_an_all_zero_activation_row_and_stays_finite(golden):
    c = nc.CASES["zero"]
    r = nc.new_restatement(c, nc.case_params(c))
    _, caches = r.forward(t=1)
    dead = np.flatnonzero(caches[0]["n"] == 0.0)
    assert len(dead) >= 5 and not caches[0]["y"][dead].any(), "rows whose masked activation is all zero: the eps branch"
    u, i, j = nc.case_batches(c)[0]
    g = r.backward(r.gradient_at_E(r.forward(t=1)[0], u, i, j, c["lam"]), caches)
    assert all(np.isfinite(a).all() for a in g.values())
    assert int(golden["zero/finite"]) == 1 and np.isfinite(golden["zero/losses"]).all(), "the reference stays finite there"
    assert all(np.isfinite(golden["zero/P/" + n]).all() for n in r.W)


def test_restatement_gradient_is_the_loss_slope():
    """the hand-written backward pass against central differences of the restated loss, in train mode with a mask"""
    c = dict(nc.CASES["mixed"], lam=1e-2)
    init = nc.case_params(c)
    u, i, j = nc.case_batches(c)[0]
    r = nc.new_restatement(c, init)
    E, caches = r.forward(t=1)
    g = r.backward(r.gradient_at_E(E, u, i, j, c["lam"]), caches)
    rs = np.random.RandomState(0)
    for n in r.W:
        for _ in range(2):
            at = tuple(rs.randint(0, s) for s in r.W[n].shape)
            vals = []
            for eps in (1e-6, -1e-6):
                q = nc.new_restatement(c, init)
                q.W[n][at] += eps
                vals.append(q.losses(q.forward(t=1)[0], u, i, j, c["lam"])[0])
            slope = (vals[0] - vals[1]) / 2e-6
            assert abs(slope - g[n][at]) <= 1e-9 + 1e-5 * abs(slope), (n, at, slope, g[n][at])


def test_rank_case_has_distinct_top_scores():
    E = nc.run_case(nc.RANK_CASE)["r"].final()
    S = (E[0].astype(np.float32) @ E[1].astype(np.float32).T).astype(np.float64)
    top = -np.sort(-S, axis=1)[:, :11]
    # a float32 dot product of D terms is off by at most D * 2^-24 * max|score|: gaps of four times that cannot tie
    bound = E[0].shape[1] * 2.0 ** -24 * np.abs(S).max()
    assert (np.diff(top, axis=1) < -4 * bound).all(), "the top 11 scores of every user are at least %.3g apart" % (4 * bound)


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "NgcfModel", nc.FakeNgcfModel)
    monkeypatch.chdir(tmp_path)
    nc.FakeNgcfModel.built, nc.FakeNgcfModel.last = 0, None


def test_constructor_is_the_references():
    sig = inspect.signature(NGCF.__init__)
    assert list(sig.parameters)[1:] == ["name", "emb_size", "layer_sizes", "dropout_rates", "num_epochs", "learning_rate", "batch_size",
                                        "early_stopping", "lambda_reg", "trainable", "verbose", "seed", "device"]
    m = NGCF()
    assert (m.name, m.emb_size, m.layer_sizes, m.dropout_rates, m.num_epochs, m.learning_rate, m.batch_size, m.early_stopping, m.lambda_reg,
            m.trainable, m.verbose, m.seed, m.device) == ("NGCF", 64, [64, 64, 64], [0.1, 0.1, 0.1], 1000, 0.001, 1024, None, 1e-4, True,
                                                          False, 2020, 0)
    assert isinstance(m, Recommender) and not m.is_fitted and not hasattr(m, "U")
    c = NGCF(emb_size=5, seed=3).clone({"layer_sizes": [2]})
    assert (c.emb_size, c.seed, c.layer_sizes) == (5, 3, [2])
    assert list(_lib.NgcfModel.param_shapes(3, 4, 5, [6, 7])) == NAMES_2 == list(nc.param_shapes(3, 4, 5, [6, 7]))


def test_seeded_fit_reproduces_the_references_seeded_fit(device_double, golden):
    """holds the draw order of the initial values (real nn.Linears, xavier on W1 then W2, the item table, the user table) and the
    sampler's draw order: the reference's own seeded fit against the model class over the restatement, all dropout rates 0"""
    import torch

    c = nc.SEEDED["seeded"]
    ds = nc.seeded_dataset(c)
    m = nc.seeded_model(c).fit(ds)
    fake = nc.FakeNgcfModel.last
    assert nc.FakeNgcfModel.built == 1 and fake.closed and (fake.emb_size, fake.layer_sizes, fake.dropout_rates) == (c["emb"], list(c["layers"]), [0.0, 0.0])
    assert fake.dropout_key == c["seed"]
    assert len(fake.epochs) == c["epochs"] == len(m.loss_history) and fake.propagated == 1
    ds2 = nc.seeded_dataset(c)
    ds2.reset()
    for ptr, users, pos, neg in fake.epochs:
        mine = list(ds2.uij_iter(c["bs"], shuffle=True))
        assert list(np.diff(ptr)) == [len(b[0]) for b in mine] and np.diff(ptr).max() == c["bs"]
        assert all(np.array_equal(got, np.concatenate([b[q] for b in mine])) for q, got in enumerate((users, pos, neg)))
    torch.manual_seed(c["seed"])
    din = c["emb"]
    for l, dout in enumerate(c["layers"]):
        W1, W2 = torch.nn.Linear(din, dout), torch.nn.Linear(din, dout)
        torch.nn.init.xavier_uniform_(W1.weight)
        torch.nn.init.xavier_uniform_(W2.weight)
        assert np.array_equal(fake.initial["layers.%d.W1.weight" % l], W1.weight.detach().numpy())
        assert np.array_equal(fake.initial["layers.%d.W2.weight" % l], W2.weight.detach().numpy())
        assert not fake.initial["layers.%d.W1.bias" % l].any() and not fake.initial["layers.%d.W2.bias" % l].any()
        din = dout
    item = torch.nn.init.xavier_uniform_(torch.empty(c["ni"], c["emb"])).numpy()
    user = torch.nn.init.xavier_uniform_(torch.empty(c["nu"], c["emb"])).numpy()
    assert np.array_equal(fake.initial["feature_dict.user"], user) and np.array_equal(fake.initial["feature_dict.item"], item)
    for q, (mine, ref) in enumerate(((m.U, golden["seeded/U"]), (m.V, golden["seeded/V"]))):
        tol = nc.tolerance(golden["seeded/d_ref"][q], golden["seeded/max"][q])
        d = np.abs(ref.astype(np.float64) - fake.r.final()[q]).max()
        print("seeded %s: %.3g (tolerance %.3g)" % ("UV"[q], d, tol))
        assert d <= tol and mine.dtype == np.float32 and np.abs(mine.astype(np.float64) - ref).max() <= tol + 2.0 ** -24
    users = nc.score_users(c)
    got = np.array([m.score(int(u)) for u in users], np.float64)
    assert np.abs(got - golden["seeded/scores"]).max() <= 64 * 2.0 ** -24 * fake.D
    ptr = fake.epochs[0][0]
    again = nc.Restatement(fake.X, c["emb"], c["layers"], c["drop"], c["seed"], fake.initial)
    losses, _, _ = again.fit_epoch(*fake.epochs[0], c["lr"], c["lam"])
    assert m.loss_history[0] == pytest.approx(float((losses * np.diff(ptr)).sum() / ptr[-1]), rel=1e-12)


def test_seed_none_draws_the_dropout_key_from_the_os(device_double):
    c = nc.SEEDED["seeded"]
    keys = set()
    for _ in range(2):
        nc.seeded_model(c, seed=None, num_epochs=1).fit(nc.seeded_dataset(c))
        keys.add(nc.FakeNgcfModel.last.dropout_key)
    assert len(keys) == 2
    with pytest.raises(AssertionError, match="same size"):
        nc.seeded_model(c, dropout_rates=[0.1]).fit(nc.seeded_dataset(c))


def test_not_trainable_builds_nothing(device_double):
    c = nc.SEEDED["seeded"]
    m = nc.seeded_model(c, trainable=False).fit(nc.seeded_dataset(c))
    assert nc.FakeNgcfModel.built == 0 and not hasattr(m, "U") and m.is_fitted


def test_score_rank_and_score_exception(device_double):
    c = nc.SEEDED["seeded"]
    D = c["emb"] + sum(c["layers"])
    m = nc.seeded_model(c, num_epochs=1).fit(nc.seeded_dataset(c))
    s = m.score(4)
    assert m.U.shape == (c["nu"], D) and m.V.shape == (c["ni"], D)
    assert s.shape == (c["ni"],) and s.dtype == np.float32 and np.abs(s - m.V @ m.U[4]).max() <= 1e-5
    assert m.score(4, 9) == pytest.approx(float(m.V[9] @ m.U[4]))
    with pytest.raises(ScoreException, match="user_id=99"):
        m.score(99)
    with pytest.raises(ScoreException, match="item_id=77"):
        m.score(4, 77)
    ranked, scores = m.rank(4)
    assert np.array_equal(scores, s) and np.array_equal(ranked, np.lexsort((np.arange(c["ni"]), s))[::-1])
    U, V, ib, ub = m._scoring_tables()
    assert U is m.U and V is m.V and not ib.any() and not ub.any() and ib.shape == (c["ni"],) and ub.shape == (c["nu"],)
    items, top = m.rank_batch([4, 5], k=3)
    assert np.array_equal(items[0], ranked[:3]) and m.get_vector_measure() == "dot" and m.get_user_vectors() is m.U
    assert m.get_item_vectors() is m.V


def test_state_dict_round_trip_save_load(device_double, tmp_path):
    import torch

    c = nc.SEEDED["seeded"]
    ds = nc.seeded_dataset(c)
    m = nc.seeded_model(c, num_epochs=1).fit(ds)
    sd = m.state_dict()
    assert list(sd) == NAMES_2 and sd["feature_dict.user"].shape == (c["nu"], c["emb"]) and sd["layers.1.W2.weight"].shape == (3, 6)
    assert sd["feature_dict.item"] is not m.params["feature_dict.item"]
    other = NGCF()
    other.load_state_dict({n: torch.tensor(a) for n, a in sd.items()}, graph=ds)   # tensors, as the reference's state_dict holds
    assert (other.emb_size, other.layer_sizes) == (c["emb"], list(c["layers"]))
    assert np.array_equal(other.U, m.U) and np.array_equal(other.V, m.V)
    with pytest.raises(KeyError):
        other.load_state_dict({"feature_dict.user": sd["feature_dict.user"]})
    with pytest.raises(ValueError, match="expected"):
        other.load_state_dict(dict(sd, **{"feature_dict.item": np.zeros((3, 2), np.float32)}))
    with pytest.raises(ValueError, match="layers.1.W1.bias"):
        other.load_state_dict(dict(sd, **{"layers.1.W1.bias": np.zeros(9, np.float32)}))
    s4 = m.score(4)
    again = pickle.loads(pickle.dumps(m))
    assert not hasattr(again, "train_set") and "_scorer" not in again.__dict__ and np.array_equal(again.score(4), s4)
    back = NGCF.load(m.save(str(tmp_path)))
    assert back.trainable is False and np.array_equal(back.U, m.U) and np.array_equal(back.score(4), s4)
    assert all(np.array_equal(back.params[n], m.params[n]) for n in sd)


def test_a_refit_starts_from_new_parameters_and_a_new_optimiser(device_double):
    c = nc.SEEDED["seeded"]
    ds = nc.seeded_dataset(c)
    m = nc.seeded_model(c, num_epochs=1).fit(ds)
    first, U = nc.FakeNgcfModel.last, m.U.copy()
    with pytest.warns(UserWarning):
        m.fit(ds)
    assert nc.FakeNgcfModel.last is not first and first.closed and np.array_equal(m.U, U)
    assert nc.FakeNgcfModel.last.r.t == len(first.epochs[0][0]) - 1


def test_unknown_ids_are_nodes_without_edges(device_double):
    """the graph spans total_users x total_items: ids of the global maps that the train set does not hold"""
    from collections import OrderedDict

    c = nc.SEEDED["seeded"]
    u, i, r = nc.seeded_triplets(c)
    ds = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=1, global_uid_map=OrderedDict((n, n) for n in range(c["nu"] + 2)),
                       global_iid_map=OrderedDict((n, n) for n in range(c["ni"] + 3)))
    m = nc.seeded_model(c, num_epochs=1).fit(ds)
    fake = nc.FakeNgcfModel.last
    D = c["emb"] + sum(c["layers"])
    assert (fake.n_users, fake.n_items) == (c["nu"] + 2, c["ni"] + 3) and m.U.shape == (c["nu"] + 2, D)
    assert not np.diff(fake.X.indptr)[c["nu"]:].any() and fake.X.indices.max() < c["ni"]
    assert m.score(0).shape == (c["ni"] + 3,)


def test_ngcf_stops_early_on_a_validation_set(device_double, capsys):
    from collections import OrderedDict

    c = nc.SEEDED["seeded"]
    ds = nc.seeded_dataset(c)
    u, i, r = nc.seeded_triplets(dict(c, seed=c["seed"] + 1))
    val = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=1, global_uid_map=OrderedDict(ds.uid_map), global_iid_map=OrderedDict(ds.iid_map))
    m = nc.seeded_model(c, num_epochs=50, early_stopping={"min_delta": 0.5, "patience": 2}).fit(ds, val)
    fake = nc.FakeNgcfModel.last
    # Recall@20 cannot rise by 0.5 twice: the first value is the best one, two epochs later the fit stops
    assert (m.best_epoch, m.stopped_epoch, m.current_epoch) == (1, 3, 3) and len(fake.epochs) == 3 == len(m.loss_history)
    assert 0.0 <= m.best_value <= 1.0 and fake.propagated == 3, "U and V are taken after every epoch when early stopping is on"
    assert np.array_equal(m.U, fake.propagate()[0])
    assert "Early stopping:" in capsys.readouterr().out
    m = nc.seeded_model(c, num_epochs=4, early_stopping={"patience": 1}).fit(ds)
    assert len(m.loss_history) == 4 and m.stopped_epoch == 0 and m.current_epoch == 4


# ---- (3) ABI ---------------------------------------------------------------------------------------------------------------
NGCF_SYMBOLS = ["cornac_hip_ngcf_create", "cornac_hip_ngcf_destroy", "cornac_hip_ngcf_set_params", "cornac_hip_ngcf_get_params",
                "cornac_hip_ngcf_get_state", "cornac_hip_ngcf_reset_optimizer", "cornac_hip_ngcf_fit_epoch", "cornac_hip_ngcf_propagate"]


def test_abi_declares_binds_and_refuses_without_a_device():
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in NGCF_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    section = header[header.index("NGCF (Wang et al. 2019)"):]
    for cited in ("ngcf.py:14-37", "ngcf.py:110-117", "ngcf.py:65-100", "ngcf.py:170-185", "recom_ngcf.py:"):
        assert cited in section, cited
    assert "ngcf.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    source = open(os.path.join(ROOT, "cornac_amd", "csrc", "ngcf.hip")).read()
    assert "kNgcfWgradRows = %d" % _lib.NgcfModel.WGRAD_ROWS in source and "atomic" not in source.replace("No atomics", "")
    L = _lib.lib()
    assert L.cornac_hip_ngcf_set_params(None, None, None, None) == 1 and L.cornac_hip_ngcf_get_params(None, None, None, None) == 1
    assert L.cornac_hip_ngcf_get_state(None, None, None, None, None, None, None, None) == 1 and L.cornac_hip_ngcf_reset_optimizer(None) == 1
    assert L.cornac_hip_ngcf_propagate(None, None, None) == 1 and L.cornac_hip_ngcf_destroy(None) == 0
    assert "ngcf handle is NULL" in L.cornac_hip_last_error().decode()
    X = sp.random(6, 8, 0.5, format="csr", random_state=1)
    X.sort_indices()
    ok = dict(emb_size=8, layer_sizes=[8], dropout_rates=[0.0])
    for kw, text in ((dict(emb_size=0), "ngcf: emb_size = 0 .* 1 <= emb_size <= 256"),
                     (dict(emb_size=257), "ngcf: emb_size = 257 .* 1 <= emb_size <= 256"),
                     (dict(layer_sizes=[8, 0], dropout_rates=[0, 0]), "ngcf: layer size 1 = 0 .* 1 <= size <= 256"),
                     (dict(layer_sizes=[257]), "ngcf: layer size 0 = 257 .* 1 <= size <= 256"),
                     (dict(layer_sizes=[], dropout_rates=[]), "ngcf: num_layers = 0 .* 1 <= num_layers <= 8"),
                     (dict(layer_sizes=[4] * 9, dropout_rates=[0] * 9), "ngcf: num_layers = 9 .* 1 <= num_layers <= 8"),
                     (dict(dropout_rates=[1.0]), "ngcf: dropout rate 0 = 1 .* 0 <= p < 1"),
                     (dict(dropout_rates=[-0.1]), "ngcf: dropout rate 0 = -0.1 .* 0 <= p < 1")):
        with pytest.raises(_lib.HipError, match=text) as e:
            _lib.NgcfModel(X, **dict(ok, **kw))
        assert e.value.code == 1
    bad = X.copy()
    row = int(np.flatnonzero(np.diff(bad.indptr) >= 2)[0])
    a = bad.indptr[row]
    bad.indices[a], bad.indices[a + 1] = bad.indices[a + 1], bad.indices[a]
    h, ip, ix = ctypes.c_void_p(), np.ascontiguousarray(bad.indptr, np.int64), np.ascontiguousarray(bad.indices, np.int32)
    sizes, rates = np.array([8], np.int32), np.array([0], np.float32)
    assert L.cornac_hip_ngcf_create(ctypes.byref(h), 0, 6, 8, ip.ctypes.data, ix.ctypes.data, 8, 1, sizes.ctypes.data, rates.ctypes.data, 0) == 1
    assert not h and "ngcf: the training matrix needs sorted indices without repeats" in L.cornac_hip_last_error().decode()
    assert L.cornac_hip_ngcf_create(ctypes.byref(h), 0, 1 << 30, 1 << 30, ip.ctypes.data, ix.ctypes.data, 8, 1, sizes.ctypes.data, rates.ctypes.data, 0) == 1
    assert "ngcf: n_users + n_items must be below 2^31" in L.cornac_hip_last_error().decode()
    n = _lib.NgcfModel.MAX_STEP + 1
    ptr, ids = np.array([0, n], np.int64), np.zeros(n, np.int32)
    vp = lambda a: a.ctypes.data   # noqa: E731
    assert L.cornac_hip_ngcf_fit_epoch(None, 1, vp(ptr), vp(ids), vp(ids), vp(ids), 0.1, 0.0, None, None, None) == 1
    assert re.search(r"ngcf: step 0 has 16385 triplets, .* 1 <= batch_size <= 16384", L.cornac_hip_last_error().decode())
    assert L.cornac_hip_ngcf_fit_epoch(None, 1, vp(np.array([0, 4], np.int64)), vp(ids), vp(ids), vp(ids), 0.1, 0.0, None, None, None) == 1
    assert "ngcf handle is NULL" in L.cornac_hip_last_error().decode()
    assert (_lib.NgcfModel.PIECE, _lib.NgcfModel.MAX_STEP, _lib.NgcfModel.WGRAD_ROWS) == (512, 16384, 2048)
