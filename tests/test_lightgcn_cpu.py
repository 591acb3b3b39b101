"""LightGCN without a GPU: (1) the float64 restatement of tests/lightgcn_cases.py against the golden that the reference's own
lightgcn.Model, construct_graph and LightGCN.fit wrote (tables, Adam's state, losses, final embeddings, scores), the
tolerance rule's condition and the cases' own conditions; (2) the model class's host logic over a device double served by the
restatement: the seeded fit against the reference's own seeded fit, the draw order, one fit_epoch per epoch, early stopping,
state_dict, save / load; (3) Recommender.early_stop against scripted values; (4) the ABI and its refusals."""
import ctypes
import inspect
import os
import pickle
import re

import numpy as np
import pytest
import scipy.sparse as sp

import fake_device
import lightgcn_cases as lc
from conftest import ROOT, load_golden
from cornac_amd import Dataset, LightGCN, Recommender, ScoreException, _lib

STATS = ("d_ref", "d_ref_m", "d_ref_v", "move", "max", "max_m", "max_v")


@pytest.fixture(scope="module")
def golden():
    return load_golden("lightgcn_ref")


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases_and_their_conditions(golden):
    assert sorted(golden["cases"]) == sorted(list(lc.CASES) + list(lc.SEEDED))
    assert set(lc.CASES) == {"d1", "d8", "d33", "d64", "d65", "d256", "l0", "l4reg", "lam0", "hub"}
    for name, c in lc.CASES.items():
        for kind in STATS:
            assert golden["%s/%s" % (name, kind)].shape == (2,) and np.isfinite(golden["%s/%s" % (name, kind)]).all()
        share = lc.check_condition(golden, name)
        print("%s: the device's tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
        X, batches = lc.case_graph(c), lc.case_batches(c)
        tu, ti = lc.totals(c)
        assert X.shape == (tu, ti) and X.has_sorted_indices and len(batches) >= 3 and [len(b[0]) for b in batches] == list(c["steps"])
        deg_u, deg_i = np.diff(X.indptr), np.bincount(X.indices, minlength=ti)
        assert (deg_u[:c["nu"]] > 0).all() and (deg_i[:c["ni"]] > 0).all() and not deg_u[c["nu"]:].any() and not deg_i[c["ni"]:].any()
        later = np.concatenate([b[0] for b in batches[1:]])
        assert batches[0][0][0] == 0 and 0 not in later, "user 0: the first step only"
        assert all(b[0].max() < c["nu"] for b in batches), "no batch names a user without edges"
        assert all((b[1] == 1).sum() * 3 >= len(b[1]) for b in batches if len(b[1]) >= 5), "a third of the positives are item 1"
        assert all(len(np.intersect1d(b[1], b[2])) > 0 for b in batches if len(b[1]) >= 2), "an item is positive and negative in one step"
        assert len(np.intersect1d(batches[-1][1], batches[-1][2])) > 0
    c = lc.CASES["d8"]
    assert (c["iso_u"], c["iso_i"]) == (2, 1) and any((b[2] == lc.totals(c)[1] - 1).any() for b in lc.case_batches(c))
    assert (lc.CASES["d64"]["iso_u"], lc.CASES["d64"]["iso_i"]) == (3, 2)
    assert lc.CASES["l0"]["L"] == 0 and lc.CASES["l4reg"]["L"] == 4 and lc.CASES["l4reg"]["lam"] == 1e-2 and lc.CASES["lam0"]["lam"] == 0.0
    assert {c["d"] for c in lc.CASES.values()} >= {1, 8, 33, 64, 65, 256}
    print("seeded: %.3g of a table's movement" % lc.check_condition(golden, "seeded"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "lightgcn_ref.npz")) < 1024 * 1024


def test_hub_row_spans_at_least_three_pieces():
    assert lc.PIECE == _lib.LightGcnModel.PIECE
    X = lc.case_graph(lc.CASES["hub"])
    hub = int(np.bincount(X.indices)[0])
    assert hub == lc.CASES["hub"]["nu"] and -(-hub // _lib.LightGcnModel.PIECE) >= 3
    assert np.diff(X.indptr).max() <= _lib.LightGcnModel.PIECE   # (and nothing else is split)


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_restatement_against_the_reference(golden, name):
    run = lc.run_case(name)
    r = run["r"]
    assert np.isfinite(run["losses"]).all() and r.t == len(lc.CASES[name]["steps"])
    assert float(golden[name + "/d_ref"].max()) <= 1e-6 and float(golden[name + "/d_ref_loss"]) <= 1e-6
    if name not in lc.FULL_CASES:
        return
    for q, n in enumerate(lc.TABLES):
        for kind, mine, stat in (("P", r.tables(), "d_ref"), ("M", r.tables(r.M), "d_ref_m"), ("V", r.tables(r.V), "d_ref_v")):
            d = np.abs(golden["%s/%s/%s" % (name, kind, n)].astype(np.float64) - mine[q]).max()
            assert d == golden["%s/%s" % (name, stat)][q], (name, kind, n, d)
    assert np.abs(golden[name + "/losses"] - run["losses"]).max() == float(golden[name + "/d_ref_loss"])
    E = r.final()
    assert max(np.abs(golden[name + "/E/" + n].astype(np.float64) - E[q]).max() for q, n in enumerate(lc.TABLES)) <= 1e-6
    users = lc.score_users(lc.CASES[name])
    assert np.abs(golden[name + "/scores"] - E[0][users] @ E[1].T).max() <= 1e-5


def test_isolated_rows_stay_in_place_and_the_rest_moves():
    for name in ("d8", "d64"):
        c, run = lc.CASES[name], lc.run_case(name)
        still_u, still_i = lc.still_rows(name)
        assert list(still_u) == list(range(c["nu"], c["nu"] + c["iso_u"])), "exactly the users without edges"
        # an isolated item that was drawn as a negative has a gradient of its own; one that never was stays
        drawn = np.unique(np.concatenate([np.concatenate(b[1:]) for b in lc.case_batches(c)]))
        assert list(still_i) == [i for i in range(c["ni"], c["ni"] + c["iso_i"]) if i not in drawn]
        assert np.array_equal(run["r"].tables()[0][still_u], run["init"][0][still_u].astype(np.float64))


def test_restatement_gradient_is_the_loss_slope():
    """P(gradient at E) is dL/dE0: compared with central differences of the restated loss"""
    c = dict(lc.CASES["d8"], lam=1e-2)
    init = lc.case_params(c)
    u, i, j = lc.case_batches(c)[0]
    r = lc.new_restatement(c, init)
    g = r.P(r.gradient(r.P(r.W), u, i, j, c["lam"]))
    rs = np.random.RandomState(0)
    for _ in range(12):
        at = (rs.randint(0, c["nu"] + c["ni"]), rs.randint(0, c["d"]))
        vals = []
        for eps in (1e-6, -1e-6):
            q = lc.new_restatement(c, init)
            q.W[at] += eps
            vals.append(q.losses(q.P(q.W), u, i, j, c["lam"])[0])
        slope = (vals[0] - vals[1]) / 2e-6
        assert abs(slope - g[at]) <= 1e-9 + 1e-5 * abs(slope), (at, slope, g[at])


def test_rank_case_has_distinct_top_scores():
    E = lc.run_case(lc.RANK_CASE)["r"].final()
    S = (E[0].astype(np.float32) @ E[1].astype(np.float32).T).astype(np.float64)
    top = -np.sort(-S, axis=1)[:, :11]
    # a float32 dot product of 64 terms is off by at most 64 * 2^-24 * max|score|: gaps of four times that cannot tie
    bound = 64 * 2.0 ** -24 * np.abs(S).max()
    assert (np.diff(top, axis=1) < -4 * bound).all(), "the top 11 scores of every user are at least %.3g apart" % (4 * bound)


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "LightGcnModel", lc.FakeLightGcnModel)
    monkeypatch.chdir(tmp_path)
    lc.FakeLightGcnModel.built, lc.FakeLightGcnModel.last = 0, None


def test_constructor_is_the_references():
    sig = inspect.signature(LightGCN.__init__)
    assert list(sig.parameters)[1:] == ["name", "emb_size", "num_epochs", "learning_rate", "batch_size", "num_layers", "early_stopping",
                                        "lambda_reg", "trainable", "verbose", "seed", "device"]
    m = LightGCN()
    assert (m.name, m.emb_size, m.num_epochs, m.learning_rate, m.batch_size, m.num_layers, m.early_stopping, m.lambda_reg, m.trainable,
            m.verbose, m.seed, m.device) == ("LightGCN", 64, 1000, 0.001, 1024, 3, None, 1e-4, True, False, 2020, 0)
    assert isinstance(m, Recommender) and not m.is_fitted and not hasattr(m, "U")
    c = LightGCN(emb_size=5, seed=3).clone({"num_layers": 2})
    assert (c.emb_size, c.seed, c.num_layers) == (5, 3, 2)


def test_seeded_fit_reproduces_the_references_seeded_fit(device_double, golden):
    """holds the draw order of the initial tables (item first) and the sampler's draw order: the reference's own seeded fit, with
    its own initial tables and its own uij_iter, against the model class over the restatement"""
    import torch

    c = lc.SEEDED["seeded"]
    ds = lc.seeded_dataset(c)
    m = lc.seeded_model(c).fit(ds)
    fake = lc.FakeLightGcnModel.last
    assert lc.FakeLightGcnModel.built == 1 and fake.closed and (fake.emb_size, fake.num_layers) == (c["d"], c["L"])
    # one fit_epoch per epoch, holding uij_iter's batches unchanged
    assert len(fake.epochs) == c["epochs"] == len(m.loss_history) and fake.propagated == 1
    ds2 = lc.seeded_dataset(c)
    ds2.reset()
    for ptr, users, pos, neg in fake.epochs:
        mine = list(ds2.uij_iter(c["bs"], shuffle=True))
        assert list(np.diff(ptr)) == [len(b[0]) for b in mine] and np.diff(ptr).max() == c["bs"]
        assert all(np.array_equal(got, np.concatenate([b[q] for b in mine])) for q, got in enumerate((users, pos, neg)))
    # the draw order: the item table first
    torch.manual_seed(c["seed"])
    item = torch.nn.init.xavier_uniform_(torch.empty(c["ni"], c["d"])).numpy()
    user = torch.nn.init.xavier_uniform_(torch.empty(c["nu"], c["d"])).numpy()
    assert np.array_equal(fake.initial[0], user) and np.array_equal(fake.initial[1], item)
    for q, (mine, ref) in enumerate(((m.U, golden["seeded/U"]), (m.V, golden["seeded/V"]))):
        tol = lc.tolerance(golden["seeded/d_ref"][q], golden["seeded/max"][q])
        d = np.abs(ref.astype(np.float64) - fake.r.final()[q]).max()
        print("seeded %s: %.3g (tolerance %.3g)" % (lc.TABLES[q], d, tol))
        assert d <= tol and mine.dtype == np.float32 and np.abs(mine.astype(np.float64) - ref).max() <= tol + 2.0 ** -24
    users = lc.score_users(c)
    got = np.array([m.score(int(u)) for u in users], np.float64)
    assert np.abs(got - golden["seeded/scores"]).max() <= 64 * 2.0 ** -24
    # the per-epoch loss is the sample-weighted mean of the steps' total loss
    ptr = fake.epochs[0][0]
    again = lc.Restatement(fake.X, c["d"], c["L"], *fake.initial)
    losses, _, _ = again.fit_epoch(*fake.epochs[0], c["lr"], c["lam"])
    assert m.loss_history[0] == pytest.approx(float((losses * np.diff(ptr)).sum() / ptr[-1]), rel=1e-12)


def test_not_trainable_builds_nothing(device_double):
    c = lc.SEEDED["seeded"]
    m = lc.seeded_model(c, trainable=False).fit(lc.seeded_dataset(c))
    assert lc.FakeLightGcnModel.built == 0 and not hasattr(m, "U") and m.is_fitted


def test_score_rank_and_score_exception(device_double):
    c = lc.SEEDED["seeded"]
    m = lc.seeded_model(c, num_epochs=1).fit(lc.seeded_dataset(c))
    s = m.score(4)
    assert s.shape == (c["ni"],) and s.dtype == np.float32 and np.abs(s - m.V @ m.U[4]).max() <= 1e-6
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


def test_state_dict_round_trip_save_load(device_double, tmp_path):
    import torch

    c = lc.SEEDED["seeded"]
    ds = lc.seeded_dataset(c)
    m = lc.seeded_model(c, num_epochs=1).fit(ds)
    sd = m.state_dict()
    assert list(sd) == ["feature_dict.user", "feature_dict.item"] and sd["feature_dict.user"].shape == (c["nu"], c["d"])
    assert sd["feature_dict.item"].shape == (c["ni"], c["d"]) and sd["feature_dict.user"] is not m.params["feature_dict.user"]
    other = LightGCN(num_layers=c["L"])
    other.load_state_dict({n: torch.tensor(a) for n, a in sd.items()}, graph=ds)   # tensors, as the reference's state_dict holds
    assert other.emb_size == c["d"] and np.array_equal(other.U, m.U) and np.array_equal(other.V, m.V)
    with pytest.raises(KeyError):
        other.load_state_dict({"feature_dict.user": sd["feature_dict.user"]})
    with pytest.raises(ValueError, match="expected"):
        other.load_state_dict({"feature_dict.user": sd["feature_dict.user"], "feature_dict.item": np.zeros((3, 2), np.float32)})
    s4 = m.score(4)
    again = pickle.loads(pickle.dumps(m))
    assert not hasattr(again, "train_set") and "_scorer" not in again.__dict__ and np.array_equal(again.score(4), s4)
    back = LightGCN.load(m.save(str(tmp_path)))
    assert back.trainable is False and np.array_equal(back.U, m.U) and np.array_equal(back.score(4), s4)
    assert all(np.array_equal(back.params[n], m.params[n]) for n in sd)


def test_a_refit_starts_from_new_tables_and_a_new_optimiser(device_double):
    c = lc.SEEDED["seeded"]
    ds = lc.seeded_dataset(c)
    m = lc.seeded_model(c, num_epochs=1).fit(ds)
    first, U = lc.FakeLightGcnModel.last, m.U.copy()
    with pytest.warns(UserWarning):
        m.fit(ds)
    assert lc.FakeLightGcnModel.last is not first and first.closed and np.array_equal(m.U, U)
    assert lc.FakeLightGcnModel.last.r.t == len(first.epochs[0][0]) - 1


def test_unknown_ids_are_nodes_without_edges(device_double):
    """the graph spans total_users x total_items: ids of the global maps that the train set does not hold"""
    from collections import OrderedDict

    c = lc.SEEDED["seeded"]
    u, i, r = lc.seeded_triplets(c)
    ds = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=1, global_uid_map=OrderedDict((n, n) for n in range(c["nu"] + 2)),
                       global_iid_map=OrderedDict((n, n) for n in range(c["ni"] + 3)))
    m = lc.seeded_model(c, num_epochs=1).fit(ds)
    fake = lc.FakeLightGcnModel.last
    assert (fake.n_users, fake.n_items) == (c["nu"] + 2, c["ni"] + 3) and m.U.shape == (c["nu"] + 2, c["d"])
    assert np.array_equal(m.params["feature_dict.user"][c["nu"]:], fake.initial[0][c["nu"]:]), "no gradient: in place"
    assert m.score(0).shape == (c["ni"] + 3,)


# ---- (3) early stopping ------------------------------------------------------------------------------------------------------
class Scripted(Recommender):
    def __init__(self, values):
        super().__init__("scripted")
        self.values = list(values)

    def monitor_value(self, train_set, val_set):
        return self.values.pop(0)


def _run(values, **kw):
    m = Scripted(values)
    m.reset_info()
    out = []
    while m.values:
        out.append(m.early_stop(None, None, **kw))
        if out[-1]:
            break
    return m, out


def test_early_stop_against_scripted_values(capsys):
    m, out = _run([0.1, 0.2, 0.2, 0.15, 0.3])   # patience 0: the first epoch without improvement stops; an equal value improves
    assert out == [False, False, False, True] and (m.best_epoch, m.stopped_epoch, m.best_value, m.current_epoch) == (3, 4, 0.2, 4)
    assert "best epoch = 3, stopped epoch = 4" in capsys.readouterr().out
    m, out = _run([0.1, 0.2, 0.25, 0.5], min_delta=0.1)   # a rise below min_delta does not count
    assert out == [False, False, True] and (m.best_epoch, m.stopped_epoch, m.best_value) == (2, 3, 0.2)
    m, out = _run([0.5, 0.4, 0.3, 0.6, 0.1, 0.2, 0.3], patience=3)   # the wait starts again after an improvement
    assert out == [False] * 6 + [True] and (m.best_epoch, m.stopped_epoch, m.wait) == (4, 7, 3)
    m, out = _run([None] * 5, patience=1)   # nothing to watch: never stops, the epochs are still counted
    assert out == [False] * 5 and (m.current_epoch, m.best_epoch, m.stopped_epoch, m.best_value) == (5, 0, 0, float("-inf"))
    assert Recommender("plain").monitor_value(None, None) is None
    capsys.readouterr()


def test_lightgcn_stops_early_on_a_validation_set(device_double, capsys, monkeypatch):
    c = lc.SEEDED["seeded"]
    ds = lc.seeded_dataset(c)
    u, i, r = lc.seeded_triplets(dict(c, seed=c["seed"] + 1))
    from collections import OrderedDict

    val = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=1, global_uid_map=OrderedDict(ds.uid_map), global_iid_map=OrderedDict(ds.iid_map))
    m = lc.seeded_model(c, num_epochs=50, early_stopping={"min_delta": 0.5, "patience": 2}).fit(ds, val)
    fake = lc.FakeLightGcnModel.last
    # Recall@20 cannot rise by 0.5 twice: the first value is the best one, two epochs later the fit stops
    assert (m.best_epoch, m.stopped_epoch, m.current_epoch) == (1, 3, 3) and len(fake.epochs) == 3 == len(m.loss_history)
    assert 0.0 <= m.best_value <= 1.0 and fake.propagated == 3, "U and V are taken after every epoch when early stopping is on"
    assert np.array_equal(m.U, fake.propagate()[0])
    assert "Early stopping:" in capsys.readouterr().out
    # without a validation set the monitored value is None and nothing stops
    m = lc.seeded_model(c, num_epochs=4, early_stopping={"patience": 1}).fit(ds)
    assert len(m.loss_history) == 4 and m.stopped_epoch == 0 and m.current_epoch == 4


# ---- (4) ABI ---------------------------------------------------------------------------------------------------------------
LIGHTGCN_SYMBOLS = ["cornac_hip_lightgcn_create", "cornac_hip_lightgcn_destroy", "cornac_hip_lightgcn_set_params",
                    "cornac_hip_lightgcn_get_params", "cornac_hip_lightgcn_get_state", "cornac_hip_lightgcn_reset_optimizer",
                    "cornac_hip_lightgcn_fit_epoch", "cornac_hip_lightgcn_propagate"]


def test_abi_declares_binds_and_refuses_without_a_device():
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in LIGHTGCN_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    section = header[header.index("LightGCN (He et al. 2020)"):]
    for cited in ("lightgcn.py:13-41", "lightgcn.py:44-117", "lightgcn.py:119-134", "recom_lightgcn.py:"):
        assert cited in section, cited
    assert "lightgcn.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    L = _lib.lib()
    assert L.cornac_hip_lightgcn_set_params(None, None, None) == 1 and L.cornac_hip_lightgcn_get_params(None, None, None) == 1
    assert L.cornac_hip_lightgcn_get_state(None, None, None, None, None, None) == 1 and L.cornac_hip_lightgcn_reset_optimizer(None) == 1
    assert L.cornac_hip_lightgcn_propagate(None, None, None) == 1 and L.cornac_hip_lightgcn_destroy(None) == 0
    X = sp.random(6, 8, 0.5, format="csr", random_state=1)
    X.sort_indices()
    for kw, text in ((dict(emb_size=0), "lightgcn: emb_size = 0 .* 1 <= emb_size <= 256"),
                     (dict(emb_size=257), "lightgcn: emb_size = 257 .* 1 <= emb_size <= 256"),
                     (dict(num_layers=9), "lightgcn: num_layers = 9 .* 0 <= num_layers <= 8"),
                     (dict(num_layers=-1), "lightgcn: num_layers = -1 .* 0 <= num_layers <= 8")):
        with pytest.raises(_lib.HipError, match=text) as e:
            _lib.LightGcnModel(X, **kw)
        assert e.value.code == 1
    bad = X.copy()
    row = int(np.flatnonzero(np.diff(bad.indptr) >= 2)[0])
    a = bad.indptr[row]
    bad.indices[a], bad.indices[a + 1] = bad.indices[a + 1], bad.indices[a]
    h, ip, ix = ctypes.c_void_p(), np.ascontiguousarray(bad.indptr, np.int64), np.ascontiguousarray(bad.indices, np.int32)
    assert L.cornac_hip_lightgcn_create(ctypes.byref(h), 0, 6, 8, ip.ctypes.data, ix.ctypes.data, 8, 3) == 1 and not h
    assert "lightgcn: the training matrix needs sorted indices without repeats" in L.cornac_hip_last_error().decode()
    # a step above MAX_STEP is refused by its shape alone
    n = _lib.LightGcnModel.MAX_STEP + 1
    ptr, ids = np.array([0, n], np.int64), np.zeros(n, np.int32)
    vp = lambda a: a.ctypes.data   # noqa: E731
    assert L.cornac_hip_lightgcn_fit_epoch(None, 1, vp(ptr), vp(ids), vp(ids), vp(ids), 0.1, 0.0, None, None, None) == 1
    assert re.search(r"lightgcn: step 0 has 16385 triplets, .* 1 <= batch_size <= 16384", L.cornac_hip_last_error().decode())
    assert L.cornac_hip_lightgcn_fit_epoch(None, 1, vp(np.array([0, 4], np.int64)), vp(ids), vp(ids), vp(ids), 0.1, 0.0, None, None, None) == 1
    assert "lightgcn handle is NULL" in L.cornac_hip_last_error().decode()
    assert (_lib.LightGcnModel.PIECE, _lib.LightGcnModel.MAX_STEP) == (512, 16384)
