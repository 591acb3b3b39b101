"""EASE without a GPU: (1) the float64 restatement (tests/ease_cases.py) against what the reference's own EASE wrote into
tests/golden/ease_ref.npz — the Gram matrix and the scores bit for bit, the weights within the recorded distance, which
itself stays a sixteenth under the textbook bound; (2) the host logic of cornac_amd.EASE through a device double that calls
the restatement; (3) the ABI entry points are declared and bound."""
import inspect
import os
import pickle
import re
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

import ease_cases as ec
import fake_device
from conftest import ROOT, load_golden
from cornac_amd import EASE, Dataset, Experiment, RatioSplit, Recommender, ScoreException, _lib
from cornac_amd import metrics as mm


@pytest.fixture(scope="module")
def golden():
    return load_golden("ease_ref")


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases_the_issue_counts(golden):
    assert sorted(golden["configs"]) == sorted(ec.CONFIGS)
    shapes = {"A": (60, 40, 600), "Ai": (60, 40, 600), "R": (150, 100, 2000), "T": (200, 129, 2500)}
    for name, (cname, lamb) in ec.CONFIGS.items():
        g, c = ec.golden_config(golden, name), ec.case(cname)
        assert (c["nu"], c["ni"], len(c["r"])) == shapes[cname]
        assert all(np.array_equal(g[n], c[n]) for n in "uir"), "the golden's triplets are the case's"
        assert g["B"].shape == (c["ni"], c["ni"]) and np.isfinite(g["B"]).all() and (np.diag(g["B"]) == 0).all()
        assert (g["B"] < 0).any(), "B is stored unclamped"
        assert ("G" in g) == (cname in ec.GRAM_CASES)
        for tag in ("", "_pos"):
            assert g["scores" + tag].shape == (ec.N_SCORE_USERS, c["ni"]) and g["pair_scores" + tag].shape == (ec.N_PAIRS,)
    assert set(ec.case("A")["r"]) == {1.0, 2.0, 3.0, 4.0, 5.0} and set(ec.case("Ai")["r"]) == {1.0}
    assert (ec.case("R")["r"] % 1 != 0).all() and (ec.case("T")["r"] % 1 != 0).all(), "real-valued ratings"
    assert sorted(l for c, l in ec.CONFIGS.values() if c == "A") == [0.5, 500.0]


@pytest.mark.parametrize("cname", ec.GRAM_CASES)
def test_restatement_gram_is_the_references(golden, cname):
    name = next(n for n in sorted(ec.CONFIGS) if ec.CONFIGS[n][0] == cname)
    g = ec.golden_config(golden, name)
    G = ec.gram(g["X"])
    print("%s: restatement G vs reference: max difference %.3g (allowed: 0, bit for bit)" % (cname, np.abs(G - g["G"]).max()))
    assert ec.same_bits(G, g["G"])


@pytest.mark.parametrize("name", sorted(ec.CONFIGS))
def test_restatement_scores_are_the_references(golden, name):
    """from the golden's B (and its exact clamp): the full rows and the single entries, bit for bit"""
    g = ec.golden_config(golden, name)
    c = ec.case(ec.CONFIGS[name][0])
    users, (pu, pi) = ec.score_users(c), ec.score_pairs(c)
    for tag, B in (("", g["B"]), ("_pos", ec.clamp(g["B"]))):
        rows = np.array([ec.score_user(g["X"], B, int(u)) for u in users])
        pairs = np.array([ec.score_pair(g["X"], B, int(u), int(i)) for u, i in zip(pu, pi)])
        print("%s%s: scores differ by %.3g, pairs by %.3g (allowed: 0)" % (
            name, tag, np.abs(rows - g["scores" + tag]).max(), np.abs(pairs - g["pair_scores" + tag]).max()))
        assert ec.same_bits(rows, g["scores" + tag]) and ec.same_bits(pairs, g["pair_scores" + tag])


@pytest.mark.parametrize("name", sorted(ec.CONFIGS))
def test_restatement_weights_against_the_reference(golden, name):
    g = ec.golden_config(golden, name)
    G = ec.gram(g["X"])
    B = ec.weights(ec.invert(G, g["lamb"]), False)
    diff, recorded, ceiling = float(np.abs(B - g["B"]).max()), ec.RESTATEMENT_VS_REFERENCE[name], ec.ceiling(G, g["lamb"], g["B"])
    print("%s: max|B restatement - B reference| = %.3g (recorded %.3g); CEILING %.3g, a sixteenth of it %.3g" % (
        name, diff, recorded, ceiling, ceiling / 16))
    assert diff <= recorded
    assert recorded <= ceiling / 16
    assert (np.diag(B) == 0).all()
    pos = ec.weights(ec.invert(G, g["lamb"]), True)
    assert (pos >= 0).all() and not np.signbit(pos).any() and np.array_equal(pos, ec.clamp(B))


def test_restatement_blocking_and_error():
    """every block count of the device tests agrees with NumPy's inverse; a non-positive pivot names its block"""
    for n in (1, 63, 64, 65, 129):
        X = ec.sized_matrix(n, "real", n)
        B, want = ec.fit(X, 0.5, False), ec.numpy_formula(X, 0.5, False)
        assert np.abs(B - want).max() <= ec.ceiling(ec.gram(X), 0.5, want) / 16
    bad = np.eye(130)
    bad[70, 70] = -2.0
    with pytest.raises(ec.NotPositiveDefinite, match="not positive definite at block 1"):
        ec.invert(bad, 0.5)


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "EaseModel", ec.FakeEaseModel)
    monkeypatch.chdir(tmp_path)
    ec.FakeEaseModel.built, ec.FakeEaseModel.last = 0, None


def test_constructor_is_the_references():
    m = EASE()
    assert (m.name, m.lamb, m.posB, m.trainable, m.verbose, m.seed, m.B, m.U, m.device) == \
        ("EASEᴿ", 500, True, True, True, None, None, None, 0)
    assert list(inspect.signature(EASE.__init__).parameters)[1:] == [
        "name", "lamb", "posB", "trainable", "verbose", "seed", "B", "U", "device"]
    assert isinstance(m, Recommender) and not m.is_fitted
    assert (m.get_vector_measure(), m.get_user_vectors(), m.get_item_vectors()) == ("dot", None, None)


@pytest.mark.parametrize("name", sorted(ec.CONFIGS))
def test_fit_gives_the_goldens_weights_and_scores(device_double, golden, name):
    g = ec.golden_config(golden, name)
    cname, lamb = ec.CONFIGS[name]
    c = ec.case(cname)
    users, (pu, pi) = ec.score_users(c), ec.score_pairs(c)
    for posB, tag in ((True, "_pos"), (False, "")):
        m = EASE(lamb=lamb, posB=posB, verbose=False).fit(ec.dataset(cname))
        want = ec.clamp(g["B"]) if posB else g["B"]
        assert isinstance(m.B, np.ndarray) and m.B.dtype == np.float64 and m.B.shape == (c["ni"], c["ni"])
        assert np.abs(m.B - want).max() <= ec.RESTATEMENT_VS_REFERENCE[name] and (np.diag(m.B) == 0).all()
        assert (m.B >= 0).all() == posB
        assert sp.issparse(m.U) and m.U.format == "csr" and ec.same_bits(m.U.toarray(), g["X"].toarray())
        assert m.get_user_vectors() is m.U and m.get_item_vectors() is m.B
        tol = 2 * np.abs(g["X"]).sum(axis=1).max() * ec.RESTATEMENT_VS_REFERENCE[name]
        s = m.score(int(users[3]))
        assert s.shape == (c["ni"],) and s.dtype == np.float64 and np.abs(s - g["scores" + tag][3]).max() <= tol
        assert np.abs(m.score_batch(users) - g["scores" + tag]).max() <= tol
        assert abs(m.score(int(pu[0]), int(pi[0])) - g["pair_scores" + tag][0]) <= tol
        assert s[7] == m.score(int(users[3]), 7) == m.score_batch([users[3]])[0][7]
        # the golden's own table assigned: the reference's scores, bit for bit
        m.B = want
        assert ec.same_bits(m.score_batch(users), g["scores" + tag])
        assert ec.same_bits(m.rate_batch(pu, pi, clipping=False), g["pair_scores" + tag])


def test_unknown_users_and_items_raise(device_double):
    m = EASE(lamb=10, verbose=False).fit(ec.dataset("A"))
    for bad in (60, -1):
        with pytest.raises(ScoreException, match="user"):
            m.score(bad)
        with pytest.raises(ScoreException, match="user"):
            m.score(bad, 3)
        with pytest.raises(ScoreException):
            m.score_batch([0, bad])
    for bad in (40, -1):
        with pytest.raises(ScoreException, match="item"):
            m.score(0, bad)
    assert m.rate(60, 0) == m.default_score() == m.global_mean
    u, i = np.array([0, 3, 59, 60, 7, -1]), np.array([1, 39, 0, 2, 40, 3])
    got = m.rate_batch(u, i)
    assert np.array_equal(got, [m.rate(int(a), int(b)) for a, b in zip(u, i)])
    assert got[3] == got[4] == got[5] == m.global_mean and (got >= 1).all() and (got <= 5).all()


def test_bad_lamb_and_ratings_are_value_errors(device_double):
    ds = ec.dataset("A")
    for lamb in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lamb"):
            EASE(lamb=lamb, verbose=False).fit(ds)
    c = ec.case("A")
    r = c["r"].copy()
    r[17] = np.nan
    with pytest.raises(ValueError, match="finite"):
        EASE(lamb=10, verbose=False).fit(Dataset.from_arrays(c["u"], c["i"], r, num_users=60, num_items=40))
    assert ec.FakeEaseModel.built == 0, "refused before anything reaches the device"


def test_fit_retrains_whatever_trainable_says(device_double):
    ds = ec.dataset("A")
    stale = np.full((40, 40), 7.0)
    m = EASE(lamb=10, trainable=False, B=stale, verbose=False)
    assert m.B is stale
    m.fit(ds)
    assert m.B is not stale and np.array_equal(m.B, ec.fit(ec.case_matrix(ec.case("A")), 10, True)) and m.trainable is False
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.lamb = 500
        m.fit(ds)
    assert np.array_equal(m.B, ec.fit(ec.case_matrix(ec.case("A")), 500, True))


def test_scorer_life_cycle_clone_save_load_pickle(device_double, tmp_path):
    ds = ec.dataset("R")
    m = EASE(lamb=10, posB=False, verbose=False, seed=3).fit(ds)
    first = ec.FakeEaseModel.last
    assert ec.FakeEaseModel.built == 1 and m._scorer is first and not first.closed, "fit keeps its handle for scoring"
    assert m._scorer_row_count() == 0 and m.batch_num_items == 100 and m.register_exclusions(1, [0], [0, 0], []) is False
    s = m.score(4)
    m.score(5)
    m.score(5, 7)
    assert ec.FakeEaseModel.built == 1
    # a reassigned B reaches the device
    m.B = ec.clamp(m.B)
    t = m.score(4)
    assert ec.FakeEaseModel.built == 2 and first.closed and not np.array_equal(s, t)
    assert np.array_equal(t, ec.score_user(m.U, m.B, 4)) and np.array_equal(ec.FakeEaseModel.last.table, m.B)
    m.invalidate_scorer()
    assert "_scorer" not in m.__dict__ and ec.FakeEaseModel.last.closed
    assert np.array_equal(m.score(4), t) and ec.FakeEaseModel.built == 3
    # pickling drops the device state; save / load / clone work without a handle
    again = pickle.loads(pickle.dumps(m))
    assert "_scorer" not in again.__dict__ and not hasattr(again, "train_set") and np.array_equal(again.B, m.B)
    assert np.array_equal(again.score(4), t)
    built = ec.FakeEaseModel.built
    back = EASE.load(m.save(str(tmp_path)))
    assert ec.FakeEaseModel.built == built, "neither save nor load needs a handle"
    assert back.trainable is False and "_scorer" not in back.__dict__ and ec.same_bits(back.B, m.B)
    assert np.array_equal(back.score(4), t) and back.score(4, 9) == t[9] and ec.FakeEaseModel.built == built + 1
    c = m.clone({"lamb": 7})
    assert (c.lamb, c.posB, c.seed, c.device, c.name, c.verbose) == (7, False, 3, 0, m.name, False) and not c.is_fitted
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(ds)
    assert np.array_equal(m.score(4), s) and first.closed


def test_rank_orders_score_under_the_pinned_tie_rule(device_double):
    m = EASE(lamb=10, verbose=False).fit(ec.dataset("Ai"))
    for u in (2, 31):
        s = m.score(u)
        ranked, scores = m.rank(u)
        assert np.array_equal(scores, s) and len(ranked) == 40
        assert np.array_equal(ranked, np.lexsort((np.arange(40), s))[::-1]), "descending score, ties by descending item index"
        assert np.array_equal(s[ranked], np.sort(s)[::-1])
    ranked, scores = m.rank(2, item_indices=np.array([5, 1, 30]))
    assert np.array_equal(scores, m.score(2)[[5, 1, 30]]) and sorted(ranked) == [1, 5, 30]


def _feedback(seed=8):
    rs = np.random.RandomState(seed)
    keys = rs.permutation(50 * 30)[:600]
    return [("u%d" % (k // 30), "i%d" % (k % 30), float(rs.randint(1, 6))) for k in keys]


def test_experiment_with_ratio_split(device_double, capsys):
    split = RatioSplit(_feedback(), test_size=0.2, exclude_unknowns=True, seed=123, verbose=False)
    models = [EASE(lamb=10, verbose=False), EASE(lamb=500, posB=False, name="EASE-neg", verbose=False)]
    ex = Experiment(split, models, [mm.RMSE(), mm.Recall(k=10), mm.NDCG(k=10)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["EASEᴿ", "EASE-neg"]
    for r in ex.result:
        row = r.metric_avg_results
        assert {"RMSE", "Recall@10", "NDCG@10"} <= set(row) and np.isfinite(row["RMSE"])
        assert 0.0 < row["Recall@10"] <= 1.0
    capsys.readouterr()


def test_same_report_as_the_references_ease(device_double):
    from oracle import ref_loader

    if not ref_loader.available():
        pytest.skip("reference not available / oracle/_ref not built")
    import importlib

    ns = ref_loader.load()
    RefEASE = importlib.import_module("cornac.models.ease.recom_ease").EASE
    c = ec.case("A")
    data = [("u%d" % u, "i%d" % i, float(r)) for u, i, r in zip(c["u"], c["i"], c["r"])]
    kw = dict(test_size=0.2, exclude_unknowns=True, seed=5, rating_threshold=3.0, verbose=False)
    rm = ns.metrics
    for lamb, posB in ((10.0, True), (0.5, False)):
        ref_test, _ = ns.eval_methods.RatioSplit(data, **kw).evaluate(
            RefEASE(lamb=lamb, posB=posB, verbose=False), [rm.Recall(k=10), rm.NDCG(k=10), rm.AUC(), rm.MAP()], user_based=True)
        my_test, _ = RatioSplit(data, **kw).evaluate(
            EASE(lamb=lamb, posB=posB, verbose=False), [mm.Recall(k=10), mm.NDCG(k=10), mm.AUC(), mm.MAP()], user_based=True)
        assert list(ref_test.metric_avg_results) == list(my_test.metric_avg_results)
        for name, v in ref_test.metric_avg_results.items():
            if "(s)" not in name:
                print("lamb %g posB %s %s: reference %.12g, here %.12g" % (lamb, posB, name, v, my_test.metric_avg_results[name]))
                assert my_test.metric_avg_results[name] == pytest.approx(v, rel=1e-9), (lamb, posB, name)


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------------
EASE_SYMBOLS = ["cornac_hip_ease_create", "cornac_hip_ease_destroy", "cornac_hip_ease_gram", "cornac_hip_ease_invert",
                "cornac_hip_ease_weights", "cornac_hip_ease_fit", "cornac_hip_ease_get_table", "cornac_hip_ease_set_table",
                "cornac_hip_ease_score_users", "cornac_hip_ease_score_pairs"]


def _raw_create(X, n_users=None, n_items=None):
    import ctypes as C

    h = C.c_void_p()
    ip, ix, d = X.indptr.astype(np.int64), X.indices.astype(np.int32), X.data.astype(np.float64)
    _lib.check(_lib.lib().cornac_hip_ease_create(C.byref(h), 0, X.shape[0] if n_users is None else n_users,
                                                 X.shape[1] if n_items is None else n_items, ip.ctypes.data,
                                                 ix.ctypes.data, d.ctypes.data))


def test_abi_declares_and_binds_the_ease_entry_points():
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in EASE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    assert "recom_ease.py" in header[header.index("EASE (Steck 2019)"):]
    assert "ease.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    # argument checks need no device: NULL handles and bad matrices are refused with the invalid-argument status
    L = _lib.lib()
    assert L.cornac_hip_ease_gram(None) == 1 and L.cornac_hip_ease_invert(None, 1.0) == 1 and L.cornac_hip_ease_weights(None, 1) == 1
    assert L.cornac_hip_ease_fit(None, 1.0, 1) == 1 and L.cornac_hip_ease_get_table(None, None) == 1
    assert L.cornac_hip_ease_set_table(None, None) == 1 and L.cornac_hip_ease_score_users(None, None, 0, None) == 1
    assert L.cornac_hip_ease_score_pairs(None, None, None, 0, None) == 1 and L.cornac_hip_ease_destroy(None) == 0
    X = sp.csr_matrix(np.array([[1.0, 2.0], [0.0, 3.0]]))
    bad = X.copy()
    bad.indices[:2] = [1, 0]
    with pytest.raises(_lib.HipError, match="sorted indices"):
        _raw_create(bad)
    for value in (np.nan, np.inf):
        bad = X.copy()
        bad.data[1] = value
        with pytest.raises(_lib.HipError, match="not finite"):
            _raw_create(bad)
    with pytest.raises(_lib.HipError, match="out of range"):
        _raw_create(X, n_items=1)
    with pytest.raises(_lib.HipError, match="positive"):
        _raw_create(X, n_users=0)
