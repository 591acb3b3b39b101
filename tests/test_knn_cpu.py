"""KNN without a GPU: (1) the float64 restatement (tests/knn_cases.py) against what the reference's own UserKNN / ItemKNN
wrote into tests/golden/knn_ref.npz over its compiled extension — the similarity table bit for bit, the scores within the
derived bound — and the fixture kept honest: the order-free selection equals the heap replay, three simpler tie rules do
not; (2) the host logic of cornac_amd.UserKNN / ItemKNN through a device double that calls the restatement; (3) the ABI
entry points are declared and bound."""
import inspect
import os
import pickle
import re

import numpy as np
import pytest
import scipy.sparse as sp

import fake_device
import knn_cases as kc
from conftest import ROOT, load_golden
from cornac_amd import Dataset, Experiment, ItemKNN, RatioSplit, Recommender, ScoreException, UserKNN, _lib
from cornac_amd import knn as knn_mod
from cornac_amd import metrics as mm


@pytest.fixture(scope="module")
def golden():
    return load_golden("knn_ref")


golden_case, dataset, make_model = kc.golden_case, kc.dataset, kc.make_model


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases_and_what_the_issue_counts(golden):
    assert sorted(golden["configs"]) == sorted(kc.CONFIGS) and tuple(golden["ks"]) == kc.KS
    for name, (cname, model, _) in kc.CONFIGS.items():
        g, c = golden_case(golden, name), kc.case(cname)
        assert all(np.array_equal(g[n], c[n]) for n in "uir"), "the golden's triplets are the case's"
        assert g["scores"].shape == (len(kc.KS), kc.N_SCORE_USERS, c["ni"]) and g["pair_scores"].shape == (len(kc.KS), kc.N_PAIRS)
        assert np.isfinite(g["scores"]).all() and g["sim0"].has_sorted_indices
        assert (g["sim0"].data != 0).all() and (g["sim0"].diagonal() != 0).all(), "no stored zeros; the diagonal is kept"
    a, b = kc.case("A"), kc.case("B")
    assert (a["nu"], a["ni"], len(a["r"])) == (60, 40, 600) and (b["nu"], b["ni"], len(b["r"])) == (150, 100, 2000)
    assert set(a["r"]) == {1.0, 2.0, 3.0, 4.0, 5.0} and set(kc.case("Ai")["r"]) == {1.0}
    # a single common column gives exactly +-1, implicit data exactly 1 for every co-rated pair: ties are the normal case
    for name in ("A/item_cosine", "A/user_cosine"):
        d = golden_case(golden, name)["sim0"].data
        print("%s: %d of %d similarities are exactly +-1" % (name, (np.abs(d) == 1).sum(), len(d)))
        assert (np.abs(d) == 1).sum() > 100
    assert (golden_case(golden, "A/item_implicit")["sim0"].data == 1.0).all()
    assert (golden_case(golden, "A/item_implicit")["mean_arr"] == 0).all()


@pytest.mark.parametrize("name", sorted(kc.CONFIGS))
def test_restatement_similarity_is_the_references(golden, name):
    """bit for bit, the sparsity pattern included; the host preparation with it (mean_arr and the centred ratings)"""
    g = golden_case(golden, name)
    W, mean, rat = kc.prepare_config(name)
    S = kc.similarity(W)
    assert np.array_equal(S.indptr, g["sim0"].indptr) and np.array_equal(S.indices, g["sim0"].indices), "sparsity pattern"
    diff = kc.max_rel_diff(S.data, g["sim0"].data)
    print("%s: restatement vs reference, un-amplified: %.3g relative (recorded %.3g)" % (name, diff, kc.RESTATEMENT_VS_REFERENCE[name]))
    assert diff <= kc.RESTATEMENT_VS_REFERENCE[name] and kc.RESTATEMENT_VS_REFERENCE[name] <= kc.CEILING / 16
    if kc.RESTATEMENT_VS_REFERENCE[name] == 0:
        assert kc.same_csr(S, g["sim0"])
    assert np.array_equal(mean, g["mean_arr"]) and kc.same_csr(rat, g["rat"])


def test_the_quotient_is_the_compiled_one_not_the_written_one(golden):
    """sqrt(d1) * sqrt(d2), as the source spells it, is NOT what the extension computes once built with -ffast-math"""
    g = golden_case(golden, "A/item_cosine")
    S = kc.similarity_as_written(kc.prepare_config("A/item_cosine")[0])
    assert np.array_equal(S.indices, g["sim0"].indices)
    diff = kc.max_rel_diff(S.data, g["sim0"].data)
    print("as written vs reference: %.3g relative" % diff)
    assert 0 < diff < 1e-15


@pytest.mark.parametrize("name", sorted(n for n in kc.CONFIGS if kc.CONFIGS[n][2].get("amplify", 1.0) != 1.0))
def test_amplified_table_within_two_ulp(golden, name):
    g = golden_case(golden, name)
    alpha = kc.CONFIGS[name][2]["amplify"]
    for label, got in (("element by element", kc.amplify(g["sim0"], alpha)),
                       ("the model's vectorised form", knn_mod._amplify(g["sim0"].copy(), alpha))):
        ulps, rel = kc.ulp_diff(got.data, g["sim"].data), kc.max_rel_diff(got.data, g["sim"].data)
        print("%s, %s: %d ulp, %.3g relative to the golden (allowed: 2 ulp)" % (name, label, ulps, rel))
        assert ulps <= 2
    assert not np.array_equal(g["sim"].data, g["sim0"].data)


@pytest.mark.parametrize("name", sorted(kc.CONFIGS))
def test_restatement_scores_agree_with_the_reference(golden, name):
    g = golden_case(golden, name)
    cname, model, _ = kc.CONFIGS[name]
    c = kc.case(cname)
    N, Q, user_mode = kc.tables(model, g["sim"], g["rat"])
    users, (pu, pi) = kc.score_users(c), kc.score_pairs(c)
    worst = 0.0
    for a, k in enumerate(kc.KS):
        tol = kc.score_tolerance(k, np.abs(g["r"]).max(), np.abs(g["mean_arr"]).max())
        for select in (kc.replay_select, kc.orderfree_select):
            got = np.array([g["mean_arr"][u] + kc.score_row(N, Q, int(u), user_mode, k, select) for u in users])
            diff = np.abs(got - g["scores"][a]).max()
            worst = max(worst, diff / tol)
            assert diff <= tol, (k, select.__name__, diff, tol)
        v = [np.asarray(Q[int(u)].todense()).ravel() for u in pu]
        pairs = np.array([g["mean_arr"][u] + kc.score_item(N, v[n], int(i), user_mode, k) for n, (u, i) in enumerate(zip(pu, pi))])
        assert np.abs(pairs - g["pair_scores"][a]).max() <= tol
    print("%s: largest score difference is %.3g of its bound" % (name, worst))


def test_orderfree_selection_equals_the_replay_on_tie_heavy_inputs():
    rs = np.random.RandomState(0)
    for trial in range(20000):
        n, k = int(rs.randint(0, 40)), int(rs.randint(1, 12))
        levels = int(rs.randint(1, 6))
        w = rs.choice(np.array([-1.0, -0.5, 0.25, 0.5, 1.0, 2.0])[:levels + 1], n)
        s = rs.choice(np.array([-2.0, -1.0, 1e-8, 1.0, 2.0, 3.0])[:int(rs.randint(1, 7))], n)
        cands = [(float(a), float(b), j) for j, (a, b) in enumerate(zip(w, s))]
        assert sorted(kc.orderfree_select(cands, k)) == sorted(kc.replay_select(cands, k)), (trial, cands, k)


@pytest.mark.parametrize("name", ["A/item_cosine", "A/user_cosine"])
def test_simpler_tie_rules_fail_on_case_a(golden, name):
    """keeps the fixture honest: at k = 3 the golden has ties at the k-th weight, and none of the simpler rules gives the
    reference's outputs there"""
    g = golden_case(golden, name)
    cname, model, _ = kc.CONFIGS[name]
    c = kc.case(cname)
    N, Q, user_mode = kc.tables(model, g["sim"], g["rat"])
    users, k, a = kc.score_users(c), 3, kc.KS.index(3)
    tol = kc.score_tolerance(k, np.abs(g["r"]).max(), np.abs(g["mean_arr"]).max())
    ties = sum(kc.boundary_ties(N, Q, int(u), user_mode, k) for u in users)
    assert ties > 0
    for rule, select in kc.SIMPLER_TIE_RULES.items():
        got = np.array([g["mean_arr"][u] + kc.score_row(N, Q, int(u), user_mode, k, select) for u in users])
        wrong = int((np.abs(got - g["scores"][a]) > tol).sum())
        print("%s: %d boundary ties among %d outputs; 'ties by %s' gets %d wrong" % (name, ties, got.size, rule, wrong))
        assert wrong > 0, rule


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
class FakeKnnSimilarity:
    """_lib.KnnSimilarity served by the restatement; records what the model handed over"""
    last = None

    def __init__(self, W, device=0):
        assert sp.issparse(W) and W.format == "csr" and W.dtype == np.float64
        self.W, self.device, self.closed = W.copy(), device, False
        FakeKnnSimilarity.last = self

    def run(self, rows_per_pass=0):
        return kc.similarity(self.W)

    def close(self):
        self.closed = True


class FakeKnnScorer:
    MAX_K = _lib.KNN_MAX_K
    built = 0
    last = None

    def __init__(self, N, Q, user_mode, device=0):
        assert N.shape[1] == Q.shape[1]
        self.N, self.Q, self.user_mode, self.closed = N.copy(), Q.copy(), bool(user_mode), False
        FakeKnnScorer.built += 1
        FakeKnnScorer.last = self

    def score_users(self, users, k):
        assert 1 <= k <= self.MAX_K
        return np.array([kc.score_row(self.N, self.Q, int(u), self.user_mode, k) for u in users]).reshape(len(users), self.N.shape[0])

    def score_pairs(self, users, items, k):
        assert 1 <= k <= self.MAX_K
        return np.array([kc.score_item(self.N, np.asarray(self.Q[int(u)].todense()).ravel(), int(i), self.user_mode, k)
                         for u, i in zip(users, items)])

    def close(self):
        self.closed = True


@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "KnnSimilarity", FakeKnnSimilarity)
    monkeypatch.setattr(_lib, "KnnScorer", FakeKnnScorer)
    monkeypatch.chdir(tmp_path)
    FakeKnnScorer.built, FakeKnnScorer.last, FakeKnnSimilarity.last = 0, None, None


def test_constructors_are_the_references():
    for cls, default_name in ((UserKNN, "UserKNN"), (ItemKNN, "ItemKNN")):
        m = cls()
        assert (m.name, m.k, m.similarity, m.mean_centered, m.weighting, m.amplify, m.trainable, m.verbose, m.seed, m.device) == \
            (default_name, 20, "cosine", False, None, 1.0, True, True, None, 0)
        assert list(inspect.signature(cls.__init__).parameters)[1:] == [
            "name", "k", "similarity", "mean_centered", "weighting", "amplify", "num_threads", "trainable", "verbose", "seed",
            "device"]
        assert isinstance(m, Recommender) and cls(num_threads=7).num_threads == 7
        with pytest.raises(ValueError, match="Invalid similarity choice"):
            cls(similarity="jaccard")
        with pytest.raises(ValueError, match="Invalid weighting choice"):
            cls(weighting="tfidf")
        for bad in (0, -1, _lib.KNN_MAX_K + 1):
            with pytest.raises(ValueError, match=str(_lib.KNN_MAX_K)):
                cls(k=bad)
        assert cls(k=_lib.KNN_MAX_K).k == _lib.KNN_MAX_K and cls(k=1).k == 1
    assert _lib.KNN_MAX_K >= 64 and knn_mod.KNN_MAX_K == _lib.KNN_MAX_K


@pytest.mark.parametrize("name", sorted(kc.CONFIGS))
def test_fit_gives_the_goldens_tables(device_double, golden, name):
    g = golden_case(golden, name)
    _, model, kw = kc.CONFIGS[name]
    m = make_model(name).fit(dataset(name))
    assert FakeKnnSimilarity.last.closed and kc.same_csr(FakeKnnSimilarity.last.W, kc.prepare_config(name)[0])
    assert sp.issparse(m.sim_mat) and m.sim_mat.format == "csr" and m.sim_mat.dtype == np.float64
    assert np.array_equal(m.mean_arr, g["mean_arr"])
    assert np.array_equal(m.sim_mat.indptr, g["sim"].indptr) and np.array_equal(m.sim_mat.indices, g["sim"].indices)
    if kw.get("amplify", 1.0) == 1.0:
        assert kc.same_csr(m.sim_mat, g["sim"])
    else:
        assert kc.ulp_diff(m.sim_mat.data, g["sim"].data) <= 2
    if model == "user":
        assert kc.same_csr(m.iu_mat, g["rat"]) and not hasattr(m, "ui_mat")
    else:
        assert kc.same_csr(m.ui_mat, g["rat"]) and not hasattr(m, "iu_mat")
    # scores: the golden's table assigned (the amplified one differs in its last bits), k = 5
    m.sim_mat = g["sim"]
    m.k = 5
    a = kc.KS.index(5)
    tol = kc.score_tolerance(5, np.abs(g["r"]).max(), np.abs(g["mean_arr"]).max())
    c = kc.case(kc.CONFIGS[name][0])
    users, (pu, pi) = kc.score_users(c)[:3], kc.score_pairs(c)
    for b, u in enumerate(users):
        s = m.score(int(u))
        assert s.shape == (c["ni"],) and s.dtype == np.float64 and np.abs(s - g["scores"][a, b]).max() <= tol
    assert np.abs(m.score_batch(users) - g["scores"][a, :3]).max() <= tol
    for n in range(5):
        assert abs(m.score(int(pu[n]), int(pi[n])) - g["pair_scores"][a, n]) <= tol
    sc = FakeKnnScorer.last
    assert sc.user_mode == (model == "user") and sc.N.shape[0] == c["ni"]
    assert FakeKnnScorer.built == 1, "one scorer for all of these calls"


@pytest.mark.parametrize("cls", [UserKNN, ItemKNN])
def test_unknown_users_and_items_raise(device_double, cls):
    m = cls(verbose=False).fit(dataset("A/user_cosine"))
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
    m.k = _lib.KNN_MAX_K + 1
    with pytest.raises(ValueError, match=str(_lib.KNN_MAX_K)):
        m.score(0)


@pytest.mark.parametrize("name", ["A/user_pearson", "A/item_adjusted"])
def test_scorer_life_cycle_clone_save_load_pickle(device_double, golden, name, tmp_path):
    ds = dataset(name)
    m = make_model(name, k=3).fit(ds)
    assert "_scorer" not in m.__dict__, "built lazily"
    s = m.score(4)
    first = FakeKnnScorer.last
    assert FakeKnnScorer.built == 1 and m._scorer is first and m._scorer_row_count() == 0
    m.score(5)
    m.score(5, 7)
    assert FakeKnnScorer.built == 1
    # a replaced sim_mat reaches the scorer
    half = m.sim_mat.copy()
    half.data = np.where(np.arange(len(half.data)) % 2 == 0, half.data, -half.data)
    m.sim_mat = half
    t = m.score(4)
    assert FakeKnnScorer.built == 2 and first.closed and not np.array_equal(s, t)
    N, Q, um = kc.tables(kc.CONFIGS[name][1], half, m.iu_mat if um_is_user(name) else m.ui_mat)
    assert np.array_equal(t, m.mean_arr[4] + kc.score_row(N, Q, 4, um, 3))
    m.invalidate_scorer()
    assert "_scorer" not in m.__dict__ and FakeKnnScorer.last.closed
    m.score(4)
    assert FakeKnnScorer.built == 3
    # pickling drops the device state; save / load / clone work
    again = pickle.loads(pickle.dumps(m))
    assert "_scorer" not in again.__dict__ and not hasattr(again, "train_set") and kc.same_csr(again.sim_mat, m.sim_mat)
    assert np.array_equal(again.score(4), t)
    back = type(m).load(m.save(str(tmp_path)))
    assert back.trainable is False and np.array_equal(back.score(4), t) and np.array_equal(back.mean_arr, m.mean_arr)
    c = m.clone()
    assert (c.k, c.similarity, c.mean_centered, c.weighting, c.amplify, c.seed, c.device, c.name) == \
        (3, m.similarity, m.mean_centered, None, 1.0, 1, 0, m.name)
    assert not c.is_fitted and not hasattr(c, "sim_mat") and m.clone({"k": 7}).k == 7
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(ds)
    assert "_scorer" not in m.__dict__, "fit drops the scorer"
    assert np.array_equal(m.score(4), s)


def um_is_user(name):
    return kc.CONFIGS[name][1] == "user"


def test_rank_orders_score_under_the_pinned_tie_rule(device_double):
    m = make_model("A/item_implicit", k=3).fit(dataset("A/item_implicit"))
    s = m.score(2)
    assert len(np.unique(s)) < len(s), "implicit data: many tied scores"
    ranked, scores = m.rank(2, k=10)
    assert np.array_equal(scores, s) and len(ranked) == 40
    assert np.array_equal(ranked, np.lexsort((np.arange(40), s))[::-1]), "descending score, ties by descending item index"


def test_rate_batch_is_rate_pair_by_pair(device_double):
    m = make_model("A/user_cosine", k=5).fit(dataset("A/user_cosine"))
    u, i = np.array([0, 3, 59, 60, 7, -1]), np.array([1, 39, 0, 2, 40, 3])
    got = m.rate_batch(u, i)
    assert np.array_equal(got, [m.rate(int(a), int(b)) for a, b in zip(u, i)])
    assert got[3] == got[4] == got[5] == m.global_mean and (got >= 1).all() and (got <= 5).all()
    raw = m.rate_batch(u[:3], i[:3], clipping=False)
    assert np.array_equal(raw, [m.score(int(a), int(b)) for a, b in zip(u[:3], i[:3])])


def test_experiment_over_the_examples_models(device_double, capsys):
    """the reference's examples/knn_movielens.py with synthetic feedback and the import changed: RatioSplit + Experiment
    over its eight models, RMSE as there plus Recall"""
    rs = np.random.RandomState(8)
    keys = rs.permutation(50 * 30)[:600]
    data = [("u%d" % (k // 30), "i%d" % (k % 30), float(rs.randint(1, 6))) for k in keys]
    split = RatioSplit(data, test_size=0.2, exclude_unknowns=True, seed=123, verbose=False)
    K = 50
    models = [UserKNN(k=K, similarity="cosine", name="UserKNN-Cosine", verbose=False),
              UserKNN(k=K, similarity="pearson", name="UserKNN-Pearson", verbose=False),
              UserKNN(k=K, similarity="cosine", amplify=2.0, name="UserKNN-Amplified", verbose=False),
              UserKNN(k=K, similarity="cosine", weighting="idf", name="UserKNN-IDF", verbose=False),
              UserKNN(k=K, similarity="cosine", weighting="bm25", name="UserKNN-BM25", verbose=False),
              ItemKNN(k=K, similarity="cosine", name="ItemKNN-Cosine", verbose=False),
              ItemKNN(k=K, similarity="pearson", name="ItemKNN-Pearson", verbose=False),
              ItemKNN(k=K, similarity="cosine", mean_centered=True, name="ItemKNN-AdjustedCosine", verbose=False)]
    ex = Experiment(split, models, [mm.RMSE(), mm.Recall(k=10)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == [m.name for m in models]
    for r in ex.result:
        row = r.metric_avg_results
        assert {"RMSE", "Recall@10"} <= set(row) and np.isfinite(row["RMSE"]) and 0 < row["RMSE"] < 4
        assert 0.0 <= row["Recall@10"] <= 1.0
    capsys.readouterr()


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------------
def test_abi_declares_and_binds_the_knn_entry_points():
    sim = ["cornac_hip_knn_sim_create", "cornac_hip_knn_sim_run", "cornac_hip_knn_sim_nnz", "cornac_hip_knn_sim_get",
           "cornac_hip_knn_sim_destroy"]
    scorer = ["cornac_hip_knn_scorer_create", "cornac_hip_knn_scorer_score_users", "cornac_hip_knn_scorer_score_pairs",
              "cornac_hip_knn_scorer_destroy"]
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in sim + scorer:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    block = header[header.index("Neighbourhood models"):]
    assert "similarity.pyx" in block and "similarity.h" in block and "recom_knn.py" in block
    assert int(re.search(r"#define CORNAC_HIP_KNN_MAX_K (\d+)", header).group(1)) == _lib.KNN_MAX_K == _lib.KnnScorer.MAX_K
    assert "knn.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    # argument checks need no device: NULL handles and bad tables are refused with the invalid-argument status
    L = _lib.lib()
    assert L.cornac_hip_knn_sim_run(None, 0) == 1 and L.cornac_hip_knn_sim_get(None, None, None, None) == 1
    assert L.cornac_hip_knn_scorer_score_users(None, None, 0, 1, None) == 1
    assert L.cornac_hip_knn_scorer_score_pairs(None, None, None, 0, 1, None) == 1
    assert L.cornac_hip_knn_sim_destroy(None) == 0 and L.cornac_hip_knn_scorer_destroy(None) == 0
    W = sp.csr_matrix(np.array([[1.0, 2.0], [0.0, 3.0]]))
    W.indices[:2] = [1, 0]   # unsorted
    W.has_sorted_indices = True
    with pytest.raises(_lib.HipError, match="sorted indices"):
        _raw_sim_create(W)


def _raw_sim_create(W):
    import ctypes as C

    h = C.c_void_p()
    ip, ix, d = W.indptr.astype(np.int64), W.indices.astype(np.int32), W.data.astype(np.float64)
    _lib.check(_lib.lib().cornac_hip_knn_sim_create(C.byref(h), 0, 2, 2, ip.ctypes.data, ix.ctypes.data, d.ctypes.data))
