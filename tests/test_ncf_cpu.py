"""NCF without a GPU: (1) the float64 restatement of tests/ncf_cases.py against the golden that the reference's own GMF / MLP /
NeuMF modules and _fit_pt wrote (tables, state, losses, scores), the tolerance rule's condition and the kink condition for
every case; (2) the model classes' host logic over a device double served by the restatement: the seeded fit against the
reference's own seeded fit, state_dict, from_pretrained, save / load / clone, the refusals, an Experiment; (3) the ABI."""
import inspect
import os
import pickle
import re

import numpy as np
import pytest

import fake_device
import ncf_cases as nc
from conftest import ROOT, load_golden
from cornac_amd import GMF, MLP, NeuMF, Experiment, RatioSplit, Recommender, _lib
from cornac_amd import metrics as mm

CLASSES = {"GMF": GMF, "MLP": MLP, "NeuMF": NeuMF}
STATS = ("d_ref", "d_ref_s1", "d_ref_s2", "move", "max", "max_s1", "max_s2")


@pytest.fixture(scope="module")
def golden():
    return load_golden("ncf_ref")


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases_the_issue_counts(golden):
    assert sorted(golden["cases"]) == sorted(list(nc.CASES) + list(nc.SEEDED))
    C = nc.CASES.values()
    assert {1, 8, 33, 64, 65} <= {c["f"] for c in C}
    assert {(2, 1), (64, 32, 16, 8), (66, 33, 7), (130, 65, 3)} <= {c["layers"] for c in C}
    assert {1, 5, 64, 65, 1280} <= {n for c in C for n in c["steps"]} and {0, 4} == {c["nn"] for c in C} and {0.0, 0.01} == {c["reg"] for c in C}
    assert {(c["kind"], c["learner"]) for n, c in nc.CASES.items() if n.startswith("kl/")} == {(k, l) for k in nc.KINDS for l in nc.LEARNERS}
    assert {(c["kind"], c["act"]) for n, c in nc.CASES.items() if n.startswith("act/")} == {(k, a) for k in ("MLP", "NeuMF") for a in nc.ACTS}
    for name, c in nc.CASES.items():
        names = nc.NAMES(c["kind"], c["layers"])
        assert len(c["steps"]) >= 3 and c["steps"][-1] <= c["steps"][0], name
        for kind in STATS:
            assert golden["%s/%s" % (name, kind)].shape == (len(names),) and np.isfinite(golden["%s/%s" % (name, kind)]).all()
        share = nc.check_condition(golden, name)
        print("%s: the device's tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
        for q, n in enumerate(names):   # exactly the tables without a gradient stay in place
            assert (golden[name + "/move"][q] == 0.0) == (n in nc.UNUSED(c["kind"])), (name, n)
        batches = nc.case_batches(c)
        later = np.concatenate([b[0] for b in batches[1:]])
        assert batches[0][0][0] == 0 and 0 not in later, "user 0: the first step only"
        assert all((b[1] != c["ni"] - 1).all() for b in batches), "the last item never appears"
        assert all((b[1] == 1).sum() >= len(b[1]) // 3 for b in batches if len(b[1]) >= 5), "item 1 repeats"
        assert all(b[2].all() for b in batches) == (c["nn"] == 0)
    for name in nc.SEEDED:
        print("%s: %.3g of a table's movement" % (name, nc.check_condition(golden, name)))
    for name in nc.FULL_CASES:
        c = nc.CASES[name]
        assert golden[name + "/scores"].shape == (len(nc.score_users(c)), c["ni"]) and golden[name + "/losses"].shape == (len(c["steps"]),)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ncf_ref.npz")) < 1024 * 1024


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_kinked_activations_stay_clear_of_their_kinks_and_sat_saturates(name):
    run = nc.run_case(name)   # (asserts 6 < max|logit| < 10 on the first step of a "sat" case)
    c = nc.CASES[name]
    if c["act"] in nc.KINKS and c["kind"] != "GMF":
        assert run["r"].kink_distance >= nc.KINK_MARGIN, "%s: a pre-activation lies %.3g from a kink" % (name, run["r"].kink_distance)
    assert np.isfinite(run["losses"]).all()


@pytest.mark.parametrize("name", nc.FULL_CASES)
def test_restatement_against_the_references_tables(golden, name):
    c, run = nc.CASES[name], nc.run_case(name)
    r = run["r"]
    for q, n in enumerate(nc.NAMES(c["kind"], c["layers"])):
        for kind, mine, stat in (("P", r.P, "d_ref"), ("S1", r.S1, "d_ref_s1"), ("S2", r.S2, "d_ref_s2")):
            ref = golden["%s/%s/%s" % (name, kind, n)]
            d = np.abs(ref.astype(np.float64) - mine[n]).max()
            assert d == golden["%s/%s" % (name, stat)][q], (name, kind, n, d)
            assert d <= 1e-6, (name, kind, n, d)
    assert np.abs(golden[name + "/losses"] - run["losses"]).max() <= 1e-5 * max(1.0, np.abs(run["losses"]).max())
    f32 = nc.new_restatement(c, {n: golden["%s/P/%s" % (name, n)] for n in r.names})
    tol = 64 * 2.0 ** -24 * (1 + np.abs(f32.logits(nc.score_users(c))).max())
    assert np.abs(f32.scores(nc.score_users(c)) - golden[name + "/scores"]).max() <= tol
    assert np.abs(f32.pair_scores(*nc.score_pairs(c)) - golden[name + "/pair_scores"]).max() <= tol


def test_restatement_gradients_are_the_loss_slopes():
    """one sgd step moves each table by -lr * dL/dtable: compared with central differences of the restated loss"""
    c = dict(nc.CASES["kl/NeuMF/sgd"])
    init = {n: a.astype(np.float64) for n, a in nc.case_params(c).items()}
    u, i, y = nc.case_batches(c)[0]

    def loss_at(tabs):
        r = nc.new_restatement(c, tabs)
        p = r.forward(u, i)["p"]
        return float(np.mean(-(y * np.log(p) + (1 - y) * np.log1p(-p))))

    r = nc.new_restatement(c, init)
    r.step(u, i, y, 1.0, 0.0, "sgd")
    rs = np.random.RandomState(0)
    for n in r.names:
        grad = init[n] - r.P[n]
        if n in nc.UNUSED("NeuMF"):
            assert not grad.any()
            continue
        for _ in range(3):
            at = tuple(rs.randint(0, s) for s in init[n].shape)
            if "user_embedding" in n:
                at = (int(u[rs.randint(len(u))]),) + at[1:]
            hi, lo = {k: v.copy() for k, v in init.items()}, {k: v.copy() for k, v in init.items()}
            hi[n][at] += 1e-6
            lo[n][at] -= 1e-6
            slope = (loss_at(hi) - loss_at(lo)) / 2e-6
            assert abs(slope - grad[at]) <= 1e-8 + 1e-5 * abs(slope), (n, at, slope, grad[at])


def test_rank_case_has_distinct_top_probabilities(golden):
    """the GPU's GMF ranking check compares orderings where the reference's float32 probabilities do not tie"""
    s = golden[nc.RANK_CASE + "/all_scores"]
    distinct = [len(np.unique(np.sort(row)[::-1][:11])) == 11 for row in s]
    assert np.mean(distinct) >= 0.9


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "NcfModel", nc.FakeNcfModel)
    monkeypatch.chdir(tmp_path)
    nc.FakeNcfModel.built, nc.FakeNcfModel.last = 0, None


def test_constructors_are_the_references():
    base = ["reg", "num_epochs", "batch_size", "num_neg", "lr", "learner", "backend", "early_stopping", "trainable", "verbose", "seed", "device"]
    assert list(inspect.signature(GMF.__init__).parameters)[1:] == ["name", "num_factors"] + base
    assert list(inspect.signature(MLP.__init__).parameters)[1:] == ["name", "layers", "act_fn"] + base
    assert list(inspect.signature(NeuMF.__init__).parameters)[1:] == ["name", "num_factors", "layers", "act_fn"] + base
    for cls in CLASSES.values():
        m = cls()
        assert (m.name, m.reg, m.num_epochs, m.batch_size, m.num_neg, m.lr, m.learner, m.backend, m.early_stopping, m.trainable, m.verbose,
                m.seed, m.device) == (cls.__name__, 0.0, 20, 256, 4, 0.001, "adam", "tensorflow", None, True, True, None, 0)
        assert isinstance(m, Recommender) and not m.is_fitted and not hasattr(m, "params")
    assert (GMF().num_factors, MLP().layers, MLP().act_fn, NeuMF().num_factors, NeuMF().layers) == (8, (64, 32, 16, 8), "relu", 8, (64, 32, 16, 8))
    c = NeuMF(num_factors=5, layers=(12, 7, 5), seed=3, lr=0.1).clone({"num_neg": 2})
    assert (c.num_factors, c.layers, c.seed, c.lr, c.num_neg) == (5, (12, 7, 5), 3, 0.1, 2) and not c.is_fitted


@pytest.mark.parametrize("name", sorted(nc.SEEDED))
def test_seeded_fit_reproduces_the_references_seeded_fit(device_double, golden, name):
    """holds the construction order of the initial draws and the sampler's draw order: the reference's own seeded fit, with its
    own initial tables and its own uir_iter, against the model class over the restatement"""
    c = nc.SEEDED[name]
    m = nc.seeded_model(c).fit(nc.seeded_dataset(c))
    fake = nc.FakeNcfModel.last
    assert len(fake.epochs) == c["epochs"] and fake.sampled == 0 and len(m.loss_history) == c["epochs"]
    ptr, users, items, labels = fake.epochs[0]
    assert np.diff(ptr).max() == c["bs"] * (1 + c["nn"]) and labels[:c["bs"]].all() and not labels[c["bs"]:ptr[1]].any()
    assert np.array_equal(users[c["bs"]:ptr[1]], users[:c["bs"]].repeat(c["nn"])), "negatives follow user-major"
    for q, n in enumerate(nc.case_names(name)):
        ref = golden["%s/P/%s" % (name, n)]
        tol = nc.tolerance(golden[name + "/d_ref"][q], golden[name + "/max"][q])
        d = np.abs(ref.astype(np.float64) - fake.r.P[n]).max()
        print("%s %s: %.3g (tolerance %.3g)" % (name, n, d, tol))
        assert d <= tol and m.params[n].dtype == np.float32
    f32_tol = 64 * 2.0 ** -24 * 8
    users = nc.score_users(c)
    assert np.abs(m.score_batch(users).astype(np.float64) - golden[name + "/scores"]).max() <= f32_tol
    pu, pi = nc.score_pairs(c)
    assert np.abs(np.array([m.score(int(u), int(i)) for u, i in zip(pu, pi)], np.float64) - golden[name + "/pair_scores"]).max() <= f32_tol
    # without a seed the samples are drawn on the device
    nc.seeded_model(c, seed=None, num_epochs=2).fit(nc.seeded_dataset(c))
    assert nc.FakeNcfModel.last.sampled == 2


def test_state_dict_round_trip_save_load_pickle(device_double, tmp_path):
    import torch

    for name in sorted(nc.SEEDED):
        c = nc.SEEDED[name]
        ds = nc.seeded_dataset(c)
        m = nc.seeded_model(c, num_epochs=1).fit(ds)
        names = nc.case_names(name)
        sd = m.state_dict()
        want = nc.shapes(c["kind"], c["nu"], c["ni"], c["f"], c["layers"])
        assert list(sd) == list(names) and all(sd[n].shape == want[n] and sd[n] is not m.params[n] for n in names)
        s4 = m.score(4)
        assert s4.dtype == np.float32 and s4.shape == (c["ni"],) and (s4 > 0).all() and (s4 < 1).all()
        assert s4[9] == m.score(4, 9) == m.score_batch([4])[0][9]
        other = CLASSES[c["kind"]]()
        other.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})   # tensors, as the reference's state_dict holds
        assert (getattr(other, "num_factors", 0) if c["kind"] != "MLP" else 0, tuple(getattr(other, "layers", ())) if c["kind"] != "GMF" else ()) == (c["f"], c["layers"])
        other.act_fn = c["act"]
        other.num_users, other.num_items = c["nu"], c["ni"]
        assert np.array_equal(other.score(4), s4)
        again = pickle.loads(pickle.dumps(m))
        assert "_ncf_handle" not in again.__dict__ and not hasattr(again, "train_set") and np.array_equal(again.score(4), s4)
        back = CLASSES[c["kind"]].load(m.save(str(tmp_path)))
        assert back.trainable is False and "_ncf_handle" not in back.__dict__ and "_scorer" not in back.__dict__
        assert all(np.array_equal(back.params[n], m.params[n]) for n in names) and np.array_equal(back.score_batch([4, 5]), m.score_batch([4, 5]))
        m.params["logit.bias"] = m.params["logit.bias"] + np.float32(1.0)   # an edited table reaches the device
        assert not np.array_equal(m.score(4), s4)
        with pytest.raises(KeyError):
            other.load_state_dict({n: a for n, a in sd.items() if n != names[-1]})
        bad = dict(sd)
        bad[names[-1]] = np.zeros((2,), np.float32)
        with pytest.raises(ValueError, match="expected"):
            other.load_state_dict(bad)
        from oracle import ref_loader

        if ref_loader.available():   # the arrays load into the reference's module and back
            import importlib

            ref_loader.load()
            mod = importlib.import_module("cornac.models.ncf.backend_pt")
            net = {"GMF": lambda: mod.GMF(c["nu"], c["ni"], c["f"]), "MLP": lambda: mod.MLP(c["nu"], c["ni"], c["layers"], c["act"]),
                   "NeuMF": lambda: mod.NeuMF(c["nu"], c["ni"], c["f"], c["layers"], c["act"])}[c["kind"]]()
            net.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})
            fresh = CLASSES[c["kind"]]()
            fresh.load_state_dict(net.state_dict())
            assert all(np.array_equal(fresh.params[n], sd[n]) for n in names)


def test_from_pretrained_is_section_3_4_1(device_double):
    cg, cm, cn = (nc.SEEDED["seeded/" + k] for k in nc.KINDS)
    ds = nc.seeded_dataset(cn)
    g, p = nc.seeded_model(cg, num_epochs=1).fit(ds), nc.seeded_model(cm, num_epochs=1).fit(ds)
    n = nc.seeded_model(cn, num_epochs=0).from_pretrained(g, p, alpha=0.25)
    assert n.pretrained and n.alpha == 0.25
    n.fit(ds)
    a, b = np.float32(0.25), np.float32(0.75)
    assert np.array_equal(n.params["logit.weight"], np.concatenate([a * g.params["logit.weight"], b * p.params["logit.weight"]], axis=1))
    assert np.array_equal(n.params["logit.bias"], a * g.params["logit.bias"] + b * p.params["logit.bias"])
    assert all(np.array_equal(n.params["gmf." + k], v) for k, v in g.params.items())
    assert all(np.array_equal(n.params["mlp." + k], v) for k, v in p.params.items())
    assert n.params["logit.weight"].dtype == np.float32 and n.params["logit.weight"].shape == (1, 10)
    # the combined model scores between its parents' logits' blend: at alpha the logit is the blend itself
    lg = lambda s: np.log(s.astype(np.float64) / (1 - s.astype(np.float64)))   # noqa: E731
    assert np.abs(lg(n.score(3)) - (0.25 * lg(g.score(3)) + 0.75 * lg(p.score(3)))).max() < 1e-4
    assert "pretrained_gmf" not in pickle.loads(pickle.dumps(n)).__dict__
    with pytest.raises(ValueError, match="pretrained"):
        nc.seeded_model(dict(cn, f=7, layers=(12, 7, 7))).from_pretrained(g, p).fit(ds)


def test_refusals(device_double):
    c = nc.SEEDED["seeded/NeuMF"]
    ds = nc.seeded_dataset(c)
    with pytest.raises(NotImplementedError, match="early_stopping"):
        nc.seeded_model(c, early_stopping={"min_delta": 0.0, "patience": 1}).fit(ds)
    with pytest.raises(ValueError, match="learners"):
        nc.seeded_model(c, learner="lbfgs").fit(ds)
    with pytest.raises(ValueError, match="act_fn"):
        nc.seeded_model(c, act_fn="gelu").fit(ds)
    with pytest.raises(ValueError, match="must equal num_factors"):
        nc.seeded_model(c, num_factors=4).fit(ds)
    assert nc.FakeNcfModel.built == 0
    m = nc.seeded_model(c, trainable=False).fit(ds)
    assert nc.FakeNcfModel.built == 0 and not hasattr(m, "params")
    m = nc.seeded_model(c, backend="pytorch", num_epochs=1).fit(ds)   # accepted and ignored
    first = nc.FakeNcfModel.last
    m.fit(ds)   # every fit starts from new tables and a new optimiser, as the reference's does
    assert nc.FakeNcfModel.last is not first and first.closed and nc.FakeNcfModel.last.r.t == len(nc.FakeNcfModel.last.epochs[0][0]) - 1


def test_gmf_scoring_tables_order_items_as_score_does(device_double):
    c = nc.SEEDED["seeded/GMF"]
    m = nc.seeded_model(c).fit(nc.seeded_dataset(c))
    U, V, ib, ub = m._scoring_tables()
    assert U.shape == (c["nu"], c["f"]) and V is m.params["item_embedding.weight"] and (ub == 0).all() and (ib == m.params["logit.bias"][0]).all()
    assert m._scoring_tables()[0] is U, "cached: the fused scorer is not rebuilt per call"
    for u in (0, 3, c["nu"] - 1):
        s = m.score(u).astype(np.float64)
        logits = V.astype(np.float64) @ U[u] + ib
        assert np.array_equal(np.argsort(-logits, kind="stable"), np.argsort(-s, kind="stable")) or len(np.unique(s)) < len(s)
        ranked, scores = m.rank(u)
        assert np.array_equal(scores, m.score(u)) and np.array_equal(ranked[:5], np.argsort(-logits, kind="stable")[:5])


def _feedback(seed=8):
    rs = np.random.RandomState(seed)
    keys = rs.permutation(50 * 30)[:600]
    return [("u%d" % (k // 30), "i%d" % (k % 30), float(rs.randint(1, 6))) for k in keys]


def test_experiment_with_ratio_split(device_double, capsys):
    split = RatioSplit(_feedback(), test_size=0.2, exclude_unknowns=True, seed=123, verbose=False)
    kw = dict(num_epochs=2, batch_size=32, num_neg=2, lr=0.01, seed=1, verbose=False)
    models = [GMF(num_factors=4, **kw), MLP(layers=(8, 4), **kw), NeuMF(num_factors=4, layers=(8, 4), act_fn="tanh", **kw)]
    ex = Experiment(split, models, [mm.Recall(k=10), mm.NDCG(k=10)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["GMF", "MLP", "NeuMF"]
    for r in ex.result:
        assert 0.0 < r.metric_avg_results["Recall@10"] <= 1.0
    capsys.readouterr()


def test_verbose_prints_one_line_per_epoch(device_double, capsys):
    c = nc.SEEDED["seeded/GMF"]
    nc.seeded_model(c, verbose=True).fit(nc.seeded_dataset(c))
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("GMF epoch")]
    assert len(lines) == c["epochs"]


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------------
NCF_SYMBOLS = ["cornac_hip_ncf_create", "cornac_hip_ncf_destroy", "cornac_hip_ncf_n_tables", "cornac_hip_ncf_set_params",
               "cornac_hip_ncf_get_params", "cornac_hip_ncf_get_state", "cornac_hip_ncf_reset_optimizer", "cornac_hip_ncf_fit_epoch",
               "cornac_hip_ncf_draw_epoch", "cornac_hip_ncf_fit_epoch_sampled", "cornac_hip_ncf_score_users", "cornac_hip_ncf_score_pairs"]


def test_abi_declares_and_binds_the_ncf_entry_points():
    import scipy.sparse as sp

    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in NCF_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    section = header[header.index("Neural collaborative filtering (He et al. 2017)"):]
    for cited in ("backend_pt.py:", "recom_ncf_base.py:", "recom_gmf.py:", "recom_mlp.py:", "recom_neumf.py:"):
        assert cited in section, cited
    assert "ncf.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    # argument checks need no device: NULL handles are refused with the invalid-argument status
    L = _lib.lib()
    assert L.cornac_hip_ncf_set_params(None, None) == 1 and L.cornac_hip_ncf_get_params(None, None) == 1
    assert L.cornac_hip_ncf_get_state(None, None, None, None) == 1 and L.cornac_hip_ncf_reset_optimizer(None) == 1
    assert L.cornac_hip_ncf_n_tables(None, None) == 1
    assert L.cornac_hip_ncf_fit_epoch(None, 1, None, None, None, None, 0.1, 0.0, 0, None, None) == 1
    assert L.cornac_hip_ncf_draw_epoch(None, 1, 0, 0, 0, None, None, None, None) == 1
    assert L.cornac_hip_ncf_fit_epoch_sampled(None, 1, 0, 0, 0, 0.1, 0.0, 0, None, None) == 1
    assert L.cornac_hip_ncf_score_users(None, None, 0, None) == 1 and L.cornac_hip_ncf_score_pairs(None, None, None, 0, None) == 1
    assert L.cornac_hip_ncf_destroy(None) == 0
    # the limits are named without a device
    X = sp.random(6, 8, 0.5, format="csr", random_state=1)
    for kind, kw, text in (("GMF", dict(num_factors=0), "GMF: num_factors = 0 .* 1 <= num_factors <= 256"),
                           ("NeuMF", dict(num_factors=257, layers=(8, 257)), "NeuMF: num_factors = 257 .* 1 <= num_factors <= 256"),
                           ("MLP", dict(layers=(8,)), "MLP: len\\(layers\\) = 1 .* 2 <= len\\(layers\\) <= 8"),
                           ("MLP", dict(layers=(8,) * 9), "MLP: len\\(layers\\) = 9 .* 2 <= len\\(layers\\) <= 8"),
                           ("MLP", dict(layers=(7, 4)), "MLP: layers\\[0\\] = 7 must be even"),
                           ("MLP", dict(layers=(514, 4)), "MLP: layers\\[0\\] = 514 .* 2 <= layers\\[0\\] <= 512"),
                           ("MLP", dict(layers=(8, 257)), "MLP: layers\\[1\\] = 257 .* 1 <= width <= 256"),
                           ("MLP", dict(layers=(8, 4, 0)), "MLP: layers\\[2\\] = 0 .* 1 <= width <= 256"),
                           ("NeuMF", dict(num_factors=8, layers=(8, 4)), "NeuMF: layers\\[-1\\] = 4 must equal num_factors = 8")):
        with pytest.raises(_lib.HipError, match=text):
            _lib.NcfModel(kind, X, **kw)
    bad = X.copy()
    bad.data[0] = np.nan
    with pytest.raises(_lib.HipError, match="GMF: the value of the training matrix .* is not finite"):
        _lib.NcfModel("GMF", bad, 4)
    assert _lib.NcfModel.NAMES("NeuMF", (64, 32, 16, 8))[:4] == ("logit.weight", "logit.bias", "gmf.user_embedding.weight", "gmf.item_embedding.weight")
    assert len(_lib.NcfModel.NAMES("NeuMF", (64, 32, 16, 8))) == 16 and len(_lib.NcfModel.NAMES("NeuMF", (8, 4))) == 12
    for kind in nc.KINDS:
        assert _lib.NcfModel.NAMES(kind, (12, 7, 5)) == nc.NAMES(kind, (12, 7, 5))
        assert _lib.NcfModel.shapes(kind, 6, 8, 5, (12, 7, 5)) == nc.shapes(kind, 6, 8, 5, (12, 7, 5))
    assert _lib.NcfModel.ACTS == nc.ACTS and _lib.NcfModel.LEARNERS == nc.LEARNERS and _lib.NcfModel.UNUSED("NeuMF") == nc.UNUSED("NeuMF")
