"""MMMF without a GPU: (1) the numpy restatement of recom_mmmf.pyx:126-158 against the reference's own compiled loop
(tests/golden/mmmf_ref.npz), bit for bit, and the fixture's condition; (2) epochs chain; (3) the host logic of
cornac_amd.MMMF through the device double; (4) the ABI; (5) the hogwild step cases of tests/mmmf_cases.py are fair and
their checks sharp."""
import inspect
import os
import pickle
import re

import numpy as np
import pytest

import mmmf_cases as mc
from conftest import ROOT, load_golden, synth_dataset
from cornac_amd import BPR, MMMF, Experiment, RatioSplit, _lib
from cornac_amd import metrics as mm
from oracle import oracle as orc


@pytest.fixture(scope="module")
def golden(oracle):
    return load_golden("mmmf_ref")


def _golden_run(fx, name, epochs_per_call):
    dt = np.float32 if name.endswith("f32") else np.float64
    U, V, B = (fx[name + "/" + t].astype(dt) for t in ("U0", "V0", "B0"))
    gp, gn = orc.MT19937(int(fx["mt_seeds"][0])), orc.MT19937(int(fx["mt_seeds"][1]))
    lr, reg = fx["hyper"]
    stats = []
    for n in epochs_per_call:
        stats += mc.mmmf_fit(fx["indptr"], fx["indices"], 40, U, V, B, lr, reg, n, gp, gn)
    return U, V, B, stats


# ---- (1) the restatement is the reference's loop ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k5_f32", "k5_f64", "k15_f32", "k15_f64"])
def test_restatement_reproduces_the_reference_bit_for_bit(golden, name):
    assert name in list(golden["cases"])
    epochs = int(golden[name + "/epochs"])
    U, V, B, stats = _golden_run(golden, name, [epochs])
    for tab, got in zip("UVB", (U, V, B)):
        want = golden[name + "/" + tab]
        assert got.dtype == want.dtype and np.array_equal(got, want), "%s: table %s differs from the reference's" % (name, tab)
    assert np.array_equal(np.array(stats), golden[name + "/stats"])
    assert not np.array_equal(U, golden[name + "/U0"].astype(U.dtype)) and np.abs(B).max() > 0
    # the fixture's condition: in every epoch both branches hold at least 10 % of the non-skipped samples
    for correct, skipped in stats:
        share = correct / (600 - skipped)
        print("%s: correct share %.3f, skipped share %.3f" % (name, share, skipped / 600))
        assert 0.1 <= share <= 0.9


# ---- (2) epochs chain -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k5_f32", "k5_f64"])
def test_epochs_chain_across_calls(golden, name):
    one = _golden_run(golden, name, [3])
    two = _golden_run(golden, name, [1, 2])
    for a, b in zip(one[:3], two[:3]):
        assert np.array_equal(a, b)
    assert one[3] == two[3]


# ---- (3) host logic through the double ---------------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    mc.install(monkeypatch)
    monkeypatch.chdir(tmp_path)


@pytest.fixture(scope="module")
def ds():
    return synth_dataset(60, 40, 700, seed=4)


KW = dict(k=5, max_iter=2, learning_rate=0.05, lambda_reg=0.01)


def test_constructor_is_the_references():
    m = MMMF()
    assert (m.name, m.k, m.max_iter, m.learning_rate, m.lambda_reg, m.trainable, m.verbose, m.seed, m.use_bias) == \
        ("MMMF", 10, 100, 0.001, 0.01, True, False, None, True)
    assert isinstance(m, BPR) and "use_bias" not in inspect.signature(MMMF.__init__).parameters
    with pytest.raises(TypeError):
        MMMF(use_bias=False)
    assert MMMF._pairwise_loss == "hinge" and BPR._pairwise_loss == "bpr"


def test_seeded_fit_draws_tables_then_seeds_and_is_the_restatement(device_double, ds, oracle):
    m = MMMF(seed=123, **KW).fit(ds)
    rs = np.random.RandomState(123)
    U = ((rs.uniform(0, 1, (ds.num_users, 5)).astype(np.float32) - 0.5) / 5)
    V = ((rs.uniform(0, 1, (ds.num_items, 5)).astype(np.float32) - 0.5) / 5)
    B = np.zeros(ds.num_items, np.float32)
    sp, sn = (orc.rngvector_seed(rs.randint(2 ** 31)) for _ in range(2))  # recom_bpr.pyx:190-191, after _init, in this order
    X = ds.matrix
    stats = mc.mmmf_fit(X.indptr, X.indices, ds.num_items, U, V, B, 0.05, 0.01, 2, orc.MT19937(sp), orc.MT19937(sn))
    assert np.array_equal(m.u_factors, U) and np.array_equal(m.i_factors, V) and np.array_equal(m.i_biases, B)
    assert m.fit_stats == [(sum(c for c, _ in stats), sum(s for _, s in stats))]
    assert np.abs(m.i_biases).max() > 0


def test_init_params_are_updated_in_place_and_float64_trains_in_double(device_double, ds):
    rs = np.random.RandomState(3)
    U, V, Bi = rs.normal(0, 0.1, (ds.num_users, 5)), rs.normal(0, 0.1, (ds.num_items, 5)), np.zeros(ds.num_items)
    U0 = U.copy()
    m = MMMF(seed=5, init_params={"U": U, "V": V, "Bi": Bi}, **KW).fit(ds)
    assert m.u_factors is U and U.dtype == np.float64 and not np.array_equal(U, U0) and m.trains_float64
    assert m.score(3).dtype == np.float64
    U32 = U0.astype(np.float32)
    m32 = MMMF(seed=5, init_params={"U": U32}, **KW).fit(ds)
    assert m32.u_factors is U32 and not np.array_equal(U32, U0.astype(np.float32))
    with pytest.raises(ValueError, match="dtype mismatch"):
        MMMF(seed=5, init_params={"U": U0.copy()}, **KW).fit(ds)  # float64 U with drawn float32 V


def test_verbose_fit_reports_per_epoch(device_double, ds, capsys):
    m = MMMF(seed=1, verbose=True, **KW).fit(ds)
    assert len(m.fit_stats) == 2 and "Optimization finished!" in capsys.readouterr().out


def test_clone_pickle_save_and_pretrained(device_double, ds, tmp_path):
    m = MMMF(seed=9, mode="hogwild", **KW).fit(ds)
    c = m.clone()
    assert type(c) is MMMF and (c.k, c.max_iter, c.learning_rate, c.seed, c.mode) == (5, 2, 0.05, 9, "hogwild")
    assert m.clone({"k": 7}).k == 7
    back = MMMF.load(m.save(str(tmp_path)))
    assert type(back) is MMMF and np.array_equal(back.i_factors, m.i_factors) and np.array_equal(back.score(3), m.score(3))
    again = pickle.loads(pickle.dumps(m))
    assert np.array_equal(again.u_factors, m.u_factors)
    pre = MMMF(trainable=False, init_params={"U": m.u_factors.copy(), "V": m.i_factors.copy(), "Bi": m.i_biases.copy()}, **KW).fit(ds)
    assert np.array_equal(pre.u_factors, m.u_factors) and np.array_equal(pre.score(3), m.score(3))


def test_experiment_runs_mmmf_beside_bpr(device_double, capsys):
    rs = np.random.RandomState(8)
    keys = rs.permutation(70 * 50)[:1500]
    data = [("u%d" % (k // 50), "i%d" % (k % 50), float(rs.randint(1, 6))) for k in keys]
    split = RatioSplit(data, test_size=0.2, rating_threshold=1.0, seed=123)
    ex = Experiment(split, [BPR(k=10, max_iter=3, learning_rate=0.01, seed=123), MMMF(k=10, max_iter=3, learning_rate=0.01, seed=123)],
                    [mm.AUC(), mm.Recall(k=20)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["BPR", "MMMF"]
    assert all(np.isfinite(v) for v in ex.result[1].metric_avg_results.values())
    capsys.readouterr()


def test_the_multi_gpu_bpr_trainers_refuse_another_loss(ds):
    from cornac_amd import dist

    for fit in (dist.fit_bpr_sharded, dist.fit_bpr_ring):
        with pytest.raises(TypeError, match="hinge"):
            fit(MMMF(mode="hogwild", **KW), ds)
    dist._require_bpr_loss(BPR())  # BPR and its other subclasses pass


# ---- (4) ABI -------------------------------------------------------------------------------------------------------------------
def test_abi_declares_exports_and_binds_the_mmmf_entry_points():
    names = ["cornac_hip_mmmf_fit_epochs", "cornac_hip_mmmf_fit_epochs_f64", "cornac_hip_mmmf_hogwild_enqueue"]
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in names:
        assert re.search(r"\bint %s\s*\(cornac_hip_bpr_t h" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    assert "recom_mmmf.pyx" in header
    for method in ("mmmf_fit_epochs", "mmmf_fit_epochs_f64", "mmmf_hogwild_enqueue"):
        assert callable(getattr(_lib.BprTrainer, method))
    assert _lib.lib().cornac_hip_mmmf_fit_epochs(None, 1, 0.1, 0.1, 0, None, None) == 1  # a NULL handle is refused, no device needed
    assert _lib.lib().cornac_hip_mmmf_hogwild_enqueue(None, 1, 0.1, 0.1) == 1


# ---- (5) the step cases are fair, the checks sharp ------------------------------------------------------------------------------
def test_a_zero_score_is_a_violator():
    U, V, B = np.zeros((1, 4), np.float32), np.zeros((2, 4), np.float32), np.zeros(2, np.float32)
    assert mc.mmmf_fit(None, None, None, U, V, B, 0.05, 0.01, triplets=([0], [0], [1])) == [(0, 0)]
    assert B[0] == np.float32(0.05) and B[1] == np.float32(-0.05)
    U2, V2, B2 = np.zeros((1, 4), np.float32), np.zeros((2, 4), np.float32), np.zeros(2, np.float32)
    assert mc.mmmf_fit(None, None, None, U2, V2, B2, 0.05, 0.01, triplets=([0], [0], [1]), fault="ge_zero") == [(1, 0)]
    assert not np.array_equal(B, B2)  # `score >= 0` would have left the tables alone


_figures = {}


@pytest.mark.parametrize("name", mc.NAMES)
def test_step_case_is_fair_and_its_checks_sharp(oracle, name):
    c = mc.case(name)
    n = len(c.trip[0])
    amb, flip, clean, viol = c.ambiguous.mean(), c.flippable.mean(), c.clean.mean(), c.viol.mean()
    print("\n%s: %d triplets, violators %.3f, ambiguous %.4f, flippable %.4f, clean %.3f, left out U %.4f V %.4f B %.4f" % (
        name, n, viol, amb, flip, clean, c.left_out["U"], c.left_out["V"], c.left_out["B"]))
    assert amb <= mc.CAP_AMBIGUOUS and flip <= mc.CAP_FLIPPABLE and clean >= mc.MIN_CLEAN
    assert all(v <= mc.CAP_LEFT_OUT for v in c.left_out.values())
    cv = c.clean & ~c.ambiguous
    assert (cv & c.viol).sum() >= 100 and (cv & ~c.viol).sum() >= 100  # both branches are exercised on clean triplets
    # T_CLEAN: the float32 restatement step against the float64 step on the clean rows
    got32 = mc.sequential(c, mc.LR_A, dtype=np.float32)
    worst = mc.check_a(c, got32)
    _figures.setdefault("clean", {})[name] = max(worst.values())
    # C: three orders of application in float64 against the Jacobi sum
    rs = np.random.RandomState(5)
    ratio = 0.0
    for order in (None, rs.permutation(n), rs.permutation(n)):
        seq = mc.sequential(c, mc.LR_B, order)
        for tab, g in zip("UVB", seq):
            rows, err = mc.errors_b(c, tab, g)
            path = c.jac[tab]["path"][rows]
            assert (err[path == 0] == 0).all()
            if (path > 0).any():
                ratio = max(ratio, float((err[path > 0] / path[path > 0]).max()))
    print("%s: float32 step vs float64 step %.3g; |sequential - jacobi| / path %.4g -> C %.3g (have %.3g)" % (
        name, max(worst.values()), ratio, bc_round(4 * ratio), mc.C[name]))
    assert mc.C[name] == bc_round(4 * ratio)
    # the checks pass on a right update (float32 restatement, launch order) ...
    mc.check_z(c, mc.sequential(c, 0.0, dtype=np.float32), int((~c.viol).sum()), c.skipped)
    right_b = mc.sequential(c, mc.LR_B, dtype=np.float32)
    mc.check_b(c, right_b)
    # ... and reject the wrong ones
    for fault in ("correct_writes_reg", "violator_skipped", "temp_aliasing", "bias_untouched", "wrong_sign_j"):
        with pytest.raises(AssertionError):
            mc.check_a(c, mc.sequential(c, mc.LR_A, fault=fault, dtype=np.float32))
        if fault not in ("temp_aliasing",):  # (second order in lr: launch A's to notice)
            with pytest.raises(AssertionError):
                mc.check_b(c, mc.sequential(c, mc.LR_B, fault=fault, dtype=np.float32))
    # one lost and one doubled update, on a checked row where one update exceeds twice the tolerance
    for tab in "UVB":
        j = c.jac[tab]
        rows = c.rows_b[tab]
        tol = mc.tolerance_b(c, tab)[rows]
        vis = rows[(j["touches"][rows] == 1) & (j["path"][rows] > 2 * tol)]
        assert len(vis) > 0.25 * (j["touches"][rows] > 0).sum(), "one update shows on too few rows of table " + tab
        for sign in (-1.0, 1.0):
            wrong = [t.copy() for t in right_b]
            ti = "UVB".index(tab)
            wrong[ti][vis[0]] = (wrong[ti][vis[0]].astype(np.float64) + sign * j["sum"][vis[0]]).astype(np.float32)
            with pytest.raises(AssertionError):
                mc.check_b(c, wrong)


def bc_round(v):
    return mc.bc.round_up_1sig(v)


def test_t_clean_follows_its_rule(oracle):
    """(after the cases above: their float32-step figures)"""
    fig = _figures.setdefault("clean", {})
    for name in mc.NAMES:
        if name not in fig:  # (run on its own)
            c = mc.case(name)
            fig[name] = max(mc.check_a(c, mc.sequential(c, mc.LR_A, dtype=np.float32)).values())
    worst = max(fig.values())
    print("float32 restatement step vs float64 step over the clean rows of all cases: %.3g -> T_CLEAN %.3g" % (
        worst, bc_round(4 * worst)))
    assert mc.T_CLEAN == bc_round(4 * worst)
