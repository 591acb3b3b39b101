"""RecVAE without a GPU: (1) the float64 restatement (tests/recvae_cases.py) against what the reference's own VAE / RecVAE.run
/ RecVAE.fit wrote into tests/golden/recvae_ref.npz; (2) the host logic of cornac_amd.RecVAE through a device double that
calls the restatement; (3) the ABI entry points are declared and bound.

(1) Measured by the golden's generator with the restatement below, 9 steps (6 at i64 and i65) of the case's schedule: the
reference's float32 tables lie 1.6e-07 to 3.0e-07 from the restatement (far, with fc_mu near 100: 1.1e-05), while the tables
moved 2e-3 to 9e-3 (far: 3e-2 to 6e-2), so the device's tolerance max(16 d_ref, 4 ulp) is 0.02 % to 0.08 % of a table's
movement (far: 0.30 %), under the 1 % the condition asks; the steps' losses agree to 1.5e-07 .. 7.7e-07 relative (b1, whose
reference run carries rounding noise in the tables that are exact here: 1.3e-05).  At hidden_dim 1 the gradient of every
table below ln5.bias is 0 in exact arithmetic, the restatement leaves them bit for bit in place, and the reference's float32
run moves them by up to 1.9e-3 (rounding noise that Adam scales up to whole steps): the golden marks them `exact`, and the
tests hold them bit for bit instead of to a d_ref that says nothing."""
import inspect
import os
import pickle
import re
import warnings

import numpy as np
import pytest

import fake_device
import recvae_cases as rc
from conftest import ROOT, load_golden
from cornac_amd import Experiment, RatioSplit, Recommender, RecVAE, ScoreException, _lib
from cornac_amd import metrics as mm


@pytest.fixture(scope="module")
def golden():
    return load_golden("recvae_ref")


def golden_params(golden, name):
    return {n: golden["%s/P/%d" % (name, q)] for q, n in enumerate(rc.NAMES)}


# ---- (1) restatement against the reference ---------------------------------------------------------------------------------
def test_golden_holds_the_cases_the_issue_counts(golden):
    assert sorted(golden["cases"]) == sorted(rc.CASES)
    C = rc.CASES.values()
    assert {1, 63, 64, 65, 257, 1031} <= {c["ni"] for c in C} and {1, 7, 64, 65} <= {c["h"] for c in C}
    assert {1, 5, 33} <= {c["k"] for c in C} and {1, 16, 100} <= {c["bs"] for c in C}
    assert any(c["gamma"] for c in C) and any(not c["gamma"] and c["beta"] for c in C) and any(c["not_alternating"] for c in C)
    for name, c in rc.CASES.items():
        assert c["bs"] == 1 or c["nu"] % c["bs"] != 0, name
        kinds = [p["kind"] for p in rc.case_passes(c)]
        assert kinds == (["joint"] * 3 if c["not_alternating"] else ["enc", "dec", "enc"])
        for kind in ("d_ref", "d_ref_m", "d_ref_v", "move", "max", "max_m", "max_v", "exact"):
            assert golden["%s/%s" % (name, kind)].shape == (26,) and np.isfinite(golden["%s/%s" % (name, kind)]).all()
        share = rc.check_condition(golden, name)
        print("%s: the device's tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
        exact = {n for q, n in enumerate(rc.TRAINABLE) if golden[name + "/exact"][q]}
        below_ln5_bias = set(rc.ENC_NAMES[:rc.ENC_NAMES.index("encoder.ln5.bias")])
        assert exact == ((below_ln5_bias if c["h"] == 1 else set()) | (set(rc.DEC_NAMES) if c["ni"] == 1 else set())), (name, exact)
        X, p0 = rc.case_matrix(c), rc.case_passes(c)[0]
        if c["ni"] >= 8:
            T = X.tocsc()
            assert T[:, 1].nnz == 0 and sorted(T[:, 2].indices) == [0, 1] and X[3].nnz == 1 and (X.data == 0).sum() == 1
            assert list(p0["order"][:2]) == [0, 1] and not p0["keep"][X.indptr[4]:X.indptr[5]].any() and X[4].nnz > 1
            assert p0["keep"][X.indices == 2].all()
    M = rc.dataset("i257").matrix
    assert M.nnz == rc.case_matrix(rc.CASES["i257"]).nnz and (M.data == 0).sum() == 1, "the Dataset keeps the stored zero stored"
    for name in rc.FULL_CASES:
        c = rc.CASES[name]
        assert golden[name + "/logits"].shape == (len(rc.score_users(c)), c["ni"]) and golden[name + "/losses"].shape == (rc.n_steps(c), 3)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "recvae_ref.npz")) < 300 * 1024


def test_far_case_underflows_unshifted():
    """what the case is for: in its first forward some latent entries have all three mixture terms below -104, where
    float32's exp gives 0 and an unshifted logsumexp gives -inf; the posterior term lies far below the wide one"""
    c = rc.CASES["far"]
    r = rc.Restatement(rc.case_matrix(c), c["h"], c["k"], rc.case_params(c))
    p = rc.case_passes(c)[0]
    users = p["order"][:c["bs"]]
    f = r.forward(users, r.keep_matrix(p["keep"])[users], 2.0, p["eps"][users].astype(np.float64), c["gamma"], c["beta"])
    a, lse, _ = r.mixture(f["z"], f["post_mu"], f["post_lv"])
    gone = (a < -104).all(axis=-1)
    print("far: %d of %d latent entries have every mixture term below -104; the posterior term is up to %.3g below the wide one" % (
        gone.sum(), gone.size, (a[..., 2] - a[..., 1]).max()))
    assert gone.sum() >= 10 and np.isfinite(lse).all() and (a[..., 2] - a[..., 1]).max() > 1000
    with np.errstate(divide="ignore"):
        assert np.isinf(np.log(np.exp(a.astype(np.float32)).sum(axis=-1))).any(), "an unshifted float32 logsumexp is -inf there"


@pytest.mark.parametrize("name", rc.FULL_CASES)
def test_restatement_against_the_references_tables(golden, name):
    c = rc.CASES[name]
    r, losses, init = rc.run_case(name)
    ref = golden_params(golden, name)
    worst = {"P": max(float(np.abs(ref[n].astype(np.float64) - r.P[n]).max()) for n in rc.NAMES)}
    for kind, mine in (("M", r.M), ("V", r.V)):
        worst[kind] = max(float(np.abs(golden["%s/%s/%d" % (name, kind, q)].astype(np.float64) - mine[n]).max()) for q, n in enumerate(rc.TRAINABLE))
    move = min(float(np.abs(r.P[n] - init[n]).max()) for n in rc.TRAINABLE)
    rel = float(np.max(np.abs(losses - golden[name + "/losses"]) / np.abs(losses)))
    print("%s: max|restatement - reference| tables %.3g, exp_avg %.3g, exp_avg_sq %.3g; the tables moved at least %.3g; losses %.3g "
          "relative (bound 2e-5)" % (name, worst["P"], worst["M"], worst["V"], move, rel))
    # float32 against float64 over 9 steps: a few units in the last place of tables of size about 1 (6e-8 each)
    assert worst["P"] <= 64 * 2.0 ** -24 and worst["P"] < 1e-3 * move
    assert np.allclose(golden[name + "/d_ref"], [np.abs(ref[n].astype(np.float64) - r.P[n]).max() for n in rc.TRAINABLE], rtol=1e-3, atol=1e-12)
    assert worst["M"] <= 2 * golden[name + "/d_ref_m"].max() + 1e-12 and worst["V"] <= 2 * golden[name + "/d_ref_v"].max() + 1e-14
    assert rel <= 2e-5 and (r.t_enc, r.t_dec) == tuple(golden[name + "/t"])
    if not c["not_alternating"]:
        assert not np.array_equal(r.P["prior.encoder_old.fc2.weight"], init["prior.encoder_old.fc2.weight"])
        assert not np.array_equal(r.P["prior.encoder_old.fc2.weight"], r.P["encoder.fc2.weight"]), "the old encoder differs from the new"
    # the reference's own logits in evaluation mode at its own tables
    at_ref = rc.Restatement(rc.case_matrix(c), c["h"], c["k"], ref)
    users, (pu, pi) = rc.score_users(c), rc.score_pairs(c)
    want = at_ref.logits(users)
    bound = 64 * 2.0 ** -24 * (1 + np.abs(want).max())
    print("%s: the reference's logits vs the restatement's at the same tables: %.3g (bound %.3g)" % (name, np.abs(golden[name + "/logits"] - want).max(), bound))
    assert np.abs(golden[name + "/logits"] - want).max() <= bound
    assert np.abs(golden[name + "/pair_logits"] - at_ref.logits(pu)[np.arange(len(pu)), pi]).max() <= bound


@pytest.mark.parametrize("kind", ["enc", "dec", "joint"])
def test_restatement_gradients_are_the_loss_slopes(kind):
    """the hand-written backward against central differences of the restatement's own loss: every trainable table, under both
    KL weights, with an old encoder that differs from the new one"""
    for name in ("i63", "joint/beta"):
        c = rc.CASES[name]
        X, p = rc.case_matrix(c), rc.case_passes(c)[0]
        users = p["order"][:c["bs"]]
        base = rc.Restatement(X, c["h"], c["k"], rc.case_params(c))
        K, eps = base.keep_matrix(p["keep"])[users], p["eps"][users].astype(np.float64)

        def loss(params):
            return rc.Restatement(X, c["h"], c["k"], params).forward(users, K, 2.0, eps, c["gamma"], c["beta"])["loss"]

        G = base.gradients(base.forward(users, K, 2.0, eps, c["gamma"], c["beta"]), kind != "dec", kind != "enc")
        assert set(G) == set((rc.ENC_NAMES if kind != "dec" else ()) + (rc.DEC_NAMES if kind != "enc" else ())), "only what steps is computed"
        rs = np.random.RandomState(4)
        for n in G:
            idx = tuple(rs.randint(s) for s in base.P[n].shape)
            if n == "encoder.fc1.weight":
                idx = (idx[0], int(X[users[0]].indices[np.flatnonzero(K[0, X[users[0]].indices])[0]]))   # a kept entry of the batch
            up, dn = ({m: a.copy() for m, a in base.P.items()} for _ in range(2))
            up[n][idx] += 1e-6
            dn[n][idx] -= 1e-6
            slope, g = (loss(up) - loss(dn)) / 2e-6, G[n][idx]
            assert abs(slope - g) <= 1e-6 * max(1.0, abs(g)) + 1e-8, (name, n, slope, g)


# ---- (2) host logic over a device double -----------------------------------------------------------------------------------
@pytest.fixture()
def device_double(monkeypatch, tmp_path):
    fake_device.install(monkeypatch)
    monkeypatch.setattr(_lib, "RecvaeModel", rc.FakeRecvaeModel)
    monkeypatch.chdir(tmp_path)
    rc.FakeRecvaeModel.built, rc.FakeRecvaeModel.last = 0, None


KW = dict(hidden_dim=7, latent_dim=5, batch_size=16, n_epochs=2, n_enc_epochs=2, n_dec_epochs=1, lr=1e-3, seed=9)


def test_constructor_is_the_references():
    m = RecVAE()
    assert (m.name, m.hidden_dim, m.latent_dim, m.batch_size, m.beta, m.gamma, m.lr, m.n_epochs, m.n_enc_epochs, m.n_dec_epochs,
            m.not_alternating, m.trainable, m.verbose, m.seed, m.use_gpu, m.device) == (
        "RecVae", 600, 200, 500, None, 0.005, 5e-4, 50, 3, 1, False, True, False, None, True, 0)
    names = ["name", "hidden_dim", "latent_dim", "batch_size", "beta", "gamma", "lr", "n_epochs", "n_enc_epochs", "n_dec_epochs",
             "not_alternating", "trainable", "verbose", "seed", "use_gpu"]
    assert list(inspect.signature(RecVAE.__init__).parameters)[1:] == names + ["device"]
    assert isinstance(m, Recommender) and not m.is_fitted and not hasattr(m, "recvae")
    c = RecVAE(use_gpu=False, **KW).clone({"latent_dim": 3})
    assert (c.latent_dim, c.hidden_dim, c.seed, c.use_gpu, c.n_epochs) == (3, 7, 9, False, 2) and not c.is_fitted
    from oracle import ref_loader

    if ref_loader.available():
        import importlib

        ref_loader.load()
        ref = importlib.import_module("cornac.models.recvae.recom_recvae").RecVAE
        theirs = inspect.signature(ref.__init__).parameters
        assert list(theirs)[1:] == names
        mine = inspect.signature(RecVAE.__init__).parameters
        assert all(theirs[n].default == mine[n].default for n in names)


def reference_layers(n_items, hidden, latent):
    """the reference's construction order, restated with torch's layers: (53 tables, in state_dict order)"""
    import torch

    def encoder():
        out = []
        for l in range(5):
            fc = torch.nn.Linear(n_items if l == 0 else hidden, hidden)
            ln = torch.nn.LayerNorm(hidden, eps=0.1)
            out += [fc.weight, fc.bias, ln.weight, ln.bias]
        for _ in range(2):
            fc = torch.nn.Linear(hidden, latent)
            out += [fc.weight, fc.bias]
        return out

    enc, old = encoder(), encoder()
    dec = torch.nn.Linear(latent, n_items)
    pri = [torch.zeros(1, latent), torch.zeros(1, latent), torch.full((1, latent), 10.0)]
    return {n: t.detach().numpy() for n, t in zip(rc.NAMES, enc + pri + old + [dec.weight, dec.bias])}


def test_seeded_init_schedule_and_draw_order(device_double, monkeypatch):
    """torch's calls recorded: manual_seed, the layers, then per step the mask (only under dropout) and the noise, and between
    outer epochs one mask row and one noise row per user with a rating >= 1; the passes and update_prior in fit's order"""
    import torch

    name = "i63"
    c = rc.CASES[name]
    ds = rc.dataset(name, seed=4)
    calls = []
    real_empty, real_zeros = torch.empty, torch.zeros

    class Recorded:
        def __init__(self, t, how):
            self.t, self.how = t, how

        def bernoulli_(self, p):
            calls.append(("bernoulli", self.how, tuple(self.t.shape), p))
            return self.t.bernoulli_(p)

        def normal_(self, mean=0, std=1):
            calls.append(("normal", self.how, tuple(self.t.shape), mean, std))
            return self.t.normal_(mean=mean, std=std)

    def recorded(real, how):   # (calls with keywords are torch's own, from inside nn.Linear: passed through)
        return lambda *s, **kw: real(*s, **kw) if kw or not all(isinstance(x, int) for x in s) else Recorded(real(*s), how)

    with monkeypatch.context() as mp:
        mp.setattr(torch, "empty", recorded(real_empty, "empty"))
        mp.setattr(torch, "zeros", recorded(real_zeros, "zeros"))
        m = RecVAE(**KW).fit(ds)
    fake = rc.FakeRecvaeModel.last
    sizes = [16, 16, 5]
    step = lambda b, drop: ([("bernoulli", "empty", (b, 63), 0.5)] if drop else []) + [("normal", "zeros", (b, 5), 0, 0.01)]   # noqa: E731
    enc = [x for b in sizes for x in step(b, True)]
    dec = [x for b in sizes for x in step(b, False)]
    positives = int(sum((ds.matrix[u].data >= 1).any() for u in range(37)))
    burn = [("bernoulli", "empty", (1, 63), 0.5), ("normal", "zeros", (1, 5), 0, 0.01)] * positives
    assert positives == 37 and calls == enc + enc + dec + burn + enc + enc + dec, "no burn after the last outer epoch"
    kinds = [(x[0],) if x[0] == "update_prior" else (x[0], x[2], x[3], x[4]) for x in fake.calls]
    e, d = ("fit_epoch", 0.5, True, False), ("fit_epoch", 0.0, False, True)
    assert kinds == [e, e, ("update_prior",), d, e, e, ("update_prior",), d]
    assert all(x[5] is not None and x[6] is not None for x in fake.calls if x[0] == "fit_epoch" and x[3])
    assert all(x[5] is None and x[6] is not None for x in fake.calls if x[0] == "fit_epoch" and not x[3])
    # the same fit by hand: the reference's layers after manual_seed, the data set's orders, torch's draws
    torch.manual_seed(9)
    r = rc.Restatement(ds.matrix, 7, 5, reference_layers(63, 7, 5))
    init = {n: a.astype(np.float32) for n, a in r.P.items()}
    assert np.array_equal(init["prior.logvar_uniform_prior"], np.full((1, 5), 10, np.float32)) and (init["encoder.ln3.weight"] == 1).all()
    assert not np.array_equal(init["encoder.fc2.weight"], init["prior.encoder_old.fc2.weight"]), "the old encoder has its own draw"
    hand = rc.dataset(name, seed=4)
    X, history = hand.matrix, []
    for epoch in range(2):
        for kind in ("enc", "enc", "prior", "dec"):
            if kind == "prior":
                r.update_prior()
                continue
            order = np.concatenate(list(hand.user_iter(16, shuffle=True)))
            keep, eps = np.ones(X.nnz, np.uint8), np.zeros((37, 5), np.float32)
            for p0 in range(0, 37, 16):
                users = order[p0:p0 + 16]
                if kind == "enc":
                    mask = torch.empty(len(users), 63).bernoulli_(0.5).numpy()
                    for b, u in enumerate(users):
                        keep[X.indptr[u]:X.indptr[u + 1]] = mask[b, X.indices[X.indptr[u]:X.indptr[u + 1]]]
                eps[users] = torch.zeros(len(users), 5).normal_(mean=0, std=0.01).numpy()
            history.append(r.fit_epoch(order, 16, 1e-3, 0.005, None, 0.5 if kind == "enc" else 0.0, kind == "enc", kind == "dec", keep, eps)[:, 2].mean())
        if epoch == 0:
            for _ in range(37):
                torch.empty(1, 63).bernoulli_(0.5)
                torch.zeros(1, 5).normal_(mean=0, std=0.01)
    assert list(m.recvae) == list(rc.NAMES) and all(a.dtype == np.float32 for a in m.recvae.values())
    assert all(np.array_equal(m.recvae[n], r.P[n].astype(np.float32)) for n in rc.NAMES)
    assert np.allclose(m.loss_history, history, rtol=1e-12) and (fake.r.t_enc, fake.r.t_dec) == (12, 6)
    again = RecVAE(**KW).fit(rc.dataset(name, seed=4))
    assert all(np.array_equal(m.recvae[n], again.recvae[n]) for n in rc.NAMES), "a seeded fit repeats itself"
    # without a seed: the device generator, no host draws
    free = RecVAE(**dict(KW, seed=None)).fit(rc.dataset(name, seed=4))
    assert all(x[5] is None and x[6] is None for x in rc.FakeRecvaeModel.last.calls if x[0] == "fit_epoch")
    assert np.isfinite(free.recvae["decoder.weight"]).all()


@pytest.mark.parametrize("name", sorted(rc.SEEDED))
def test_seeded_fit_through_the_restatement_is_the_references(golden, device_double, name):
    """the reference's own seeded RecVAE.fit (float32, recorded) against cornac_amd.RecVAE.fit over the float64 restatement:
    initial bits, batch orders, masks, noise and the draws its per-epoch evaluation burns all have to be the reference's for
    this to hold.  A wrong draw moves a table by a whole Adam step, 1e-3; float32 against float64 is 1e-7: the bound lies
    between.  seed2 runs two outer epochs, across the evaluation's draws."""
    s = rc.SEEDED[name]
    c = rc.CASES[s["case"]]
    ds = rc.dataset(s["case"], seed=s["seed"])
    orders = []
    real = ds.user_iter
    ds.user_iter = lambda bs, shuffle=False: (orders.append(b) or b for b in real(bs, shuffle))
    RecVAE(hidden_dim=c["h"], latent_dim=c["k"], batch_size=c["bs"], gamma=c["gamma"], beta=c["beta"], lr=c["lr"], n_epochs=s["n_epochs"],
           n_enc_epochs=s["n_enc_epochs"], n_dec_epochs=s["n_dec_epochs"], not_alternating=s["not_alternating"], seed=s["seed"]).fit(ds)
    assert np.array_equal(np.concatenate(orders), golden[name + "/order"]), "Dataset.user_iter takes the users in the reference's order"
    exact = rc.FakeRecvaeModel.last.r
    worst = max(float(np.abs(golden["%s/P/%d" % (name, q)].astype(np.float64) - exact.P[n]).max()) for q, n in enumerate(rc.NAMES))
    print("%s: the reference's seeded float32 tables lie at most %.3g from the restated fit" % (name, worst))
    assert worst <= 1e-5 and s["n_epochs"] == (2 if name == "seed2" else 1)


def test_not_alternating_never_updates_the_prior(device_double):
    ds = rc.dataset("i63", seed=4)
    m = RecVAE(**dict(KW, not_alternating=True)).fit(ds)
    fake = rc.FakeRecvaeModel.last
    assert [(x[0], x[2], x[3], x[4]) for x in fake.calls] == [("fit_epoch", 0.5, True, True)] * 2 and (fake.r.t_enc, fake.r.t_dec) == (6, 6)
    import torch

    torch.manual_seed(9)
    init = reference_layers(63, 7, 5)
    assert all(np.array_equal(m.recvae["prior.encoder_old." + n], init["prior.encoder_old." + n]) for n in rc.ENCODER), \
        "the old encoder keeps its own initial draw"
    assert len(m.loss_history) == 2


def test_refit_continues_and_trainable_false_trains_nothing(device_double):
    ds = rc.dataset("i63", seed=4)
    m = RecVAE(**dict(KW, n_epochs=1)).fit(ds)
    first = {n: a.copy() for n, a in m.recvae.items()}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m.fit(ds)
    fake = rc.FakeRecvaeModel.last
    assert (fake.r.t_enc, fake.r.t_dec) == (6, 3), "new Adams per fit, as fit() builds them"
    r = rc.Restatement(ds.matrix, 7, 5, first)
    for x in fake.calls:
        if x[0] == "update_prior":
            r.update_prior()
        else:
            r.fit_epoch(x[1], 16, 1e-3, 0.005, None, x[2], x[3], x[4], x[5], x[6])
    assert all(np.array_equal(m.recvae[n], r.P[n].astype(np.float32)) for n in rc.NAMES), "the second fit starts from the first's weights"
    assert not np.array_equal(m.recvae["decoder.weight"], first["decoder.weight"])
    built = rc.FakeRecvaeModel.built
    frozen = RecVAE(trainable=False, **KW)
    frozen.load_state_dict(m.state_dict())
    frozen.r_mat = ds.matrix
    frozen.fit(ds)
    assert rc.FakeRecvaeModel.built == built and all(np.array_equal(frozen.recvae[n], m.recvae[n]) for n in rc.NAMES)
    assert np.array_equal(frozen.score(4), m.score(4))


def test_refusals(device_double):
    ds = rc.dataset("i63", seed=4)
    for gamma, beta in ((None, None), (0, 0), (0.0, None), (None, 0.0)):
        with pytest.raises(ValueError, match="gamma or beta"):
            RecVAE(gamma=gamma, beta=beta).fit(ds)
    assert rc.FakeRecvaeModel.built == 0, "refused before anything reaches the device"
    m = RecVAE(**dict(KW, n_epochs=1)).fit(ds)
    for bad in (37, -1):
        with pytest.raises(ScoreException, match="user"):
            m.score(bad)
        with pytest.raises(ScoreException, match="user"):
            m.score(bad, 3)
        with pytest.raises(ScoreException):
            m.score_batch([0, bad])
    for bad in (63, -1):
        with pytest.raises(ScoreException, match="item"):
            m.score(0, bad)
    assert m.rate(37, 0) == m.default_score()
    with pytest.raises(KeyError):
        m.load_state_dict({"encoder.fc1.weight": np.zeros((7, 63))})
    bad = m.state_dict()
    bad["decoder.weight"] = np.zeros((62, 5), np.float32)
    with pytest.raises(ValueError, match="decoder.weight"):
        m.load_state_dict(bad)


def test_state_dict_round_trip_save_load_pickle(device_double, tmp_path):
    import torch

    ds = rc.dataset("i63", seed=4)
    m = RecVAE(**dict(KW, n_epochs=1)).fit(ds)
    sd = m.state_dict()
    assert list(sd) == list(rc.NAMES) and all(sd[n].shape == rc.shapes(63, 7, 5)[n] and sd[n] is not m.recvae[n] for n in rc.NAMES)
    s4 = m.score(4)
    assert s4.dtype == np.float32 and s4.shape == (63,) and abs(float(np.exp(s4).sum()) - 1.0) > 1e-3, "logits, not probabilities"
    assert s4[9] == m.score(4, 9) == m.score_batch([4])[0][9]
    built = rc.FakeRecvaeModel.built
    other = RecVAE(**KW)
    other.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})   # tensors, as the reference's state_dict holds
    other.r_mat, other.num_users, other.num_items = ds.matrix, 37, 63
    assert np.array_equal(other.score(4), s4) and rc.FakeRecvaeModel.built == built + 1
    again = pickle.loads(pickle.dumps(m))
    assert "_recvae_handle" not in again.__dict__ and not hasattr(again, "train_set") and np.array_equal(again.score(4), s4)
    back = RecVAE.load(m.save(str(tmp_path)))
    assert back.trainable is False and "_recvae_handle" not in back.__dict__ and "_scorer" not in back.__dict__
    assert all(np.array_equal(back.recvae[n], m.recvae[n]) for n in rc.NAMES) and np.array_equal(back.score_batch([4, 5]), m.score_batch([4, 5]))
    # an edited table reaches the device
    m.recvae["decoder.bias"] = m.recvae["decoder.bias"] + np.float32(1.0) * (np.arange(63) % 2).astype(np.float32)
    assert not np.array_equal(m.score(4), s4)
    from oracle import ref_loader

    if ref_loader.available():   # the arrays load into the reference's VAE and back
        import importlib

        ref_loader.load()
        vae = importlib.import_module("cornac.models.recvae.recvae").VAE(hidden_dim=7, latent_dim=5, input_dim=63)
        vae.load_state_dict({n: torch.tensor(a) for n, a in sd.items()})
        assert list(vae.state_dict()) == list(rc.NAMES)
        fresh = RecVAE(**KW)
        fresh.load_state_dict(vae.state_dict())
        assert all(np.array_equal(fresh.recvae[n], sd[n]) for n in rc.NAMES)
        vae.eval()   # evaluation semantics: the reference's own forward without dropout and noise gives score()'s logits
        with torch.no_grad():
            theirs = vae(torch.tensor(ds.matrix[4].toarray(), dtype=torch.float32), calculate_loss=False).numpy()[0]
        assert np.abs(theirs - s4).max() <= 64 * 2.0 ** -24 * (1 + np.abs(s4).max())


def test_scoring_tables_order_items_as_score_does(device_double):
    ds = rc.dataset("i257", seed=4)
    m = RecVAE(hidden_dim=7, latent_dim=5, batch_size=100, n_epochs=1, n_enc_epochs=1, seed=2).fit(ds)
    U, V, ib, ub = m._scoring_tables()
    assert U.shape == (250, 5) and V is m.recvae["decoder.weight"] and ib is m.recvae["decoder.bias"] and (ub == 0).all()
    assert m._scoring_tables()[0] is U, "cached: the fused scorer is not rebuilt per call"
    for u in (0, 3, 249):
        s = m.score(u).astype(np.float64)
        logits = V.astype(np.float64) @ U[u] + ib
        assert np.abs(logits - s).max() <= 64 * 2.0 ** -24 * (1 + np.abs(s).max())
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
    models = [RecVAE(hidden_dim=6, latent_dim=4, n_epochs=2, batch_size=16, seed=1),
              RecVAE(hidden_dim=6, latent_dim=4, n_epochs=2, batch_size=16, seed=1, gamma=None, beta=0.2, not_alternating=True, name="RecVAE-beta")]
    ex = Experiment(split, models, [mm.Recall(k=10), mm.NDCG(k=10)], user_based=True)
    ex.run()
    assert [r.model_name for r in ex.result] == ["RecVae", "RecVAE-beta"]
    for r in ex.result:
        assert 0.0 < r.metric_avg_results["Recall@10"] <= 1.0
    capsys.readouterr()


def test_verbose_runs_the_per_epoch_evaluation(device_double, capsys):
    ds = rc.dataset("i257", seed=4)
    RecVAE(hidden_dim=7, latent_dim=5, batch_size=100, n_epochs=2, n_enc_epochs=1, seed=2, verbose=True).fit(ds)
    out = capsys.readouterr().out
    assert out.count("ndcg100") == 2 and out.count("negative_elbo") == 4
    RecVAE(hidden_dim=7, latent_dim=5, batch_size=100, n_epochs=1, n_enc_epochs=1, seed=2).fit(ds)
    assert "ndcg100" not in capsys.readouterr().out


# ---- (3) ABI presence ----------------------------------------------------------------------------------------------------
RECVAE_SYMBOLS = ["cornac_hip_recvae_create", "cornac_hip_recvae_destroy", "cornac_hip_recvae_set_params", "cornac_hip_recvae_get_params",
                  "cornac_hip_recvae_get_state", "cornac_hip_recvae_reset_optimizer", "cornac_hip_recvae_update_prior",
                  "cornac_hip_recvae_get_prior_posterior", "cornac_hip_recvae_fit_epoch", "cornac_hip_recvae_encode_users",
                  "cornac_hip_recvae_score_users", "cornac_hip_recvae_score_pairs"]


def test_abi_declares_and_binds_the_recvae_entry_points():
    header = open(os.path.join(ROOT, "include", "cornac_hip.h")).read()
    for name in RECVAE_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % name, header), name
        assert name in _lib.SYMBOLS
        assert getattr(_lib.lib(), name).argtypes is not None, name + " is not bound"
    section = header[header.index("RecVAE (Shenbin et al. 2020"):]
    assert "recvae.py" in section and "recom_recvae.py" in section
    assert "recvae.hip" in open(os.path.join(ROOT, "cornac_amd", "csrc", "Makefile")).read()
    assert _lib.RecvaeModel.NAMES == rc.NAMES and _lib.RecvaeModel.TRAINABLE == rc.TRAINABLE
    assert _lib.RecvaeModel.shapes(63, 7, 5) == rc.shapes(63, 7, 5)
    # argument checks need no device: NULL handles are refused with the invalid-argument status
    L = _lib.lib()
    assert L.cornac_hip_recvae_set_params(None, None) == 1 and L.cornac_hip_recvae_get_params(None, None) == 1
    assert L.cornac_hip_recvae_get_state(None, None, None, None, None) == 1 and L.cornac_hip_recvae_reset_optimizer(None) == 1
    assert L.cornac_hip_recvae_update_prior(None) == 1 and L.cornac_hip_recvae_get_prior_posterior(None, None, None) == 1
    assert L.cornac_hip_recvae_fit_epoch(None, None, 1, 0.1, 0.005, 0.0, 0.5, 1, 0, None, None, 0, None) == 1
    assert L.cornac_hip_recvae_encode_users(None, None, 0, None, None) == 1 and L.cornac_hip_recvae_score_users(None, None, 0, None) == 1
    assert L.cornac_hip_recvae_score_pairs(None, None, None, 0, None) == 1 and L.cornac_hip_recvae_destroy(None) == 0
    X = rc.case_matrix(rc.CASES["b1"])
    for kw, text in ((dict(hidden=4, latent=257), "1 <= latent_dim <= 256"), (dict(hidden=1025, latent=4), "1 <= hidden_dim <= 1024")):
        with pytest.raises(_lib.HipError, match=text):
            _lib.RecvaeModel(X, **kw)
    bad = X.copy()
    bad.indices[:2] = bad.indices[:2][::-1].copy()
    if X.indptr[1] >= 2:
        bad.has_sorted_indices = True
        with pytest.raises(_lib.HipError, match="sorted indices"):
            _lib.RecvaeModel(bad, 3, 2)
    bad = X.copy()
    bad.data[0] = np.nan
    with pytest.raises(_lib.HipError, match="not finite"):
        _lib.RecvaeModel(bad, 3, 2)
