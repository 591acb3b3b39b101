"""RecVAE on the device, through the C ABI (`_lib.RecvaeModel`) and through cornac_amd.RecVAE, against (a) the float64
restatement of tests/recvae_cases.py and (b) what the reference's own VAE / RecVAE.run / RecVAE.fit wrote into
tests/golden/recvae_ref.npz (tests/test_recvae_cpu.py holds (a) against (b)).

Parameters, Adam's m and Adam's v are each compared table by table with the tolerance
    max(16 * d_ref, 4 units in the last float32 place of max|table|),
d_ref = the reference's own float32 distance to the restatement, read from the golden; for every parameter table that
tolerance stays under 1 % of the table's recorded movement (recvae_cases.check_condition: at most 0.26 % over the cases, as
the golden's generator printed).  Tables whose gradient is 0 in exact arithmetic (hidden_dim 1: everything below ln5.bias;
one item: the decoder) are held bit for bit instead, with m = v = 0: the reference's float32 run moves them by rounding noise
that Adam scales up to whole steps, so its distance says nothing there.  The moments are compared because Adam's early
updates are nearly lr * sign(g): a gradient wrong by a constant factor leaves the parameters right and only m and v wrong.
Every check prints the measured difference next to its tolerance.

Losses (mll, kld, negative_elbo per step) are held to 1e-4 relative, as for VAECF.  Logits: a chain of about hidden + row
length float32 roundings per layer, held to 64 * 2^-24 * (1 + max|logit|) absolute.

The seeded fits have no d_ref in the golden (their initial tables come from torch's generator): there d_ref is measured in
the test, as the distance of the reference's recorded float32 tables from the same fit run through the float64 restatement.

Measured on an MI355X, over the 10 cases: parameters at most 0.20 of their tolerance, m at most 0.49, v at most 0.50 (each
tolerance under 0.30 % of its table's movement); losses at most 1.3e-05 relative (b1; 1.7e-06 otherwise); two runs the same
bits.  Item 2's fc1 column moved 1.2e-03 after its last gradient and ended 4.4e-09 from the restatement.  Logits at most
2.5e-07 from the restatement and 6.0e-07 from the reference's float32 logits (bounds 7e-06 to 1e-05); mu and logvar within
3.4e-07, rows of 1300 entries included; rank_batch equal to the sorted score_batch for the 241 of 250 users whose top
logits lie further apart than twice the bound; the device's mask keeps 0.479 / 0.730 of 2000 entries at p = 0.5 / 0.25;
both seeded fits within their measured 16 d_ref (d_ref at most 2.4e-07).
"""
import functools

import numpy as np
import pytest

import recvae_cases as rc
from conftest import load_golden
from cornac_amd import RecVAE, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("recvae_ref")


@functools.lru_cache(maxsize=None)
def restated(name):
    """computed once per case, shared and left unchanged"""
    r, losses, init = rc.run_case(name)
    for d in (r.P, r.M, r.V):
        for a in d.values():
            a.setflags(write=False)
    return r, losses, init


def golden_params(golden, name):
    return {n: golden["%s/P/%d" % (name, q)] for q, n in enumerate(rc.NAMES)}


class handle:
    """a device model that is closed when the block ends"""

    def __init__(self, name, params=None):
        c = rc.CASES[name]
        self.m = _lib.RecvaeModel(rc.case_matrix(c), c["h"], c["k"])
        self.m.set_params(rc.case_params(c) if params is None else params)

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


@functools.lru_cache(maxsize=None)
def device_run(name, upto=None):
    with handle(name) as m:
        losses = rc.run_passes(m, rc.CASES[name], upto=upto)
        P = m.get_params()
        M, V, te, td = m.get_state()
    return P, M, V, (te, td), losses


def compare(golden, name, what, got, want, kind):
    """every trainable table of `got` against `want` under the rule; returns the worst difference / tolerance"""
    worst = 0.0
    for q, n in enumerate(rc.TRAINABLE):
        tol = rc.table_tolerance(golden, name, q, kind, [float(golden["%s/max%s" % (name, kind)][q])])
        diff = float(np.abs(got[n].astype(np.float64) - want[n]).max())
        print("%s %s %s: device vs restatement %.3g; tolerance %.3g" % (name, what, n, diff, tol))
        assert got[n].dtype == np.float32 and got[n].shape == want[n].shape
        assert diff <= tol, (name, what, n, diff, tol)
        worst = max(worst, diff / tol if tol else 0.0)
    return worst


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_steps_against_the_restatement(golden, name):
    c = rc.CASES[name]
    share = rc.check_condition(golden, name)
    r, r_losses, init = restated(name)
    P, M, V, t, losses = device_run(name)
    print("%s: the tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
    assert t == (r.t_enc, r.t_dec) == tuple(golden[name + "/t"]) and min(t) >= 2 and (c["bs"] == 1 or c["nu"] % c["bs"] != 0)
    wp = compare(golden, name, "param", P, r.P, "")
    wm = compare(golden, name, "m", M, r.M, "_m")
    wv = compare(golden, name, "v", V, r.V, "_v")
    for n in rc.NAMES:
        if n not in rc.TRAINABLE and not (n.startswith("prior.encoder_old") and not c["not_alternating"]):
            assert np.array_equal(P[n], init[n]), "the prior tables (and the old encoder without update_prior) stay as set: " + n
    rel = float(np.max(np.abs(losses - r_losses) / np.maximum(1e-30, np.abs(r_losses))))
    print("%s: worst share of the tolerance: params %.3g, m %.3g, v %.3g; losses %.3g relative (allowed 1e-4)" % (name, wp, wm, wv, rel))
    assert losses.shape == (rc.n_steps(c), 3) and (np.abs(losses - r_losses) <= 1e-4 * np.abs(r_losses)).all()
    device_run.cache_clear()
    again = device_run(name)
    for a, b in zip((P, M, V), again[:3]):
        assert all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in a), "two runs give the same bits"
    assert np.array_equal(losses, again[4])
    if c["ni"] >= 8:
        W1, D = "encoder.fc1.weight", "decoder.weight"
        assert np.array_equal(P[W1][:, 1].view(np.uint32), init[W1][:, 1].view(np.uint32)), "an item nobody holds: its fc1 column stays in place"
        assert (M[W1][:, 1] == 0).all() and (V[W1][:, 1] == 0).all()
        if c["mu_scale"] == 1.0:   # (at z in the hundreds the softmax is saturated: the item's probability is 0 in float32)
            assert np.abs(P[D][1] - init[D][1]).max() > 1e-4, "... and its decoder row still moves (softmax reaches every item)"
    if c["h"] == 1:
        for n in ("fc1.weight", "fc1.bias", "ln1.weight", "fc2.weight", "fc5.weight", "fc5.bias", "ln5.weight"):
            n = "encoder." + n
            assert np.array_equal(P[n].view(np.uint32), init[n].view(np.uint32)), "LayerNorm of one element passes nothing back: " + n
        assert not np.array_equal(P["encoder.ln5.bias"], init["encoder.ln5.bias"])


def test_an_item_held_in_the_first_batch_only_keeps_moving(golden):
    """the dense-Adam trap: item 2 is held by users 0 and 1 only, who open the first pass; after that step its fc1 column has
    g = 0 in every step of that pass, and m != 0 still moves it"""
    name = "i63"
    c = rc.CASES[name]
    X, p0 = rc.case_matrix(c), rc.case_passes(c)[0]
    assert sorted(X.tocsc()[:, 2].indices) == [0, 1] and c["bs"] > 1 and list(p0["order"][:2]) == [0, 1]
    one = rc.Restatement(X, c["h"], c["k"], rc.case_params(c))
    users = p0["order"][:c["bs"]]
    one.step(users, one.keep_matrix(p0["keep"])[users], 2.0, p0["eps"][users], c["lr"], c["gamma"], c["beta"], True, False)
    full = rc.Restatement(X, c["h"], c["k"], rc.case_params(c))
    rc.run_passes(full, c, upto=1)
    P = device_run(name, upto=1)[0]
    W1 = "encoder.fc1.weight"
    tol = rc.table_tolerance(golden, name, 0, "", [float(golden[name + "/max"][0])])
    since, diff = float(np.abs(P[W1][:, 2] - one.P[W1][:, 2]).max()), float(np.abs(P[W1][:, 2] - full.P[W1][:, 2]).max())
    print("item 2's fc1 column: moved %.3g since step 1 (a sparse Adam would give 0); %.3g from the restatement, tolerance %.3g" % (since, diff, tol))
    assert diff <= tol and since > 100 * tol


def test_update_prior_copies_the_encoder_and_caches_its_posterior():
    name = "i63"
    c = rc.CASES[name]
    users = np.arange(c["nu"], dtype=np.int32)
    with handle(name) as m:
        p = rc.case_passes(c)[0]
        m.fit_epoch(p["order"], c["bs"], c["lr"], c["gamma"], c["beta"], p["rate"], True, False, keep=p["keep"], eps=p["eps"])
        before = m.prior_posterior()
        m.update_prior()
        P = m.get_params()
        cached, fresh = m.prior_posterior(), m.encode_users(users, with_logvar=True)
    for n in rc.ENCODER:
        assert np.array_equal(P["prior.encoder_old." + n].view(np.uint32), P["encoder." + n].view(np.uint32)), n
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(cached, fresh)), \
        "the cached old-encoder output is encode_users under the old tables"
    assert not np.array_equal(before[0], cached[0])
    init = rc.Restatement(rc.case_matrix(c), c["h"], c["k"], rc.case_params(c))
    want = init.encode(users, "prior.encoder_old.")
    assert all(np.abs(a - b).max() <= 64 * 2.0 ** -24 * (1 + np.abs(b).max()) for a, b in zip(before, want))


def test_device_draws_repeat_under_a_seed_and_differ_under_another():
    name = "i257"
    c = rc.CASES[name]
    order = np.arange(c["nu"], dtype=np.int32)[::-1].copy()

    def run(seed, rate=0.5):
        with handle(name) as m:
            losses = [m.fit_epoch(order, c["bs"], c["lr"], c["gamma"], c["beta"], rate, True, True, seed=seed) for _ in range(2)]
            return m.get_params(), np.concatenate(losses)

    (a, la), (b, lb), (d, ld) = run(11), run(11), run(12)
    assert all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in rc.NAMES) and np.array_equal(la, lb)
    assert any(not np.array_equal(a[n], d[n]) for n in rc.NAMES) and not np.array_equal(la, ld)
    assert all(np.isfinite(a[n]).all() for n in rc.NAMES) and np.isfinite(la).all() and not np.array_equal(la[:3], la[3:])
    eps = np.zeros((c["nu"], c["k"]), np.float32)
    with handle(name) as m:   # lr = 0: the same tables in both passes, so only the mask differs
        full = m.fit_epoch(order, c["bs"], 0.0, c["gamma"], c["beta"], 0.0, True, True, eps=eps)
        half = m.fit_epoch(order, c["bs"], 0.0, c["gamma"], c["beta"], 0.5, True, True, eps=eps, seed=5)
    assert np.isfinite(half).all() and not np.array_equal(full, half), "dropout changes the forward pass"


def test_device_mask_keeps_about_one_minus_p():
    """the mask itself, read back through fc1's first moment: after one step over all users, m of fc1's column i is nonzero
    exactly where item i has a kept entry (a kept entry adds x_e gp1 to the column's gradient).  Here every one of 2000 items
    is held by exactly one user, so the share of touched columns is the kept share: 1 - p within four standard deviations
    of a mean of 2000 coin flips, 4 sqrt(p (1 - p) / 2000) <= 0.045"""
    import scipy.sparse as sp

    nu, ni = 40, 2000
    c = rc._c(nu, ni, 7, 5, nu, seed=50)
    X = sp.csr_matrix((1.0 + np.arange(ni) % 5, (np.arange(ni) % nu, np.arange(ni))), shape=(nu, ni))
    X.sort_indices()
    for rate in (0.5, 0.25):
        m = _lib.RecvaeModel(X, c["h"], c["k"])
        try:
            m.set_params(rc.case_params(c))
            m.fit_epoch(np.arange(nu, dtype=np.int32), nu, 0.0, c["gamma"], c["beta"], rate, True, False, seed=77)
            M = m.get_state()[0]
        finally:
            m.close()
        share = float((M["encoder.fc1.weight"] != 0).any(axis=0).mean())
        bound = 4 * np.sqrt(rate * (1 - rate) / ni)
        print("rate %.2f: %.4f of the entries kept, expected %.2f +- %.3f" % (rate, share, 1 - rate, bound))
        assert abs(share - (1 - rate)) <= bound


def logit_bound(want):
    return 64.0 * 2.0 ** -24 * (1.0 + float(np.abs(want).max()))


@pytest.mark.parametrize("name", rc.FULL_CASES)
def test_scores_against_the_restatement_and_the_golden(golden, name):
    c = rc.CASES[name]
    params = golden_params(golden, name)
    r = rc.Restatement(rc.case_matrix(c), c["h"], c["k"], params)
    users, (pu, pi) = rc.score_users(c), rc.score_pairs(c)
    with handle(name, params) as m:
        got = m.get_params()
        assert all(np.array_equal(got[n], params[n]) for n in rc.NAMES), "set / get round trip, both fc1.weight transposed and back"
        rows, pairs, everyone = m.score_users(users), m.score_pairs(pu, pi), m.score_users(np.arange(c["nu"]))
        mu, lv = m.encode_users(users, with_logvar=True)
        with pytest.raises(_lib.HipError, match="user %d out of range" % c["nu"]):
            m.score_users([0, c["nu"]])
        with pytest.raises(_lib.HipError, match="item %d out of range" % c["ni"]):
            m.score_pairs([0], [c["ni"]])
        assert m.score_users(np.zeros(0, np.int32)).shape == (0, c["ni"])
    want = r.logits(users)
    tol = logit_bound(want)
    d_rest, d_gold = np.abs(rows - want).max(), np.abs(rows.astype(np.float64) - golden[name + "/logits"]).max()
    w_mu, w_lv = r.encode(users)
    print("%s: logits vs restatement %.3g, vs the reference's float32 logits %.3g (bound %.3g, twice it); mu differs by %.3g, logvar by %.3g" % (
        name, d_rest, d_gold, tol, np.abs(mu - w_mu).max(), np.abs(lv - w_lv).max()))
    assert rows.dtype == np.float32 and d_rest <= tol and d_gold <= 2 * tol
    assert np.abs(mu - w_mu).max() <= logit_bound(w_mu) and np.abs(lv - w_lv).max() <= logit_bound(w_lv)
    assert np.array_equal(rows, everyone[users]) and np.array_equal(pairs, everyone[pu, pi]), "one row, many rows, pairs: the same bits"
    assert np.abs(pairs.astype(np.float64) - golden[name + "/pair_logits"]).max() <= 2 * logit_bound(r.logits(pu))


def test_rows_longer_than_one_input_chunk():
    """the input layer sums a row in chunks of 512 entries: rows of 1300 (three chunks), 513, 512 and 3 entries, with and
    without dropout, against the restatement; and a row's bits do not depend on who shares its batch"""
    import scipy.sparse as sp

    nu, ni = 5, 1400
    c = rc._c(nu, ni, 65, 5, 3, seed=60)
    rs = np.random.RandomState(60)
    rows = [np.sort(rs.choice(ni, n, replace=False)) for n in (1300, 513, 512, 3, 700)]
    X = sp.csr_matrix((np.concatenate([rs.randint(1, 6, len(r)) for r in rows]).astype(np.float64), np.concatenate(rows),
                       np.cumsum([0] + [len(r) for r in rows])), shape=(nu, ni))
    params = rc.case_params(c)
    r = rc.Restatement(X, c["h"], c["k"], params)
    users = np.arange(nu, dtype=np.int32)
    keep = (rs.rand(X.nnz) < 0.5).astype(np.uint8)
    eps = (0.01 * rs.standard_normal((nu, c["k"]))).astype(np.float32)
    m = _lib.RecvaeModel(X, c["h"], c["k"])
    try:
        m.set_params(params)
        mu, lv = m.encode_users(users, with_logvar=True)
        alone = [m.encode_users([u]) for u in users]
        losses = m.fit_epoch(users[::-1].copy(), 3, 0.0, c["gamma"], c["beta"], 0.5, True, False, keep=keep, eps=eps)
    finally:
        m.close()
    w_mu, w_lv = r.encode(users)
    want = r.fit_epoch(users[::-1], 3, 0.0, c["gamma"], c["beta"], 0.5, True, False, keep, eps)
    print("long rows: mu differs by %.3g (bound %.3g), logvar by %.3g; losses by %.3g relative" % (
        np.abs(mu - w_mu).max(), logit_bound(w_mu), np.abs(lv - w_lv).max(), np.abs(losses / want - 1).max()))
    assert np.abs(mu - w_mu).max() <= logit_bound(w_mu) and np.abs(lv - w_lv).max() <= logit_bound(w_lv)
    assert all(np.array_equal(a[0].view(np.uint32), mu[u].view(np.uint32)) for u, a in enumerate(alone))
    assert (np.abs(losses - want) <= 1e-4 * np.abs(want)).all()


def test_more_ids_than_one_chunk_holds(golden):
    """the chunk loop past its first chunk (b0 > 0): the entry points take min(1024, 256 MiB / (4 n_items)) users per chunk,
    which is 1024 at these item counts, so 1 025 ids make a second chunk of one"""
    name = "i63"
    c = rc.CASES[name]
    n = 1025
    assert n > min(1024, (256 << 20) // (4 * c["ni"])), "more than one chunk's worth"
    users, items = np.arange(n) % c["nu"], np.arange(n) % c["ni"]
    with handle(name, golden_params(golden, name)) as m:
        everyone, codes = m.score_users(np.arange(c["nu"])), m.encode_users(np.arange(c["nu"]))
        rows, mu, pairs = m.score_users(users), m.encode_users(users), m.score_pairs(users, items)
    assert rows.shape == (n, c["ni"]) and np.array_equal(rows.view(np.uint32), everyone[users].view(np.uint32))
    assert mu.shape == (n, c["k"]) and np.array_equal(mu.view(np.uint32), codes[users].view(np.uint32))
    assert pairs.shape == (n,) and np.array_equal(pairs.view(np.uint32), everyone[users, items].view(np.uint32))


def test_rank_batch_is_the_sort_of_score_batch(golden):
    """encode_users + the fused scorer against sorting the handle's logits, where these do not tie or nearly tie: the scorer
    sums the latent products in another order, so two logits closer than the logits' bound may swap"""
    name = "i257"
    c = rc.CASES[name]
    params = golden_params(golden, name)
    users = np.arange(c["nu"], dtype=np.int32)
    with handle(name, params) as m:
        mu, S = m.encode_users(users), m.score_users(users)
    sc = _lib.Scorer(mu, params["decoder.weight"], params["decoder.bias"], np.zeros(c["nu"], np.float32))
    try:
        items, _ = sc.rank_topk(users, 20)
    finally:
        sc.close()
    order = np.argsort(-S.astype(np.float64), axis=1, kind="stable")[:, :21]
    top = np.take_along_axis(S, order, axis=1).astype(np.float64)
    clear = (np.diff(top, axis=1) < -2 * logit_bound(S)).all(axis=1)
    print("rank_batch vs sorted score_batch: %d of %d users have 21 top logits further apart than twice the bound; all of those agree: %s" % (
        clear.sum(), len(users), np.array_equal(items[clear], order[clear, :20])))
    assert clear.sum() >= 0.9 * len(users) and np.array_equal(items[clear], order[clear, :20])


def serve_draws(monkeypatch, c, passes):
    """torch's two draws serve the case's mask and noise, in the order fit asks for them"""
    import torch

    X = rc.case_matrix(c)
    K = rc.Restatement(X, c["h"], c["k"]).keep_matrix
    queue = []
    for p in passes:
        for p0 in range(0, c["nu"], c["bs"]):
            users = p["order"][p0:p0 + c["bs"]]
            if p["rate"]:
                queue.append(("mask", K(p["keep"])[users]))
            queue.append(("eps", p["eps"][users]))

    class Served:
        def __init__(self, shape):
            self.shape = tuple(shape)

        def bernoulli_(self, p):
            kind, a = queue.pop(0)
            assert kind == "mask" and a.shape == self.shape and p == 0.5
            return torch.tensor(a)

        def normal_(self, mean=0, std=1):
            kind, a = queue.pop(0)
            assert kind == "eps" and a.shape == self.shape and (mean, std) == (0, 0.01)
            return torch.tensor(a)

    monkeypatch.setattr(torch, "empty", lambda *shape: Served(shape))
    monkeypatch.setattr(torch, "zeros", lambda *shape: Served(shape))
    return queue


def test_fit_end_to_end(golden, monkeypatch, tmp_path):
    """cornac_amd.RecVAE.fit on a full golden case: the case's tables loaded, the data set yielding the case's orders, torch
    serving the case's masks and noise"""
    name = "i257"
    c, passes = rc.CASES[name], rc.case_passes(rc.CASES[name])
    queue = serve_draws(monkeypatch, c, passes)
    ds = rc.dataset(name)
    orders = [p["order"] for p in passes]
    monkeypatch.setattr(ds, "user_iter", lambda bs, shuffle=False: iter(np.array_split(orders.pop(0), range(bs, c["nu"], bs))))
    m = RecVAE(hidden_dim=c["h"], latent_dim=c["k"], batch_size=c["bs"], gamma=c["gamma"], beta=c["beta"], lr=c["lr"], n_epochs=1,
               n_enc_epochs=1, n_dec_epochs=1, seed=3)
    m.load_state_dict(rc.case_params(c))
    m.fit(ds)
    # (the case's third pass is the next outer epoch's first encoder pass: run it as a refit would not, by hand)
    assert len(queue) == 3 + 3 and len(m.loss_history) == 2
    r2 = rc.Restatement(rc.case_matrix(c), c["h"], c["k"], rc.case_params(c))
    rc.run_passes(r2, c, upto=2)
    for q, n in enumerate(rc.TRAINABLE):
        tol = rc.table_tolerance(golden, name, q, "", [float(golden[name + "/max"][q])])
        diff = float(np.abs(m.recvae[n] - r2.P[n]).max())
        print("fit %s: %.3g from the restatement after two passes, tolerance %.3g" % (n, diff, tol))
        assert diff <= tol
    users = rc.score_users(c)
    r = rc.Restatement(rc.case_matrix(c), c["h"], c["k"], m.state_dict())
    S = m.score_batch(users)
    assert np.abs(S - r.logits(users)).max() <= logit_bound(r.logits(users))
    assert np.array_equal(m.score(int(users[1])), S[1]) and m.score(int(users[1]), 7) == S[1][7]
    items, _ = m.rank_batch(users, k=5)
    ranked, scores = m.rank(int(users[1]))
    assert np.array_equal(scores, S[1]) and np.array_equal(ranked[:5], items[1])
    back = RecVAE.load(m.save(str(tmp_path)))
    assert "_recvae_handle" not in back.__dict__ and np.array_equal(back.score_batch(users), S)


@pytest.mark.parametrize("name", sorted(rc.SEEDED))
def test_seeded_fit_follows_the_references_seeded_run(golden, name, monkeypatch):
    """the device's seeded fit against the reference's recorded one; d_ref is measured here: the reference's float32 tables
    against the same seeded fit through the float64 restatement (which also shows that the draws are the reference's)"""
    from cornac_amd import recvae as host

    s = rc.SEEDED[name]
    c = rc.CASES[s["case"]]
    kw = dict(hidden_dim=c["h"], latent_dim=c["k"], batch_size=c["bs"], gamma=c["gamma"], beta=c["beta"], lr=c["lr"], n_epochs=s["n_epochs"],
              n_enc_epochs=s["n_enc_epochs"], n_dec_epochs=s["n_dec_epochs"], not_alternating=s["not_alternating"], seed=s["seed"])
    dev = RecVAE(**kw).fit(rc.dataset(s["case"], seed=s["seed"]))
    with monkeypatch.context() as mp:
        mp.setattr(host._lib, "RecvaeModel", rc.FakeRecvaeModel)
        RecVAE(**kw).fit(rc.dataset(s["case"], seed=s["seed"]))
        exact = rc.FakeRecvaeModel.last.r
    for q, n in enumerate(rc.NAMES):
        ref = golden["%s/P/%d" % (name, q)]
        d_ref = float(np.abs(ref.astype(np.float64) - exact.P[n]).max())
        tol = rc.tolerance(d_ref, ref)
        diff = float(np.abs(dev.recvae[n].astype(np.float64) - exact.P[n]).max())
        print("%s %s: device vs restatement %.3g; tolerance %.3g (16 x %.3g)" % (name, n, diff, tol, d_ref))
        assert d_ref <= 1e-5 and diff <= tol, (name, n, d_ref, diff, tol)


def test_limits_are_named():
    X = rc.case_matrix(rc.CASES["b1"])
    for kw, text in ((dict(hidden=4, latent=257), "1 <= latent_dim <= 256"), (dict(hidden=1025, latent=4), "1 <= hidden_dim <= 1024"),
                     (dict(hidden=4, latent=0), "1 <= latent_dim <= 256"), (dict(hidden=0, latent=4), "1 <= hidden_dim <= 1024")):
        with pytest.raises(_lib.HipError, match=text):
            _lib.RecvaeModel(X, **kw)
    m = _lib.RecvaeModel(X, 3, 2)
    try:
        order = np.arange(5, dtype=np.int32)
        for bs in (0, 1025):
            with pytest.raises(_lib.HipError, match="1 <= batch_size <= 1024"):
                m.fit_epoch(order, bs, 1e-3, 0.005, None, 0.5, True, False)
        with pytest.raises(_lib.HipError, match="user 5 out of range"):
            m.fit_epoch(np.array([0, 1, 2, 3, 5], np.int32), 2, 1e-3, 0.005, None, 0.5, True, False)
        with pytest.raises(_lib.HipError, match="user 3 occurs twice"):
            m.fit_epoch(np.array([0, 1, 3, 3, 4], np.int32), 2, 1e-3, 0.005, None, 0.5, True, False)
    finally:
        m.close()
