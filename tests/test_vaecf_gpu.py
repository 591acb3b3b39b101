"""VAECF on the device, through the C ABI (`_lib.VaecfModel`) and through cornac_amd.VAECF, against (a) the float64
restatement of tests/vaecf_cases.py and (b) what the reference's own VAE / learn wrote into tests/golden/vaecf_ref.npz
(tests/test_vaecf_cpu.py holds (a) against (b)).

Parameters, Adam's m and Adam's v are each compared table by table with the tolerance
    max(16 * d_ref, 4 units in the last float32 place of max|table|),
d_ref = the reference's own float32 distance to the restatement, read from the golden; for every parameter table that
tolerance stays under 1 % of the table's recorded movement (vaecf_cases.check_condition).  The moments are compared because
Adam's early updates are nearly lr * sign(g): a gradient wrong by a constant factor leaves the parameters right and only m
and v wrong.  Every check prints the measured difference next to its tolerance.

Losses: a batch-mean loss is a float32 sum of n_items terms per user, so it is held to 1e-4 relative (n_items <= 1031
roundings of 6e-8 each at the worst).  Scores: p carries the logit's absolute error as a relative one; the logit is a chain
of about h + row length float32 roundings, so p is held to 64 * 2^-24 * (1 + max|logit|) relative plus 1e-30.

Measured on an MI355X, over the 28 cases: parameters at most 1.36e-06 from the restatement and at most 0.23 of their
tolerance (tolerances 4.2e-08 .. 1.1e-05, each under 0.18 % of its table's movement); m at most 3.6e-07 and 0.25 of its
tolerance; v at most 1.1e-07 and 0.55 of its tolerance; losses at most 1.5e-07 relative; two runs the same bits.  Item 2's W1
row moved 3.0e-03 after its last gradient and ended 7.1e-09 from the restatement.  Scores at most 0.026 of their bound from
the restatement and 0.025 of twice it from the reference's float32 scores; h2 within 3.4e-08; rank_batch equal to the sorted
score_batch for all 250 users.
"""
import functools

import numpy as np
import pytest

import vaecf_cases as vc
from conftest import load_golden
from cornac_amd import VAECF, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("vaecf_ref")


@functools.lru_cache(maxsize=None)
def restated(name):
    """computed once per case, shared and left unchanged"""
    r, losses, init = vc.run_case(name)
    for d in (r.P, r.M, r.V):
        for a in d.values():
            a.setflags(write=False)
    return r, losses, init


class handle:
    """a device model that is closed when the block ends"""

    def __init__(self, name, params=None):
        c = vc.CASES[name]
        self.m = _lib.VaecfModel(vc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"])
        self.m.set_params(vc.case_params(c) if params is None else params)

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


def device_run(name):
    c, noise = vc.CASES[name], vc.case_noise(vc.CASES[name])
    with handle(name) as m:
        losses = np.concatenate([m.fit_epoch(c["bs"], c["lr"], c["beta"], eps=noise[e])[1] for e in range(c["epochs"])])
        P = m.get_params()
        M, V, t = m.get_state()
    return P, M, V, t, losses


def compare(golden, name, what, got, want, kind_d, kind_max):
    """every table of `got` against `want` under the rule; returns the worst difference / tolerance"""
    worst = 0.0
    for q, n in enumerate(vc.NAMES):
        d_ref, top = float(golden["%s/%s" % (name, kind_d)][q]), float(golden["%s/%s" % (name, kind_max)][q])
        tol = max(16.0 * d_ref, 4.0 * vc.ulp32(top))
        diff = float(np.abs(got[n].astype(np.float64) - want[n]).max())
        print("%s %s %s: device vs restatement %.3g; tolerance %.3g (16 x %.3g, 4 ulp %.3g)" % (
            name, what, vc.SHORT[n], diff, tol, d_ref, 4.0 * vc.ulp32(top)))
        assert got[n].dtype == np.float32 and got[n].shape == want[n].shape
        assert diff <= tol, (name, what, n, diff, tol)
        worst = max(worst, diff / tol)
    return worst


@pytest.mark.parametrize("name", sorted(vc.CASES))
def test_steps_against_the_restatement(golden, name):
    c = vc.CASES[name]
    share = vc.check_condition(golden, name)
    r, r_losses, init = restated(name)
    P, M, V, t, losses = device_run(name)
    print("%s: the tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
    assert t == vc.n_steps(c) == r.t and vc.n_steps(c) >= 3 and (c["bs"] == 1 or c["nu"] % c["bs"] != 0)
    wp = compare(golden, name, "param", P, r.P, "d_ref", "max")
    wm = compare(golden, name, "m", M, r.M, "d_ref_m", "max_m")
    wv = compare(golden, name, "v", V, r.V, "d_ref_v", "max_v")
    rel = float(np.max(np.abs(losses - r_losses) / np.maximum(1.0, np.abs(r_losses))))
    print("%s: worst share of the tolerance: params %.3g, m %.3g, v %.3g; losses %.3g relative (allowed 1e-4)" % (name, wp, wm, wv, rel))
    assert rel <= 1e-4
    again = device_run(name)
    for a, b in zip((P, M, V), again[:3]):
        assert all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in vc.NAMES), "two runs give the same bits"
    assert np.array_equal(losses, again[4])
    if c["ni"] >= 8:
        W1, D1 = vc.NAMES[0], vc.NAMES[8]
        assert np.array_equal(P[W1][:, 1], init[W1][:, 1]), "an item nobody holds: its W1 row stays in place"
        assert (M[W1][:, 1] == 0).all() and (V[W1][:, 1] == 0).all()
        if c["lik"] == "mult":
            assert np.abs(P[D1][1] - init[D1][1]).max() > 1e-4, "... and its D1 row still moves under mult"


def test_an_item_held_in_the_first_batch_only_keeps_moving(golden):
    """the dense-Adam trap: item 2 is held by users 0 and 1 only, so after step 1 its W1 row has g = 0, and m != 0 still
    moves it in every later step"""
    name = "i63"
    c = vc.CASES[name]
    X = vc.case_matrix(c)
    assert sorted(X.tocsc()[:, 2].indices) == [0, 1] and c["bs"] > 1
    one = vc.Restatement(X, c["k"], c["h"], c["act"], c["lik"], vc.case_params(c))
    one.step(0, c["bs"], vc.case_noise(c)[0][:c["bs"]], c["lr"], c["beta"])
    r, _, _ = restated(name)
    P = device_run(name)[0]
    W1 = vc.NAMES[0]
    tol = max(16.0 * float(golden[name + "/d_ref"][0]), 4.0 * vc.ulp32(float(golden[name + "/max"][0])))
    since, diff = float(np.abs(P[W1][:, 2] - one.P[W1][:, 2]).max()), float(np.abs(P[W1][:, 2] - r.P[W1][:, 2]).max())
    print("item 2's W1 row: moved %.3g since step 1 (a sparse Adam would give 0); %.3g from the restatement, tolerance %.3g" % (since, diff, tol))
    assert diff <= tol and since > 100 * tol


def test_device_noise_repeats_under_a_seed_and_differs_under_another():
    name = "i63"
    c = vc.CASES[name]

    def run(seed):
        with handle(name) as m:
            losses = [m.fit_epoch(c["bs"], c["lr"], c["beta"], eps=None, seed=seed)[1] for _ in range(2)]
            return m.get_params(), np.concatenate(losses)

    (a, la), (b, lb), (d, ld) = run(11), run(11), run(12)
    assert all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in vc.NAMES) and np.array_equal(la, lb)
    assert any(not np.array_equal(a[n], d[n]) for n in vc.NAMES) and not np.array_equal(la, ld)
    assert all(np.isfinite(a[n]).all() for n in vc.NAMES) and np.isfinite(la).all()
    # the noise is standard normal: the first epoch's losses stay near those of the case's own standard normal noise
    ref = restated(name)[1][:len(la) // 2]
    assert np.all(np.abs(la[:len(ref)] - ref) < 0.2 * np.abs(ref))


def score_tolerance(r, users, want):
    return 64.0 * 2.0 ** -24 * (1.0 + float(np.abs(r.logits(users)).max())) * np.abs(want) + 1e-30


@pytest.mark.parametrize("name", vc.FULL_CASES)
def test_scores_against_the_restatement_and_the_golden(golden, name):
    c = vc.CASES[name]
    params = {n: golden["%s/P/%s" % (name, vc.SHORT[n])] for n in vc.NAMES}
    r = vc.Restatement(vc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"], params)
    users, (pu, pi) = vc.score_users(c), vc.score_pairs(c)
    with handle(name, params) as m:
        got = m.get_params()
        assert all(np.array_equal(got[n], params[n]) for n in vc.NAMES), "set / get round trip, W1 transposed and back"
        rows, pairs, everyone = m.score_users(users), m.score_pairs(pu, pi), m.score_users(np.arange(c["nu"]))
        h2 = m.encode_users(users)
        with pytest.raises(_lib.HipError, match="user %d out of range" % c["nu"]):
            m.score_users([0, c["nu"]])
        with pytest.raises(_lib.HipError, match="item %d out of range" % c["ni"]):
            m.score_pairs([0], [c["ni"]])
        assert m.score_users(np.zeros(0, np.int32)).shape == (0, c["ni"])
    want = r.scores(users)
    tol = score_tolerance(r, users, want)
    d_rest, d_gold = np.abs(rows - want), np.abs(rows.astype(np.float64) - golden[name + "/scores"])
    print("%s: scores vs restatement at most %.3g of their bound, vs the reference's float32 scores %.3g of twice it; h2 differs by %.3g" % (
        name, (d_rest / tol).max(), (d_gold / (2 * tol)).max(), np.abs(h2 - r.h2(users)).max()))
    assert rows.dtype == np.float32 and (d_rest <= tol).all() and (d_gold <= 2 * tol).all()
    assert np.abs(h2 - r.h2(users)).max() <= 64 * 2.0 ** -24 * (1.0 + np.abs(r.h2(users)).max())
    assert np.array_equal(rows, everyone[users]) and np.array_equal(pairs, everyone[pu, pi]), "one row, many rows, pairs: the same bits"
    want_pairs = golden[name + "/pair_scores"]
    assert (np.abs(pairs.astype(np.float64) - want_pairs) <= 2 * score_tolerance(r, pu, r.scores(pu)[np.arange(len(pu)), pi])).all()
    if c["lik"] == "mult":
        assert np.abs(everyone.astype(np.float64).sum(axis=1) - 1.0).max() <= 1e-5
    if name == "sat":   # what the case is for: in the first step's forward (with its noise) some held item has p < 1e-6
        start = vc.Restatement(vc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"], vc.case_params(c))
        p = start.forward(start.B, vc.case_noise(c)[0])["p"]
        print("sat: the smallest p of a held item in the first forward is %.3g" % p[start.B > 0].min())
        assert (p[start.B > 0] < 1e-6).any(), "the saturated case: some held item has p < 1e-6"


def test_more_ids_than_one_chunk_holds(golden):
    """the chunk loop past its first chunk (b0 > 0): the entry points take min(1024, 256 MiB / (4 n_items)) users per chunk,
    which is 1024 at 131 items (256 MiB / 524 bytes is about 512 000), so 1 025 ids make a second chunk of one"""
    name = min(vc.FULL_CASES, key=lambda n: (vc.CASES[n]["nu"] * vc.CASES[n]["ni"], vc.FULL_CASES.index(n)))
    c = vc.CASES[name]
    cap = min(1024, (256 << 20) // (4 * c["ni"]))
    n = 1025
    assert n > cap, "more than one chunk's worth"
    params = {p: golden["%s/P/%s" % (name, vc.SHORT[p])] for p in vc.NAMES}
    users, items = np.arange(n) % c["nu"], np.arange(n) % c["ni"]
    with handle(name, params) as m:
        everyone, codes = m.score_users(np.arange(c["nu"])), m.encode_users(np.arange(c["nu"]))
        rows, h2, pairs = m.score_users(users), m.encode_users(users), m.score_pairs(users, items)
    assert rows.shape == (n, c["ni"]) and np.array_equal(rows.view(np.uint32), everyone[users].view(np.uint32))
    assert h2.shape == (n, c["h"]) and np.array_equal(h2.view(np.uint32), codes[users].view(np.uint32))
    assert pairs.shape == (n,) and np.array_equal(pairs.view(np.uint32), everyone[users, items].view(np.uint32))


def test_rank_batch_is_the_sort_of_score_batch(golden):
    """encode_users + the fused scorer on logits against sorting the probabilities, where these do not tie"""
    name = "i257"
    c = vc.CASES[name]
    params = {n: golden["%s/P/%s" % (name, vc.SHORT[n])] for n in vc.NAMES}
    users = np.arange(c["nu"], dtype=np.int32)
    with handle(name, params) as m:
        H2, S = m.encode_users(users), m.score_users(users)
    sc = _lib.Scorer(H2, params[vc.NAMES[8]], params[vc.NAMES[9]], np.zeros(c["nu"], np.float32))
    try:
        items, _ = sc.rank_topk(users, 20)
    finally:
        sc.close()
    order = np.argsort(-S.astype(np.float64), axis=1, kind="stable")[:, :21]
    top = np.take_along_axis(S, order, axis=1)
    clear = (np.diff(top.astype(np.float64), axis=1) < 0).all(axis=1)
    print("rank_batch vs sorted score_batch: %d of %d users have 21 distinct top probabilities; all of those agree: %s" % (
        clear.sum(), len(users), np.array_equal(items[clear], order[clear, :20])))
    assert clear.sum() >= 0.9 * len(users) and np.array_equal(items[clear], order[clear, :20])


def test_fit_end_to_end(golden, monkeypatch, tmp_path):
    """cornac_amd.VAECF.fit on a full golden case: the case's tables loaded, torch.randn serving the case's noise"""
    import torch

    name = "i257"
    c, noise = vc.CASES[name], vc.case_noise(vc.CASES[name])
    queue = [noise[e, u0:u0 + c["bs"]] for e in range(c["epochs"]) for u0 in range(0, c["nu"], c["bs"])]

    def randn(b, k):
        e = queue.pop(0)
        assert e.shape == (b, k)
        return torch.tensor(e)

    monkeypatch.setattr(torch, "randn", randn)
    m = VAECF(k=c["k"], autoencoder_structure=[c["h"]], act_fn=c["act"], likelihood=c["lik"], n_epochs=c["epochs"], batch_size=c["bs"],
              learning_rate=c["lr"], beta=c["beta"], seed=3)
    m.load_state_dict(vc.case_params(c))
    m.fit(vc.dataset(name))
    assert not queue
    want = {n: golden["%s/P/%s" % (name, vc.SHORT[n])].astype(np.float64) for n in vc.NAMES}
    compare(golden, name, "fit", m.state_dict(), want, "d_ref", "max")   # (the reference's tables are d_ref from the restatement's)
    users = vc.score_users(c)
    r = vc.Restatement(vc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"], m.state_dict())
    S = m.score_batch(users)
    assert (np.abs(S - r.scores(users)) <= score_tolerance(r, users, r.scores(users))).all()
    assert np.array_equal(m.score(int(users[1])), S[1]) and m.score(int(users[1]), 7) == S[1][7]
    items, _ = m.rank_batch(users, k=5)
    ranked, scores = m.rank(int(users[1]))
    assert np.array_equal(scores, S[1]) and np.array_equal(ranked[:5], items[1])
    back = VAECF.load(m.save(str(tmp_path)))
    assert "_vae_handle" not in back.__dict__ and np.array_equal(back.score_batch(users), S)


def test_limits_are_named():
    X = vc.case_matrix(vc.CASES["b1"])
    for kw, text in ((dict(k=257, h=4), "1 <= k <= 256"), (dict(k=4, h=1025), "1 <= h <= 1024"), (dict(k=0, h=4), "1 <= k <= 256")):
        with pytest.raises(_lib.HipError, match=text):
            _lib.VaecfModel(X, **kw)
    m = _lib.VaecfModel(X, 2, 3)
    try:
        for bs in (0, 1025):
            with pytest.raises(_lib.HipError, match="1 <= batch_size <= 1024"):
                m.fit_epoch(bs, 1e-3, 1.0, eps=np.zeros((5, 2), np.float32))
    finally:
        m.close()
