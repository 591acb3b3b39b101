"""BiVAECF on the device, through the C ABI (`_lib.BivaeModel`) and through cornac_amd.BiVAECF, against (a) the float64
restatement of tests/bivae_cases.py and (b) what the reference's own BiVAE / learn wrote into tests/golden/bivae_ref.npz
(tests/test_bivaecf_cpu.py holds (a) against (b)).

The 12 parameter tables, Adam's m and v, and the four factor tables theta, beta, mu_theta, mu_beta are each compared table by
table with the tolerance
    max(16 * d_ref, 4 units in the last float32 place of max|table|),
d_ref = the reference's own float32 distance to the restatement, read from the golden; for every parameter table that
tolerance stays under 1 % of the table's recorded movement (bivae_cases.check_condition).  The moments are compared because
Adam's early updates are nearly lr * sign(g): a gradient wrong by a constant factor leaves the parameters right and only m
and v wrong.  Every check prints the measured difference next to its tolerance.

Losses: a batch-mean loss is a float32 sum of at most 1031 terms per row (the dense pass's partial sums, then the held
entries), so it is held to 1e-4 relative.  Scores: p carries the logit's absolute error as a relative one; the logit is a
chain of k float32 roundings, so p is held to 64 * 2^-24 * (1 + max|logit|) relative plus 1e-30, and to twice that against
the golden's float32 scores.

Device noise: under a few NumPy seeds the restatement's first-epoch losses of case i63 stay within 7 % of those under the
case's own noise (measured on the CPU), so the 20 % band of test_vaecf_gpu.py is kept.

Measured on an MI355X, over the 31 cases: parameters at most 1.6e-07 from the restatement and at most 0.34 of their
tolerance (tolerances 3.1e-09 .. 2.3e-06, each under 0.035 % of its table's movement); m at most 1.9e-06 and 0.35 of its
tolerance; v at most 1.6e-06 and 0.55 of its tolerance; the factor tables at most 5.8e-07 and 0.12 of theirs; losses at most
3.7e-05 relative; two runs the same bits.  Item 2's column of the users' W1 moved 3.0e-03 after its first gradient and ended
1.4e-08 from the restatement.  Scores at most 0.025 of their bound from the restatement and 0.014 of twice it from the
reference's float32 scores; rank_batch equal to the sorted score_batch for all 250 users; first-epoch losses under device
noise within 5 % of those under the case's noise.  `tools/bivaecf_epoch.py`, synthetic ML-20M shape, host clock, two
alternating rounds: defaults (k 10, h 20, batch 100) epoch 2.02 s (item step 4.00 ms, user step 0.68 ms) against 10.9 s of
the torch loop (28.5 ms, 2.34 ms); k 50, h 100, batch 500: 0.90 s (9.71 ms, 1.35 ms) against 13.2 s (112 ms, 25.7 ms).
"""
import functools

import numpy as np
import pytest

import bivae_cases as bc
from conftest import load_golden
from cornac_amd import BiVAECF, _lib
from cornac_amd.bivaecf import BiVAETables

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("bivae_ref")


@functools.lru_cache(maxsize=None)
def restated(name):
    """computed once per case, shared and left unchanged"""
    r, losses, init = bc.run_case(name)
    for d in (r.P, r.M, r.V, r.F):
        for a in d.values():
            a.setflags(write=False)
    return r, losses, init


class handle:
    """a device model that is closed when the block ends"""

    def __init__(self, name, params=None, factors=None):
        c = bc.CASES[name]
        self.m = _lib.BivaeModel(bc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"])
        self.m.set_params(bc.case_params(c) if params is None else params)
        self.m.set_factors(**(bc.case_factors(c) if factors is None else factors))

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


def device_run(name):
    c = bc.CASES[name]
    ni, nu = bc.case_noise(c)
    with handle(name) as m:
        losses = np.concatenate([m.fit_epoch(c["bs"], c["lr"], c["beta"], eps_item=ni[e], eps_user=nu[e])[2] for e in range(c["epochs"])])
        m.infer_means()
        P, F = m.get_params(), m.get_factors()
        M, V, tu, ti = m.get_state()
    return P, M, V, F, (ti, tu), losses


def compare(golden, name, what, got, want, kind_d, kind_max, names=bc.NAMES):
    """every table of `got` against `want` under the rule; returns the worst difference / tolerance"""
    worst = 0.0
    for n in names:
        q = bc.TABLES.index(n)
        d_ref, top = float(golden["%s/%s" % (name, kind_d)][q]), float(golden["%s/%s" % (name, kind_max)][q])
        tol = bc.tolerance(d_ref, top)
        diff = float(np.abs(got[n].astype(np.float64) - want[n]).max())
        print("%s %s %s: device vs restatement %.3g; tolerance %.3g (16 x %.3g, 4 ulp %.3g)" % (
            name, what, bc.SHORT.get(n, n), diff, tol, d_ref, 4.0 * bc.ulp32(top)))
        assert got[n].dtype == np.float32 and got[n].shape == want[n].shape
        assert diff <= tol, (name, what, n, diff, tol)
        worst = max(worst, diff / tol)
    return worst


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_steps_against_the_restatement(golden, name):
    c = bc.CASES[name]
    share = bc.check_condition(golden, name)
    r, r_losses, init = restated(name)
    P, M, V, F, t, losses = device_run(name)
    print("%s: the tolerance is at most %.3g of a table's movement (allowed: under 0.01)" % (name, share))
    assert t == bc.n_steps(c) == (r.t["item"], r.t["user"]) and c["epochs"] >= 2
    wp = compare(golden, name, "param", P, r.P, "d_ref", "max")
    wm = compare(golden, name, "m", M, r.M, "d_ref_m", "max_m")
    wv = compare(golden, name, "v", V, r.V, "d_ref_v", "max_v")
    wf = compare(golden, name, "factor", F, r.F, "d_ref", "max", bc.FACTORS)
    rel = float(np.max(np.abs(losses - r_losses) / np.maximum(1.0, np.abs(r_losses))))
    print("%s: worst share of the tolerance: params %.3g, m %.3g, v %.3g, factor tables %.3g; losses %.3g relative (allowed 1e-4)" % (
        name, wp, wm, wv, wf, rel))
    assert losses.shape == r_losses.shape and rel <= 1e-4
    again = device_run(name)
    for a, b in zip((P, M, V, F), again[:4]):
        assert all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in a), "two runs give the same bits"
    assert np.array_equal(losses, again[5])
    if c["ni"] >= 8:
        uW1, iW1 = bc.NAMES[0], bc.NAMES[6]
        assert np.array_equal(P[uW1][:, 1], init[uW1][:, 1]), "an item nobody holds: its column of the users' W1 stays in place"
        assert (M[uW1][:, 1] == 0).all() and (V[uW1][:, 1] == 0).all()
        # ... and as an EMPTY ROW of the item side it is encoded from the bias alone, trains the item tables and stays finite
        assert np.isfinite(F["beta"][1]).all() and np.isfinite(F["mu_beta"][1]).all() and np.abs(F["mu_beta"][1]).max() > 0
        assert all(np.isfinite(P[n]).all() for n in bc.NAMES) and np.abs(P[iW1] - init[iW1]).max() > 0


def test_a_column_held_in_the_first_batch_only_keeps_moving(golden):
    """the dense-Adam trap: item 2 is held by users 0 and 1 only, so in the user pass its column of the users' W1 has a
    gradient in the first batch alone, and m != 0 still moves it in every later step of the pass"""
    name = "i63"
    c = bc.CASES[name]
    X = bc.case_matrix(c)
    assert sorted(X.tocsc()[:, 2].indices) == [0, 1] and c["bs"] > 1
    ni, nu = bc.case_noise(c)
    one = bc.Restatement(X, c["k"], c["h"], c["act"], c["lik"], bc.case_params(c), bc.case_factors(c))
    for r0 in range(0, c["ni"], c["bs"]):   # the first epoch's item pass, then ONE user step
        one.step("item", r0, min(c["bs"], c["ni"] - r0), ni[0, 0, r0:r0 + c["bs"]], ni[0, 1, r0:r0 + c["bs"]], c["lr"], c["beta"])
    one.step("user", 0, c["bs"], nu[0, 0, :c["bs"]], nu[0, 1, :c["bs"]], c["lr"], c["beta"])
    r, _, _ = restated(name)
    P = device_run(name)[0]
    W1 = bc.NAMES[0]
    tol = bc.tolerance(golden[name + "/d_ref"][0], golden[name + "/max"][0])
    since, diff = float(np.abs(P[W1][:, 2] - one.P[W1][:, 2]).max()), float(np.abs(P[W1][:, 2] - r.P[W1][:, 2]).max())
    print("item 2's column of the users' W1: moved %.3g since the first user step (a sparse Adam would give far less); %.3g from the "
          "restatement, tolerance %.3g" % (since, diff, tol))
    assert diff <= tol and since > 100 * tol


def test_device_noise_repeats_under_a_seed_and_differs_under_another():
    name = "i63"
    c = bc.CASES[name]

    def run(seed):
        with handle(name) as m:
            losses = [m.fit_epoch(c["bs"], c["lr"], c["beta"], seed=seed)[2] for _ in range(2)]
            return dict(m.get_params(), **m.get_factors()), np.concatenate(losses)

    (a, la), (b, lb), (d, ld) = run(11), run(11), run(12)
    assert all(np.array_equal(a[n].view(np.uint32), b[n].view(np.uint32)) for n in a) and np.array_equal(la, lb)
    assert any(not np.array_equal(a[n], d[n]) for n in bc.NAMES) and not np.array_equal(la, ld)
    assert all(np.isfinite(a[n]).all() for n in a) and np.isfinite(la).all()
    # the noise is keyed by the step: the second epoch does not repeat the first
    assert not np.array_equal(la[:len(la) // 2], la[len(la) // 2:])
    # the noise is standard normal: the first epoch's losses stay near those of the case's own standard normal noise
    ref = restated(name)[1][:len(la) // 2]
    print("first-epoch losses under device noise / under the case's noise: %s" % np.round(la[:len(ref)] / ref, 4))
    assert np.all(np.abs(la[:len(ref)] - ref) < 0.2 * np.abs(ref))


def score_tolerance(r, users, want):
    return 64.0 * 2.0 ** -24 * (1.0 + float(np.abs(r.logits(users)).max())) * np.abs(want) + 1e-30


def golden_tables(golden, name):
    return ({n: golden["%s/P/%s" % (name, bc.SHORT[n])] for n in bc.NAMES}, {n: golden["%s/F/%s" % (name, n)] for n in bc.FACTORS})


@pytest.mark.parametrize("name", bc.FULL_CASES)
def test_scores_against_the_restatement_and_the_golden(golden, name):
    c = bc.CASES[name]
    params, factors = golden_tables(golden, name)
    r = bc.Restatement(bc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"], params, factors)
    users, (pu, pi) = bc.score_users(c), bc.score_pairs(c)
    with handle(name, params, factors) as m:
        got, gotf = m.get_params(), m.get_factors()
        assert all(np.array_equal(got[n], params[n]) for n in bc.NAMES), "set / get round trip, both W1 transposed and back"
        assert all(np.array_equal(gotf[n], factors[n]) for n in bc.FACTORS)
        rows, pairs, everyone = m.score_users(users), m.score_pairs(pu, pi), m.score_users(np.arange(c["nu"]))
        with pytest.raises(_lib.HipError, match="user %d out of range" % c["nu"]):
            m.score_users([0, c["nu"]])
        with pytest.raises(_lib.HipError, match="item %d out of range" % c["ni"]):
            m.score_pairs([0], [c["ni"]])
        with pytest.raises(_lib.HipError, match="user -1 out of range"):
            m.score_pairs([-1], [0])
        assert m.score_users(np.zeros(0, np.int32)).shape == (0, c["ni"]) and m.score_pairs([], []).shape == (0,)
        m.infer_means()   # mu does not depend on theta or beta: the means again, from the reference's tables
        means = m.get_factors()
    want = r.scores(users)
    tol = score_tolerance(r, users, want)
    d_rest, d_gold = np.abs(rows - want), np.abs(rows.astype(np.float64) - golden[name + "/scores"])
    print("%s: scores vs restatement at most %.3g of their bound, vs the reference's float32 scores %.3g of twice it" % (
        name, (d_rest / tol).max(), (d_gold / (2 * tol)).max()))
    assert rows.dtype == np.float32 and (d_rest <= tol).all() and (d_gold <= 2 * tol).all()
    assert np.array_equal(rows, everyone[users]) and np.array_equal(pairs, everyone[pu, pi]), "one row, many rows, pairs: the same bits"
    ds = bc.dataset(name)
    scaled = pairs.astype(np.float64) * (ds.max_rating - ds.min_rating) + ds.min_rating
    ptol = 2 * score_tolerance(r, pu, r.scores(pu)[np.arange(len(pu)), pi]) * (ds.max_rating - ds.min_rating)
    assert (np.abs(scaled - golden[name + "/pair_scores"]) <= ptol + 4 * bc.ulp32(ds.max_rating)).all()
    compare(golden, name, "infer_means", means, factors, "d_ref", "max", ("mu_theta", "mu_beta"))
    assert np.array_equal(means["theta"], factors["theta"]) and np.array_equal(means["beta"], factors["beta"])


def test_more_ids_than_one_chunk_holds(golden):
    """the chunk loop past its first chunk (b0 > 0): the entry points take min(1024, 256 MiB / (4 n_items)) users per chunk,
    which is 1024 at 131 items, so 1 025 ids make a second chunk of one"""
    name = min(bc.FULL_CASES, key=lambda n: (bc.CASES[n]["nu"] * bc.CASES[n]["ni"], bc.FULL_CASES.index(n)))
    c = bc.CASES[name]
    cap = min(1024, (256 << 20) // (4 * c["ni"]))
    n = 1025
    assert n > cap, "more than one chunk's worth"
    params, factors = golden_tables(golden, name)
    users, items = np.arange(n) % c["nu"], np.arange(n) % c["ni"]
    with handle(name, params, factors) as m:
        everyone = m.score_users(np.arange(c["nu"]))
        rows, pairs = m.score_users(users), m.score_pairs(users, items)
    assert rows.shape == (n, c["ni"]) and np.array_equal(rows.view(np.uint32), everyone[users].view(np.uint32))
    assert pairs.shape == (n,) and np.array_equal(pairs.view(np.uint32), everyone[users, items].view(np.uint32))


def test_rank_batch_is_the_sort_of_score_batch(golden):
    """the fused scorer on the logits <mu_theta, mu_beta> against sorting the probabilities, where these do not tie
    (tests/test_bivaecf_cpu.py asserts that the restatement alone has 21 distinct top probabilities for 90 % of this case's users)"""
    name = "i257"
    c = bc.CASES[name]
    params, factors = golden_tables(golden, name)
    users = np.arange(c["nu"], dtype=np.int32)
    with handle(name, params, factors) as m:
        S = m.score_users(users)
    sc = _lib.Scorer(factors["mu_theta"], factors["mu_beta"], np.zeros(c["ni"], np.float32), np.zeros(c["nu"], np.float32))
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
    """cornac_amd.BiVAECF.fit on a full golden case: the case's tables loaded, torch.randn serving the case's noise"""
    import torch

    name = "i257"
    c = bc.CASES[name]
    queue = bc.noise_queue(c)

    def randn(b, k):
        e = queue.pop(0)
        assert e.shape == (b, k)
        return torch.tensor(e)

    monkeypatch.setattr(torch, "randn", randn)
    m = BiVAECF(k=c["k"], encoder_structure=[c["h"]], act_fn=c["act"], likelihood=c["lik"], n_epochs=c["epochs"], batch_size=c["bs"],
                learning_rate=c["lr"], beta_kl=c["beta"], seed=3)
    m.bivae = BiVAETables(bc.case_params(c), **bc.case_factors(c))
    m.fit(bc.dataset(name))
    assert not queue and np.shape(m.loss_history) == (c["epochs"], 2)
    params, factors = golden_tables(golden, name)
    compare(golden, name, "fit", m.bivae.state_dict(), {n: a.astype(np.float64) for n, a in params.items()}, "d_ref", "max")
    compare(golden, name, "fit", {n: getattr(m.bivae, n) for n in bc.FACTORS}, {n: a.astype(np.float64) for n, a in factors.items()},
            "d_ref", "max", bc.FACTORS)   # (the reference's tables are d_ref from the restatement's)
    si = bc.n_steps(c)[0] // c["epochs"]
    want = golden[name + "/losses"].reshape(c["epochs"], -1)
    assert np.allclose(m.loss_history, np.stack([want[:, :si].sum(axis=1) / c["ni"], want[:, si:].sum(axis=1) / c["nu"]], axis=1), rtol=1e-4)
    users = bc.score_users(c)
    r = bc.Restatement(bc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"], {}, {n: getattr(m.bivae, n) for n in bc.FACTORS})
    S = m.score_batch(users)
    assert (np.abs(S - r.scores(users)) <= score_tolerance(r, users, r.scores(users))).all()
    assert np.array_equal(m.score(int(users[1])), S[1])
    assert m.score(int(users[1]), 7) == np.float64(S[1][7]) * (m.max_rating - m.min_rating) + m.min_rating
    items, _ = m.rank_batch(users, k=5)
    ranked, scores = m.rank(int(users[1]))
    assert np.array_equal(scores, S[1]) and np.array_equal(ranked[:5], items[1])
    back = BiVAECF.load(m.save(str(tmp_path)))
    assert "_bivae_handle" not in back.__dict__ and np.array_equal(back.score_batch(users), S)


def test_limits_are_named():
    X = bc.case_matrix(bc.CASES["b1"])
    for kw, text in ((dict(k=257, h=4), "1 <= k <= 256"), (dict(k=4, h=1025), "1 <= h <= 1024"), (dict(k=0, h=4), "1 <= k <= 256")):
        with pytest.raises(_lib.HipError, match=text):
            _lib.BivaeModel(X, **kw)
    m = _lib.BivaeModel(X, 2, 3)
    try:
        for bs in (0, 1025):
            with pytest.raises(_lib.HipError, match="1 <= batch_size <= 1024"):
                m.fit_epoch(bs, 1e-3, 1.0)
    finally:
        m.close()
