"""NCF on the device, through the C ABI (`_lib.NcfModel`) and through cornac_amd.GMF / MLP / NeuMF, against (a) the float64
restatement of tests/ncf_cases.py and (b) what the reference's own modules and _fit_pt wrote into tests/golden/ncf_ref.npz
(tests/test_ncf_cpu.py holds (a) against (b)).

Parameters and the learner's state arrays are each compared table by table with the tolerance
    max(16 * d_ref, 4 units in the last float32 place of max|table|),
d_ref = the reference's own float32 distance to the restatement, read from the golden; for every parameter table that
tolerance stays under 1 % of the table's recorded movement (ncf_cases.check_condition); a table that does not move is
compared bit for bit.  Every check prints the measured difference next to its tolerance.

Losses: a step's loss sums at most 1 280 float32 terms and is held to 1e-4 relative.  Scores: p carries the logit's absolute
error as a relative one, so p is held to 64 * 2^-24 * (1 + max|logit|) against the restatement and to twice that against
the reference's float32 scores.

Measured on an MI355X, over the 44 cases: parameters at most 0.51 of their tolerance, the first state array 0.27, the second
0.66; losses at most 2.5e-06 relative; two runs the same bits.  Under Adam user 0's rows moved 1.6e-03 after their last
gradient (1 100 to 1 800 tolerances) and ended within 2.6e-08 of the restatement.  Scores at most 0.024 of their bound from the
restatement and 0.014 of twice it from the reference's float32 scores; GMF's rank_batch equal to the sorted score_batch for
all 37 users; user 1's eight admissible negatives drawn 62 to 93 times each over 50 epochs (expected 75, s.d. 8.1)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ncf_cases as nc
from conftest import load_golden
from cornac_amd import GMF, MLP, NeuMF, Dataset, _lib

pytestmark = pytest.mark.gpu
CLASSES = {"GMF": GMF, "MLP": MLP, "NeuMF": NeuMF}


@pytest.fixture(scope="module")
def golden():
    return load_golden("ncf_ref")


@functools.lru_cache(maxsize=None)
def restated(name):
    """computed once per case, shared and left unchanged"""
    run = nc.run_case(name)
    for d in (run["r"].P, run["r"].S1, run["r"].S2, run["after1"]):
        for a in d.values():
            a.setflags(write=False)
    return run


class handle:
    """a device model that is closed when the block ends"""

    def __init__(self, c, params=None, X=None):
        X = sp.csr_matrix((c["nu"], c["ni"]), dtype=np.float64) if X is None else X
        self.m = _lib.NcfModel(c["kind"], X, c["f"], c["layers"], c["act"])
        if params is not None:
            self.m.set_params(params)

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


@functools.lru_cache(maxsize=None)
def device_run(name):
    c = nc.CASES[name]
    with handle(c, nc.case_params(c)) as m:
        _, losses = m.fit_epoch(*nc.epoch_arrays(nc.case_batches(c)), c["lr"], c["reg"], c["learner"])
        P = m.get_params()
        S1, S2, t = m.get_state()
    return P, S1, S2, t, losses


def compare(golden, name, what, got, want, kind_d, kind_max):
    """every table of `got` against `want` under the rule; returns the worst difference / tolerance"""
    worst = 0.0
    for q, n in enumerate(nc.case_names(name)):
        tol = nc.tolerance(golden["%s/%s" % (name, kind_d)][q], golden["%s/%s" % (name, kind_max)][q])
        d = float(np.abs(got[n].astype(np.float64) - want[n]).max())
        worst = max(worst, d / tol)
        print("%s %s %s: %.3g (tolerance %.3g)" % (name, what, n, d, tol))
        assert got[n].dtype == np.float32 and d <= tol, (name, what, n, d, tol)
    return worst


# ---- steps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_steps_against_the_restatement(golden, name):
    c, run = nc.CASES[name], restated(name)
    P, S1, S2, t, losses = device_run(name)
    assert t == len(c["steps"]) and np.isfinite(losses).all()
    r = run["r"]
    shares = [compare(golden, name, "P", P, r.P, "d_ref", "max"), compare(golden, name, "S1", S1, r.S1, "d_ref_s1", "max_s1"),
              compare(golden, name, "S2", S2, r.S2, "d_ref_s2", "max_s2")]
    rel = float(np.abs(losses - run["losses"]).max() / np.abs(run["losses"]).max())
    print("%s: worst shares of the tolerance %s, losses %.3g relative (allowed 1e-4)" % (name, ["%.3g" % s for s in shares], rel))
    assert rel <= 1e-4
    for q, n in enumerate(nc.case_names(name)):   # a table without movement: bit for bit
        if golden[name + "/move"][q] == 0.0:
            assert np.array_equal(P[n].view(np.uint32), run["init"][n].view(np.uint32)), n


@pytest.mark.parametrize("name", ["f65", "l66", "n8", "kl/NeuMF/rmsprop", "kr/NeuMF/adagrad"])
def test_two_runs_give_the_same_bits(name):
    c = nc.CASES[name]
    first = device_run(name)
    with handle(c, nc.case_params(c)) as m:
        _, losses = m.fit_epoch(*nc.epoch_arrays(nc.case_batches(c)), c["lr"], c["reg"], c["learner"])
        P = m.get_params()
        S1, S2, _ = m.get_state()
    for got, want in ((P, first[0]), (S1, first[1]), (S2, first[2])):
        assert all(np.array_equal(got[n].view(np.uint32), want[n].view(np.uint32)) for n in got)
    assert np.array_equal(losses, first[4])


@pytest.mark.parametrize("name", sorted(n for n, c in nc.CASES.items() if c["kind"] == "NeuMF"))
def test_neumf_tables_without_a_gradient_stay_as_they_are(name):
    P, S1, S2, _, _ = device_run(name)
    init = restated(name)["init"]
    for n in nc.UNUSED("NeuMF"):
        assert np.array_equal(P[n].view(np.uint32), init[n].view(np.uint32)), n
        assert not S1[n].any() and not S2[n].any(), n


def test_a_row_untouched_since_step_one_still_moves_under_adam(golden):
    name = "kl/NeuMF/adam"
    run = restated(name)
    P = device_run(name)[0]
    for q, n in enumerate(nc.case_names(name)):
        if "user_embedding" not in n:
            continue
        tol = nc.tolerance(golden[name + "/d_ref"][q], golden[name + "/max"][q])
        moved = float(np.abs(run["r"].P[n][0] - run["after1"][n][0]).max())
        d = float(np.abs(P[n][0].astype(np.float64) - run["r"].P[n][0]).max())
        print("%s user 0: moved %.3g since step 1 (%.0f tolerances), device %.3g from the restatement (tolerance %.3g)" % (n, moved, moved / tol, d, tol))
        assert moved > 100 * tol and d <= tol


@pytest.mark.parametrize("learner", ["sgd", "rmsprop", "adagrad"])
@pytest.mark.parametrize("kind", nc.KINDS)
def test_untouched_rows_stay_bit_equal_without_weight_decay(kind, learner):
    name = "kl/%s/%s" % (kind, learner)
    c = nc.CASES[name]
    assert c["reg"] == 0.0
    P, S1, _, _, _ = device_run(name)
    init = restated(name)["init"]
    for n in nc.case_names(name):
        if "item_embedding" in n:   # the last item never appears
            assert np.array_equal(P[n][-1].view(np.uint32), init[n][-1].view(np.uint32)), n
            assert not S1[n][-1].any(), n
        if "user_embedding" in n and learner == "rmsprop":   # user 0's square_avg decays after step 1
            assert (S1[n][0] > 0).any() and np.abs(S1[n][0] - restated(name)["r"].S1[n][0]).max() < 1e-6 * S1[n][0].max() + 1e-30


# ---- scores ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", nc.FULL_CASES)
def test_scores_against_the_restatement_and_the_reference(golden, name):
    c = nc.CASES[name]
    tabs = {n: golden["%s/P/%s" % (name, n)] for n in nc.case_names(name)}
    f32 = nc.new_restatement(c, tabs)
    users, (pu, pi) = nc.score_users(c), nc.score_pairs(c)
    with handle(c, tabs) as m:
        S = m.score_users(users)
        pairs = m.score_pairs(pu, pi)
        one = np.stack([m.score_users([u])[0] for u in users])
        every = m.score_users(np.arange(c["nu"]))
        assert S.dtype == np.float32 and S.shape == (len(users), c["ni"])
        assert np.array_equal(S.view(np.uint32), one.view(np.uint32)) and np.array_equal(S.view(np.uint32), every[users].view(np.uint32))
        assert np.array_equal(pairs.view(np.uint32), every[pu, pi].view(np.uint32)), "pairs are the rows' entries, bit for bit"
        # more ids than one chunk holds
        rs = np.random.RandomState(3)
        many_u, many_i = rs.randint(0, c["nu"], 5000), rs.randint(0, c["ni"], 5000)
        assert np.array_equal(m.score_pairs(many_u, many_i).view(np.uint32), every[many_u, many_i].view(np.uint32))
        if c["ni"] <= 32:
            assert np.array_equal(m.score_users(many_u[:1100]).view(np.uint32), every[many_u[:1100]].view(np.uint32))
        for bad_u, bad_i, text in (([c["nu"]], None, "user %d out of range" % c["nu"]), ([-1], None, "user -1 out of range"),
                                   ([0], [c["ni"]], "item %d out of range" % c["ni"]), ([0], [-2], "item -2 out of range")):
            with pytest.raises(_lib.HipError, match="%s: %s" % (c["kind"], text)):
                m.score_users(bad_u) if bad_i is None else m.score_pairs(bad_u, bad_i)
    bound = 64 * 2.0 ** -24 * (1 + np.abs(f32.logits(users)).max())
    want = f32.scores(users)
    d_r = float((np.abs(S - want) / want).max())
    d_g = float((np.abs(S.astype(np.float64) - golden[name + "/scores"]) / want).max())
    d_p = float((np.abs(pairs.astype(np.float64) - golden[name + "/pair_scores"]) / f32.pair_scores(pu, pi)).max())
    print("%s scores: %.3g from the restatement (bound %.3g), %.3g / %.3g from the reference (bound %.3g)" % (name, d_r, bound, d_g, d_p, 2 * bound))
    assert d_r <= bound and d_g <= 2 * bound and d_p <= 2 * bound


def test_a_saturated_sample_gives_a_finite_loss_and_no_gradient():
    name = "f33"   # labels all 1
    c = nc.CASES[name]
    params = dict(nc.case_params(c))
    params["logit.bias"] = np.array([-200.0], np.float32)   # p = 0 exactly in float32
    u, i, y = nc.case_batches(c)[0]
    with handle(c, params) as m:
        assert (m.score_pairs(u, i) == 0.0).all()
        _, losses = m.fit_epoch(*nc.epoch_arrays([(u, i, y)]), c["lr"], c["reg"], c["learner"])
        P = m.get_params()
    print("saturated step loss %r" % (losses,))
    assert losses.shape == (1,) and losses[0] == 100.0
    assert all(np.isfinite(a).all() for a in P.values())
    assert all(np.array_equal(P[n], params[n]) for n in P), "p (1 - p) = 0: torch's backward gives a zero gradient"


def test_gmf_rank_batch_is_the_sort_of_score_batch(golden):
    name = nc.RANK_CASE
    c = nc.CASES[name]
    ds = Dataset.from_arrays(np.arange(c["nu"]), np.arange(c["nu"]) % c["ni"], np.ones(c["nu"]), num_users=c["nu"], num_items=c["ni"])
    m = GMF(num_factors=c["f"], num_epochs=0, verbose=False, seed=1).fit(ds)
    m.load_state_dict({n: golden["%s/P/%s" % (name, n)] for n in nc.case_names(name)})
    users = np.arange(c["nu"])
    S = m.score_batch(users)
    top, _ = m.rank_batch(users, k=10)
    distinct = 0
    for r in users:
        order = np.argsort(-S[r].astype(np.float64), kind="stable")
        if len(np.unique(S[r][order[:11]])) == 11:
            distinct += 1
            assert np.array_equal(top[r], order[:10]), r
    print("GMF rank_batch == sorted score_batch for %d of %d users (the others' top probabilities tie)" % (distinct, len(users)))
    assert distinct >= 0.9 * len(users)
    ranked, scores = m.rank(3)
    assert np.array_equal(scores, S[3]) and np.array_equal(ranked[:10], top[3])


# ---- the sampler -------------------------------------------------------------------------------------------------------------
NU, NI = 12, 10


@functools.lru_cache(maxsize=None)
def sampler_matrix():
    """user 0 holds every item but 7; user 1 holds items 0 and 3 and a stored 0.0 at item 5; the rest hold a few ratings 1..5"""
    rs = np.random.RandomState(17)
    D = np.zeros((NU, NI))
    for u in range(2, NU):
        held = rs.permutation(NI)[:rs.randint(1, 6)]
        D[u, held] = rs.randint(1, 6, len(held))
    D[0] = 3.0
    D[0, 7] = 0.0
    D[1, [0, 3]] = 4.0
    rows, cols = np.nonzero(D)
    rows, cols, vals = np.append(rows, 1), np.append(cols, 5), np.append(D[rows, cols], 0.0)
    X = sp.csr_matrix((vals, (rows, cols)), shape=(NU, NI))
    X.sort_indices()
    assert X.nnz == len(vals) and X[1].nnz == 3
    return X


SAMPLER = dict(kind="GMF", nu=NU, ni=NI, f=4, layers=(), act="relu")


def test_draw_epoch():
    X = sampler_matrix()
    D = X.toarray()
    stored = set(zip(*X.nonzero())) | {(1, 5)}
    bs, nn = 7, 4
    counts, zero_drawn = np.zeros(NI), 0
    with handle(SAMPLER, X=X) as m:
        a, b = m.draw_epoch(bs, nn, seed=5, epoch=0), m.draw_epoch(bs, nn, seed=5, epoch=0)
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "one seed and epoch: the same arrays"
        assert not np.array_equal(a[2], m.draw_epoch(bs, nn, seed=6, epoch=0)[2]) and not np.array_equal(a[2], m.draw_epoch(bs, nn, seed=5, epoch=1)[2])
        for epoch in range(50):
            ptr, users, items, labels = m.draw_epoch(bs, nn, seed=5, epoch=epoch)
            assert ptr[0] == 0 and ptr[-1] == X.nnz * (1 + nn) == len(users) and len(ptr) == -(-X.nnz // bs) + 1
            pos = []
            for s0, s1 in zip(ptr[:-1], ptr[1:]):
                nb = (s1 - s0) // (1 + nn)
                assert labels[s0:s0 + nb].all() and not labels[s0 + nb:s1].any()
                assert np.array_equal(users[s0 + nb:s1], users[s0:s0 + nb].repeat(nn)), "negatives follow their positives, user-major"
                pos += list(zip(users[s0:s0 + nb].tolist(), items[s0:s0 + nb].tolist()))
                neg_u, neg_i = users[s0 + nb:s1], items[s0 + nb:s1]
                assert (neg_i >= 0).all() and (neg_i < NI).all() and not (D[neg_u, neg_i] > 0).any(), "no negative is stored with a value > 0"
                assert (neg_i[neg_u == 0] == 7).all(), "the user holding all items but one gets that one"
                counts += np.bincount(neg_i[neg_u == 1], minlength=NI)
                zero_drawn += int((neg_i[neg_u == 1] == 5).sum())
            assert sorted(pos) == sorted(stored) and len(pos) == X.nnz, "the positives are a permutation of the stored entries"
        full = X.tolil()
        full[2, :] = 1.0
        with handle(SAMPLER, X=full.tocsr()) as bad:
            bad.draw_epoch(bs, 0, seed=1)   # nothing to draw: fine
            with pytest.raises(_lib.HipError, match="GMF: user 2 rates every item positively"):
                bad.draw_epoch(bs, nn, seed=1)
            with pytest.raises(_lib.HipError, match="GMF: user 2 rates every item positively"):
                bad.fit_epoch_sampled(bs, nn, 0.01)
        with pytest.raises(_lib.HipError, match="1 <= batch_size \\* \\(1 \\+ num_neg\\) <= 16384"):
            m.draw_epoch(4000, 4)
    n = counts.sum()
    assert n == 50 * 3 * nn and zero_drawn > 0, "the stored 0.0 can be drawn and is"
    admissible = np.array([j not in (0, 3) for j in range(NI)])
    assert not counts[~admissible].any()
    p = 1.0 / admissible.sum()
    sd = np.sqrt(n * p * (1 - p))
    print("user 1's negatives over 50 epochs: %s (expected %.1f each, standard deviation %.2f)" % (counts[admissible], n * p, sd))
    assert (np.abs(counts[admissible] - n * p) <= 5 * sd).all()


def test_fit_epoch_sampled_is_fit_epoch_on_the_drawn_samples():
    X = sampler_matrix()
    c = dict(SAMPLER, kind="NeuMF", f=3, layers=(8, 5, 3), act="tanh")
    params = {n: (np.random.RandomState(q).standard_normal(s) * 0.3).astype(np.float32)
              for q, (n, s) in enumerate(nc.shapes("NeuMF", NU, NI, 3, (8, 5, 3)).items())}
    out = []
    for sampled in (True, False):
        with handle(c, params, X=X) as m:
            for epoch in range(2):
                if sampled:
                    total, steps = m.fit_epoch_sampled(7, 4, 0.01, 0.001, "adam", seed=9, epoch=epoch)
                else:
                    total, steps = m.fit_epoch(*m.draw_epoch(7, 4, seed=9, epoch=epoch), 0.01, 0.001, "adam")
            out.append((m.get_params(), m.get_state(), steps, total))
    (Pa, (Sa, Ta, ta), la, tot_a), (Pb, (Sb, Tb, tb), lb, tot_b) = out
    assert ta == tb == 2 * -(-X.nnz // 7) and np.array_equal(la, lb) and tot_a == tot_b
    for n in Pa:
        assert np.array_equal(Pa[n].view(np.uint32), Pb[n].view(np.uint32)) and np.array_equal(Sa[n], Sb[n]) and np.array_equal(Ta[n], Tb[n])
    assert any(not np.array_equal(Pa[n], params[n]) for n in Pa)


# ---- end to end ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(nc.SEEDED))
def test_seeded_fit_end_to_end(golden, name, tmp_path):
    c = nc.SEEDED[name]
    m = nc.seeded_model(c).fit(nc.seeded_dataset(c))
    compare(golden, name, "P", m.params, {n: golden["%s/P/%s" % (name, n)].astype(np.float64) for n in nc.case_names(name)}, "d_ref", "max")
    users, (pu, pi) = nc.score_users(c), nc.score_pairs(c)
    S = m.score_batch(users)
    bound = 2 * 64 * 2.0 ** -24 * 8
    assert np.abs(S.astype(np.float64) - golden[name + "/scores"]).max() <= bound
    assert np.abs(np.array([m.score(int(u), int(i)) for u, i in zip(pu, pi)]) - golden[name + "/pair_scores"]).max() <= bound
    ranked, scores = m.rank(int(users[1]))
    assert np.array_equal(scores, S[1]) and sorted(ranked.tolist()) == list(range(c["ni"]))
    order = np.argsort(-S[1].astype(np.float64), kind="stable")
    if len(np.unique(S[1])) == c["ni"]:
        assert np.array_equal(ranked, order)
    back = CLASSES[c["kind"]].load(m.save(str(tmp_path)))
    assert np.array_equal(back.score_batch(users).view(np.uint32), S.view(np.uint32))
    again = nc.seeded_model(c).fit(nc.seeded_dataset(c))
    assert all(np.array_equal(again.params[n].view(np.uint32), m.params[n].view(np.uint32)) for n in m.params), "a seeded fit repeats itself"
    free = nc.seeded_model(c, seed=None, num_epochs=3).fit(nc.seeded_dataset(c))   # the device sampler
    assert all(np.isfinite(a).all() for a in free.params.values()) and free.loss_history[-1] < free.loss_history[0]
