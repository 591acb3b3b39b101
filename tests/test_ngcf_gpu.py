"""NGCF on the device, through the C ABI (`_lib.NgcfModel`) and through cornac_amd.NGCF, against (a) the float64 restatement of
tests/ngcf_cases.py and (b) what the reference's own Model, construct_graph and NGCF.fit wrote into tests/golden/ngcf_ref.npz
(tests/test_ngcf_cpu.py holds (a) against (b)).

Every parameter (the two tables, every W and b) and Adam's m and v of each are compared one by one with the tolerance
    max(16 * d_ref, 4 units in the last float32 place of max|table|),
d_ref = the reference's own float32 distance to the restatement, read from the golden; for every parameter that tolerance stays
under 1 % of its recorded movement (ngcf_cases.check_condition; only a one-column layer's parameters are left out, by name).  The three losses of every step are held to
max(16 * d_ref_loss, 4 ulp).  Every check prints the measured difference next to its tolerance.  The restatement applies the
numpy restatement of the device's dropout mask, so a case with dropout passes only if the two masks are equal.

Among the two tables the largest share of the tolerance is `big`'s user table, 6.1e-6 against a tolerance of 1.5e-5, and it is one entry of 19 200: entry (218, 31),
whose first gradient is 3.8e-9 in the restatement, the smallest of the table (median 1.7e-4) and below Adam's eps = 1e-8.  The
first update lr g / (|g| + eps) then multiplies an error of g by lr eps / (|g| + eps)^2 = 5.3e4, so 1.2e-10 of float32 rounding
in a gradient whose summands are about 1e-4 shows as 6e-6; 99.9 % of the table's entries are within 1.9e-8.  The reference's
own distance there depends on its summation order, which is why the golden's generator runs torch on one thread."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import ngcf_cases as nc
from conftest import load_golden
from cornac_amd import NGCF, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("ngcf_ref")


@functools.lru_cache(maxsize=None)
def restated(name):
    """computed once per case, shared and left unchanged"""
    run = nc.run_case(name)
    for a in list(run["r"].W.values()) + list(run["r"].M.values()) + list(run["r"].V.values()) + [run["losses"]]:
        a.setflags(write=False)
    return run


class handle:
    """a device model that is closed when the block ends"""

    def __init__(self, c, params=None):
        self.m = _lib.NgcfModel(nc.case_graph(c), c["emb"], c["layers"], c["drop"], dropout_key=nc.KEY)
        if params is not None:
            self.m.set_params(params)

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


@functools.lru_cache(maxsize=None)
def run_device(name):
    """the case's steps in one fit_epoch: (params, (m, v, t), losses [steps x 3], (U, V))"""
    c = nc.CASES[name]
    with handle(c, nc.case_params(c)) as m:
        losses = np.stack(m.fit_epoch(*nc.epoch_arrays(nc.case_batches(c)), c["lr"], c["lam"]), axis=1)
        return m.get_params(), m.get_state(), losses, m.propagate()


def bits(run):
    return list(run[0].values()) + list(run[1][0].values()) + list(run[1][1].values()) + list(run[3])


@pytest.mark.parametrize("name", sorted(nc.CASES))
def test_steps_against_the_restatement(golden, name):
    c, run = nc.CASES[name], restated(name)
    r = run["r"]
    params, (m, v, t), losses, final = run_device(name)
    assert t == r.t == len(c["steps"]) and list(params) == list(r.W)
    worst, failed = 0.0, []
    for q, n in enumerate(r.W):
        for what, got, want, stat, top in (("table", params[n], r.W[n], "d_ref", "max"), ("m", m[n], r.M[n], "d_ref_m", "max_m"),
                                           ("v", v[n], r.V[n], "d_ref_v", "max_v")):
            tol = nc.tolerance(golden["%s/%s" % (name, stat)][q], golden["%s/%s" % (name, top)][q])
            d = np.abs(got.astype(np.float64) - want).max()
            worst = max(worst, d / tol)
            print("%s %s %s: %.3g (tolerance %.3g)" % (name, n, what, d, tol))
            assert got.dtype == np.float32 and np.isfinite(got).all()
            if not d <= tol:
                failed.append((n, what, d, tol))
    ltol = nc.loss_tolerance(golden, name, np.abs(run["losses"]).max())
    dl = np.abs(losses - run["losses"]).max()
    print("%s losses: %.3g (tolerance %.3g); worst table share %.3g" % (name, dl, ltol, worst))
    assert not failed, failed
    assert dl <= ltol
    if name in nc.FULL_CASES:   # the eval-mode embeddings against the restatement's over the device's own float32 parameters
        f32 = {n: a.astype(np.float64) for n, a in params.items()}
        mine = np.concatenate(r.final(f32))
        # ngcf_cases.embedding_bound: a running forward error analysis in u = 2^-24, from the row length (the hop's sum), the
        # widths (the GEMM's and the norm's sums) and the depth (each layer's error enters the next)
        bound = nc.embedding_bound(r, f32) + 2.0 ** -149
        d = np.abs(np.concatenate(final).astype(np.float64) - mine)
        print("%s E: %.3g, at most %.3g of the summation bound (largest bound %.3g)" % (name, d.max(), (d / bound).max(), bound.max()))
        assert final[0].dtype == np.float32 and (d <= bound).all()
    print("%s: share of the tables' movement %.3g" % (name, nc.check_condition(golden, name)))


@pytest.mark.parametrize("name", nc.REPEAT_CASES)
def test_two_runs_give_the_same_bits(name):
    a = run_device(name)
    b = run_device.__wrapped__(name)
    for x, y in zip(bits(a), bits(b)):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a[2], b[2])


def test_reset_optimizer_then_the_same_epoch_equals_a_fresh_handle():
    c = nc.CASES["mixed"]
    init, epoch = nc.case_params(c), nc.epoch_arrays(nc.case_batches(c))
    with handle(c, init) as m:
        first = m.fit_epoch(*epoch, c["lr"], c["lam"])
        fresh = list(m.get_params().values()) + list(m.get_state()[0].values()) + list(m.get_state()[1].values())
        m.reset_optimizer()
        sm, sv, t = m.get_state()
        assert t == 0 and not any(a.any() for a in list(sm.values()) + list(sv.values()))
        m.set_params(init)
        again = m.fit_epoch(*epoch, c["lr"], c["lam"])   # the same Adam steps 1, 2, 3: the same dropout masks
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        now = list(m.get_params().values()) + list(m.get_state()[0].values()) + list(m.get_state()[1].values())
        for x, y in zip(fresh, now):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert m.get_state()[2] == len(c["steps"])


def test_propagate_on_a_graph_with_no_edges():
    """s = 0 and c = 0: layer by layer normalize(leaky_relu(X W1^T + b1)); eval mode, so the rates do not matter"""
    rs = np.random.RandomState(0)
    m = _lib.NgcfModel(sp.csr_matrix((5, 7)), 8, [130, 3], [0.5, 0.5], dropout_key=1)
    try:
        params = {n: rs.uniform(-0.5, 0.5, s).astype(np.float32) for n, s in m.shapes.items()}
        m.set_params(params)
        U, V = m.propagate()
        X = np.concatenate([params["feature_dict.user"], params["feature_dict.item"]]).astype(np.float64)
        parts = [X]
        for l in range(2):
            z = X @ params["layers.%d.W1.weight" % l].astype(np.float64).T + params["layers.%d.W1.bias" % l]
            a = np.where(z > 0, z, 0.2 * z)
            X = a / np.maximum(np.sqrt((a * a).sum(axis=1, keepdims=True)), 1e-12)
            parts.append(X)
        want = np.concatenate(parts, axis=1)
        d = np.abs(np.concatenate([U, V]).astype(np.float64) - want).max()
        # rows of unit norm; a float32 dot product of at most 131 terms and a norm of at most 130, two layers deep
        print("no edges: %.3g (bound %.3g)" % (d, 4 * 140 * 2.0 ** -24))
        assert U.shape == (5, 141) and V.shape == (7, 141) and d <= 4 * 140 * 2.0 ** -24
    finally:
        m.close()


def test_seeded_fit_end_to_end(golden):
    c = nc.SEEDED["seeded"]
    m = nc.seeded_model(c).fit(nc.seeded_dataset(c))
    for q, (mine, n) in enumerate(((m.U, "U"), (m.V, "V"))):
        tol = nc.tolerance(golden["seeded/d_ref"][q], golden["seeded/max"][q])
        d = np.abs(mine.astype(np.float64) - golden["seeded/" + n]).max()
        d_ref = float(golden["seeded/d_ref"][q])
        print("seeded %s: %.3g from the reference's seeded fit (tolerance %.3g + d_ref %.3g, movement %.3g)" % (n, d, tol, d_ref, golden["seeded/move"][q]))
        assert d <= tol + d_ref, "the device within its tolerance of the restatement, which lies d_ref from the reference"
    assert len(m.loss_history) == c["epochs"] and m.loss_history[-1] < m.loss_history[0]
    users = nc.score_users(c)
    got = np.array([m.score(int(u)) for u in users], np.float64)
    D = c["emb"] + sum(c["layers"])
    assert np.abs(got - golden["seeded/scores"]).max() <= 64 * 2.0 ** -24 * D
    again = nc.seeded_model(c).fit(nc.seeded_dataset(c))
    assert np.array_equal(again.U.view(np.uint32), m.U.view(np.uint32)) and np.array_equal(again.V.view(np.uint32), m.V.view(np.uint32))


def test_seeded_fit_at_the_default_dropout_repeats_and_learns():
    c = nc.SEEDED["seeded"]
    kw = dict(layer_sizes=[6, 6, 6], dropout_rates=[0.1, 0.1, 0.1], num_epochs=4)
    a, b = (nc.seeded_model(c, **kw).fit(nc.seeded_dataset(c)) for _ in range(2))
    assert np.array_equal(a.U.view(np.uint32), b.U.view(np.uint32)) and np.array_equal(a.V.view(np.uint32), b.V.view(np.uint32))
    assert all(np.array_equal(a.params[n].view(np.uint32), b.params[n].view(np.uint32)) for n in a.params)
    assert np.isfinite(a.loss_history).all() and a.loss_history[-1] < a.loss_history[0], a.loss_history
    other = nc.seeded_model(c, seed=c["seed"] + 1, **kw).fit(nc.seeded_dataset(c))
    assert not np.array_equal(other.U, a.U)


def test_rank_batch_is_the_sort_of_score():
    """over the RANK_CASE's fitted embeddings, whose top scores are distinct (tests/test_ngcf_cpu.py)"""
    c = nc.CASES[nc.RANK_CASE]
    final = run_device(nc.RANK_CASE)[3]
    m = NGCF(emb_size=c["emb"], layer_sizes=list(c["layers"]), dropout_rates=list(c["drop"]))
    m.num_users, m.num_items = nc.totals(c)
    m.U, m.V = final
    users = np.arange(c["nu"])
    items, scores = m.rank_batch(users, k=10)
    for r, u in enumerate(users):
        s = m.score(int(u))
        order = np.lexsort((np.arange(len(s)), s))[::-1][:10]
        assert np.array_equal(items[r], order) and np.array_equal(scores[r], s[order])


def test_refusals_on_the_device():
    c = nc.CASES["mixed"]
    with handle(c, nc.case_params(c)) as m:
        ptr = np.array([0, 2], np.int64)
        for users, pos, neg, text in (([0, 99], [0, 0], [0, 0], "user 99 out of range"), ([0, 1], [0, 77], [0, 0], "positive item 77 out of range"),
                                      ([0, 1], [0, 0], [-1, 0], "negative item -1 out of range")):
            with pytest.raises(_lib.HipError, match="ngcf: " + text):
                m.fit_epoch(ptr, users, pos, neg, 0.1, 0.0)
        assert m.get_state()[2] == 0
    X = nc.case_graph(c)
    for kw, text in ((dict(dropout_rates=[1.0]), "ngcf: dropout rate 0 = 1 .* 0 <= p < 1"),
                     (dict(layer_sizes=[257]), "ngcf: layer size 0 = 257 .* 1 <= size <= 256"),
                     (dict(emb_size=257), "ngcf: emb_size = 257 .* 1 <= emb_size <= 256"),
                     (dict(layer_sizes=[], dropout_rates=[]), "ngcf: num_layers = 0 .* 1 <= num_layers <= 8")):
        args = dict(dict(emb_size=8, layer_sizes=[8], dropout_rates=[0.0]), **kw)
        with pytest.raises(_lib.HipError, match=text):
            _lib.NgcfModel(X, **args)
