"""LightGCN on the device, through the C ABI (`_lib.LightGcnModel`) and through cornac_amd.LightGCN, against (a) the float64
restatement of tests/lightgcn_cases.py and (b) what the reference's own Model, construct_graph and LightGCN.fit wrote into
tests/golden/lightgcn_ref.npz (tests/test_lightgcn_cpu.py holds (a) against (b)).

The two parameter tables and Adam's m and v of each are compared table by table with the tolerance
    max(16 * d_ref, 4 units in the last float32 place of max|table|),
d_ref = the reference's own float32 distance to the restatement, read from the golden; for the parameter tables that
tolerance stays under 1 % of the table's recorded movement (lightgcn_cases.check_condition); a row that the restatement leaves
exactly in place is compared bit for bit.  The three losses of every step are held to max(16 * d_ref_loss, 4 ulp).  Every
check prints the measured difference next to its tolerance."""
import functools

import numpy as np
import pytest

import lightgcn_cases as lc
from conftest import load_golden
from cornac_amd import LightGCN, _lib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden("lightgcn_ref")


@functools.lru_cache(maxsize=None)
def restated(name):
    """computed once per case, shared and left unchanged"""
    run = lc.run_case(name)
    for a in (run["r"].W, run["r"].M, run["r"].V, run["losses"]):
        a.setflags(write=False)
    return run


class handle:
    """a device model that is closed when the block ends"""

    def __init__(self, c, params=None):
        self.m = _lib.LightGcnModel(lc.case_graph(c), c["d"], c["L"])
        if params is not None:
            self.m.set_params(*params)

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


def run_device(name):
    """the case's steps in one fit_epoch: (params, state, losses [steps x 3], final embeddings)"""
    c = lc.CASES[name]
    with handle(c, lc.case_params(c)) as m:
        losses = np.stack(m.fit_epoch(*lc.epoch_arrays(lc.case_batches(c)), c["lr"], c["lam"]), axis=1)
        return m.get_params(), m.get_state(), losses, m.propagate()


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_steps_against_the_restatement(golden, name):
    c, run = lc.CASES[name], restated(name)
    r = run["r"]
    lc.check_condition(golden, name)
    params, state, losses, final = run_device(name)
    assert state[4] == r.t == len(c["steps"])
    worst = 0.0
    for q, n in enumerate(lc.TABLES):
        for what, got, want, stat, top in (("table", params[q], r.tables()[q], "d_ref", "max"), ("m", state[q], r.tables(r.M)[q], "d_ref_m", "max_m"),
                                           ("v", state[2 + q], r.tables(r.V)[q], "d_ref_v", "max_v")):
            tol = lc.tolerance(golden["%s/%s" % (name, stat)][q], golden["%s/%s" % (name, top)][q])
            d = np.abs(got.astype(np.float64) - want).max()
            worst = max(worst, d / tol)
            print("%s %s %s: %.3g (tolerance %.3g)" % (name, n, what, d, tol))
            assert got.dtype == np.float32 and d <= tol, (name, n, what, d, tol)
    for q, rows in enumerate(lc.still_rows(name)):   # no gradient ever reaches these rows: bit for bit in place
        assert np.array_equal(params[q][rows].view(np.uint32), run["init"][q][rows].view(np.uint32)), (name, lc.TABLES[q])
        assert not state[q][rows].any() and not state[2 + q][rows].any()
    ltol = lc.loss_tolerance(golden, name, np.abs(run["losses"]).max())
    dl = np.abs(losses - run["losses"]).max()
    print("%s losses: %.3g (tolerance %.3g); worst table share %.3g" % (name, dl, ltol, worst))
    assert dl <= ltol
    if name in lc.FULL_CASES:   # the final embeddings against the restatement's over the device's own float32 tables
        f32 = lc.new_restatement(c, params)
        mine, reach = f32.final(), f32.tables(f32.P(np.abs(f32.W)))
        # a float32 sum of n terms is off by at most n 2^-24 times the sum of their magnitudes: per hop a row's edges and the
        # running sum, then the division; the magnitudes are bounded entry by entry by P(|E0|)
        gamma = (c["L"] * (int(np.diff(f32.A.indptr).max()) + 1) + 2) * 2.0 ** -24
        for q, n in enumerate(lc.TABLES):
            d = np.abs(final[q].astype(np.float64) - mine[q])
            bound = gamma * reach[q] + 2.0 ** -149
            print("%s E %s: %.3g, at most %.3g of the summation bound" % (name, n, d.max(), (d / bound).max()))
            assert final[q].dtype == np.float32 and (d <= bound).all()


@pytest.mark.parametrize("name", lc.REPEAT_CASES)
def test_two_runs_give_the_same_bits(name):
    a, b = run_device(name), run_device(name)
    for x, y in zip(a[0] + a[1][:4] + a[3], b[0] + b[1][:4] + b[3]):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert np.array_equal(a[2], b[2])


def test_reset_optimizer_then_the_same_epoch_equals_a_fresh_handle():
    c = lc.CASES["d33"]
    init, epoch = lc.case_params(c), lc.epoch_arrays(lc.case_batches(c))
    with handle(c, init) as m:
        first = m.fit_epoch(*epoch, c["lr"], c["lam"])
        fresh = m.get_params(), m.get_state()
        m.reset_optimizer()
        assert m.get_state()[4] == 0 and not any(a.any() for a in m.get_state()[:4])
        m.set_params(*init)
        again = m.fit_epoch(*epoch, c["lr"], c["lam"])
        assert all(np.array_equal(x, y) for x, y in zip(first, again))
        for x, y in zip(fresh[0] + fresh[1][:4], m.get_params() + m.get_state()[:4]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        assert m.get_state()[4] == len(c["steps"])


def test_propagate_with_no_layers_and_no_edges():
    import scipy.sparse as sp

    c = lc.CASES["l0"]
    init = lc.case_params(c)
    with handle(c, init) as m:
        assert all(np.array_equal(a, b) for a, b in zip(m.propagate(), init)), "L = 0: the final embeddings are the tables"
    m = _lib.LightGcnModel(sp.csr_matrix((5, 7)), 8, 3)
    try:
        rs = np.random.RandomState(0)
        user, item = rs.rand(5, 8).astype(np.float32), rs.rand(7, 8).astype(np.float32)
        m.set_params(user, item)
        U, V = m.propagate()   # every node isolated: (E0 + 0 + 0 + 0) / 4
        assert np.array_equal(U, user / np.float32(4)) and np.array_equal(V, item / np.float32(4))
    finally:
        m.close()


def test_seeded_fit_end_to_end(golden):
    c = lc.SEEDED["seeded"]
    m = lc.seeded_model(c).fit(lc.seeded_dataset(c))
    for q, (mine, n) in enumerate(((m.U, "U"), (m.V, "V"))):
        tol = lc.tolerance(golden["seeded/d_ref"][q], golden["seeded/max"][q])
        d = np.abs(mine.astype(np.float64) - golden["seeded/" + n]).max()
        d_ref = float(golden["seeded/d_ref"][q])
        print("seeded %s: %.3g from the reference's seeded fit (tolerance %.3g + d_ref %.3g, movement %.3g)" % (n, d, tol, d_ref, golden["seeded/move"][q]))
        assert d <= tol + d_ref, "the device within its tolerance of the restatement, which lies d_ref from the reference"
    assert len(m.loss_history) == c["epochs"] and m.loss_history[-1] < m.loss_history[0]
    users = lc.score_users(c)
    got = np.array([m.score(int(u)) for u in users], np.float64)
    assert np.abs(got - golden["seeded/scores"]).max() <= 64 * 2.0 ** -24
    again = lc.seeded_model(c).fit(lc.seeded_dataset(c))
    assert np.array_equal(again.U.view(np.uint32), m.U.view(np.uint32)) and np.array_equal(again.V.view(np.uint32), m.V.view(np.uint32))


def test_rank_batch_is_the_sort_of_score_batch():
    """over the RANK_CASE's fitted tables, whose top scores are distinct (tests/test_lightgcn_cpu.py)"""
    c = lc.CASES[lc.RANK_CASE]
    params, _, _, final = run_device(lc.RANK_CASE)
    m = LightGCN(emb_size=c["d"], num_layers=c["L"])
    m.num_users, m.num_items = lc.totals(c)
    m.U, m.V = final
    users = np.arange(c["nu"])
    items, scores = m.rank_batch(users, k=10)
    for r, u in enumerate(users):
        s = m.score(int(u))
        order = np.lexsort((np.arange(len(s)), s))[::-1][:10]
        assert np.array_equal(items[r], order) and np.array_equal(scores[r], s[order])


def test_refusals_on_the_device():
    c = lc.CASES["d8"]
    with handle(c, lc.case_params(c)) as m:
        ptr = np.array([0, 2], np.int64)
        for users, pos, neg, text in (([0, 99], [0, 0], [0, 0], "user 99 out of range"), ([0, 1], [0, 77], [0, 0], "positive item 77 out of range"),
                                      ([0, 1], [0, 0], [-1, 0], "negative item -1 out of range")):
            with pytest.raises(_lib.HipError, match="lightgcn: " + text):
                m.fit_epoch(ptr, users, pos, neg, 0.1, 0.0)
        assert m.get_state()[4] == 0
