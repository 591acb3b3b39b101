"""GPU parity tests of the VBPR minibatch path (cornac_hip_vbpr_*)."""
import numpy as np
import pytest

from cornac_amd import VBPR, _lib
from test_oracle_golden import _vbpr_case

pytestmark = pytest.mark.gpu


def test_vbpr_matches_torch_oracle_and_reference_golden():
    """same batches (mirrored sampler), analytic gradients + dense Adam on the device vs torch autograd +
    torch.optim.Adam: every learned table within 1e-4 of the oracle and of the real reference's golden."""
    from oracle.vbpr_oracle import VBPROracle

    fx, ds, kw = _vbpr_case()
    m = VBPR(verbose=False, **kw).fit(ds)
    o = VBPROracle(**kw).fit(ds)
    for name, key in (("beta_item", "Bi"), ("gamma_user", "Gu"), ("gamma_item", "Gi"), ("theta_user", "Tu"),
                      ("emb_matrix", "E"), ("beta_prime", "Bp"), ("theta_item", "theta_item"),
                      ("visual_bias", "visual_bias")):
        a = np.asarray(getattr(m, name), np.float64).reshape(np.asarray(getattr(o, name)).shape)
        assert np.abs(a - getattr(o, name)).max() <= 1e-4, (name, np.abs(a - getattr(o, name)).max())
        assert np.abs(a - fx[key].reshape(a.shape)).max() <= 1e-4, name
    assert np.abs(m.score(0) - fx["score0"]).max() < 1e-4
    ranked, _ = m.rank(0, k=5)
    assert len(ranked) == ds.num_items and np.all(np.diff(m.score(0)[ranked[:5]]) <= 0)
    assert m.loss_history[-1] < m.loss_history[0]


def test_vbpr_single_step_gradients_against_autograd():
    """one Adam step from random parameters on a batch with duplicate users/items: after step 1 Adam moves
    every parameter with a non-zero gradient by ~lr * sign(grad), so comparing the updated tables checks the
    analytic gradient's support and sign everywhere, and its value through the second step."""
    import torch

    rs = np.random.RandomState(0)
    nu, ni, k, k2, nf, B = 12, 9, 4, 3, 20, 16
    F = rs.uniform(0, 1, (ni, nf)).astype(np.float32)
    P = {"Bi": rs.normal(0, .1, ni), "Gu": rs.normal(0, .3, (nu, k)), "Gi": rs.normal(0, .3, (ni, k)),
         "Tu": rs.normal(0, .3, (nu, k2)), "E": rs.normal(0, .3, (nf, k2)), "Bp": rs.normal(0, .3, nf)}
    P = {n: v.astype(np.float32) for n, v in P.items()}
    u = rs.randint(0, 5, B).astype(np.int32)  # duplicates on purpose
    i = rs.randint(0, ni, B).astype(np.int32)
    j = ((i + 1 + rs.randint(0, ni - 1, B)) % ni).astype(np.int32)
    lr, lw, lb, le = 0.01, 0.02, 0.03, 0.004
    tr = _lib.VbprTrainer(F, nu, ni, k, k2)
    tr.set_params(**P)
    tr.fit_batches(u, i, j, B, lr, lw, lb, le)
    tr.fit_batches(u, i, j, B, lr, lw, lb, le)
    got = tr.get_params()
    tr.close()
    T = {n: torch.tensor(v if n != "Bp" else v.reshape(-1, 1), requires_grad=True) for n, v in P.items()}
    opt = torch.optim.Adam([T[n] for n in ("Bi", "Gu", "Gi", "Tu", "E", "Bp")], lr=lr)
    Ft = torch.tensor(F)
    ul, il, jl = (torch.tensor(x, dtype=torch.long) for x in (u, i, j))
    for _ in range(2):
        gu, tu = T["Gu"][ul], T["Tu"][ul]
        bi_, bj_ = T["Bi"][il], T["Bi"][jl]
        gi, gj = T["Gi"][il], T["Gi"][jl]
        fd = Ft[il] - Ft[jl]
        # [B] + [B, 1] broadcasts to B x B exactly like the reference's Xuij (recom_vbpr.py:242-248)
        X = bi_ - bj_ + (gu * (gi - gj)).sum(1) + (tu * fd.mm(T["E"])).sum(1) + fd.mm(T["Bp"])
        l2 = lambda *ts: sum(t.pow(2).sum() for t in ts) / 2  # noqa: E731
        loss = (-torch.nn.functional.logsigmoid(X).sum() + l2(gu, gi, gj, tu) * lw + l2(bi_) * lb + l2(bj_) * lb / 10
                + l2(T["E"], T["Bp"]) * le)
        opt.zero_grad()
        loss.backward()
        opt.step()
    for n in got:
        want = T[n].detach().numpy().reshape(got[n].shape)
        assert np.abs(got[n] - want).max() < 2e-5, (n, np.abs(got[n] - want).max())


def test_vbpr_errors():
    from cornac_amd.recommender import CornacException
    from conftest import synth_dataset

    with pytest.raises(CornacException):
        VBPR(verbose=False).fit(synth_dataset(20, 15, 100, seed=1))


# --- the device step against the float64 reference (oracle/vbpr_oracle.py:steps_f64) at its shape and schedule edges.
# The cases and the float32 drift the tolerance rests on are pinned on the CPU in tests/test_vbpr_cpu.py.

def _trainer(c):
    nu, ni, nf, k, k2 = c["dims"]
    tr = _lib.VbprTrainer(c["F"], nu, ni, k, k2)
    tr.set_params(**c["P"])
    return tr


def _check_tables(got, want, c, batches):
    """every table within DEVICE_TOL of the float64 steps, moved by at least 1e-3, and its never-touched rows
    bit-identical to their start"""
    from test_vbpr_cpu import DEVICE_TOL, TABLES

    for n in TABLES:
        g, w = got[n].astype(np.float64).reshape(-1), want[n].reshape(-1)
        err = np.abs(g - w).max()
        assert err <= DEVICE_TOL, (n, err, int(np.abs(g - w).argmax()))
        assert np.abs(w - np.asarray(c["P"][n], np.float64).reshape(-1)).max() >= 1e-3, n
    nu, ni = c["dims"][:2]
    users = np.setdiff1d(np.arange(nu), np.concatenate([b[0] for b in batches]))
    items = np.setdiff1d(np.arange(ni), np.concatenate([np.concatenate([b[1], b[2]]) for b in batches]))
    for n, rows in (("Gu", users), ("Tu", users), ("Gi", items), ("Bi", items)):
        assert np.array_equal(got[n][rows], np.asarray(c["P"][n], np.float32)[rows]), n
    return users, items


def _check_item_tables(tr, got, F):
    """theta_item = F E and visual_bias = F beta' from the E / beta' the device returned, in float64: only the item-table
    kernel's own rounding is measured (bound 1e-5 * sum_f |F_if| |E_fc|)"""
    theta, vb = tr.item_tables()
    F64 = F.astype(np.float64)
    for table, got_t in (("E", theta), ("Bp", vb)):
        W = got[table].astype(np.float64).reshape(F.shape[1], -1)
        want, bound = F64 @ W, np.abs(F64) @ np.abs(W)
        err = np.abs(got_t.astype(np.float64).reshape(want.shape) - want)
        assert np.all(err <= 1e-5 * bound), (table, float((err / bound).max()))


@pytest.mark.parametrize("name", ["b1_k1", "k2_129", "k65_k2_127", "k12_k2_255", "k2_256_b61", "b513", "sparse_50k",
                                  "nfeat_20k"])
def test_vbpr_shape_matrix_against_float64_steps(name):
    """one call per shape case of tests/test_vbpr_cpu.py:SHAPES (lr 0.01, lambda_e > 0, ragged last batch where the
    pair count says so, >= 9 steps: the four stamp sets wrap twice): every table within 2e-5 of the float64 steps, the
    call's NLL within rtol 1e-5 of the reference's sum, and the item tables of the learned E / beta'"""
    from oracle.vbpr_oracle import steps_f64
    from test_vbpr_cpu import LB, LE, LR, LW, shape_case

    c = shape_case(name)
    assert len(c["batches"]) >= 9
    want, want_nll = steps_f64(c["F"], c["P"], c["batches"], LR, LW, LB, LE)
    tr = _trainer(c)
    try:
        nll = tr.fit_batches(c["u"], c["i"], c["j"], c["batch_size"], LR, LW, LB, LE)
        got = tr.get_params()
        _check_tables(got, want, c, c["batches"])
        assert nll == pytest.approx(sum(want_nll), rel=1e-5)
        _check_item_tables(tr, got, c["F"])
    finally:
        tr.close()


def test_vbpr_row_schedule_against_float64_steps():
    """the hand-written schedule (tests/test_vbpr_cpu.py:SCHEDULE): rows in every batch, at gaps of 1-4 steps (stamp set
    s & 3 is re-used every fourth step), only in the first batch, i at t and j at t + 1, three times in one batch, an
    i == j triplet, a ragged last batch and never-touched rows — all within 2e-5 of the float64 steps, the untouched
    rows bit-identical"""
    from oracle.vbpr_oracle import steps_f64
    from test_vbpr_cpu import LB, LE, LR, LW, schedule_case, schedule_classes

    c = schedule_case()
    classes = schedule_classes(c["batches"], *c["dims"][:2])
    assert classes["gaps 1-4"] == [1, 2, 3, 4] and all(classes.values()), classes
    want, want_nll = steps_f64(c["F"], c["P"], c["batches"], LR, LW, LB, LE)
    tr = _trainer(c)
    try:
        nll = tr.fit_batches(c["u"], c["i"], c["j"], c["batch_size"], LR, LW, LB, LE)
        got = tr.get_params()
    finally:
        tr.close()
    users, items = _check_tables(got, want, c, c["batches"])
    assert len(users) and len(items)
    assert nll == pytest.approx(sum(want_nll), rel=1e-5)


def test_vbpr_call_boundaries_continue_one_adam_sequence():
    """on one handle: 5 batches, an empty call, a call shorter than one batch, a call rejected for an out-of-range id,
    4 batches at a larger batch_size (DF, proj and W grow) == ONE float64 run over the good calls' batches; the empty and
    the rejected call leave no trace (no Adam step counted), and each call's NLL is the reference's sum over its steps"""
    from oracle.vbpr_oracle import steps_f64
    from test_vbpr_cpu import LB, LE, LR, LW, random_params, split

    rs = np.random.RandomState(21)
    nu, ni, nf, k, k2 = 40, 30, 300, 8, 20
    c = dict(F=rs.uniform(0, 1, (ni, nf)).astype(np.float32), P=random_params(nu, ni, nf, k, k2, rs),
             dims=(nu, ni, nf, k, k2))

    def draw(n):
        u, i = rs.randint(0, nu, n).astype(np.int32), rs.randint(0, ni, n).astype(np.int32)
        return u, i, ((i + 1 + rs.randint(0, ni - 1, n)) % ni).astype(np.int32)

    calls = [(draw(5 * 8), 8), (draw(0), 8), (draw(3), 8), (draw(4 * 20), 20)]
    batches = [b for (u, i, j), bs in calls for b in split(u, i, j, bs)]
    assert [len(b[0]) for b in batches] == [8] * 5 + [3] + [20] * 4
    want, want_nll = steps_f64(c["F"], c["P"], batches, LR, LW, LB, LE)
    per_call = [sum(want_nll[:5]), 0.0, want_nll[5], sum(want_nll[6:])]
    tr = _trainer(c)
    try:
        got_nll = []
        for q, ((u, i, j), bs) in enumerate(calls):
            if q == 3:  # the rejected call, between two good ones
                bad_u, bad_i, bad_j = draw(16)
                bad_j[9] = ni
                with pytest.raises(_lib.HipError):
                    tr.fit_batches(bad_u, bad_i, bad_j, 8, LR, LW, LB, LE)
            got_nll.append(tr.fit_batches(u, i, j, bs, LR, LW, LB, LE))
        got = tr.get_params()
    finally:
        tr.close()
    _check_tables(got, want, c, batches)
    assert got_nll[1] == 0.0
    for g, w in zip(got_nll, per_call):
        assert g == pytest.approx(w, rel=1e-5)


def test_vbpr_model_ragged_epochs_match_the_oracle():
    """VBPR(k=7, k2=150, batch_size=33) on 500 pairs (every epoch ends with a ragged batch of 5) vs VBPROracle on the
    same sampler: every learned table within 1e-4; score(u) is beta + visual_bias + <gamma_u, gamma_i> + <theta_u,
    theta_item_i> of the model's own tables"""
    from conftest import synth_dataset
    from cornac_amd.data import ImageFeatures
    from oracle.vbpr_oracle import VBPROracle

    ds = synth_dataset(60, 45, 500, seed=4)
    assert len(ds.uir_tuple[0]) % 33 != 0
    ds.item_image = ImageFeatures(np.random.RandomState(8).uniform(0, 1, (ds.num_items, 37)).astype(np.float32))
    kw = dict(k=7, k2=150, batch_size=33, n_epochs=3, learning_rate=0.01, lambda_e=1e-3, seed=6)
    m = VBPR(verbose=False, **kw).fit(ds)
    o = VBPROracle(**kw).fit(ds)
    for name in ("beta_item", "gamma_user", "gamma_item", "theta_user", "emb_matrix", "beta_prime", "theta_item",
                 "visual_bias"):
        want = np.asarray(getattr(o, name), np.float64)
        err = np.abs(np.asarray(getattr(m, name), np.float64).reshape(want.shape) - want).max()
        assert err <= 1e-4, (name, err)
    B, VB = np.asarray(m.beta_item, np.float64), np.asarray(m.visual_bias, np.float64)
    Gu, Gi = np.asarray(m.gamma_user, np.float64), np.asarray(m.gamma_item, np.float64)
    Tu, Ti = np.asarray(m.theta_user, np.float64), np.asarray(m.theta_item, np.float64)
    for u in (0, 17, 59):
        want = B + VB + Gi @ Gu[u] + Ti @ Tu[u]
        bound = np.abs(B) + np.abs(VB) + np.abs(Gi) @ np.abs(Gu[u]) + np.abs(Ti) @ np.abs(Tu[u])
        assert np.all(np.abs(m.score(u).astype(np.float64) - want) <= 1e-5 * bound + 1e-7), u


def test_vbpr_rejections():
    """k2 = 257 and n_feat one over the LDS staging bound at create, batch 62 at k2 = 256 (61 passes in the shape
    matrix) and an out-of-range id (also inside the call-boundary test) raise instead of launching"""
    F = np.zeros((2, 8), np.float32)
    with pytest.raises(_lib.HipError):
        _lib.VbprTrainer(F, 3, 2, 4, 257)
    k2 = 10
    n_feat = (160 * 1024) // 4 - 256 - k2 + 1  # (n_feat + 256 + k2) * 4 B > 160 KB
    with pytest.raises(_lib.HipError):
        _lib.VbprTrainer(np.zeros((1, n_feat), np.float32), 3, 1, 4, k2)
    # the bound itself is accepted, and its item tables (n_feat + 256 floats of LDS per workgroup) launch
    rs = np.random.RandomState(0)
    F = rs.uniform(0, 1, (2, n_feat - 1)).astype(np.float32)
    tr = _lib.VbprTrainer(F, 3, 2, 4, k2)
    try:
        tr.set_params(E=rs.normal(0, 0.01, (n_feat - 1, k2)), Bp=rs.normal(0, 0.01, n_feat - 1))
        _check_item_tables(tr, tr.get_params(), F)
    finally:
        tr.close()
    tr = _lib.VbprTrainer(np.random.RandomState(0).uniform(0, 1, (5, 16)).astype(np.float32), 4, 5, 4, 256)
    try:
        u, i, j = np.zeros(62, np.int32), np.zeros(62, np.int32), np.ones(62, np.int32)
        with pytest.raises(_lib.HipError):
            tr.fit_batches(u, i, j, 62, 0.01, 0.01, 0.01, 0.0)
        for bad in (-1, 5):
            with pytest.raises(_lib.HipError):
                tr.fit_batches(u[:4], i[:4], np.full(4, bad, np.int32), 4, 0.01, 0.01, 0.01, 0.0)
    finally:
        tr.close()
