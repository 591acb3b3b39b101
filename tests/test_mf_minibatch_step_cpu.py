"""The minibatch MF step checks' own ground (tests/mf_minibatch_cases.py), without a device: the oracle's float64 mode leaves
its float32 default as it was, the two torch runs meet the tolerance rule's condition on every case and table, and the case
table has the properties that tests/test_mf_minibatch_step_gpu.py relies on."""
import numpy as np
import pytest

import mf_minibatch_cases as mc
from oracle import mf_minibatch_oracle


def _fit_before(U, V, Bu, Bi, mu, rid, cid, val, batches, optimizer="sgd", lr=0.01, reg=0.02, use_bias=True, keep=None,
                keep_scale=1.0):
    """oracle/mf_minibatch_oracle.fit as it stood before it learnt `dtype` and `return_state`, kept to compare bits with"""
    import torch

    make = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "rmsprop": torch.optim.RMSprop,
            "adagrad": torch.optim.Adagrad}[optimizer]
    P = [torch.tensor(np.array(U, np.float32), requires_grad=True), torch.tensor(np.array(V, np.float32), requires_grad=True)]
    if use_bias:
        P += [torch.tensor(np.array(Bu, np.float32).reshape(-1, 1), requires_grad=True),
              torch.tensor(np.array(Bi, np.float32).reshape(-1, 1), requires_grad=True)]
    opt = make(P, lr=lr, weight_decay=reg)
    rid_t, cid_t = torch.as_tensor(np.asarray(rid, np.int64)), torch.as_tensor(np.asarray(cid, np.int64))
    val_t = torch.as_tensor(np.asarray(val, np.float32))
    losses = []
    for b, ids in enumerate(batches):
        ids = torch.as_tensor(np.asarray(ids, np.int64))
        u, i, r = rid_t[ids], cid_t[ids], val_t[ids]
        ue, ie = P[0][u], P[1][i]
        if keep is not None:
            ue = ue * (torch.as_tensor(np.asarray(keep[b][0], np.float32)) * float(keep_scale))
            ie = ie * (torch.as_tensor(np.asarray(keep[b][1], np.float32)) * float(keep_scale))
        pred = (ue * ie).sum(dim=1, keepdim=True)
        if use_bias:
            pred = pred + P[2][u] + P[3][i] + float(mu)
        loss = ((pred.squeeze(1) - r) ** 2).sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    out = [p.detach().numpy() for p in P]
    if not use_bias:
        out += [np.array(Bu, np.float32), np.array(Bi, np.float32)]
    return out[0], out[1], out[2].reshape(-1), out[3].reshape(-1), losses


SMALL = [n for n in sorted(mc.CASES) if mc.CASES[n]["n"] <= 400 and mc.CASES[n]["nu"] <= 40]


@pytest.mark.parametrize("name", [n for n in SMALL if n.startswith(("k17/", "k33/", "seg185/", "drop/k", "drop/p1"))])
def test_default_dtype_is_the_oracle_as_it_was(name):
    c, d = mc.CASES[name], mc.inputs(name)
    args = ([d[t] for t in mc.TABLES] + [mc.MU, d["rid"], d["cid"], d["val"], d["batches"], c["opt"], c["lr"], c["reg"], c["use_bias"]])
    kw = dict(keep=d["keep"], keep_scale=d["keep_scale"])
    want = _fit_before(*args, **kw)
    for got in (mf_minibatch_oracle.fit(*args, **kw), mf_minibatch_oracle.fit(*args, dtype=np.float32, return_state=True, **kw)[:5],
                mc.reference(name, "float32")):
        for a, b in zip(got[:4], want[:4]):
            assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert got[4] == float(np.sum(np.asarray(want[4], np.float64))) and mf_minibatch_oracle.fit(*args, **kw)[4] == want[4]


@pytest.mark.parametrize("opt", mc.OPTS)
def test_float64_mode_and_the_state_it_returns(opt):
    """float64 tensors, float32-rounded scalars; the state is the optimiser's own: none for SGD, and for the others what the
    step formulas give for a row with one gradient (user 0) and for a row with none at reg 0 (the last item: all zero)"""
    name = "k17/" + opt
    c, d = mc.CASES[name], mc.inputs(name)
    out = mc.oracle_fit(c, [d[t] for t in mc.TABLES], d, d["batches"], np.float64, return_state=True)
    assert all(a.dtype == np.float64 for a in out[:4]) and len(out[5]) == 4
    want = {"sgd": set(), "adam": {"step", "exp_avg", "exp_avg_sq"}, "rmsprop": {"step", "square_avg"}, "adagrad": {"step", "sum"}}[opt]
    for q, st in enumerate(out[5]):
        assert set(st) == want
        for n, a in st.items():
            if n != "step":
                assert a.dtype == np.float64 and a.size == out[q].size
            else:
                assert float(a) == len(d["batches"])
    if opt != "sgd" and c["reg"] == 0:
        for n in want - {"step"}:
            assert not out[5][1][n][-1].any() and out[5][0][n][0].any()
    # the scalars: a float64 run handed the rounded values itself gives the same bits, one handed 0.05 unrounded would not
    c2 = dict(c, lr=float(np.float32(c["lr"])), reg=float(np.float32(c["reg"])))
    again = mc.oracle_fit(c2, [d[t] for t in mc.TABLES], d, d["batches"], np.float64)
    assert all(np.array_equal(a, b) for a, b in zip(out[:4], again[:4]))
    assert float(np.float32(0.05)) != 0.05 and float(np.float32(0.01)) != 0.01


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_the_references_meet_the_condition(name):
    worst = mc.check_condition(name)
    tols, ltol = mc.tolerances(name)
    f32, f64 = mc.reference(name, "float32"), mc.reference(name)
    assert all(np.isfinite(a).all() for a in f64[:4]) and np.isfinite(f64[4]) and f64[4] > 0
    print("%s: worst tolerance / movement %.3g; tolerances %s; movements %s; loss %.6g (tolerance %.3g, float32 run off by %.3g)"
          % (name, worst, ["%.3g" % t for t in tols], ["%.3g" % m for m in mc.movements(name)], f64[4], ltol, abs(f32[4] - f64[4])))
    assert ltol <= 1e-3 * f64[4]   # 16 * the float32 sum's own error stays small beside the sum


@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_the_cases_have_the_properties_the_device_tests_rely_on(name):
    c, d = mc.CASES[name], mc.inputs(name)
    users, items = mc.position_rows(name)
    n, bs = c["n"], c["bs"]
    assert len(d["batches"]) >= 4 and sum(len(b) for b in d["batches"]) == n == len(d["order"])
    assert not np.array_equal(d["order"], np.arange(n)) and d["order"].min() >= 0 and d["order"].max() < n
    assert len(np.unique(d["order"])) == n - (1 if c["dup"] else 0)
    if c["dup"]:
        assert d["order"][bs + 1] == d["order"][bs + 2]   # inside the second batch
    if c["distinct"]:
        for a in range(0, n, bs):
            m = len(users[a:a + bs])
            assert len(np.unique(users[a:a + bs])) == m == len(np.unique(items[a:a + bs]))
    else:
        assert users[0] == 0 and (users[:bs] == 0).sum() >= 1 and not (users[bs:] == 0).any()
        assert (items != c["ni"] - 1).all()
        for a in range(0, n, bs):
            m = len(items[a:a + bs])
            if m >= 5:
                share = (items[a:a + bs] == mc.ITEM).mean()
                # a third by construction, plus what the draw adds, less the one a repeated index may overwrite
                assert (m // 3 - int(c["dup"])) / m <= share <= 0.5, (a, share)
    if c["drop"] is not None:
        assert d["keep_u"].shape == (n, c["k"]) == d["keep_i"].shape
        if c["drop"] < 1.0:
            assert not d["keep_u"][bs + 3].any() and not d["keep_i"][bs + 4].any()
            # masks differ from position to position, and a rating's mask is not the mask at the place it is stored
            assert c["k"] == 1 or len(np.unique(d["keep_u"], axis=0)) > 1
            assert not np.array_equal(d["keep_u"][d["order"]], d["keep_u"]) and not np.array_equal(d["keep_i"][d["order"]], d["keep_i"])
        else:
            assert not d["keep_u"].any() and not d["keep_i"].any() and d["keep_scale"] == 0.0 and c["reg"] > 0


def test_which_cases_cross_the_grid_limits():
    grad = sorted(n for n, c in mc.CASES.items() if c["bs"] > mc.GRAD_STRIDE and c["n"] > c["bs"])
    assert grad == sorted(["gstride/%s" % o for o in mc.OPTS] + ["drop/gstride/adam", "drop/gstride/sgd"])
    for n in grad:   # full batches above the grid's reach and a short last one
        assert [len(b) for b in mc.inputs(n)["batches"]] == [70000, 70000, 70000, 1000] and mc.CASES[n]["k"] == 3
    total = lambda c: (c["nu"] + c["ni"]) * c["k"] + (c["nu"] + c["ni"] if c["use_bias"] else 0)
    apply = sorted(n for n, c in mc.CASES.items() if total(c) > mc.APPLY_STRIDE)
    assert apply == sorted("astride/%s" % o for o in mc.OPTS)
    for n in apply:   # U alone is above one pass: its tail, V, Bu and Bi belong to the second
        c = mc.CASES[n]
        assert mc.APPLY_STRIDE < c["nu"] * c["k"] < total(c) < 2 * mc.APPLY_STRIDE
    assert (mc.CASES["seg185/sgd"]["nu"] * mc.CASES["seg185/sgd"]["k"]) % 256 == 185 and (mc.CASES["seg185/sgd"]["nu"] * 5) % 64 != 0
    assert (mc.CASES["seg256/sgd"]["nu"] * mc.CASES["seg256/sgd"]["k"]) % 256 == 0
    # every optimiser runs at every shape, with both reg values and without biases
    for o in mc.OPTS:
        mine = [c for c in mc.CASES.values() if c["opt"] == o]
        assert {c["reg"] for c in mine} == {0.0, 0.05} and {c["use_bias"] for c in mine} == {True, False}
        assert {c["k"] for c in mine} >= {1, 15, 16, 17, 32, 33, 100, 3, 128} and {c["bs"] for c in mine} >= {1, 15, 16, 17, 50, 64, 70000}


@pytest.mark.parametrize("name", sorted(n for n, c in mc.CASES.items() if mc.keeps_state(c)))
def test_user0_moves_by_its_state_alone(name):
    """after step 1 user 0 has no gradient any more: what moves its row is the optimiser's state (and weight decay)"""
    tol = mc.tolerances(name)[0][0]
    move = mc.user0_movement(name)
    print("%s: user 0 moved %.3g after its last gradient = %.0f tolerances of %.3g" % (name, move, move / tol, tol))
    assert move > 100 * tol


@pytest.mark.parametrize("name", sorted(n for n, c in mc.CASES.items() if c["opt"] == "rmsprop" and c["reg"] == 0 and not c["distinct"]))
def test_rmsprop_without_weight_decay_leaves_user0_where_step_1_put_it(name):
    assert mc.user0_movement(name) == 0.0


@pytest.mark.parametrize("opt,use_bias,p", mc.MODEL_CASES)
def test_model_level_references_meet_the_condition(opt, use_bias, p):
    """the golden runs train for many epochs and move their tables by 0.02 to 1.7; float32 torch itself ends up to 4.4e-06 from
    float64 torch there (Adam with dropout 0.5), so the rule's tolerance is 1.7e-07 to 7.0e-05: under 1.3e-04 of the movement
    everywhere, under the golden tests' absolute 1e-4 / 2e-5 everywhere but for Adam with dropout 0.5, and a tenth of them for
    SGD only: what float32 torch itself allows.  The golden tests stay beside these and hold their own gates."""
    m = mc.model_reference(opt, use_bias, p)
    worst = mc.check_moves(m["tols"], m["moves"], m["f32"], m["init"], (opt, use_bias, p))
    print("%s bias %s p %s: tolerances %s, movements %s, worst share %.3g" % (opt, use_bias, p, ["%.3g" % t for t in m["tols"]],
                                                                             ["%.3g" % x for x in m["moves"]], worst))
