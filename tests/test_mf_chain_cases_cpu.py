"""The cases of tests/test_mf_chain_gpu.py are fair: the oracle alone, no device.  Every case trains (finite, the
factors move), its (user, item) pairs repeat, it sits on the side of the dataflow launch's thresholds it is meant for,
and the ownership rule of mf_build_chain — restated in mf_chain_cases.owns_users — picks the side each sorted store names.
"""
import numpy as np
import pytest

import mf_chain_cases as mc


@pytest.mark.parametrize("kind,k,use_bias", mc.ALL_CASES)
def test_case_trains_and_its_pairs_repeat(oracle, kind, k, use_bias):
    c = mc.case(kind, k)
    U, V, Bu, Bi, loss = mc.reference(kind, k, use_bias)
    assert all(np.isfinite(a).all() for a in (U, V, Bu, Bi, loss))
    assert np.abs(U - c["U"]).max() > 1e-3 and np.abs(V - c["V"]).max() > 1e-3, "the run did not move the factors"
    assert loss[-1] < loss[0]
    if use_bias:
        assert np.abs(Bu).max() > 1e-3 and np.abs(Bi).max() > 1e-3
    else:
        assert not Bu.any() and not Bi.any()
    n = len(c["stars"])
    assert len(np.unique(c["uid"] * c["ni"] + c["iid"])) < n, "no (user, item) pair repeats"
    assert c["uid"].min() >= 0 and c["uid"].max() < c["nu"] and c["iid"].min() >= 0 and c["iid"].max() < c["ni"]
    assert c["U"].dtype == c["V"].dtype == c["stars"].dtype == np.float32
    assert c["mu"] == float(np.float32(c["mu"])) and abs(c["mu"] - c["stars"].astype(np.float64).mean()) < 1e-5


def test_shapes_sit_on_the_thresholds_they_are_meant_for():
    assert len(mc.case("edge", 1)["stars"]) == 4096 and mc.case("edge", 1)["nu"] == 64 and mc.case("edge", 1)["ni"] == 48
    assert len(mc.case("nnz4095", 5)["stars"]) == 4095 and len(mc.case("nnz4096", 5)["stars"]) == 4096
    assert max(mc.K_CHAIN) == 256 and mc.K_LEVELS == 257
    # both sides of every register-slice switch of the dataflow kernel (k <= 64 R)
    assert {(k + 63) // 64 for k in mc.K_CHAIN} == {1, 2, 3, 4}
    assert all(k in mc.K_CHAIN and k + 1 in mc.K_CHAIN + (mc.K_LEVELS,) for k in (64, 128, 192, 256))
    assert max(len(mc.case(kind, k)["stars"]) for kind, k, _ in mc.ALL_CASES) == 5000


@pytest.mark.parametrize("order", mc.ORDERS)
def test_order_cases_and_the_ownership_rule(order):
    c = mc.case("order_" + order, 10)
    uid, iid = c["uid"], c["iid"]
    assert np.bincount(iid, minlength=c["ni"])[3] >= 1000 and np.bincount(uid, minlength=c["nu"])[299] == 1
    if order == "user":
        assert (np.diff(uid) >= 0).all()
    if order == "item":
        assert (np.diff(iid) >= 0).all()
    if order in mc.OWN_USER:
        assert mc.owns_users(uid, iid) == bool(mc.OWN_USER[order])
    else:
        # no adjacency to speak of: the side with the longer hottest row, item 3
        adj = max((uid[1:] == uid[:-1]).sum(), (iid[1:] == iid[:-1]).sum())
        assert adj * 10 <= len(uid) * 3 and not mc.owns_users(uid, iid)
    for k in mc.ORDER_K:   # the index arrays do not depend on k
        assert np.array_equal(mc.case("order_" + order, k)["uid"], uid) and np.array_equal(mc.case("order_" + order, k)["iid"], iid)


def test_the_ownership_rule_on_the_other_cases():
    """shuffled random stores: no adjacency, the longer hottest row decides (a tie goes to the items)"""
    for kind, k, _ in mc.ALL_CASES:
        c = mc.case(kind, k)
        if kind.startswith("order_"):
            continue
        max_u, max_i = np.bincount(c["uid"]).max(), np.bincount(c["iid"]).max()
        assert mc.owns_users(c["uid"], c["iid"]) == bool(max_u > max_i)
