"""GPU parity tests of the WMF minibatch path (cornac_hip_wmf_*) against oracle/wmf_oracle.py."""
import numpy as np
import pytest
import scipy.sparse as sp

from cornac_amd import WMF, _lib
import wmf_cases as wc
from conftest import load_golden, synth_dataset
from oracle.wmf_oracle import WmfOracle

pytestmark = pytest.mark.gpu


def _run_both(R, U, V, batches, lu, lv, a, b, lr):
    o = WmfOracle(U, V, R, lu, lv, a, b, lr)
    lo = np.array(o.fit_batches(batches))
    tr = _lib.WmfTrainer(R, U.shape[1])
    tr.set_factors(U, V)
    lg = tr.fit_batches(batches, lu, lv, a, b, lr)
    Ug, Vg = tr.get_factors()
    tr.close()
    return o, lo, Ug, Vg, lg


@pytest.mark.parametrize("nu,ni,k,bs", [(300, 200, 24, 64), (129, 257, 5, 128), (1000, 90, 200, 37), (64, 3, 33, 2),
                                         (700, 300, 128, 128), (517, 260, 100, 77), (40000, 256, 128, 128),
                                         (128, 140, 128, 128), (129, 140, 120, 100), (5, 130, 128, 128), (33000, 200, 97, 128)])
def test_steps_match_oracle(nu, ni, k, bs):
    """k in 97..128 takes the wave-specialised kernel (wmf_ws.inc): full and ragged user tiles, ragged batches, and at
    40 000 users several tiles per workgroup (the Adam sweep of a tile runs beside the products of the next one); exactly one
    tile, one row over a tile, fewer users than one slice (the tables are padded to whole tiles + one: rows that do not exist
    must stay out of the result and out of the loss), 33 000 users = 258 tiles on 256 workgroups (two of them sweep a real
    previous tile, the others only the scratch tile)"""
    c = wc.legacy_case(nu, ni, k, bs)   # (the generator lives beside the other cases: test_wmf_cpu.py reads it too)
    R, U, V, batches = c["R"], c["U"], c["V"], c["batches"]
    o, lo, Ug, Vg, lg = _run_both(R, U, V, batches, 0.02, 0.03, 1.0, 0.01, 0.005)
    assert np.abs(Ug - o.U).max() <= 1e-4, np.abs(Ug - o.U).max()
    assert np.abs(Vg - o.V).max() <= 1e-4, np.abs(Vg - o.V).max()
    assert np.allclose(lg, lo, rtol=2e-5), np.abs(lg / lo - 1).max()


def test_steps_match_oracle_without_the_unobserved_weight():
    """b = 0: G carries nothing to recover a prediction from, the fix-up recomputes the dot products (both fused kernels)"""
    for nu, ni, k in [(300, 150, 128), (300, 150, 40)]:
        rs = np.random.RandomState(k)
        keys = rs.permutation(nu * ni)[:5000]
        R = sp.csc_matrix((rs.randint(1, 6, 5000).astype(np.float32), (keys // ni, keys % ni)), shape=(nu, ni))
        U = rs.normal(0, 0.2, (nu, k)).astype(np.float32)
        V = rs.normal(0, 0.2, (ni, k)).astype(np.float32)
        perm = rs.permutation(ni)
        batches = [perm[s:s + 128] for s in range(0, ni, 128)] * 2
        o, lo, Ug, Vg, lg = _run_both(R, U, V, batches, 0.02, 0.03, 1.0, 0.0, 0.005)
        assert np.abs(Ug - o.U).max() <= 1e-4 and np.abs(Vg - o.V).max() <= 1e-4
        assert np.allclose(lg, lo, rtol=2e-5)


def test_fixture_and_model_surface():
    fx = load_golden("wmf_small")
    from cornac_amd import Dataset

    ds = Dataset.from_uir([(int(u), int(i), float(r)) for u, i, r in zip(fx["users"], fx["items"], fx["ratings"])], seed=123)
    kw = dict(k=int(fx["k"]), lambda_u=float(fx["lambda_u"]), lambda_v=float(fx["lambda_v"]), a=float(fx["a"]),
              b=float(fx["b"]), learning_rate=float(fx["lr"]), batch_size=int(fx["batch_size"]), max_iter=int(fx["max_iter"]))
    m = WMF(verbose=False, seed=7, init_params={"U": fx["U0"].copy(), "V": fx["V0"].copy()}, **kw).fit(ds)
    assert np.abs(m.U - fx["U"]).max() <= 1e-4 and np.abs(m.V - fx["V"]).max() <= 1e-4
    assert m.loss_history[-1] < m.loss_history[0]
    s = m.score(0)
    assert np.abs(s - m.V @ m.U[0]).max() < 1e-5
    ranked, scores = m.rank(0, k=5)
    assert len(ranked) == len(scores) and scores[ranked[0]] == scores.max() and np.all(np.diff(scores[ranked[:5]]) <= 0)
    # explicit zeros and empty columns: the weights fall back to b and nothing breaks
    R = sp.csc_matrix((np.array([0.0, 2.0], np.float32), (np.array([0, 1]), np.array([0, 0]))), shape=(4, 3))
    U = np.full((4, 2), 0.1, np.float32); V = np.full((3, 2), 0.2, np.float32)
    o, lo, Ug, Vg, lg = _run_both(R, U, V, [np.array([0, 2]), np.array([1])], 0.01, 0.01, 1.0, 0.5, 0.01)
    assert np.abs(Ug - o.U).max() <= 1e-6 and np.abs(Vg - o.V).max() <= 1e-6 and np.allclose(lg, lo, rtol=1e-6)


def test_training_learns_and_errors():
    ds = synth_dataset(400, 150, 6000, seed=3)
    m = WMF(k=16, max_iter=15, learning_rate=0.01, verbose=False, seed=1).fit(ds)
    assert m.loss_history[-1] < 0.85 * m.loss_history[0]
    with pytest.raises(ValueError):
        WMF(k=4, batch_size=500, verbose=False).fit(ds)
    tr = _lib.WmfTrainer(ds.csc_matrix, 4)
    with pytest.raises(_lib.HipError):
        tr.fit_batches([np.array([10 ** 6])], 0.1, 0.1, 1, 0.01, 0.01)
    tr.close()


def test_hip_wmf_matches_the_reference_codes_fixture():
    """cornac_amd.WMF on the device against tests/golden/wmf_ref.npz — U, V and score() as learned by the reference's own
    WMF code (cornac/models/wmf/recom_wmf.py + wmf.py over oracle/tf1_shim; tests/golden/make_wmf_ref_golden.py) from its
    own initialisation and batch order: north_star's 1e-4"""
    from cornac_amd import Dataset

    fx = load_golden("wmf_ref")
    ds = Dataset.from_uir([(int(u), int(i), float(r)) for u, i, r in zip(fx["users"], fx["items"], fx["ratings"])], seed=123)
    kw = {n: (int(fx[n]) if n in ("k", "max_iter", "batch_size", "seed") else float(fx[n]))
          for n in ("k", "max_iter", "batch_size", "learning_rate", "lambda_u", "lambda_v", "a", "b", "seed")}
    m = WMF(verbose=False, **kw).fit(ds)
    assert np.abs(m.U - fx["U"]).max() <= 1e-4 and np.abs(m.V - fx["V"]).max() <= 1e-4
    for t, u in enumerate(fx["score_users"]):
        assert np.abs(m.score(int(u)) - fx["scores"][t]).max() <= 1e-4


# ---- against the float64 oracle, on all three kernel paths (tests/wmf_cases.py) ----------------------------------------
# The user side of a step is one of three implementations, chosen from ld = round_up(k, 32): LDS-fused (ld <= 96),
# wave-specialised (ld == 128), unfused (ld >= 160).  Every case below is compared with the oracle run in float64: at
# wmf_cases.T on the elements whose Adam step is well conditioned, at 2 lr on the few the oracle flags (an element whose
# gradient is within float32 rounding of zero moves by +- lr on step 1 whichever way the rounding falls); the losses at
# rtol 2e-5; rows of V no batch has touched bit-identical to the input.  tests/test_wmf_cpu.py checks, in the reference
# alone, that the cases are fair (few flagged elements, the clip exercised on each path but not dominant) and ties T to them.


def _cus():
    return _lib.device_info()["compute_units"]


def _device_run(case, calls=None):
    """the case on the device; `calls`: the batch list split into several fit_batches calls"""
    tr = _lib.WmfTrainer(case["R"], case["k"])
    try:
        tr.set_factors(case["U"], case["V"])
        losses = [tr.fit_batches(part, case["lu"], case["lv"], case["a"], case["b"], case["lr"])
                  for part in (calls if calls is not None else [case["batches"]])]
        U, V = tr.get_factors()
    finally:
        tr.close()
    return U, V, np.concatenate(losses)


def _check(name, case, got, ref=None):
    o, lo = ref if ref is not None else wc.run_oracle(case)
    U, V, lg = got
    wc.compare(o, U, V, case["lr"], name)
    print("%s loss: max rel err %.3g" % (name, np.abs(lg / lo - 1).max()))
    assert np.allclose(lg, lo, rtol=2e-5), np.abs(lg / lo - 1).max()
    rest = np.setdiff1d(np.arange(V.shape[0]), np.concatenate(case["batches"]))
    assert np.array_equal(V[rest], case["V"][rest]), "rows of V outside every batch moved"
    return o, lo


@pytest.mark.parametrize("name", [n for n in wc.CASES if not n.startswith("model_")])
def test_case_matches_the_float64_oracle(name):
    cus = _cus()
    case = wc.CASES[name](cus)
    nu = case["U"].shape[0]
    if name.startswith("lds_scale"):
        tiles, wgs = -(-nu // 128), 2 * cus
        assert wc.path_of(case["k"]) == "lds" and tiles > wgs, "the case must give a workgroup more than one user tile"
        if "exact" not in name:   # per_wg = 2, so the last workgroups have no tile at all, and the last tile is ragged
            assert -(-tiles // wgs) == 2 and -(-tiles // 2) < wgs and nu % 128 != 0
    if name.startswith("unfused_scale"):
        chunk = -(-max(16, -(-nu // 512)) // 16) * 16
        assert wc.path_of(case["k"]) == "unfused" and chunk > 16 and nu % chunk != 0
    _check(name, case, _device_run(case))


def test_unsorted_columns_give_the_sorted_matrix_result():
    """cornac_hip_wmf_create sorts the rows of a column itself (the fused kernels walk a column with a cursor): the same
    matrix with every column's entries shuffled.  Not bit-equal: the dV partials are summed with float atomics."""
    a, b = wc.fixup_pattern_case(128), wc.fixup_pattern_case(128, unsorted=True)
    assert not b["R"].has_sorted_indices and (a["R"] != b["R"]).nnz == 0
    ref = wc.run_oracle(a)
    Ua, Va, la = _device_run(a)
    Ub, Vb, lb = _device_run(b)
    _check("unsorted", b, (Ub, Vb, lb), ref)
    fu, fv = ref[0].flagged(wc.T)
    assert np.abs(Ua - Ub)[~fu].max() <= wc.T and np.abs(Va - Vb)[~fv].max() <= wc.T and np.allclose(la, lb, rtol=2e-5)


def test_k_above_1024_is_rejected():
    R = sp.csc_matrix(np.eye(4, dtype=np.float32))
    with pytest.raises(_lib.HipError):
        _lib.WmfTrainer(R, 1025)
    _lib.WmfTrainer(R, 1024).close()


@pytest.mark.parametrize("k", [80, 128, 200])
def test_call_boundaries(k):
    """the same batch list in one call, split over three calls (one of them a single batch) with an empty call between;
    set_factors on a used handle restarts the moments, the step count and the batch tags"""
    case = wc.batch_edge_case(k)
    ref = wc.run_oracle(case)
    bl = case["batches"]
    one = _device_run(case)
    _check("one call", case, one, ref)
    split = _device_run(case, calls=[bl[:3], [], bl[3:4], bl[4:]])
    _check("three calls", case, split, ref)
    fu, fv = ref[0].flagged(wc.T)
    assert np.abs(one[0] - split[0])[~fu].max() <= wc.T and np.abs(one[1] - split[1])[~fv].max() <= wc.T
    # a used handle (other factors, other batches, so every tag and moment is stale), then set_factors and the case
    rs = np.random.RandomState(k)
    tr = _lib.WmfTrainer(case["R"], k)
    try:
        tr.set_factors(rs.normal(0, 0.3, case["U"].shape), rs.normal(0, 0.3, case["V"].shape))
        tr.fit_batches(bl[::-1], 0.1, 0.1, 1.0, 0.02, 0.01)
        tr.set_factors(case["U"], case["V"])
        U0, V0 = tr.get_factors()
        assert np.array_equal(U0, case["U"]) and np.array_equal(V0, case["V"])
        lg = tr.fit_batches(bl, case["lu"], case["lv"], case["a"], case["b"], case["lr"])
        _check("reused handle", case, tr.get_factors() + (lg,), ref)
    finally:
        tr.close()


@pytest.mark.parametrize("k", [80, 128, 200])
def test_rejected_call_leaves_the_state_untouched(k):
    """a call that fails its checks (id out of range, 129 items, an empty batch, the same item twice in a batch) happens
    before anything is enqueued: factors bit-identical, and the next valid call continues as if it had not been made"""
    case = wc.batch_edge_case(k)
    ref = wc.run_oracle(case)
    bl = case["batches"]
    hp = (case["lu"], case["lv"], case["a"], case["b"], case["lr"])
    ni = case["V"].shape[0]
    tr = _lib.WmfTrainer(case["R"], k)
    try:
        tr.set_factors(case["U"], case["V"])
        l1 = tr.fit_batches(bl[:3], *hp)
        before = tr.get_factors()
        for bad in ([bl[3], np.array([7, ni])], [bl[3], np.array([-1])], [np.arange(129)], [bl[3], np.zeros(0, np.int32)],
                    [bl[3], np.array([9, 11, 9])], [np.array([0] + list(range(126, 0, -1)) + [0])]):
            with pytest.raises(_lib.HipError):
                tr.fit_batches(bad, *hp)
            after = tr.get_factors()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        l2 = tr.fit_batches(bl[3:], *hp)
        _check("after rejected calls", case, tr.get_factors() + (np.concatenate([l1, l2]),), ref)
    finally:
        tr.close()


@pytest.mark.parametrize("k", [80, 200])
def test_model_matches_the_float64_oracle(k, monkeypatch):
    """cornac_amd.WMF (k = 200 is the reference's default) with init_params, against the float64 oracle driven with the
    batches the model handed to the device"""
    case = wc.model_case(k)
    seen = []
    fit = _lib.WmfTrainer.fit_batches

    def recording(self, batches, *args):
        seen.extend(np.array(x) for x in batches)
        return fit(self, batches, *args)

    monkeypatch.setattr(_lib.WmfTrainer, "fit_batches", recording)
    m = WMF(verbose=False, seed=3, init_params={"U": case["U"].copy(), "V": case["V"].copy()}, **case["model_kw"])
    m.fit(case["dataset"]())
    assert len(seen) == len(case["batches"]) and all(np.array_equal(x, y) for x, y in zip(seen, case["batches"]))
    o, _ = wc.run_oracle(case)
    wc.compare(o, m.U, m.V, case["lr"], "model k=%d" % k)
    assert len(m.loss_history) == case["model_kw"]["max_iter"] and m.loss_history[-1] < m.loss_history[0]
