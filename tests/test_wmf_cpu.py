"""CPU checks of the WMF oracle (oracle/wmf_oracle.py).  TensorFlow is absent, so the pin is the reference's own WMF
code run over oracle/tf1_shim (tests/golden/wmf_ref.npz here, the live run in tests/test_oracle_vs_reference.py); besides
that: the restated gradients are the gradients of the reference's loss expression (torch autograd of
cornac/models/wmf/wmf.py:44-48), the optimiser follows TF1 Adam's published update, and a regression fixture."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import wmf_cases as wc
from conftest import load_golden
from oracle.wmf_oracle import WmfOracle


def _case(seed=0, nu=60, ni=45, k=7, nnz=500):
    rs = np.random.RandomState(seed)
    keys = rs.permutation(nu * ni)[:nnz]
    u, i = keys // ni, keys % ni
    r = rs.randint(1, 6, nnz).astype(np.float32)
    R = sp.csc_matrix((r, (u, i)), shape=(nu, ni))
    U = rs.normal(0, 0.3, (nu, k)).astype(np.float32)
    V = rs.normal(0, 0.3, (ni, k)).astype(np.float32)
    return R, U, V


def test_first_step_matches_autograd_of_the_reference_loss():
    import torch

    R, U, V = _case()
    ids = np.array([3, 17, 5, 40, 8, 21])
    lu, lv, a, b, lr = 0.03, 0.02, 1.0, 0.05, 0.01
    o = WmfOracle(U, V, R, lu, lv, a, b, lr)
    loss = o.step(ids)
    Ut, Vt = torch.tensor(U, dtype=torch.float64, requires_grad=True), torch.tensor(V, dtype=torch.float64, requires_grad=True)
    Rb = torch.tensor(R[:, ids].toarray(), dtype=torch.float64)
    C = torch.where(Rb != 0, torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64))
    Vb = Vt[ids]
    L = (C * (Rb - Ut @ Vb.T) ** 2).sum() + lu * 0.5 * (Ut ** 2).sum() + lv * 0.5 * (Vb ** 2).sum()
    L.backward()
    assert abs(loss - L.item()) <= 1e-5 * abs(L.item())
    # step 1 of Adam: m_hat = g, v_hat = g^2  ->  delta = -lr g / (|g| + eps*)   (eps folded, TF1 form)
    for new, old, g in ((o.U, U, Ut.grad.numpy()), (o.V, V, Vt.grad.numpy())):
        g = np.clip(g, -5, 5)
        lr_t = lr * np.sqrt(1 - 0.999) / (1 - 0.9)
        want = old - lr_t * (0.1 * g) / (np.sqrt(0.001 * g * g) + 1e-8)
        assert np.abs(new - want).max() < 2e-6
    # rows of V outside the batch have zero gradient and zero moments: they must not move on step 1
    rest = np.setdiff1d(np.arange(V.shape[0]), ids)
    assert np.array_equal(o.V[rest], V[rest])


def test_sparse_adam_moves_all_rows_after_a_row_was_touched():
    """TF1's IndexedSlices Adam: a row touched in step 1 keeps moving in step 2 even if absent from that batch"""
    R, U, V = _case(1)
    o = WmfOracle(U, V, R, lr=0.01)
    o.step(np.array([0, 1, 2]))
    v1 = o.V.copy()
    o.step(np.array([3, 4]))
    assert np.abs(o.V[[0, 1, 2]] - v1[[0, 1, 2]]).max() > 1e-4
    assert np.array_equal(o.V[10:], V[10:])


def test_fixture_regression():
    fx = load_golden("wmf_small")
    R = sp.csc_matrix((fx["ratings"], (fx["users"], fx["items"])), shape=(int(fx["n_users"]), int(fx["n_items"])))
    o = WmfOracle(fx["U0"], fx["V0"], R, float(fx["lambda_u"]), float(fx["lambda_v"]), float(fx["a"]), float(fx["b"]),
                  float(fx["lr"]))
    ptr = fx["batch_ptr"]
    losses = o.fit_batches([fx["batch_ids"][ptr[t]:ptr[t + 1]] for t in range(len(ptr) - 1)])
    assert np.abs(o.U - fx["U"]).max() <= 2e-6 and np.abs(o.V - fx["V"]).max() <= 2e-6
    assert np.allclose(losses, fx["losses"], rtol=1e-6)


def _wmf_ref_case():
    from cornac_amd import Dataset

    fx = load_golden("wmf_ref")
    ds = Dataset.from_uir([(int(u), int(i), float(r)) for u, i, r in zip(fx["users"], fx["items"], fx["ratings"])], seed=123)
    kw = {n: (int(fx[n]) if n in ("k", "max_iter", "batch_size", "seed") else float(fx[n]))
          for n in ("k", "max_iter", "batch_size", "learning_rate", "lambda_u", "lambda_v", "a", "b", "seed")}
    return fx, ds, kw


def test_host_class_and_oracle_reproduce_the_reference_codes_fixture(monkeypatch):
    """tests/golden/wmf_ref.npz: what the reference's OWN WMF code learned (run over oracle/tf1_shim, see
    make_wmf_ref_golden.py) from its own xavier initialisation and item_iter shuffling.  cornac_amd.WMF with the oracle
    as device layer reproduces it to float32 rounding: initialisation, batch order, gradients, Adam, score()."""
    import fake_device

    from cornac_amd import WMF

    fake_device.install(monkeypatch)
    fx, ds, kw = _wmf_ref_case()
    m = WMF(verbose=False, **kw).fit(ds)
    assert np.abs(m.U - fx["U"]).max() < 5e-6 and np.abs(m.V - fx["V"]).max() < 5e-6
    for t, u in enumerate(fx["score_users"]):
        assert np.abs(m.score(int(u)) - fx["scores"][t]).max() < 1e-5


# ---- the float64 oracle, its conditioning bound, and the cases of tests/test_wmf_gpu.py (tests/wmf_cases.py) --------------


def test_float64_oracle_matches_autograd_of_the_reference_loss_over_three_steps():
    """three consecutive steps (moments carried, V's rows outside the batch decaying and moving) against torch autograd of
    the reference's loss expression in float64 + TF1 Adam written out; batch 2 holds an explicit zero and an empty column"""
    import torch

    R, U, V = _case(3)
    R = R.tolil()
    R[:, 9] = 0
    R = R.tocsc()
    R.eliminate_zeros()
    R.data[R.indptr[17]] = 0.0   # an explicit zero: stays "unobserved"
    assert R.indptr[9] == R.indptr[10] and R.indptr[17] < R.indptr[18]
    lu, lv, a, b, lr = 0.03, 0.02, 2.0, 0.05, 0.01
    batches = [np.array([3, 17, 5, 40, 8, 21]), np.array([9, 17, 2, 30]), np.array([5, 9, 44, 0, 1])]
    o = WmfOracle(U, V, R, lu, lv, a, b, lr, dtype=np.float64)
    f = lambda x: float(np.float32(x))   # noqa: E731  (the oracle, like the device, takes the float32 values)
    lu, lv, a, b = f(lu), f(lv), f(a), f(b)
    Uw, Vw = U.astype(np.float64), V.astype(np.float64)
    mU, vU, mV, vV = (np.zeros_like(x) for x in (Uw, Uw, Vw, Vw))
    eps, clipped = f(1e-8), 0
    for t, ids in enumerate(batches, 1):
        loss = o.step(ids)
        Ut, Vt = torch.tensor(Uw, requires_grad=True), torch.tensor(Vw, requires_grad=True)
        Rb = torch.tensor(R[:, ids].toarray(), dtype=torch.float64)
        C = torch.where(Rb != 0, torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64))
        Vb = Vt[ids]
        L = (C * (Rb - Ut @ Vb.T) ** 2).sum() + lu * 0.5 * (Ut ** 2).sum() + lv * 0.5 * (Vb ** 2).sum()
        L.backward()
        assert abs(loss - L.item()) <= 1e-12 * abs(L.item())
        gU, gV = np.clip(Ut.grad.numpy(), -5, 5), np.clip(Vt.grad.numpy(), -5, 5)   # (gV: zero rows outside the batch)
        clipped += int((np.abs(gU) == 5).sum() + (np.abs(gV) == 5).sum())
        lr_t = lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t)
        mU += 0.1 * (gU - mU); vU += 0.001 * (gU * gU - vU)
        Uw = Uw - lr_t * mU / (np.sqrt(vU) + eps)
        mV *= 0.9; vV *= 0.999   # IndexedSlices: every row decays, the batch's rows receive, every row moves
        mV[ids] += 0.1 * gV[ids]; vV[ids] += 0.001 * gV[ids] ** 2
        Vw = Vw - lr_t * mV / (np.sqrt(vV) + eps)
        assert np.abs(o.U - Uw).max() <= 1e-12 and np.abs(o.V - Vw).max() <= 1e-12, (t, np.abs(o.U - Uw).max())
    assert clipped > 0, "the case should reach the clip"


@functools.lru_cache(maxsize=None)
def _reference_figures(name):
    """one GPU case in the reference alone: float32 oracle against float64 oracle, flags, clipped shares, movement"""
    case = wc.CASES[name](wc.MI355X_CUS)
    o64, l64 = wc.run_oracle(case)
    o32, l32 = wc.run_oracle(case, np.float32)
    fu, fv = o64.flagged(wc.T)
    fig = dict(err_U=np.abs(o32.U - o64.U)[~fu].max(), err_V=np.abs(o32.V - o64.V)[~fv].max(), flag_U=fu.mean(), flag_V=fv.mean(),
               clip_U=o64.clip_share("U"), clip_V=o64.clip_share("V"), move_U=np.abs(o64.U - case["U"]).max(),
               move_V=np.abs(o64.V - case["V"]).max(), loss=np.abs(l32 / l64 - 1).max(), path=wc.path_of(case["k"]))
    print(name, {n: (v if isinstance(v, str) else float("%.3g" % v)) for n, v in fig.items()})
    return fig


@pytest.mark.parametrize("name", list(wc.CASES))
def test_gpu_case_is_fair_and_within_a_quarter_of_T_in_float32(name):
    """what every case of test_wmf_gpu.py must be IN THE REFERENCE ALONE for a comparison at T to mean something: the float32
    oracle — same step, same number format as the device, another summation order — is within T / 4 of the float64 oracle
    on the unflagged elements (T = 4 x its largest error: wmf_cases.T); few elements are flagged; neither gradient is mostly
    clipped (a clipped element hides its gradient); the tables move by far more than T"""
    fig = _reference_figures(name)
    assert fig["err_U"] <= wc.T / 4 and fig["err_V"] <= wc.T / 4
    assert fig["flag_U"] <= 5e-4 and fig["flag_V"] <= 5e-3
    assert fig["clip_U"] <= 0.3 and fig["clip_V"] <= 0.3
    assert fig["move_U"] > 100 * wc.T and fig["move_V"] > 100 * wc.T
    assert fig["loss"] <= 2e-5 / 4   # (the losses are compared at rtol 2e-5)


@pytest.mark.parametrize("path", ["lds", "ws", "unfused"])
def test_each_kernel_path_has_a_case_that_exercises_the_clip_on_both_sides(path):
    figs = [_reference_figures(n) for n in wc.CASES if n not in wc.BIG]
    assert any(f["path"] == path and f["clip_U"] >= 0.01 and f["clip_V"] >= 0.02 for f in figs)


def test_T_follows_its_rule():
    """T = 4 x the largest float32-oracle error over the unflagged elements of all cases, rounded up to one digit"""
    worst = max(max(_reference_figures(n)["err_U"], _reference_figures(n)["err_V"]) for n in wc.CASES)
    digit = 10.0 ** np.floor(np.log10(4 * worst))
    assert wc.T == pytest.approx(np.ceil(4 * worst / digit) * digit) and wc.T <= 1e-4, (worst, wc.T)


def test_the_flag_covers_every_ill_conditioned_element_of_the_40000_user_case():
    """test_steps_match_oracle's 40 000-user case (a = 1): the float32 oracle is 1.3e-4 from the float64 one on a handful of
    elements of U, 3e-7 on the rest.  Every element whose float32 error exceeds T must be one the bound flags."""
    case = wc.legacy_case(40000, 256, 128, 128)
    o64, _ = wc.run_oracle(case)
    o32, _ = wc.run_oracle(case, np.float32)
    fu, fv = o64.flagged(wc.T)
    eu, ev = np.abs(o32.U - o64.U), np.abs(o32.V - o64.V)
    print("over T: U %d V %d, flagged: U %d V %d, max err %.3g %.3g" % ((eu > wc.T).sum(), (ev > wc.T).sum(), fu.sum(), fv.sum(),
                                                                        eu.max(), ev.max()))
    assert (eu > wc.T).sum() > 0, "the case should hold ill-conditioned elements"
    assert fu[eu > wc.T].all() and fv[ev > wc.T].all()
    assert eu[fu].max() <= 2 * case["lr"] and (not fv.any() or ev[fv].max() <= 2 * case["lr"])


class _DropsAUserTileFromDV(WmfOracle):
    """a kernel-sized defect: on step `bad_step` the users 128..255 are missing from dV"""
    bad_step = 2

    def raw_gradients(self, D, Vb):
        dU, dV = super().raw_gradients(D, Vb)
        if self.t == self.bad_step:
            dV = dV - D[128:256].T @ self.U[128:256]
        return dU, dV


@pytest.mark.parametrize("name", ["k80", "fixup_pattern_k128", "unfused_scale_chunk_plus_one_k200"])
def test_a_kernel_sized_defect_moves_unflagged_elements_by_more_than_10_T(name):
    """the comparison can see what a subtly wrong kernel does: ONE non-zero left out of the fix-up of one step, or one user
    tile left out of dV in one step, in a copy of the oracle"""
    case = wc.CASES[name](wc.MI355X_CUS)
    o64, _ = wc.run_oracle(case)
    fu, fv = o64.flagged(wc.T)
    # (a) one stored rating of the second batch treated as unobserved on that step only
    o = WmfOracle(case["U"], case["V"], case["R"], case["lu"], case["lv"], case["a"], case["b"], case["lr"], dtype=np.float64)
    o.step(case["batches"][0])
    R, ids = case["R"], case["batches"][1]
    col = next(int(c) for c in ids if (R.data[R.indptr[c]:R.indptr[c + 1]] != 0).any())
    e = R.indptr[col] + int(np.flatnonzero(R.data[R.indptr[col]:R.indptr[col + 1]])[0])
    holed = R.copy()
    holed.data[e] = 0.0
    o.R = holed
    o.step(ids)
    o.R = R
    for ids in case["batches"][2:]:
        o.step(ids)
    du, dv = np.abs(o.U - o64.U)[~fu].max(), np.abs(o.V - o64.V)[~fv].max()
    print("one non-zero dropped: U %.3g V %.3g" % (du, dv))
    assert du > 10 * wc.T and dv > 10 * wc.T
    # (b) one user tile dropped from dV
    o, _ = wc.run_oracle(case, cls=_DropsAUserTileFromDV)
    dv = np.abs(o.V - o64.V)[~fv].max()
    print("one user tile dropped from dV: V %.3g" % dv)
    assert dv > 10 * wc.T
