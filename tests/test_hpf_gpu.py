"""HPF on the device, through the C ABI and through cornac_amd.HPF, against (a) scipy for the expected-log step alone, (b) the
reference's own compiled extension (tests/golden/hpf_ref.npz) and (c) the float64 restatement of its loop
(tests/hpf_cases.hpf_fit, itself held against the same golden by tests/test_hpf_cpu.py).

The device differs from the restatement in the two ways the restatement differs from the reference — the order of the sums
and three library functions (digamma, log, exp), compounded over the same iterations — so its tolerance on a case is
16 x the restatement-against-reference difference recorded for that case in tests/hpf_cases.py (one number for all four
tables, never above 1e-10); one iteration from given tables is held to 16 x the recorded one-iteration difference of the
variant.  Every check prints the measured difference next to its tolerance.

Measured on an MI355X (max relative difference; recorded in tests/hpf_cases.py next to the constants): the golden cases
3.3e-15 .. 4.4e-15 against tolerances of 7.6e-14 .. 1.6e-13; one iteration 2e-16 .. 3.2e-15 hierarchical and up to 1.2e-14
PF (long rows, k = 5) against 5.5e-14 / 5.7e-14; the expected-log step at 0.23 of its bound (0.48 on the tiny shapes); end
to end 8.3e-15 / 6.8e-15 against 1.6e-13 / 1.0e-13.
"""
import functools

import numpy as np
import pytest

import hpf_cases as hc
import nmf_cases as nc
from conftest import load_golden, synth_dataset
from cornac_amd import HPF, Dataset, ScoreException, _lib

pytestmark = pytest.mark.gpu

TABLES = ("G_s", "G_r", "L_s", "L_r")
K_EDGES = (1, 5, 8, 9, 32, 33, 64, 65, 130, 256)   # every lane-group width and slice edge
PSI_ZERO = 1.4616321449683623
ROW_SPLIT = 256   # ratings per segment of a long row (NMF's split plan)



def trainer_for(c):
    return _lib.MfTrainer(c["rid"], c["cid"], c["val"], c["nu"], c["ni"], c["k"])


def device_fit(c, n_iters, tables=None, calls=None):
    """(G_s, G_r, L_s, L_r, K_r, T_r), (group, rows_split) after n_iters from the case's start tables (or `tables`);
    calls: the iterations of each hpf_fit call"""
    tr = trainer_for(c)
    try:
        tr.hpf_set_tables(*(c["tables"] if tables is None else tables))
        for n in (calls or [n_iters]):
            tr.hpf_fit(n, c["hierarchical"])
        return tr.hpf_get_tables(), tr.hpf_form()
    finally:
        tr.close()


@functools.lru_cache(maxsize=None)
def restatement(kind, k, hier, n_iters):
    c = {"base": hc.base_case, "long": hc.long_rows_case}[kind](k, hier)
    out = hc.run_restatement(c, n_iters)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.fixture(scope="module")
def golden():
    return load_golden("hpf_ref")


# ---- 1. the expected-log step alone ----------------------------------------------------------------------------------
def elog_on_device(S, R, k):
    """S, R: flat arrays (a multiple of k long) as the user tables of a handle with one rating"""
    nu = len(S) // k
    one = np.full((1, k), 0.5)
    tr = _lib.MfTrainer(np.zeros(1, np.int64), np.zeros(1, np.int64), np.ones(1, np.float32), nu, 1, k)
    try:
        tr.hpf_set_tables(S.reshape(nu, k), R.reshape(nu, k), one, one)
        Lt, Lb = tr.hpf_elog()
    finally:
        tr.close()
    assert np.allclose(Lb, hc.elog(one, one), rtol=1e-14, atol=0)
    return Lt.ravel()


@pytest.mark.parametrize("k", [7, 64])
def test_expected_log_against_scipy(k):
    from scipy.special import digamma

    rs = np.random.RandomState(5 + k)
    edges = np.array([0.3, 1.0, np.nextafter(10.0, 0.0), 10.0, 0.05, 1e6])
    near = PSI_ZERO + rs.uniform(-1e-3, 1e-3, 20000)
    n = -(-(len(edges) + len(near) + 12000) // k) * k
    S = np.concatenate([edges, near, np.exp(rs.uniform(np.log(0.05), np.log(1e6), n - len(edges) - len(near)))])
    R = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), n))
    got = elog_on_device(S, R, k)
    want = hc.elog(S, R)
    bound = (np.abs(digamma(S)) + np.abs(np.log(R)) + 1.0 / S + 8.0) * 2.0 ** -50
    ratio = np.abs(got - want) / want / bound
    print("k=%d: %d elements, worst %.3f of the bound (at shape %.17g)" % (k, n, ratio.max(), S[ratio.argmax()]))
    assert np.isfinite(got).all() and (got > 0).all() and ratio.max() <= 1.0


def test_expected_log_of_tiny_shapes_underflows_to_zero():
    """PF's float32 gamma(0.3) draws reach 1e-24, where digamma is about -1e24: Lt = 0 by underflow, never NaN"""
    from scipy.special import digamma

    rs = np.random.RandomState(11)
    k, n = 5, 5 * 2000
    S = np.concatenate([[1e-24, 1e-30, 1e-3], 10.0 ** rs.uniform(-24, 0, n - 3)])
    R = np.exp(rs.uniform(np.log(1e-3), np.log(1e3), n))
    got = elog_on_device(S, R, k)
    want = hc.elog(S, R)
    assert np.isfinite(got).all() and (got >= 0).all()
    assert (want == 0).sum() > 100 and (got[want == 0] == 0).all() and got[0] == 0 and got[1] == 0
    normal = want > 1e-300
    bound = (np.abs(digamma(S)) + np.abs(np.log(R)) + 1.0 / S + 8.0) * 2.0 ** -50
    ratio = np.abs(got - want)[normal] / want[normal] / bound[normal]
    print("%d zeros, %d normal values at worst %.3f of the bound" % ((want == 0).sum(), normal.sum(), ratio.max()))
    assert normal.sum() > 100 and ratio.max() <= 1.0


# ---- 2. the device against the reference's compiled extension -------------------------------------------------------
@pytest.mark.parametrize("name", sorted(hc.GOLDEN_GIVEN))
def test_device_against_the_reference(golden, name):
    g = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    make, k, iters, hier = hc.GOLDEN_GIVEN[name]
    c = make(k, hier)
    assert all(np.array_equal(g[t + "0"], a) for t, a in zip(TABLES, c["tables"]))
    out, form = device_fit(c, iters)
    tol = hc.device_tolerance(name)
    diff = hc.max_rel_diff(out[:4], [g[t] for t in TABLES])
    print("%s: device vs reference %.3g (tolerance %.3g), form %r" % (name, diff, tol, form))
    assert tol <= hc.CEILING and diff <= tol
    assert ((out[4] == 1).all() and (out[5] == 1).all()) == (not hier)


# ---- 3. one iteration against the restatement -----------------------------------------------------------------------
def check_one_iteration(kind, k, hier):
    c = {"base": hc.base_case, "long": hc.long_rows_case}[kind](k, hier)
    want = restatement(kind, k, hier, 1)
    out, form = device_fit(c, 1)
    tol = hc.one_iteration_tolerance(hier)
    diff = hc.max_rel_diff(out, want)
    print("%s k=%d %s: device vs restatement %.3g (tolerance %.3g), form %r" % (kind, k, "hier" if hier else "pf", diff, tol, form))
    assert all(np.isfinite(a).all() and (a > 0).all() for a in out)
    assert form[0] == (8 if k <= 8 else 16 if k <= 16 else 32 if k <= 32 else 64)
    assert diff <= tol
    return c, out, form


@pytest.mark.parametrize("hier", [True, False])
@pytest.mark.parametrize("k", K_EDGES)
def test_one_iteration_at_every_group_width_and_slice_edge(k, hier):
    _, _, form = check_one_iteration("base", k, hier)
    assert form[1] == 0


@pytest.mark.parametrize("hier", [True, False])
@pytest.mark.parametrize("k", [5, 40])
def test_one_iteration_with_long_rows(k, hier):
    c, out, form = check_one_iteration("long", k, hier)
    cu, ci = np.bincount(c["rid"], minlength=c["nu"]), np.bincount(c["cid"], minlength=c["ni"])
    assert form[1] == (cu > ROW_SPLIT).sum() + (ci > ROW_SPLIT).sum() and form[1] >= 1, "item 3 (1000 raters) is split"
    assert (out[0][7] == hc.PRIOR).all() and (out[2][11] == hc.PRIOR).all(), "no ratings: exactly the prior"


# ---- 4. the same bits run to run, and across calls -------------------------------------------------------------------
@pytest.mark.parametrize("hier", [True, False])
def test_fits_repeat_bit_for_bit_and_chain_across_calls(hier):
    for c in (hc.base_case(5, hier), hc.long_rows_case(40, hier)):
        a, _ = device_fit(c, 3)
        b, _ = device_fit(c, 3)
        split, _ = device_fit(c, 3, calls=[1, 2])
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "two fits from the same tables differ"
        assert all(np.array_equal(x, y) for x, y in zip(a, split)), "1 + 2 iterations over two calls are not 3"
        moved = hc.max_rel_diff(a[:4], device_fit(c, 1)[0][:4])
        assert moved > 1e-6, "the later iterations changed nothing"


# ---- 5. refusals, and the handle's other state ------------------------------------------------------------------------
def test_k_257_is_refused_and_order_is_required():
    c = hc.base_case(5)
    one = np.ones((c["nu"], 257)), np.ones((c["ni"], 257))
    tr = _lib.MfTrainer(c["rid"], c["cid"], c["val"], c["nu"], c["ni"], 257)
    try:
        with pytest.raises(ValueError, match="256"):
            tr.hpf_set_tables(one[0], one[0], one[1], one[1])
        rc = _lib.lib().cornac_hip_mf_hpf_set_tables(tr.h, one[0].ctypes.data, one[0].ctypes.data, one[1].ctypes.data,
                                                     one[1].ctypes.data)
        assert rc == 1 and b"256" in _lib.lib().cornac_hip_last_error()
        with pytest.raises(_lib.HipError):
            tr.hpf_fit(1)
        assert tr.hpf_form() == (0, 0)
    finally:
        tr.close()
    tr = trainer_for(c)
    try:
        with pytest.raises(ValueError, match="strictly positive"):
            tr.hpf_set_tables(*[np.where(np.arange(t.size).reshape(t.shape) == 3, 0.0, t) for t in c["tables"]])
        with pytest.raises(_lib.HipError):
            tr.hpf_fit(1)   # before set_tables
    finally:
        tr.close()
    perm = np.random.RandomState(0).permutation(len(c["val"]))
    tr = _lib.MfTrainer(c["rid"][perm], c["cid"][perm], c["val"][perm], c["nu"], c["ni"], 5)
    try:
        tr.hpf_set_tables(*c["tables"])
        with pytest.raises(_lib.HipError, match="stored by user"):
            tr.hpf_fit(1)
    finally:
        tr.close()


def test_an_hpf_fit_leaves_the_nmf_state_of_the_handle_alone():
    c, n = hc.base_case(15), nc.base_case(15)
    assert np.array_equal(c["rid"], n["rid"])
    hyper = (n["lr"], n["lambda_u"], n["lambda_v"], n["lambda_bu"], n["lambda_bi"], 0.0)
    tr = trainer_for(c)
    try:
        tr.nmf_set_factors(n["U"], n["V"])
        tr.nmf_fit(1, *hyper, False, _lib.MODE_HOGWILD)
        before = tr.nmf_get_factors()
        tr.hpf_set_tables(*c["tables"])
        tr.hpf_fit(2, True)
        assert all(np.array_equal(a, b) for a, b in zip(before, tr.nmf_get_factors()))
        hpf_before = tr.hpf_get_tables()
        tr.nmf_fit(1, *hyper, False, _lib.MODE_HOGWILD)
        assert all(np.array_equal(a, b) for a, b in zip(hpf_before, tr.hpf_get_tables())), "and the reverse"
        two = tr.nmf_get_factors()
    finally:
        tr.close()
    tr = trainer_for(c)
    try:
        tr.nmf_set_factors(n["U"], n["V"])
        tr.nmf_fit(2, *hyper, False, _lib.MODE_HOGWILD)
        assert all(np.array_equal(a, b) for a, b in zip(two, tr.nmf_get_factors())), "NMF continued as if HPF had not run"
    finally:
        tr.close()
    want, _ = device_fit(c, 2)
    assert all(np.array_equal(a, b) for a, b in zip(hpf_before, want)), "HPF on a handle that NMF used first"


# ---- 6. end to end ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hier", [True, False])
def test_end_to_end_through_the_class(hier):
    ds = synth_dataset(60, 40, 700, seed=4)
    m = HPF(k=5, max_iter=5, seed=123, hierarchical=hier).fit(ds)
    X = ds.matrix
    rid = np.repeat(np.arange(ds.num_users), np.diff(X.indptr))
    start = hc.draw_tables(ds.num_users, ds.num_items, 5, hier, np.random.RandomState(123))
    want = hc.hpf_fit(rid, X.indices, X.data.astype(np.float32), *start, 5, hier)
    tol = hc.device_tolerance("hier_small" if hier else "pf_small")   # the same shape class and iteration count
    diff = hc.max_rel_diff((m.Gs, m.Gr, m.Ls, m.Lr, m.Theta, m.Beta), want[:4] + (want[0] / want[1], want[2] / want[3]))
    print("end to end %s: device vs restatement %.3g (tolerance %.3g)" % ("hier" if hier else "pf", diff, tol))
    assert diff <= tol
    assert np.array_equal(m.Theta, m.Gs / m.Gr) and np.array_equal(m.Beta, m.Ls / m.Lr)
    s = m.score(7)
    ref = m.Beta @ m.Theta[7]
    assert s.dtype == np.float64 and np.allclose(s, ref, rtol=1e-13, atol=0)
    assert m.score(7, 11) == m.Beta[11].dot(m.Theta[7])
    with pytest.raises(ScoreException):
        m.score(ds.num_users)
    with pytest.raises(ScoreException):
        m.score(0, ds.num_items)
    ranked, scores = m.rank(7)
    assert np.array_equal(scores, s) and len(ranked) == ds.num_items
    assert (np.diff(s[ranked]) <= 0).all() and sorted(ranked) == list(range(ds.num_items))


@pytest.mark.parametrize("name", sorted(hc.GOLDEN_SEEDED))
def test_seeded_golden_case_through_the_device(golden, name):
    g = {k[len(name) + 1:]: v for k, v in golden.items() if k.startswith(name + "/")}
    k, iters, seed, hier = hc.GOLDEN_SEEDED[name]
    data = Dataset.from_arrays(g["rid"], g["cid"], g["val"], num_users=int(g["nu"]), num_items=int(g["ni"]))
    m = HPF(k=k, max_iter=iters, seed=seed, hierarchical=hier).fit(data)
    tol = hc.device_tolerance("hier_small" if hier else "pf_small")   # the seeded case's cells and iteration count
    diff = hc.max_rel_diff((m.Theta, m.Beta, m.Gs, m.Gr, m.Ls, m.Lr), [g[t] for t in ("Z", "W") + TABLES])
    print("%s: device vs reference %.3g (tolerance %.3g)" % (name, diff, tol))
    assert diff <= tol
