"""MMMF on the MI355X (csrc/mmmf.inc): deterministic mode bit for bit against the restatement of the reference's loop
(tests/mmmf_cases.py, itself held to the reference's compiled loop by tests/test_mmmf_cpu.py), the entry points' argument
checks, one hogwild launch per kernel instantiation against the float64 step (launches Z / A / B of mmmf_cases), a whole
hogwild fit against the seed-to-seed band of the float64 restatement, and the model class."""
import functools

import numpy as np
import pytest

import mmmf_cases as mc
from conftest import synth_dataset
from cornac_amd import MMMF, Dataset, _lib, synth
from cornac_amd import eval as ev
from cornac_amd import metrics as mm
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

NU, NI, NNZ, EXTRA = 300, 200, 3000, 7  # EXTRA item rows beyond n_items: total_items > n_items
LR, REG = 0.05, 0.01


@functools.lru_cache(maxsize=1)
def _csr():
    users, items = synth.zipf_interactions(NU, NI, NNZ, 0.8, 5)
    return synth.csr_from_sorted(users, items, NU)


def _start(k, dtype):
    rs = np.random.RandomState(40 + k)
    s = (0.25 / k) ** 0.25  # scores of unit spread (bpr_step_cases._tables): both branches are taken
    return (rs.normal(0, s, (NU, k)).astype(np.float32).astype(dtype), rs.normal(0, s, (NI + EXTRA, k)).astype(np.float32).astype(dtype),
            rs.normal(0, 0.5, NI + EXTRA).astype(np.float32).astype(dtype))


def _trainer(k):
    indptr, indices = _csr()
    return _lib.BprTrainer(indptr, indices, NU, NI, NU, NI + EXTRA, k)


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _deterministic(k, dtype, oracle):
    indptr, indices = _csr()
    start = _start(k, dtype)
    want = [t.copy() for t in start]
    stats = mc.mmmf_fit(indptr, indices, NI, *want, LR, REG, 2, oracle.MT19937(101), oracle.MT19937(202))
    tr = _trainer(k)
    try:
        tr.seed_mt19937(101, 202)
        if dtype == np.float64:
            tr.set_factors_f64(*start)
            got_stats = [tr.mmmf_fit_epochs_f64(1, LR, REG) for _ in range(2)]
            got = tr.get_factors_f64()
        else:
            tr.set_factors(*start)
            got_stats = [tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_DETERMINISTIC) for _ in range(2)]
            got = tr.get_factors()
    finally:
        tr.close()
    assert got_stats == stats, "per-epoch (correct, skipped): device %s, restatement %s" % (got_stats, stats)
    for tab, g, w, s in zip("UVB", got, want, start):
        assert _bits_equal(g, w), "k = %d, table %s: max |diff| %g" % (k, tab, np.abs(g - w).max())
        assert not np.array_equal(g, s), "the run did not move table %s" % tab
    assert _bits_equal(got[1][NI:], start[1][NI:]) and _bits_equal(got[2][NI:], start[2][NI:]), "rows beyond num_items moved"
    share = stats[0][0] / (NNZ - stats[0][1])
    assert 0.1 < share < 0.9, "both branches must be taken (correct share %.2f)" % share


@pytest.mark.parametrize("k", (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 256, 257))
def test_deterministic_mode_is_the_restatement_bit_for_bit(oracle, k):
    _deterministic(k, np.float32, oracle)


@pytest.mark.parametrize("k", (5, 33, 65, 257))
def test_deterministic_float64_is_the_restatement_bit_for_bit(oracle, k):
    _deterministic(k, np.float64, oracle)


def test_epochs_chain_zero_epochs_move_nothing_and_bad_arguments_are_refused():
    k = 8
    start = _start(k, np.float32)
    tr = _trainer(k)
    try:
        tr.set_factors(*start)
        # unseeded modes
        for mode in (_lib.MODE_DETERMINISTIC, _lib.MODE_HOGWILD):
            with pytest.raises(_lib.HipError, match="seed"):
                tr.mmmf_fit_epochs(1, LR, REG, mode)
        with pytest.raises(_lib.HipError, match="seed"):
            tr.mmmf_hogwild_enqueue(64, LR, REG)
        tr.seed_mt19937(11, 12)
        tr.seed_hogwild(99)
        with pytest.raises(_lib.HipError, match="n_epochs"):
            tr.mmmf_fit_epochs(-1, LR, REG, _lib.MODE_DETERMINISTIC)
        with pytest.raises(_lib.HipError, match="unknown mode"):
            tr.mmmf_fit_epochs(1, LR, REG, 7)
        with pytest.raises(_lib.HipError, match="float64"):
            tr.mmmf_fit_epochs_f64(1, LR, REG)  # float32 tables
        # 0 epochs move nothing, in both modes
        for mode in (_lib.MODE_DETERMINISTIC, _lib.MODE_HOGWILD):
            assert tr.mmmf_fit_epochs(0, LR, REG, mode) == (0, 0)
        tr.mmmf_hogwild_enqueue(0, LR, REG)
        assert tr.sync() == (0, 0)
        assert all(_bits_equal(a, b) for a, b in zip(tr.get_factors(), start))
        # deterministic: 1 + 2 epochs in two calls == 3 in one, tables and counters
        a = tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_DETERMINISTIC) + tr.mmmf_fit_epochs(2, LR, REG, _lib.MODE_DETERMINISTIC)
        split = tr.get_factors()
        tr.set_factors(*start)
        tr.seed_mt19937(11, 12)
        b = tr.mmmf_fit_epochs(3, LR, REG, _lib.MODE_DETERMINISTIC)
        assert (a[0] + a[2], a[1] + a[3]) == b and all(_bits_equal(x, y) for x, y in zip(split, tr.get_factors()))
        # hogwild: the sample counter runs on across calls (the skip count is a function of the samples alone)
        tr.set_factors(*start)
        tr.seed_hogwild(99)
        s12 = tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_HOGWILD)[1] + tr.mmmf_fit_epochs(2, LR, REG, _lib.MODE_HOGWILD)[1]
        tr.seed_hogwild(99)
        tr.mmmf_hogwild_enqueue(NNZ // 3, LR, REG)
        tr.mmmf_hogwild_enqueue(3 * NNZ - NNZ // 3, LR, REG)
        assert tr.sync()[1] == s12
        timing = tr.last_timing()
        assert timing is not None
        # a negative population on the handle
        tr.set_negative_population(np.arange(NI, dtype=np.int32))
        for call in (lambda: tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_HOGWILD), lambda: tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_DETERMINISTIC),
                     lambda: tr.mmmf_hogwild_enqueue(64, LR, REG)):
            with pytest.raises(_lib.HipError, match="negative population"):
                call()
        tr.set_negative_population(np.zeros(0, np.int32))
        # float64 tables: the float32 entry points refuse
        tr.set_factors_f64(*(t.astype(np.float64) for t in start))
        with pytest.raises(_lib.HipError, match="float64"):
            tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_DETERMINISTIC)
        with pytest.raises(_lib.HipError, match="float64"):
            tr.mmmf_hogwild_enqueue(64, LR, REG)
        assert tr.mmmf_fit_epochs_f64(0, LR, REG) == (0, 0)
        with pytest.raises(_lib.HipError, match="n_epochs"):
            tr.mmmf_fit_epochs_f64(-1, LR, REG)
    finally:
        tr.close()
    # a conveyor-configured handle (its item tables may be gone: refused before anything is launched)
    # (on the interactions of the step cases, a shape whose LDS-bin tables the BPR step tests build as well)
    indptr, indices = mc.bc._data(20_000, 30_720, 300_000, 0.8, 1.0)
    tr = _lib.BprTrainer(indptr, indices, 20_000, 30_720, 20_000, 30_720, 16)
    try:
        tr.seed_mt19937(11, 12)
        tr.seed_hogwild(99)
        tr.conveyor_setup(1, None, 4242)
        for call in (lambda: tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_HOGWILD), lambda: tr.mmmf_fit_epochs(1, LR, REG, _lib.MODE_DETERMINISTIC),
                     lambda: tr.mmmf_hogwild_enqueue(64, LR, REG)):
            with pytest.raises(_lib.HipError, match="conveyor"):
                call()
    finally:
        tr.close()


# ---- hogwild, one launch --------------------------------------------------------------------------------------------------
def _launch(tr, c, lr):
    tr.set_factors(*c.tables)
    tr.seed_hogwild(c.seed)
    tr.mmmf_hogwild_enqueue(c.s_begin, 0.0, 0.0)  # moves the sample counter to s_begin (launch Z shows that lr = 0 moves nothing)
    tr.sync()
    tr.mmmf_hogwild_enqueue(c.n, lr, mc.REG if lr else 0.0)
    correct, skipped = tr.sync()
    return tr.get_factors(), correct, skipped


@pytest.mark.parametrize("name", mc.NAMES)
def test_hogwild_launch_matches_the_float64_step(oracle, name):
    c = mc.case(name)
    tr = _lib.BprTrainer(c.indptr, c.indices, c.nu, c.ni, c.nu, c.total_items, c.k)
    try:
        tr.kernel_timing(True)
        got, correct, skipped = _launch(tr, c, 0.0)
        z = mc.check_z(c, got, correct, skipped)
        a = mc.check_a(c, _launch(tr, c, mc.LR_A)[0])
        b = mc.check_b(c, _launch(tr, c, mc.LR_B)[0])
        ms, launches = tr.kernel_timing(False)
        assert launches == 6 and ms > 0, "kernel timing covers the MMMF launches"
    finally:
        tr.close()
    print("\n%s: %d triplets, correct %d in [%d, %d]; A violator clean-row error U %.3g V %.3g B %.3g (T_CLEAN %.3g); "
          "B error / tolerance U %.3g V %.3g B %.3g (C %.3g)" % (
              name, len(c.trip[0]), z["correct"], z["lo"], z["hi"], a["U"], a["V"], a["B"], mc.T_CLEAN, b["U"], b["V"], b["B"],
              mc.C[name]))


# ---- hogwild, whole fit ---------------------------------------------------------------------------------------------------
def test_hogwild_fit_lands_in_the_restatements_seed_to_seed_band():
    nu, ni, nnz, k, epochs = 2000, 1000, 30000, 16, 5
    users, items = synth.zipf_interactions(nu, ni, nnz, 0.8, 11)
    indptr, indices = synth.csr_from_sorted(users, items, nu)
    rs = np.random.RandomState(77)
    U0 = ((rs.uniform(0, 1, (nu, k)).astype(np.float32) - 0.5) / k)
    V0 = ((rs.uniform(0, 1, (ni, k)).astype(np.float32) - 0.5) / k)
    B0 = np.zeros(ni, np.float32)
    # the probe: 20 000 interactions, each paired with an item its user has not interacted with
    pr = np.random.RandomState(78)
    pos = pr.randint(0, nnz, 40000)
    neg = pr.randint(0, ni, 40000)
    member = orc._csr_has(indptr, indices, ni, users[pos], neg)
    pos, neg = pos[~member][:20000], neg[~member][:20000]
    assert len(pos) == 20000
    pu, pi = users[pos], items[pos]

    def share(U, V, B):
        U, V, B = (np.asarray(t, np.float64) for t in (U, V, B))
        x = B[pi] - B[neg] + (U[pu] * (V[pi] - V[neg])).sum(axis=1)
        return float((x > 0).mean())

    ref = []
    for seed in (1, 2, 3, 4):
        U, V, B = (t.astype(np.float64) for t in (U0, V0, B0))
        mc.mmmf_fit(indptr, indices, ni, U, V, B, LR, REG, epochs, rng=np.random.RandomState(seed))
        ref.append(share(U, V, B))
    lo, hi = min(ref), max(ref)
    s = hi - lo
    tr = _lib.BprTrainer(indptr, indices, nu, ni, nu, ni, k)
    try:
        tr.set_factors(U0, V0, B0)
        tr.seed_hogwild(0xC0FFEE)
        correct, skipped = tr.mmmf_fit_epochs(epochs, LR, REG, _lib.MODE_HOGWILD)
        got = share(*tr.get_factors())
    finally:
        tr.close()
    print("\nprobe share x > 0: untrained %.4f, restatement seeds %s (lo %.4f, hi %.4f, spread %.4f), device %.4f; device "
          "correct %.3f skipped %.3f of the samples" % (share(U0, V0, B0), ["%.4f" % r for r in ref], lo, hi, s, got,
                                                      correct / (epochs * nnz - skipped), skipped / (epochs * nnz)))
    assert lo - s <= got <= hi + s


# ---- model level ------------------------------------------------------------------------------------------------------------
def test_model_fit_score_rank_and_batched_evaluation(oracle):
    ds = synth_dataset(120, 80, 1500, seed=6)
    m = MMMF(k=10, max_iter=2, seed=123).fit(ds)
    assert m.effective_mode == "deterministic"
    rs = np.random.RandomState(123)
    U = ((rs.uniform(0, 1, (ds.num_users, 10)).astype(np.float32) - 0.5) / 10)
    V = ((rs.uniform(0, 1, (ds.num_items, 10)).astype(np.float32) - 0.5) / 10)
    B = np.zeros(ds.num_items, np.float32)
    sp, sn = (oracle.rngvector_seed(rs.randint(2 ** 31)) for _ in range(2))
    X = ds.matrix
    stats = mc.mmmf_fit(X.indptr, X.indices, ds.num_items, U, V, B, 0.001, 0.01, 2, oracle.MT19937(sp), oracle.MT19937(sn))
    for a, b, name in zip((m.u_factors, m.i_factors, m.i_biases), (U, V, B), "UVB"):
        assert _bits_equal(a, b), "%s: max |diff| %g" % (name, np.abs(a - b).max())
    assert m.fit_stats == [(sum(c for c, _ in stats), sum(s for _, s in stats))]
    assert m._scorer_row_count() == ds.num_users
    for u in (0, 17, ds.num_users - 1):
        want = B + V.astype(np.float64) @ U[u].astype(np.float64)
        got = m.score(u)
        assert got.dtype == np.float32 and np.allclose(got, want, rtol=1e-5, atol=1e-7)
        ranked, scores = m.rank(u, k=10)
        assert np.array_equal(scores, got) and len(ranked) == ds.num_items
        assert np.array_equal(ranked[:10], np.lexsort((np.arange(ds.num_items), got))[::-1][:10])
    users, items = ds.user_ids, ds.item_ids
    test = Dataset.build([(users[u], items[i], 5.0) for u in range(0, ds.num_users, 7) for i in (5, 20, 60)],
                         global_uid_map=ds.uid_map, global_iid_map=ds.iid_map, seed=1)
    metrics = lambda: [mm.Recall(k=20), mm.NDCG(k=20), mm.AUC()]  # noqa: E731
    avg, _ = ev.ranking_eval(m, metrics(), ds, test)
    plain = type("PlainModel", (), {"rank": lambda self, **kw: m.rank(**kw)})()
    avg2, _ = ev.ranking_eval(plain, metrics(), ds, test)
    assert np.allclose(avg, avg2, atol=1e-9) and all(np.isfinite(avg))


def test_float64_init_params_train_and_score_in_double(oracle):
    ds = synth_dataset(120, 80, 1500, seed=6)
    rs = np.random.RandomState(2)
    init = lambda: {"U": rs.normal(0, 0.3, (ds.num_users, 6)), "V": rs.normal(0, 0.3, (ds.num_items, 6)),  # noqa: E731
                    "Bi": np.zeros(ds.num_items)}
    ip = init()
    want = [a.copy() for a in (ip["U"], ip["V"], ip["Bi"])]
    m = MMMF(k=6, max_iter=2, learning_rate=0.05, seed=9, mode="hogwild", init_params=ip).fit(ds)  # (double: sequential whatever the mode)
    g = np.random.RandomState(9)
    sp, sn = (oracle.rngvector_seed(g.randint(2 ** 31)) for _ in range(2))
    X = ds.matrix
    mc.mmmf_fit(X.indptr, X.indices, ds.num_items, *want, 0.05, 0.01, 2, oracle.MT19937(sp), oracle.MT19937(sn))
    assert m.u_factors is ip["U"] and m.u_factors.dtype == np.float64
    for a, b in zip((m.u_factors, m.i_factors, m.i_biases), want):
        assert _bits_equal(a, b)
    s = m.score(3)
    assert s.dtype == np.float64 and np.allclose(s, m.i_biases + m.i_factors @ m.u_factors[3], rtol=1e-12, atol=1e-15)
    ranked, _ = m.rank(3)
    assert np.all(np.diff(s[ranked]) <= 0)
