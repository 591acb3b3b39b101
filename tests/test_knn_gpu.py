"""KNN on the device, through the C ABI (`_lib.KnnSimilarity`, `_lib.KnnScorer`) and through cornac_amd.UserKNN / ItemKNN,
against (a) the float64 restatement of tests/knn_cases.py and (b) what the reference's own models wrote into
tests/golden/knn_ref.npz (tests/test_knn_cpu.py holds (a) against (b)).

Similarity: bit for bit, the sparsity pattern included — the device sums every entry in the reference's order, rounds *, +,
sqrt and / separately and divides by sqrt(d1 * d2) (tolerance: knn_cases.device_similarity_tolerance, 0 for every golden
configuration).  Scores: within knn_cases.score_tolerance, (k + 2) 2^-51 (max|rating| + max|mean|), derived there; pairs
and repeated calls bit for bit.  Every check prints the measured difference next to its tolerance.

Measured on an MI355X: every similarity table 0 from the restatement and from the golden (pattern and bits), for every
rows_per_pass; the amplified table 0 ulp from the golden (allowed: 2); scores from the golden's tables and end to end at
most 8.9e-16 against bounds of 1.2e-14 (k = 1) .. 2.1e-13 (k = 50); the edge tables against the replay at most 6.7e-16
against 4.3e-15 .. 9.6e-14, with 8 .. 75 boundary ties among the first 160 outputs of each k."""
import numpy as np
import pytest
import scipy.sparse as sp

import knn_cases as kc
from conftest import load_golden
from cornac_amd import Dataset, ItemKNN, UserKNN, _lib

golden_case, dataset, make_model = kc.golden_case, kc.dataset, kc.make_model

pytestmark = pytest.mark.gpu

MAX_K = _lib.KNN_MAX_K
ALL_KS = kc.KS + (MAX_K,)


@pytest.fixture(scope="module")
def golden():
    return load_golden("knn_ref")


def device_similarity(W, rows_per_pass=0, runs=1):
    sim = _lib.KnnSimilarity(W)
    try:
        out = [sim.run(rows_per_pass) for _ in range(runs)]
        return out[0] if runs == 1 else out
    finally:
        sim.close()


# ---- similarity through the ABI --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge():
    W = kc.edge_matrix()
    T = W.T.tocsr()
    T.sort_indices()
    return {"wide": (W, kc.similarity(W)), "tall": (T, kc.similarity(T))}


@pytest.mark.parametrize("which", ["wide", "tall"])
def test_similarity_edges_bit_for_bit(edge, which):
    """row (wide) and column (tall) lengths 1, 63, 64, 65, 256, 257; an empty row and an empty column; stored zeros; two
    rows whose products cancel exactly: no entry"""
    W, want = edge[which]
    lengths = set(np.diff(W.indptr if which == "wide" else W.T.tocsr().indptr))
    assert {0, 1, 63, 64, 65, 256, 257} <= lengths and (W.data == 0).sum() > 10
    assert 0 in set(np.diff(W.T.tocsr().indptr)) and 0 in set(np.diff(W.indptr))
    first, second = device_similarity(W, runs=2)
    print("%s: %d entries; device vs restatement %.3g relative (allowed: 0)" % (which, first.nnz, kc.max_rel_diff(
        first.data, want.data) if first.nnz == want.nnz else np.inf))
    assert kc.same_csr(first, want), "the restatement's bits and pattern"
    assert kc.same_csr(second, first), "a second run has the same bits"
    assert first.has_sorted_indices and (first.data != 0).all()
    if which == "wide":
        assert want[65, 66] == 0 and first[65, 66] == 0 and first[65, 65] == 1.0
        assert first.indptr[1] == first.indptr[0], "the empty row has no entries, not even its diagonal"


@pytest.mark.parametrize("rows_per_pass", [0, 1, 7, 64, 100])
def test_similarity_passes_give_the_same_bits(edge, rows_per_pass):
    W, want = edge["wide"]
    assert W.shape[0] == 67
    assert kc.same_csr(device_similarity(W, rows_per_pass), want)


@pytest.mark.parametrize("name", sorted(kc.CONFIGS))
def test_similarity_vs_the_golden(golden, name):
    g = golden_case(golden, name)
    got = device_similarity(kc.prepare_config(name)[0])
    assert np.array_equal(got.indptr, g["sim0"].indptr) and np.array_equal(got.indices, g["sim0"].indices), "sparsity pattern"
    diff, tol = kc.max_rel_diff(got.data, g["sim0"].data), kc.device_similarity_tolerance(name)
    print("%s: device vs reference %.3g relative (allowed: %.3g)" % (name, diff, tol))
    assert diff <= tol
    assert kc.same_csr(got, kc.similarity(kc.prepare_config(name)[0]))


def test_similarity_refuses_bad_tables():
    W = sp.csr_matrix(np.array([[1.0, 2.0], [0.0, 3.0]]))
    W.indices[:2] = [1, 0]
    W.has_sorted_indices = True
    with pytest.raises(_lib.HipError, match="sorted indices"):
        _lib.KnnSimilarity(W)
    sim = _lib.KnnSimilarity(sp.csr_matrix(np.eye(3)))
    with pytest.raises(_lib.HipError, match="rows_per_pass"):
        sim.run(-1)
    sim.close()


# ---- scoring through the ABI -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.CONFIGS))
def test_scores_from_the_goldens_tables(golden, name):
    g = golden_case(golden, name)
    cname, model, _ = kc.CONFIGS[name]
    c = kc.case(cname)
    N, Q, user_mode = kc.tables(model, g["sim"], g["rat"])
    users, (pu, pi) = kc.score_users(c), kc.score_pairs(c)
    sc = _lib.KnnScorer(N, Q, user_mode)
    try:
        for a, k in enumerate(ALL_KS):
            tol = kc.score_tolerance(k, np.abs(g["r"]).max(), np.abs(g["mean_arr"]).max())
            got = g["mean_arr"][users][:, None] + sc.score_users(users, k)
            pairs = g["mean_arr"][pu] + sc.score_pairs(pu, pi, k)
            if k in kc.KS:
                want, want_pairs = g["scores"][a], g["pair_scores"][a]
            else:   # beyond the golden's k: the heap replay over the golden's tables
                want = np.array([g["mean_arr"][u] + kc.score_row(N, Q, int(u), user_mode, k) for u in users])
                want_pairs = None
            diff = np.abs(got - want).max()
            print("%s, k = %d: device vs reference %.3g (allowed: %.3g)" % (name, k, diff, tol))
            assert diff <= tol
            if want_pairs is not None:
                assert np.abs(pairs - want_pairs).max() <= tol
            full = sc.score_users(pu, k)
            assert np.array_equal(sc.score_pairs(pu, pi, k), full[np.arange(len(pu)), pi]), "pairs have the full row's bits"
    finally:
        sc.close()


@pytest.fixture(scope="module")
def scoring_edge():
    return kc.scoring_edge_case()


@pytest.mark.parametrize("user_mode", [True, False])
def test_scoring_edges_against_the_replay(scoring_edge, user_mode):
    """k below, at and above the number of candidates (user 0 has exactly 1, 3, 5, 20, 50, 64 candidates in rows 3 .. 8); an
    item without entries and one without candidates; negative weights; a row of 300 entries; a table that is not symmetric
    (not even square); stored zeros of Q are no candidates"""
    N, Q = scoring_edge
    assert N.shape[0] != N.shape[1] and np.diff(N.indptr).max() == 300 and (Q.data == 0).sum() > 100
    assert (N.data < 0).any() and (Q.data < 0).any()
    v0 = np.asarray(Q[0].todense()).ravel()
    n_cand = [len(kc.candidates(N.indices[N.indptr[i]:N.indptr[i + 1]], N.data[N.indptr[i]:N.indptr[i + 1]], v0, user_mode))
              for i in range(N.shape[0])]
    assert n_cand[0] == 0 and n_cand[1] > MAX_K and n_cand[2] == 0 and n_cand[3:9] == [1, 3, 5, 20, 50, 64]
    users = np.arange(Q.shape[0])
    rating = max(np.abs(N.data).max(), np.abs(Q.data).max())
    sc = _lib.KnnScorer(N, Q, user_mode)
    try:
        for k in ALL_KS:
            got = sc.score_users(users, k)
            want = np.array([kc.score_row(N, Q, int(u), user_mode, k) for u in users])
            tol = kc.score_tolerance(k, rating, 0.0)
            ties = sum(kc.boundary_ties(N, Q, int(u), user_mode, k) for u in users[:10])
            diff = np.abs(got - want).max()
            print("user_mode = %s, k = %d: device vs replay %.3g (allowed: %.3g); %d boundary ties among the first 160 outputs"
                  % (user_mode, k, diff, tol, ties))
            assert diff <= tol
            assert (got[0, [0, 2]] == 0).all(), "no candidates: exactly 0"
            assert np.array_equal(sc.score_users(users, k), got), "a second run has the same bits"
    finally:
        sc.close()


def test_batches_of_1_and_65_with_a_repeated_user(golden):
    g = golden_case(golden, "B/user_cosine")
    N, Q, user_mode = kc.tables("user", g["sim"], g["rat"])
    sc = _lib.KnnScorer(N, Q, user_mode)
    try:
        users = np.array(list(range(40, 104)) + [43])
        many = sc.score_users(users, 20)
        assert many.shape == (65, 100) and np.array_equal(many[3], many[64]), "the repeated user's two rows"
        assert np.array_equal(sc.score_users([43], 20)[0], many[3]), "a batch of one has the batch's bits"
        for bad_k in (0, MAX_K + 1):
            with pytest.raises(_lib.HipError, match="CORNAC_HIP_KNN_MAX_K"):
                sc.score_users([0], bad_k)
        with pytest.raises(_lib.HipError, match="out of range"):
            sc.score_users([150], 5)
        with pytest.raises(_lib.HipError, match="out of range"):
            sc.score_pairs([0], [100], 5)
        assert sc.score_users([], 5).shape == (0, 100)
    finally:
        sc.close()


def test_more_pairs_than_one_chunk_holds(golden):
    """the chunk loop past its first chunk (b0 > 0): a chunk's dense rows of Q take at most 64 MiB, 8 n_neighbours bytes per
    id, which is 55 924 ids at 150 neighbours, so one more pair makes a second chunk of one.  (score_users shares the loop;
    that many users there would be millions of one-wave workgroups.)"""
    g = golden_case(golden, "B/user_cosine")
    N, Q, user_mode = kc.tables("user", g["sim"], g["rat"])
    n_items, n_neighbours, n_users = N.shape[0], N.shape[1], Q.shape[0]
    cap = (64 << 20) // (8 * n_neighbours)
    n = cap + 1
    assert n > cap >= 1, "more than one chunk's worth"
    pu, pi = np.arange(n) % n_users, (np.arange(n) // n_users) % n_items
    sc = _lib.KnnScorer(N, Q, user_mode)
    try:
        everyone = sc.score_users(np.arange(n_users), 20)
        pairs = sc.score_pairs(pu, pi, 20)
    finally:
        sc.close()
    assert pairs.shape == (n,) and np.array_equal(pairs.view(np.uint64), everyone[pu, pi].view(np.uint64))


# ---- end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(kc.CONFIGS))
def test_fit_and_score_against_the_golden(golden, name):
    g = golden_case(golden, name)
    cname, model, kw = kc.CONFIGS[name]
    c = kc.case(cname)
    amplified = kw.get("amplify", 1.0) != 1.0
    m = make_model(name).fit(dataset(name))
    assert np.array_equal(m.mean_arr, g["mean_arr"])
    assert np.array_equal(m.sim_mat.indptr, g["sim"].indptr) and np.array_equal(m.sim_mat.indices, g["sim"].indices)
    if amplified:
        ulps = kc.ulp_diff(m.sim_mat.data, g["sim"].data)
        print("%s: amplified table %d ulp from the golden (allowed: 2)" % (name, ulps))
        assert ulps <= 2
    else:
        assert kc.same_csr(m.sim_mat, g["sim"]), "every table without amplify is the golden's bit for bit"
    users, (pu, pi) = kc.score_users(c), kc.score_pairs(c)
    for own_table in ((True, False) if not amplified else (False,)):
        if not own_table:
            m.sim_mat = g["sim"]
        for a, k in enumerate(kc.KS):
            m.k = k
            tol = kc.score_tolerance(k, np.abs(g["r"]).max(), np.abs(g["mean_arr"]).max())
            got = m.score_batch(users)
            diff = np.abs(got - g["scores"][a]).max()
            print("%s, %s table, k = %d: score vs reference %.3g (allowed: %.3g)" % (name, "own" if own_table else "golden's", k,
                                                                                     diff, tol))
            assert diff <= tol
            assert np.array_equal(m.score(int(users[3])), got[3])
            pairs = np.array([m.score(int(u), int(i)) for u, i in zip(pu[:5], pi[:5])])
            assert np.abs(pairs - g["pair_scores"][a, :5]).max() <= tol


@pytest.mark.parametrize("cls", [UserKNN, ItemKNN])
def test_rank_orders_score_under_the_pinned_tie_rule(cls):
    c = kc.case("Ai")
    ds = Dataset.from_arrays(c["u"], c["i"], c["r"], num_users=c["nu"], num_items=c["ni"])
    m = cls(k=3, verbose=False).fit(ds)
    s = m.score(2)
    assert len(np.unique(s)) < len(s), "implicit data: tied scores"
    ranked, scores = m.rank(2, k=10)
    assert np.array_equal(scores, s) and len(ranked) == 40
    assert np.array_equal(ranked, np.lexsort((np.arange(40), s))[::-1]), "descending score, ties by descending item index"
    again = pickle_round_trip(m)
    assert np.array_equal(again.score(2), s)


def pickle_round_trip(m):
    import pickle

    return pickle.loads(pickle.dumps(m))
