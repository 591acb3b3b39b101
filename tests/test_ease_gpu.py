"""EASE on the device, through the C ABI (`_lib.EaseModel`) and through cornac_amd.EASE, against (a) the float64 restatement
of tests/ease_cases.py and (b) what the reference's own EASE wrote into tests/golden/ease_ref.npz (tests/test_ease_cpu.py
holds (a) against (b)).

Gram matrix and scores: bit for bit (the device sums in SciPy's order and rounds * and + separately).  Weights: within 16
times the restatement's own distance to the same reference (floor: one unit in the last place of max|B|), and that
tolerance under CEILING = 8 n 2^-52 kappa_2 max|B| (ease_cases.py).  Every check prints the measured difference next to its
tolerance.  No table is larger than 257 x 257.

Measured on an MI355X: Gram matrix and scores 0 from the restatement and from the golden everywhere; B against the golden
1.25e-16 .. 2.11e-15 (tolerances 2.0e-15 .. 4.4e-14, CEILINGs 3.4e-14 .. 3.8e-11); at the sizes 1 .. 257 the device is 0
from the restatement up to one block and at most 4.4e-16 beyond, and at most 8.9e-16 (lamb 0.5; tolerances 9.8e-15 ..
1.6e-14) and 1.9e-16 (lamb 500; 1.3e-15 .. 2.9e-15) from NumPy's formula; end-to-end scores at most 0.65 % of their bound."""
import functools

import numpy as np
import pytest

import ease_cases as ec
from conftest import load_golden
from cornac_amd import EASE, _lib

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 129, 257)   # under one block, one block, one plus one, two plus one, four plus one
LAMBS = (0.5, 500.0)


@pytest.fixture(scope="module")
def golden():
    return load_golden("ease_ref")


class handle:
    """a device model that is closed when the block ends"""

    def __init__(self, X):
        self.m = _lib.EaseModel(X)

    def __enter__(self):
        return self.m

    def __exit__(self, *exc):
        self.m.close()


# ---- Gram ----------------------------------------------------------------------------------------------------------------
def test_gram_edges_bit_for_bit():
    """real values, 257 items, column lengths 0, 1, 63, 64, 65, 256, an empty user row, stored zeros"""
    X = ec.edge_matrix()
    want = ec.gram(X)
    with handle(X) as m:
        m.gram()
        first = m.get_table()
        m.gram()
        second = m.get_table()
    print("edge matrix: device G vs restatement: max difference %.3g (allowed: 0); second run %.3g (allowed: 0)" % (
        np.abs(first - want).max(), np.abs(second - first).max()))
    assert ec.same_bits(first, want) and ec.same_bits(second, first)
    assert (first[0] == 0).all() and (first[:, 0] == 0).all(), "an item nobody rated"


@pytest.mark.parametrize("cname", ec.GRAM_CASES)
def test_gram_is_the_goldens(golden, cname):
    g = ec.golden_config(golden, next(n for n in sorted(ec.CONFIGS) if ec.CONFIGS[n][0] == cname))
    with handle(g["X"]) as m:
        m.gram()
        first = m.get_table()
        m.gram()
        second = m.get_table()
    print("%s: device G vs the reference's: max difference %.3g (allowed: 0); second run %.3g (allowed: 0)" % (
        cname, np.abs(first - g["G"]).max(), np.abs(second - first).max()))
    assert ec.same_bits(first, g["G"]) and ec.same_bits(second, first)


# ---- inverse and weights ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sized_references(n, lamb):
    """computed once per (size, lamb), shared by both values of posB and left unchanged: X, G, the restatement's and NumPy's
    unclamped B"""
    X = ec.sized_matrix(n, "real", n)
    G = ec.gram(X)
    rest, formula = ec.weights(ec.invert(G, lamb), False), ec.numpy_formula(X, lamb, False)
    for a in (G, rest, formula):
        a.setflags(write=False)
    return X, G, rest, formula


@pytest.mark.parametrize("posB", [False, True])
@pytest.mark.parametrize("lamb", LAMBS)
@pytest.mark.parametrize("n", SIZES)
def test_inverse_and_weights(n, lamb, posB):
    X, G, rest0, formula0 = sized_references(n, lamb)
    rest, formula = (ec.clamp(rest0), ec.clamp(formula0)) if posB else (rest0, formula0)
    distance = float(np.abs(rest0 - formula0).max())
    tol, ceiling = ec.device_tolerance(distance, formula0), ec.ceiling(G, lamb, formula0)
    with handle(X) as m:
        m.fit(lamb, posB)
        B = m.get_table()
        m.fit(lamb, posB)
        again = m.get_table()
        m.gram()
        m.invert(lamb)
        m.weights(posB)
        staged = m.get_table()
    d_rest, d_formula = float(np.abs(B - rest).max()), float(np.abs(B - formula).max())
    print("n = %d, lamb = %g, posB = %s: device vs restatement %.3g, vs NumPy's formula %.3g; tolerance %.3g (16 x %.3g, floor "
          "%.3g); CEILING %.3g" % (n, lamb, posB, d_rest, d_formula, tol, distance, 2.0 ** -52 * np.abs(formula0).max(initial=0), ceiling))
    assert tol <= ceiling
    assert d_rest <= tol and d_formula <= tol
    assert (np.diag(B) == 0).all() and not np.signbit(np.diag(B)).any()
    if posB:
        assert (B >= 0).all() and not np.signbit(B).any(), "no negative entry and no -0.0"
    elif n > 1:
        assert (B < 0).any()
    assert ec.same_bits(staged, B), "gram, invert, weights give the bits of fit"
    assert ec.same_bits(again, B), "two fits give the same bits"


@pytest.mark.parametrize("name", sorted(ec.CONFIGS))
def test_weights_against_the_golden(golden, name):
    g = ec.golden_config(golden, name)
    tol = ec.device_tolerance(ec.RESTATEMENT_VS_REFERENCE[name], g["B"])
    ceiling = ec.ceiling(ec.gram(g["X"]), g["lamb"], g["B"])
    assert tol <= ceiling
    with handle(g["X"]) as m:
        for posB in (False, True):
            m.fit(g["lamb"], posB)
            B = m.get_table()
            want = ec.clamp(g["B"]) if posB else g["B"]
            diff = float(np.abs(B - want).max())
            print("%s, posB = %s: device B vs the reference's %.3g; tolerance %.3g (16 x %.3g); CEILING %.3g" % (
                name, posB, diff, tol, ec.RESTATEMENT_VS_REFERENCE[name], ceiling))
            assert diff <= tol and (np.diag(B) == 0).all()
            assert not posB or ((B >= 0).all() and not np.signbit(B).any())


def test_a_table_that_is_not_positive_definite_is_a_status_not_a_fault(golden):
    small, large = ec.golden_config(golden, "A/0.5"), ec.golden_config(golden, "T/10")
    with handle(small["X"]) as m:
        m.set_table(-np.eye(40))
        with pytest.raises(_lib.HipError, match="not positive definite at block 0") as e:
            m.invert(0.5)
        assert e.value.code == 1
        m.fit(0.5, False)   # the handle is as good as new
        B = m.get_table()
    diff, tol = float(np.abs(B - small["B"]).max()), ec.device_tolerance(ec.RESTATEMENT_VS_REFERENCE["A/0.5"], small["B"])
    print("fit after the refused table: device B vs the reference's %.3g; tolerance %.3g" % (diff, tol))
    assert diff <= tol
    with handle(large["X"]) as m:
        table = np.eye(129)
        table[70, 70] = -2.0
        m.set_table(table)
        with pytest.raises(_lib.HipError, match="not positive definite at block 1"):
            m.invert(0.5)
        with pytest.raises(_lib.HipError, match="lamb"):
            m.invert(0.0)
        with pytest.raises(_lib.HipError, match="lamb"):
            m.fit(-1.0, True)
        m.fit(10.0, False)
        assert np.abs(m.get_table() - large["B"]).max() <= ec.device_tolerance(ec.RESTATEMENT_VS_REFERENCE["T/10"], large["B"])


def test_a_table_that_does_not_fit_names_the_bytes_wanted():
    """400 000 items want a 1.28 TB table, several times the device's memory: a status with the figure, no handle"""
    import scipy.sparse as sp

    X = sp.csr_matrix(([1.0], ([0], [0])), shape=(2, 400000))
    with pytest.raises(_lib.HipError, match="cannot allocate 1280000000000 bytes of device memory for the item-item table") as e:
        _lib.EaseModel(X)
    assert e.value.code == 2


# ---- scoring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ec.CONFIGS))
def test_scores_from_the_goldens_table_bit_for_bit(golden, name):
    g = ec.golden_config(golden, name)
    c = ec.case(ec.CONFIGS[name][0])
    users, (pu, pi) = ec.score_users(c), ec.score_pairs(c)
    with handle(g["X"]) as m:
        for tag, B in (("", g["B"]), ("_pos", ec.clamp(g["B"]))):
            m.set_table(B)
            assert ec.same_bits(m.get_table(), B)
            rows, pairs = m.score_users(users), m.score_pairs(pu, pi)
            print("%s%s: device scores vs the reference's: rows %.3g, pairs %.3g (allowed: 0)" % (
                name, tag, np.abs(rows - g["scores" + tag]).max(), np.abs(pairs - g["pair_scores" + tag]).max()))
            assert ec.same_bits(rows, g["scores" + tag]) and ec.same_bits(pairs, g["pair_scores" + tag])


def test_scoring_edges_bit_for_bit():
    """users with 0, 1, 64 and 257 entries; one user and 300 users in a call; duplicate users; stored zeros"""
    X = ec.scoring_edge_matrix()
    assert [int(X.indptr[u + 1] - X.indptr[u]) for u in (0, 1, 2, 300)] == [0, 1, 64, 257]
    B = np.random.RandomState(21).uniform(-1.0, 1.0, (257, 257))
    want = np.array([ec.score_user(X, B, u) for u in range(301)])
    with handle(X) as m:
        m.set_table(B)
        everyone = m.score_users(np.arange(300))
        singles = {u: m.score_users([u]) for u in (0, 1, 2, 300)}
        dup = m.score_users([5, 5, 2, 300, 5])
        rs = np.random.RandomState(22)
        pu, pi = rs.randint(0, 301, 400), rs.randint(0, 257, 400)
        pu[:4], pi[:4] = [0, 1, 2, 300], [256, 6, 70, 0]
        pairs = m.score_pairs(pu, pi)
        with pytest.raises(_lib.HipError, match="user 301 out of range"):
            m.score_users([3, 301])
        with pytest.raises(_lib.HipError, match="item 257 out of range"):
            m.score_pairs([3], [257])
        assert m.score_users(np.zeros(0, np.int32)).shape == (0, 257)
    print("300 users in one call: max difference to the restatement %.3g (allowed: 0)" % np.abs(everyone - want[:300]).max())
    assert ec.same_bits(everyone, want[:300])
    assert (singles[0] == 0).all() and not np.signbit(singles[0]).any(), "a user with no entries scores +0.0 everywhere"
    for u, got in singles.items():
        assert got.shape == (1, 257) and ec.same_bits(got[0], want[u]), u
    assert ec.same_bits(dup, want[[5, 5, 2, 300, 5]])
    print("400 pairs: max difference to the restatement %.3g (allowed: 0)" % np.abs(pairs - want[pu, pi]).max())
    assert ec.same_bits(pairs, want[pu, pi])
    assert ec.same_bits(pairs, np.array([ec.score_pair(X, B, int(u), int(i)) for u, i in zip(pu, pi)]))


def test_more_ids_than_one_chunk_holds():
    """the chunk loop past its first chunk (b0 > 0).  score_users takes min(65535, 256 MiB / (8 n_items)) users per chunk:
    65 535 at 4 items (256 MiB / 32 bytes is about 8 million), so 65 536 ids make a second chunk of one; score_pairs takes
    2^20 pairs per chunk, so 2^20 + 1 do the same"""
    import scipy.sparse as sp

    n_users, n_items = 3, 4
    X = sp.csr_matrix(np.array([[1.0, 0.0, 2.5, 0.0], [0.0, 0.0, 0.0, 0.0], [0.5, 3.0, 0.0, 4.0]]))
    B = np.random.RandomState(23).uniform(-1.0, 1.0, (n_items, n_items))
    user_cap, pair_cap = min(65535, (256 << 20) // (8 * n_items)), 1 << 20
    nu, npairs = 65536, (1 << 20) + 1
    assert nu > user_cap and npairs > pair_cap, "more than one chunk's worth"
    want_rows = np.array([ec.score_user(X, B, u) for u in range(n_users)])
    want_pairs = np.array([[ec.score_pair(X, B, u, i) for i in range(n_items)] for u in range(n_users)])
    users = np.arange(nu) % n_users
    pu, pi = np.arange(npairs) % n_users, (np.arange(npairs) // n_users) % n_items
    with handle(X) as m:
        m.set_table(B)
        rows, pairs = m.score_users(users), m.score_pairs(pu, pi)
    assert rows.shape == (nu, n_items) and ec.same_bits(rows, want_rows[users])
    assert pairs.shape == (npairs,) and ec.same_bits(pairs, want_pairs[pu, pi])


# ---- end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ec.CONFIGS))
def test_end_to_end(golden, name, tmp_path):
    g = ec.golden_config(golden, name)
    cname, lamb = ec.CONFIGS[name]
    c = ec.case(cname)
    users, (pu, pi) = ec.score_users(c), ec.score_pairs(c)
    tol_b = ec.device_tolerance(ec.RESTATEMENT_VS_REFERENCE[name], g["B"])
    row_sums = np.asarray(np.abs(g["X"]).sum(axis=1)).ravel()
    for posB, tag in ((True, "_pos"), (False, "")):
        m = EASE(lamb=lamb, posB=posB, verbose=False).fit(ec.dataset(cname))
        want_b = ec.clamp(g["B"]) if posB else g["B"]
        assert isinstance(m.B, np.ndarray) and m.B.dtype == np.float64 and np.abs(m.B - want_b).max() <= tol_b
        batch = m.score_batch(users)
        worst = 0.0
        for b, u in enumerate(users):
            s = m.score(int(u))
            tol = 2 * row_sums[u] * tol_b
            diff = float(np.abs(s - g["scores" + tag][b]).max())
            worst = max(worst, diff / tol)
            assert s.shape == (c["ni"],) and diff <= tol
            assert ec.same_bits(s, batch[b])
            i = int(pi[b])
            assert s[i] == m.score(int(u), i) == m.score_batch([u])[0][i]
            ranked, scores = m.rank(int(u))
            assert ec.same_bits(scores, s) and np.array_equal(ranked, np.lexsort((np.arange(c["ni"]), s))[::-1])
        pairs = m.rate_batch(pu, pi, clipping=False)
        pair_worst = float(np.max(np.abs(pairs - g["pair_scores" + tag]) / (2 * row_sums[pu] * tol_b)))
        print("%s, posB = %s: device B vs the reference's %.3g (tolerance %.3g); scores at most %.3g of their bound 2 sum|x| tol_B, "
              "pairs %.3g" % (name, posB, np.abs(m.B - want_b).max(), tol_b, worst, pair_worst))
        assert pair_worst <= 1.0
        back = EASE.load(m.save(str(tmp_path)))
        assert "_scorer" not in back.__dict__ and ec.same_bits(back.B, m.B)
        assert ec.same_bits(back.score_batch(users), batch) and back.score(int(pu[0]), int(pi[0])) == m.score(int(pu[0]), int(pi[0]))
