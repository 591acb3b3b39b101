"""Neighbourhood models on MI355X — constructor, learned attributes (`sim_mat`, `mean_arr`, `iu_mat` / `ui_mat`) and
`fit/score/rank` surface of the reference's `cornac.models.UserKNN` / `ItemKNN` (cornac/models/knn/recom_knn.py:91-435).
The two loops of its extension (cornac/models/knn/similarity.pyx: `compute_similarity` :51-105 and `compute_score` /
`compute_score_single` :108-201, OpenMP over rows / items, one thread when seeded) run in libcornac_hip
(`_lib.KnnSimilarity`, `_lib.KnnScorer`), in float64 like there.  The preparation of the weight matrix (mean centring,
idf / bm25 weights, amplification) is NumPy in the reference and stays NumPy on the host here.

The similarity table has the reference's bits (one summation order, the compiled extension's quotient) except after
`amplify != 1`, where two `pow` implementations meet; the scores select exactly the reference's neighbours, ties at the
k-th weight included, and sum them in another order."""
import numpy as np
from scipy.sparse import coo_matrix

from . import _lib
from .pmf import _get_rng
from .recommender import HandleScoredRecommender, Recommender, ScoreException, _table_fingerprint

EPS = 1e-8
SIMILARITIES = ["cosine", "pearson"]
WEIGHTING_OPTIONS = ["idf", "bm25"]
KNN_MAX_K = _lib.KNN_MAX_K


def _mean_centered(csr_mat):
    """recom_knn.py:34-45: every row minus its mean, in place; an exact zero becomes EPS so that the rating stays stored
    and stays a candidate.  (Row by row: np.mean's own summation gives the reference's bits.)"""
    mean_arr = np.zeros(csr_mat.shape[0])
    for r in range(csr_mat.shape[0]):
        lo, hi = csr_mat.indptr[r: r + 2]
        row = csr_mat.data[lo:hi]
        mean_arr[r] = np.mean(row)
        row -= mean_arr[r]
        row[row == 0] = EPS
    return csr_mat, mean_arr


def _amplify(sim_mat, alpha=1.0):
    """recom_knn.py:48-55: sign(w) * |w| ** alpha over the stored entries"""
    if alpha == 1.0:
        return sim_mat
    w = sim_mat.data
    out = np.power(np.abs(w), alpha)
    sim_mat.data = np.where(w > 0, out, -out)
    return sim_mat


def _idf_weight(ui_mat):
    """recom_knn.py:58-67: log(N / item count) + EPS per stored rating"""
    idf = np.log(float(ui_mat.shape[0]) / np.bincount(ui_mat.indices))
    return idf[ui_mat.indices] + EPS


def _bm25_weight(ui_mat):
    """recom_knn.py:70-88"""
    K1, B = 1.2, 0.8
    X = coo_matrix(ui_mat)
    X.data = np.ones_like(X.data)
    idf = np.log(float(X.shape[0]) / np.bincount(X.col))
    row_sums = np.ravel(X.sum(axis=1))
    length_norm = (1.0 - B) + B * row_sums / row_sums.mean()
    return (K1 + 1.0) / (K1 * length_norm[X.row] + X.data) * idf[X.col] + EPS


class _KNN(HandleScoredRecommender):
    """What the two models share: the reference's constructor (plus `device`), the preparation of the weight matrix, the
    device scorer's life cycle and the prediction surface."""

    _USER_MODE = None   # True: neighbours are users (N = iu_mat, Q = sim_mat); False: items (N = sim_mat, Q = ui_mat)

    def __init__(self, name, k=20, similarity="cosine", mean_centered=False, weighting=None, amplify=1.0, num_threads=0,
                 trainable=True, verbose=True, seed=None, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.k = k
        self.similarity = similarity
        self.mean_centered = mean_centered
        self.weighting = weighting
        self.amplify = amplify
        self.seed = seed
        self.rng = _get_rng(seed)
        self.num_threads = num_threads   # accepted for the reference's signature; the device needs no thread count
        self.device = device
        if self.similarity not in SIMILARITIES:
            raise ValueError("Invalid similarity choice, supported {}".format(SIMILARITIES))
        if self.weighting is not None and self.weighting not in WEIGHTING_OPTIONS:
            raise ValueError("Invalid weighting choice, supported {}".format(WEIGHTING_OPTIONS))
        if not 1 <= int(k) <= KNN_MAX_K:
            raise ValueError("Invalid k = {}: the device scores with 1 <= k <= {} neighbours".format(k, KNN_MAX_K))

    # ---- fit --------------------------------------------------------------------------------------
    def _weight_matrix(self, train_set, centred):
        raise NotImplementedError

    def _reweight(self, weight_mat, train_set):
        # recom_knn.py:195-199 / :375-379
        if self.weighting == "idf":
            weight_mat.data *= np.sqrt(_idf_weight(train_set.matrix))
        elif self.weighting == "bm25":
            weight_mat.data *= np.sqrt(_bm25_weight(train_set.matrix))
        return weight_mat

    def _similarity(self, weight_mat):
        sim = _lib.KnnSimilarity(weight_mat, device=self.device)
        try:
            return sim.run()
        finally:
            sim.close()

    def fit(self, train_set, val_set=None):
        Recommender.fit(self, train_set, val_set)
        ui_mat = train_set.matrix.copy()
        self.mean_arr = np.zeros(ui_mat.shape[0])
        if self.min_rating != self.max_rating:   # explicit feedback
            ui_mat, self.mean_arr = _mean_centered(ui_mat)
        weight_mat = self._weight_matrix(train_set, ui_mat)
        self._keep_ratings(ui_mat)
        self.sim_mat = _amplify(self._similarity(weight_mat), self.amplify)
        self._drop_scorer()
        return self

    # ---- prediction (recom_knn.py:212-264 / :389-435: the user's mean plus the weighted average over the k nearest neighbours)
    def _tables(self):
        """(N, Q) of the device scorer"""
        raise NotImplementedError

    def _handle_key(self):
        return tuple((id(m),) + tuple(_table_fingerprint(a) for a in (m.indptr, m.indices, m.data)) for m in self._tables())

    def _build_handle(self):
        return _lib.KnnScorer(*self._tables(), self._USER_MODE, device=self.device)

    def _check_k(self):
        if not 1 <= int(self.k) <= KNN_MAX_K:
            raise ValueError("Invalid k = {}: the device scores with 1 <= k <= {} neighbours".format(self.k, KNN_MAX_K))
        return int(self.k)

    def _user_rows(self, handle, users):
        return self.mean_arr[np.asarray(users)][:, None] + handle.score_users(users, self._check_k())

    def _pair_values(self, handle, users, items):
        return self.mean_arr[np.asarray(users)] + handle.score_pairs(users, items, self._check_k())


class UserKNN(_KNN):
    """User-based nearest neighbours.  Parameters are those of the reference (recom_knn.py:94-141); `device` picks the
    GPU, `num_threads` is accepted and ignored, and `k` must lie in 1 .. KNN_MAX_K (64).  Learned: `sim_mat` (users x users,
    scipy CSR float64), `mean_arr` and the mean-centred `iu_mat` (items x users)."""

    _USER_MODE = True

    def __init__(self, name="UserKNN", k=20, similarity="cosine", mean_centered=False, weighting=None, amplify=1.0,
                 num_threads=0, trainable=True, verbose=True, seed=None, device=0):
        super().__init__(name, k, similarity, mean_centered, weighting, amplify, num_threads, trainable, verbose, seed, device)

    def _weight_matrix(self, train_set, ui_mat):
        # recom_knn.py:190-199
        centred = self.mean_centered or self.similarity == "pearson"
        return self._reweight(ui_mat.copy() if centred else train_set.matrix.copy(), train_set)

    def _keep_ratings(self, ui_mat):
        self.iu_mat = ui_mat.T.tocsr()   # recom_knn.py:201-203: only the item-user matrix is needed for prediction

    def _tables(self):
        return self.iu_mat, self.sim_mat

    def _unknown(self, user_idx, item_idx):
        if not self.knows_user(user_idx):
            raise ScoreException("Can't make score prediction for (user_id=%d)" % user_idx)
        if item_idx is not None and not self.knows_item(item_idx):
            raise ScoreException("Can't make score prediction for (item_id=%d)" % item_idx)


class ItemKNN(_KNN):
    """Item-based nearest neighbours.  Parameters are those of the reference (recom_knn.py:270-317); `device` picks the
    GPU, `num_threads` is accepted and ignored, and `k` must lie in 1 .. KNN_MAX_K (64).  Learned: `sim_mat` (items x items,
    scipy CSR float64), `mean_arr` and the mean-centred `ui_mat` (users x items)."""

    _USER_MODE = False

    def __init__(self, name="ItemKNN", k=20, similarity="cosine", mean_centered=False, weighting=None, amplify=1.0,
                 num_threads=0, trainable=True, verbose=True, seed=None, device=0):
        super().__init__(name, k, similarity, mean_centered, weighting, amplify, num_threads, trainable, verbose, seed, device)

    def _weight_matrix(self, train_set, ui_mat):
        # recom_knn.py:366-381
        weight_mat = ui_mat.copy() if self.mean_centered else train_set.matrix.copy()
        if self.similarity == "pearson":   # centred by columns
            weight_mat, _ = _mean_centered(weight_mat.T.tocsr())
            weight_mat = weight_mat.T.tocsr()
        return self._reweight(weight_mat, train_set).T.tocsr()

    def _keep_ratings(self, ui_mat):
        self.ui_mat = ui_mat

    def _tables(self):
        return self.sim_mat, self.ui_mat
