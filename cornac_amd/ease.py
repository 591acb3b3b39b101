"""EASE on MI355X — constructor, learned attributes (`B`, `U`) and `fit/score/rank` surface of the reference's
`cornac.models.EASE` (cornac/models/ease/recom_ease.py:38-156; Steck 2019).  What the reference computes with SciPy and
NumPy on the host — the Gram matrix X^T X, the inverse of the dense SPD items x items matrix, the weights, and the sparse
row x dense matrix scores — runs in libcornac_hip (`_lib.EaseModel`), in float64 like there.

The Gram matrix and, given the same B, the scores have the reference's bits (one summation order); B itself comes from a
blocked Gauss-Jordan sweep instead of LAPACK's LU and agrees with the reference's to rounding.

One stated departure: `lamb` must be > 0 (ValueError).  The reference hands a singular G to `np.linalg.inv`."""
import numpy as np

from . import _lib
from .recommender import Recommender, ScoreException, _table_fingerprint, clip


class EASE(Recommender):
    """Embarrassingly Shallow Autoencoder.  Parameters are those of the reference (recom_ease.py:38-55): `lamb` the L2
    regularisation, `posB` drops negative weights, `B` / `U` a ready weight table (items x items) and rating matrix (users x
    items, scipy CSR); `device` picks the GPU.  Learned: `B` (float64 ndarray on the host) and `U` (the training CSR)."""

    def __init__(self, name="EASEᴿ", lamb=500, posB=True, trainable=True, verbose=True, seed=None, B=None, U=None, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.lamb = lamb
        self.posB = posB
        self.seed = seed
        self.B = B
        self.U = U
        self.device = device

    # ---- fit --------------------------------------------------------------------------------------
    def fit(self, train_set, val_set=None):
        """recom_ease.py:57-97; B is recomputed whatever `trainable` says, as there"""
        Recommender.fit(self, train_set, val_set)
        if not (np.isfinite(self.lamb) and self.lamb > 0):
            raise ValueError("Invalid lamb = {}: G + lamb I must be positive definite, so lamb > 0".format(self.lamb))
        X = train_set.matrix
        if not np.isfinite(X.data).all():
            raise ValueError("EASE needs finite ratings: the training matrix holds NaN or inf")
        self.U = X
        model = _lib.EaseModel(X, device=self.device)
        try:
            model.fit(self.lamb, self.posB)
            self.B = model.get_table()
        except Exception:
            model.close()
            raise
        self._scorer = model   # its table is B already: kept for scoring
        self._scorer_key = self._ease_key()
        return self

    # ---- prediction -------------------------------------------------------------------------------
    def _scorer_row_count(self):
        # no factor tables: rank() and the evaluators take the per-user flow over score(), as the KNN models do
        return 0

    @property
    def batch_num_items(self):
        return self.num_items

    def register_exclusions(self, token, user_indices, ex_ptr, ex_idx):
        return False   # no factor-table scorer to keep the lists on: the evaluators' per-user flow needs none

    def _ease_key(self):
        U = self.U
        return (id(U),) + tuple(_table_fingerprint(a) for a in (U.indptr, U.indices, U.data, self.B))

    def _ease_scorer(self):
        """the device handle holding U and B: the one `fit` left, or a new one after load() / an assignment to B or U"""
        key = self._ease_key()
        if self.__dict__.get("_scorer") is None or self.__dict__.get("_scorer_key") != key:
            self._drop_scorer()
            model = _lib.EaseModel(self.U, device=self.device)
            try:
                model.set_table(self.B)
            except Exception:
                model.close()
                raise
            self._scorer = model
            self._scorer_key = key
        return self._scorer

    def _unknown(self, user_idx, item_idx):
        # recom_ease.py:117-121
        if self.is_unknown_user(user_idx):
            raise ScoreException("Can't make score prediction for user %d" % user_idx)
        if item_idx is not None and self.is_unknown_item(item_idx):
            raise ScoreException("Can't make score prediction for item %d" % item_idx)

    def score(self, user_idx, item_idx=None):
        """recom_ease.py:99-126: U[user] . B, or its entry for one item"""
        self._unknown(user_idx, item_idx)
        sc = self._ease_scorer()
        if item_idx is not None:
            return sc.score_pairs([user_idx], [item_idx])[0]
        return sc.score_users([user_idx])[0]

    def score_batch(self, user_indices):
        """`score(u)` for every listed user in one call: [n, num_items] float64"""
        users = np.asarray(user_indices, dtype=np.int64).ravel()
        for u in users:
            self._unknown(int(u), None)
        return self._ease_scorer().score_users(users)

    def rate_batch(self, user_indices, item_indices, clipping=True):
        """`rate()` for many pairs in one call; pairs with an unknown user or item go through `rate()` itself"""
        u = np.asarray(user_indices, dtype=np.int64)
        i = np.asarray(item_indices, dtype=np.int64)
        known = (u >= 0) & (u < self.num_users) & (i >= 0) & (i < self.num_items)
        out = np.empty(len(u), dtype=np.float64)
        if known.any():
            pred = self._ease_scorer().score_pairs(u[known], i[known])
            out[known] = clip(pred, self.min_rating, self.max_rating) if clipping else pred
        for p in np.flatnonzero(~known):
            out[p] = self.rate(int(u[p]), int(i[p]), clipping)
        return out

    # ---- ANN surface (recom_ease.py:128-156) --------------------------------------------------------
    def get_vector_measure(self):
        return "dot"

    def get_user_vectors(self):
        return self.U

    def get_item_vectors(self):
        return self.B
