"""EASE on MI355X — constructor, learned attributes (`B`, `U`) and `fit/score/rank` surface of the reference's
`cornac.models.EASE` (cornac/models/ease/recom_ease.py:38-156; Steck 2019).  What the reference computes with SciPy and
NumPy on the host — the Gram matrix X^T X, the inverse of the dense SPD items x items matrix, the weights, and the sparse
row x dense matrix scores — runs in libcornac_hip (`_lib.EaseModel`), in float64 like there.

The Gram matrix and, given the same B, the scores have the reference's bits (one summation order); B itself comes from a
blocked Gauss-Jordan sweep instead of LAPACK's LU and agrees with the reference's to rounding.

One stated departure: `lamb` must be > 0 (ValueError).  The reference hands a singular G to `np.linalg.inv`."""
import numpy as np

from . import _lib
from .recommender import HandleScoredRecommender, Recommender, _table_fingerprint


class EASE(HandleScoredRecommender):
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
        self._keep_handle(model)   # its table is B already: kept for scoring
        return self

    # ---- prediction (recom_ease.py:99-126: U[user] . B, or its entry for one item) ------------------
    def _handle_key(self):
        U = self.U
        return (id(U),) + tuple(_table_fingerprint(a) for a in (U.indptr, U.indices, U.data, self.B))

    def _build_handle(self):
        model = _lib.EaseModel(self.U, device=self.device)
        try:
            model.set_table(self.B)
        except Exception:
            model.close()
            raise
        return model

    # ---- ANN surface (recom_ease.py:128-156) --------------------------------------------------------
    def get_vector_measure(self):
        return "dot"

    def get_user_vectors(self):
        return self.U

    def get_item_vectors(self):
        return self.B
