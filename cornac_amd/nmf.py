"""Non-negative matrix factorisation on MI355X — constructor, learned attributes (`u_factors, i_factors, u_biases, i_biases,
global_mean`) and `fit/score/rank` surface of the reference's `cornac.models.NMF` (cornac/models/nmf/recom_nmf.pyx:37-342).
The multiplicative-update loop of `NMF._fit_sgd` (recom_nmf.pyx:182-267) is replaced by `cornac_hip_mf_nmf_fit` on the MF
handle.  Scoring is MF's (`mu + Bu[u] + Bi + V U[u]` in float32), so the batched rank / ranking_eval / rating_eval kernels
serve it."""
import multiprocessing

import numpy as np

from . import _lib
from .pmf import _get_rng
from .recommender import Recommender, ScoreException, _table_fingerprint

DTYPE = np.float32


def _uniform(shape, rng):
    # cornac/utils/init_utils.py `uniform(shape, low=0.0, high=1.0, random_state, dtype=float32)`
    return rng.uniform(0.0, 1.0, shape).astype(DTYPE)


class NMF(Recommender):
    """Parameters are those of the reference (recom_nmf.pyx:40-86); `mode` as in MF: None -> deterministic when seeded
    (every row sum in the reference's single-thread order: its float32 bits), hogwild otherwise (exact sums in another,
    fixed order where the reference's threads race).  `device` picks the GPU.  `loss_history` is an extra: the loss of
    every epoch, in float64."""

    def __init__(self, name="NMF", k=15, max_iter=50, learning_rate=.005, lambda_reg=0.0, lambda_u=.06, lambda_v=.06,
                 lambda_bu=.02, lambda_bi=.02, use_bias=False, num_threads=0, trainable=True, verbose=False,
                 init_params=None, seed=None, mode=None, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.k = k
        self.max_iter = max_iter
        self.learning_rate = learning_rate
        self.lambda_reg = lambda_reg
        self.lambda_u = lambda_u
        self.lambda_v = lambda_v
        self.lambda_bu = lambda_bu
        self.lambda_bi = lambda_bi
        self.use_bias = use_bias
        self.seed = seed
        if self.lambda_reg > 0:   # recom_nmf.pyx:113-117
            self.lambda_u = self.lambda_reg
            self.lambda_v = self.lambda_reg
            self.lambda_bu = self.lambda_reg
            self.lambda_bi = self.lambda_reg
        if seed is not None:      # recom_nmf.pyx:119-124 (kept for clone(); the device has its own parallelism)
            self.num_threads = 1
        elif num_threads > 0 and num_threads < multiprocessing.cpu_count():
            self.num_threads = num_threads
        else:
            self.num_threads = multiprocessing.cpu_count()
        if mode not in (None, "deterministic", "hogwild"):
            raise ValueError(f"mode={mode} is not supported")
        self.mode = mode
        self.device = device
        self.init_params = {} if init_params is None else init_params
        self.u_factors = self.init_params.get("U", None)
        self.i_factors = self.init_params.get("V", None)
        self.u_biases = self.init_params.get("Bu", None)
        self.i_biases = self.init_params.get("Bi", None)
        self.global_mean = self.init_params.get("mu", None)

    @property
    def effective_mode(self):
        if self.mode is not None:
            return self.mode
        return "deterministic" if self.seed is not None else "hogwild"

    def _init(self):
        # recom_nmf.pyx:134-145 — one generator, U then V; sizes use num_users / num_items
        rng = _get_rng(self.seed)
        if self.u_factors is None:
            self.u_factors = _uniform((self.num_users, self.k), rng)
        if self.i_factors is None:
            self.i_factors = _uniform((self.num_items, self.k), rng)
        self.u_biases = np.zeros(self.num_users, dtype=DTYPE) if self.u_biases is None else self.u_biases
        self.i_biases = np.zeros(self.num_items, dtype=DTYPE) if self.i_biases is None else self.i_biases
        self.global_mean = self.global_mean if self.use_bias else 0.0

    def fit(self, train_set, val_set=None):
        Recommender.fit(self, train_set, val_set)
        self._init()
        if self.trainable:
            self._fit_hip(train_set)
        self._drop_scorer()
        return self

    def _fit_hip(self, train_set):
        for name in ("u_factors", "i_factors", "u_biases", "i_biases"):
            # the reference's fused-type dispatch (`floating` in _fit_sgd's signature) cannot mix tables of another type
            # with its float32 ratings
            if np.asarray(getattr(self, name)).dtype != DTYPE:
                raise TypeError("NMF: %s must be float32 like the ratings, got %s" % (name, np.asarray(getattr(self, name)).dtype))
        X = train_set.matrix   # csr_matrix: recom_nmf.pyx:168-175
        user_counts = np.ediff1d(X.indptr)
        user_ids = np.repeat(np.arange(self.num_users), user_counts).astype(X.indices.dtype)
        mode = _lib.MODE_DETERMINISTIC if self.effective_mode == "deterministic" else _lib.MODE_HOGWILD
        trainer = _lib.MfTrainer(user_ids, X.indices, X.data.astype(np.float32), self.num_users, self.num_items, self.k,
                                 device=self.device)
        try:
            trainer.nmf_set_factors(self.u_factors, self.i_factors, self.u_biases, self.i_biases)
            self.loss_history = trainer.nmf_fit(self.max_iter, self.learning_rate, self.lambda_u, self.lambda_v,
                                                self.lambda_bu, self.lambda_bi, float(self.global_mean), self.use_bias, mode)
            U, V, Bu, Bi = trainer.nmf_get_factors()
            self.u_factors[...] = U
            self.i_factors[...] = V
            self.u_biases[...] = Bu
            self.i_biases[...] = Bi
        finally:
            trainer.close()
        if self.verbose:
            print("Optimization finished!")

    # ---- prediction -------------------------------------------------------------------------------
    def _scoring_tables(self):
        src = (_table_fingerprint(self.i_biases), float(self.global_mean))
        if self.__dict__.get("_item_base") is None or self._item_base_src != src:
            self._item_base = (self.global_mean + self.i_biases).astype(DTYPE)
            self._item_base_src = src
        return self.u_factors, self.i_factors, self._item_base, self.u_biases

    def _drop_scorer(self):
        # the biases are refreshed IN PLACE by a refit: the derived item_base table must go with the device scorer
        for name in ("_item_base", "_item_base_src"):
            self.__dict__.pop(name, None)
        super()._drop_scorer()

    def score(self, user_idx, item_idx=None):
        """recom_nmf.pyx:270-302"""
        if item_idx is not None and self.is_unknown_item(item_idx):
            raise ScoreException("Can't make score prediction for item %d" % item_idx)
        if item_idx is None:
            if self.knows_user(user_idx):
                return self._get_scorer().score_user(user_idx)
            return self.global_mean + self.i_biases
        item_score = self.global_mean + self.i_biases[item_idx]
        if self.knows_user(user_idx):
            item_score += self.u_biases[user_idx]
            item_score += self.u_factors[user_idx].dot(self.i_factors[item_idx])
        return item_score

    def get_vector_measure(self):
        return "dot"

    def get_user_vectors(self):
        """recom_nmf.pyx:314-327: the extra column only with use_bias"""
        user_vectors = self.u_factors
        if self.use_bias:
            user_vectors = np.concatenate((user_vectors, np.ones([user_vectors.shape[0], 1])), axis=1)
        return user_vectors

    def get_item_vectors(self):
        """recom_nmf.pyx:329-342"""
        item_vectors = self.i_factors
        if self.use_bias:
            item_vectors = np.concatenate((item_vectors, self.i_biases.reshape((-1, 1))), axis=1)
        return item_vectors
