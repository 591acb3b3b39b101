"""Probabilistic matrix factorisation on MI355X — constructor, learned attributes (`U`, `V`) and `fit/score/rank` surface of
the reference's `cornac.models.PMF` (cornac/models/pmf/recom_pmf.py:25-252).  The per-rating RMSProp loop of
`pmf.pmf_linear` / `pmf.pmf_non_linear` (cornac/models/pmf/cython/pmf.pyx:55-173: float64, stored order, one thread
always) is replaced by `cornac_hip_mf_pmf_fit` on the MF handle; the factors come out bit-identical to that loop's.
Scoring and ranking take the float64 route (`Scorer.set_f64` / `score_user_f64`, ordering per user on the host)."""
import numpy as np

from . import _lib
from .recommender import Recommender, ScoreException

VARIANTS = ("linear", "non_linear")


def _sigmoid(x):
    # cornac/utils/common.py:29-31
    return 1. / (1. + np.exp(-x))


def _scale(values, target_min, target_max, source_min, source_max):
    # cornac/utils/common.py:34-69 with both source bounds given
    if source_min == source_max:
        source_min = 0.0
    values = (values - source_min) / (source_max - source_min)
    values = values * (target_max - target_min) + target_min
    return values


def _get_rng(seed):
    # cornac/utils/common.py:161-173: None is numpy's global RandomState, an int a fresh one, a RandomState itself
    if seed is None:
        return np.random.mtrand._rand
    if isinstance(seed, (int, np.integer)):
        return np.random.RandomState(seed)
    if isinstance(seed, np.random.RandomState):
        return seed
    raise ValueError("{} can not be used to create a numpy.random.RandomState".format(seed))


class PMF(Recommender):
    """Parameters are those of the reference (recom_pmf.py:28-75); `device` picks the GPU.  As there, a fit starts from
    `U` / `V` when the model holds them (init_params or an earlier fit) and draws the missing ones — `U` before `V` — from
    normal(0, 0.001) in float64; the RMSProp caches start from zero in every fit."""

    def __init__(self, k=5, max_iter=100, learning_rate=0.001, gamma=0.9, lambda_reg=0.001, name="PMF",
                 variant="non_linear", trainable=True, verbose=False, init_params=None, seed=None, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.k = k
        self.max_iter = max_iter
        self.learning_rate = learning_rate
        self.gamma = gamma
        self.lambda_reg = lambda_reg
        self.variant = variant
        self.seed = seed
        self.device = device
        self.init_params = {} if init_params is None else init_params
        self.U = self.init_params.get("U", None)
        self.V = self.init_params.get("V", None)

    def _init(self):
        # pmf.pyx:40-51 `_init_factors`: one generator, U then V, sized num_users / num_items
        rng = _get_rng(self.seed)
        if self.U is None:
            self.U = rng.normal(0.0, 0.001, (self.num_users, self.k)).astype(np.double)
        if self.V is None:
            self.V = rng.normal(0.0, 0.001, (self.num_items, self.k)).astype(np.double)

    def _ratings(self, train_set):
        """the `rat` argument of the reference's call (recom_pmf.py:129-135, :147): float32, mapped to [0, 1] for the
        non-linear variant unless that is the range already"""
        rat = np.array(train_set.uir_tuple[2], dtype="float32")
        if self.variant == "non_linear":
            if [self.min_rating, self.max_rating] != [0, 1]:
                rat = _scale(rat, 0.0, 1.0, self.min_rating, self.max_rating)
        return rat.astype(np.float32)

    def fit(self, train_set, val_set=None):
        Recommender.fit(self, train_set, val_set)
        if self.trainable:
            rat = self._ratings(train_set)
            if self.variant not in VARIANTS:
                raise ValueError('variant must be one of {"linear","non_linear"}')
            self._init()
            uid, iid, _ = train_set.uir_tuple
            trainer = _lib.MfTrainer(uid, iid, rat, self.num_users, self.num_items, self.k, device=self.device)
            try:
                trainer.pmf_set_factors(self.U, self.V)
                self.loss_history = trainer.pmf_fit(self.max_iter, self.learning_rate, self.lambda_reg, self.gamma,
                                                    self.variant)
                self.U, self.V = trainer.pmf_get_factors()
            finally:
                trainer.close()
            if self.verbose:
                for epoch, loss in enumerate(self.loss_history):
                    print('epoch %i, loss: %f' % (epoch, loss))
                print("Learning completed")
        elif self.verbose:
            print("%s is trained already (trainable = False)" % (self.name))
        self._drop_scorer()
        return self

    # ---- prediction -------------------------------------------------------------------------------
    def _scoring_tables(self):
        return self.U, self.V, None, None

    def _scorer_row_count(self):
        # a float64 model is not served by the float32 batched kernels: rank() and the evaluators take the per-user flow
        # over score(), in float64 like the reference's (BPR's float64 tables do the same)
        return 0

    def score(self, user_idx, item_idx=None):
        """recom_pmf.py:191-222 — with its asymmetry: all items = raw dot products, one item = the sigmoid mapped back to
        the rating range under the non-linear variant"""
        if self.is_unknown_user(user_idx):
            raise ScoreException("Can't make score prediction for user %d" % user_idx)
        if item_idx is not None and self.is_unknown_item(item_idx):
            raise ScoreException("Can't make score prediction for item %d" % item_idx)
        if item_idx is None:
            return self._get_scorer().score_user_f64(user_idx)
        user_pred = self.V[item_idx, :].dot(self.U[user_idx, :])
        if self.variant == "non_linear":
            user_pred = _sigmoid(user_pred)
            user_pred = _scale(user_pred, self.min_rating, self.max_rating, 0.0, 1.0)
        return user_pred

    def get_vector_measure(self):
        return "dot"

    def get_user_vectors(self):
        return self.U

    def get_item_vectors(self):
        return self.V
