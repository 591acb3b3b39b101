"""Hierarchical Poisson factorisation on MI355X — constructor, learned attributes (`Theta`, `Beta`, `Gs`, `Gr`, `Ls`, `Lr`)
and `fit/score/rank` surface of the reference's `cornac.models.HPF` (cornac/models/hpf/recom_hpf.py:25-243).  The
variational loop of `hpf_cpp` / `pf_cpp` (cornac/models/hpf/cpp/cpp_hpf.cpp:208-275 / :139-203: float64, one thread always)
is replaced by `cornac_hip_mf_hpf_fit` on the MF handle.  There is one mode: every sum on the device has a fixed order, so a
fit repeats itself bit for bit; against the reference the tables agree to a tolerance (its digamma, log and exp are other
implementations, and its sums run in another order).  Scoring and ranking take the float64 route like PMF."""
import numpy as np

from . import _lib
from .pmf import _get_rng
from .recommender import Recommender, ScoreException

MAX_K = _lib.MfTrainer.HPF_MAX_K
TABLES = (("Gs", "G_s"), ("Gr", "G_r"), ("Ls", "L_s"), ("Lr", "L_r"))


def _gamma(shape, scale, size, rng):
    # cornac/utils/init_utils.py:85-113 `gamma(shape, scale, size, random_state, dtype=float32)`
    return rng.gamma(shape, scale, size).astype(np.float32)


class HPF(Recommender):
    """Parameters are those of the reference (recom_hpf.py:28-77); `device` picks the GPU.  `hierarchical=False` runs plain
    Poisson factorisation (`pf_cpp`).  As there, a fit starts from `G_s`, `G_r`, `L_s`, `L_r` when the model holds them
    (init_params or an earlier fit) and draws the missing ones, in that order, from one generator: gamma(100, 0.003)
    (hierarchical) or gamma(0.3, 1 / 0.3), cast to float32 and promoted to double (hpf.pyx:118-146 / :51-79).

    Every table must be strictly positive and finite, and k <= 256: `fit` raises ValueError otherwise.  The reference
    routes the expected-log step through sparse matrices that drop entries which are not positive; that treatment of
    zeros is not reproduced (zeros can only come from init_params: every shape is >= 0.3 after one iteration and every
    rate is a sum of positive terms)."""

    def __init__(self, k=5, max_iter=100, name="HPF", trainable=True, verbose=False, hierarchical=True, seed=None,
                 init_params=None, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.k = k
        self.max_iter = max_iter
        self.hierarchical = hierarchical
        self.seed = seed
        self.device = device
        self.init_params = {} if init_params is None else init_params
        self.Theta = self.init_params.get("Theta", None)
        self.Beta = self.init_params.get("Beta", None)
        self.Gs = self.init_params.get("G_s", None)
        self.Gr = self.init_params.get("G_r", None)
        self.Ls = self.init_params.get("L_s", None)
        self.Lr = self.init_params.get("L_r", None)

    def _init(self):
        """hpf.pyx:118-146 / :51-79: one generator; G_s, G_r, L_s, L_r in this order, only the missing ones draw"""
        rng = _get_rng(self.seed)
        shape, scale = (100., 0.3 / 100.) if self.hierarchical else (0.3, 1 / 0.3)
        tables = []
        for (attr, name), rows in zip(TABLES, (self.num_users, self.num_users, self.num_items, self.num_items)):
            t = getattr(self, attr)
            if t is None:
                t = _gamma(shape, scale, rows * self.k, rng).reshape(rows, self.k)
            t = np.array(t, dtype=np.float64, order="C")
            if t.shape != (rows, self.k):
                raise ValueError("HPF: %s must be %r, got %r" % (name, (rows, self.k), t.shape))
            if not (np.isfinite(t).all() and (t > 0).all()):
                raise ValueError("HPF: %s must be strictly positive and finite (the reference's treatment of zeros is "
                                 "not reproduced)" % name)
            tables.append(t)
        return tables

    def fit(self, train_set, val_set=None):
        Recommender.fit(self, train_set, val_set)
        if self.trainable:
            if self.k > MAX_K:
                raise ValueError("HPF: k = %d is above the device's limit of %d" % (self.k, MAX_K))
            tables = self._init()
            X = train_set.matrix   # the CSR: the device needs the ratings stored by user (the sums do not depend on it)
            user_ids = np.repeat(np.arange(self.num_users), np.ediff1d(X.indptr)).astype(X.indices.dtype)
            trainer = _lib.MfTrainer(user_ids, X.indices, X.data.astype(np.float32), self.num_users, self.num_items, self.k,
                                     device=self.device)
            try:
                trainer.hpf_set_tables(*tables)
                if self.verbose:
                    print("Learning...")
                trainer.hpf_fit(self.max_iter, self.hierarchical)
                if self.verbose:
                    print("Learning completed!")
                # recom_hpf.py:168-175; kept for a later fit to continue from
                self.Gs, self.Gr, self.Ls, self.Lr = trainer.hpf_get_tables()[:4]
            finally:
                trainer.close()
            self.Theta = self.Gs / self.Gr
            self.Beta = self.Ls / self.Lr
        elif self.verbose:
            print("%s is trained already (trainable = False)" % (self.name))
        self._drop_scorer()
        return self

    # ---- prediction -------------------------------------------------------------------------------
    def _scoring_tables(self):
        return self.Theta, self.Beta, None, None

    def _scorer_row_count(self):
        # float64 tables: rank() and the evaluators take the per-user flow over score(), as PMF's do
        return 0

    def score(self, user_idx, item_idx=None):
        """recom_hpf.py:182-213"""
        if self.is_unknown_user(user_idx):
            raise ScoreException("Can't make score prediction for user %d" % user_idx)
        if item_idx is not None and self.is_unknown_item(item_idx):
            raise ScoreException("Can't make score prediction for item %d" % item_idx)
        if item_idx is None:
            return self._get_scorer().score_user_f64(user_idx)
        return np.float64(self.Beta[item_idx, :].dot(self.Theta[user_idx, :]))

    def get_vector_measure(self):
        return "dot"

    def get_user_vectors(self):
        return self.Theta

    def get_item_vectors(self):
        return self.Beta
