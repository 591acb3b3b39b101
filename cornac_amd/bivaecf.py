"""BiVAECF on MI355X — constructor, `fit/score/rank` surface and `bivae.state_dict()` of the reference's
`cornac.models.BiVAECF` (cornac/models/bivaecf/recom_bivaecf.py:24-313, bivae.py:34-276; Truong, Salah, Lauw, WSDM 2021).  What
the reference runs per batch in torch on densified rows of X and of its transpose — two forwards, the backward and Adam's
dense sweep per step, with a batch x n_users matrix of probabilities on the item side — runs in libcornac_hip
(`_lib.BivaeModel`), in float32 like there, on the sparse binary rows and without that matrix.

Seeded fits follow the reference's CPU run to rounding: with a seed the model calls `torch.manual_seed(seed)`, builds the
initial tables on the CPU in the reference's construction order (bivae.py:48-86: `randn(U, k) * 0.01` for theta,
`randn(I, k) * 0.01` for beta, `kaiming_uniform_(theta, a=sqrt(5))`, then six `torch.nn.Linear`: user fc0, user_mu, user_std,
item fc0, item_mu, item_std) for the reference's initial bits, and draws per batch two `torch.randn(B, k)` on the host, the
training forward's first, items before users within an epoch, which is what the two `randn_like(mu)` per step draw there
(torch is the generator here, nothing else of it is used).  Without a seed the noise comes from the device generator.

Stated departures, each a NotImplementedError: `encoder_structure` must have length 1, and `cap_priors` must be false on
both sides (CAP priors need the feature modalities and a third trained layer per side).

Orderings (`rank`, `rank_batch`, `ranking_eval`) come from the LOGITS <mu_theta[u], mu_beta[i]> through the fused
factor-model scorer: the sigmoid is monotone, so that is the order of `score()`, except where float32 probabilities tie
and the logits do not.  `score`, `score_batch` and `rate_batch` return the handle's probabilities; a pair's goes through
the reference's scaling from [0, 1] to [min_rating, max_rating]."""
from collections import OrderedDict

import numpy as np

from . import _lib
from .recommender import HandleScoredRecommender, Recommender, _table_fingerprint, filled_handle, float32_tables

NAMES = _lib.BivaeModel.NAMES
FACTORS = _lib.BivaeModel.FACTORS


class BiVAETables:
    """What the reference's `BiVAE` module holds, as float32 arrays on the host: `tables`, the 12 encoder tables under the
    reference's state_dict names and shapes, and the plain tensors `theta`, `beta`, `mu_theta`, `mu_beta` (bivae.py:48-53).
    Picklable, and needs no torch."""

    def __init__(self, tables, theta, beta, mu_theta, mu_beta):
        self.tables = OrderedDict((n, np.ascontiguousarray(tables[n], np.float32)) for n in NAMES)
        for n, a in zip(FACTORS, (theta, beta, mu_theta, mu_beta)):
            setattr(self, n, np.ascontiguousarray(a, np.float32))
        self._check()

    @property
    def dims(self):
        """(n_users, n_items, k, h)"""
        h, n_items = self.tables[NAMES[0]].shape
        return self.tables[NAMES[6]].shape[1], n_items, self.tables[NAMES[2]].shape[0], h

    def _check(self):
        n_users, n_items, k, h = self.dims
        want = dict(_lib.BivaeModel.shapes(n_users, n_items, k, h), **_lib.BivaeModel.factor_shapes(n_users, n_items, k))
        for n in NAMES + FACTORS:
            got = (self.tables[n] if n in self.tables else getattr(self, n)).shape
            if got != want[n]:
                raise ValueError("%s has shape %r, expected %r" % (n, got, want[n]))

    def state_dict(self):
        """the 12 tables under the reference's names and shapes (copies): they load into the reference's BiVAE"""
        return OrderedDict((n, self.tables[n].copy()) for n in NAMES)

    def load_state_dict(self, state):
        """tables (arrays or torch tensors) under the reference's names; shapes must agree with each other and with the
        factor tables"""
        if set(state) != set(NAMES):
            raise KeyError("state_dict needs exactly the keys %r" % (NAMES,))
        old = self.tables
        self.tables = float32_tables(state, NAMES)
        try:
            self._check()
        except ValueError:
            self.tables = old
            raise


class BiVAECF(HandleScoredRecommender):
    """Bilateral variational autoencoder for collaborative filtering.  Parameters are the reference's
    (recom_bivaecf.py:27-84): `k` the size of theta and beta, `encoder_structure` the hidden layer `[h]` of both encoders,
    `act_fn` in tanh / sigmoid / relu / relu6 / elu, `likelihood` in bern / gaus / pois, `n_epochs`, `batch_size`,
    `learning_rate` (Adam, one optimiser per side), `beta_kl` (the KL weight), `cap_priors` (both sides must be false),
    `seed`; `use_gpu` is accepted and ignored (the model always trains on the GPU `device`).  Learned: `bivae`, a
    `BiVAETables`; `loss_history`, per epoch `(loss_i, loss_u)` as the reference's progress bar computes them."""

    def __init__(self, name="BiVAECF", k=10, encoder_structure=[20], act_fn="tanh", likelihood="pois", n_epochs=100, batch_size=100,
                 learning_rate=0.001, beta_kl=1.0, cap_priors={"user": False, "item": False}, trainable=True, verbose=False,
                 seed=None, use_gpu=True, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.k = k
        self.encoder_structure = encoder_structure
        self.act_fn = act_fn
        self.likelihood = likelihood
        self.batch_size = batch_size
        self.n_epochs = n_epochs
        self.learning_rate = learning_rate
        self.beta_kl = beta_kl
        self.cap_priors = cap_priors
        self.seed = seed
        self.use_gpu = use_gpu
        self.device = device
        self.ignored_attrs = self.ignored_attrs + ["_bivae_handle", "_bivae_key", "_rank_tables"]

    # ---- fit --------------------------------------------------------------------------------------
    def _check_structure(self):
        if len(self.encoder_structure) != 1:
            raise NotImplementedError("BiVAECF here supports one hidden layer: encoder_structure must have length 1, got %r"
                                      % (self.encoder_structure,))
        if self.cap_priors.get("user", False) or self.cap_priors.get("item", False):
            raise NotImplementedError("BiVAECF here supports the standard normal prior only: cap_priors must be false for "
                                      "both sides, got %r" % (self.cap_priors,))
        if self.act_fn not in _lib.BivaeModel.ACTS:
            raise ValueError("Supported act_fn: {}".format(_lib.BivaeModel.ACTS))
        if self.likelihood not in _lib.BivaeModel.LIKELIHOODS:
            raise ValueError("Supported likelihoods: {}".format(_lib.BivaeModel.LIKELIHOODS))
        return int(self.encoder_structure[0])

    @staticmethod
    def _initial_tables(n_users, n_items, k, h):
        """bivae.py:48-86 in construction order, from torch's generator as it stands"""
        import torch

        theta = torch.randn(n_users, k) * 0.01
        beta = torch.randn(n_items, k) * 0.01
        torch.nn.init.kaiming_uniform_(theta, a=np.sqrt(5))
        layers = [torch.nn.Linear(*io) for io in ((n_items, h), (h, k), (h, k), (n_users, h), (h, k), (h, k))]
        tables = OrderedDict()
        for q, layer in enumerate(layers):
            tables[NAMES[2 * q]] = layer.weight.detach().numpy().astype(np.float32).copy()
            tables[NAMES[2 * q + 1]] = layer.bias.detach().numpy().astype(np.float32).copy()
        return BiVAETables(tables, theta.numpy(), beta.numpy(), np.zeros((n_users, k), np.float32), np.zeros((n_items, k), np.float32))

    def fit(self, train_set, val_set=None):
        """recom_bivaecf.py:116-191; a second fit continues from the model's tables and factor tables, with two new Adam
        as learn() builds them"""
        Recommender.fit(self, train_set, val_set)
        if not self.trainable:
            if self.verbose:
                print("%s is trained already (trainable = False)" % (self.name))
            return self
        h = self._check_structure()
        import torch

        if self.seed is not None:
            torch.manual_seed(self.seed)
        self.r_mat = train_set.matrix
        n_users, n_items = self.r_mat.shape
        k, bs = int(self.k), int(self.batch_size)
        if not hasattr(self, "bivae"):
            self.bivae = self._initial_tables(n_users, n_items, k, h)
        model = _lib.BivaeModel(self.r_mat, k, h, self.act_fn, self.likelihood, device=self.device)
        try:
            self._fill(model)
            device_seed = int(np.random.SeedSequence().entropy % (1 << 63)) if self.seed is None else 0
            self.loss_history = []
            for epoch in range(int(self.n_epochs)):
                eps = [None, None]
                if self.seed is not None:   # bivae.py:204, 220 and :234, 250: two draws per batch, items first
                    for q, n in enumerate((n_items, n_users)):
                        eps[q] = np.empty((2, n, k), np.float32)
                        for r0 in range(0, n, bs):
                            for draw in range(2):
                                eps[q][draw, r0:r0 + bs] = torch.randn(min(bs, n - r0), k).numpy()
                loss_i, loss_u, _ = model.fit_epoch(bs, self.learning_rate, self.beta_kl, eps_item=eps[0], eps_user=eps[1],
                                                    seed=device_seed)
                self.loss_history.append((loss_i / n_items, loss_u / n_users))   # (the progress bar's figures, bivae.py:254-256)
                if self.verbose:
                    print("%s epoch %d: loss_i %.6g loss_u %.6g" % ((self.name, epoch + 1) + self.loss_history[-1]))
            model.infer_means()
            self.bivae = BiVAETables(model.get_params(), **model.get_factors())
        except Exception:
            model.close()
            raise
        self._keep_handle(model)   # its tables are self.bivae's already: kept for scoring
        return self

    # ---- the reference's extras -------------------------------------------------------------------
    def get_user_vectors(self):
        """recom_bivaecf.py:237-246: mu_theta"""
        return self.bivae.mu_theta

    def get_item_vectors(self):
        """recom_bivaecf.py:248-257: mu_beta"""
        return self.bivae.mu_beta

    # ---- prediction (recom_bivaecf.py:193-225) ------------------------------------------------------
    _HANDLE_ATTRS = ("_bivae_handle", "_bivae_key")   # (`_scorer` is the fused factor scorer that the orderings use)
    _scorer_row_count = Recommender._scorer_row_count
    batch_num_items = Recommender.batch_num_items
    register_exclusions = Recommender.register_exclusions

    def _handle_key(self):
        X = self.r_mat
        return (id(X),) + tuple(_table_fingerprint(a) for a in (X.indptr, X.indices)) + tuple(
            _table_fingerprint(self.bivae.tables[n]) for n in NAMES) + tuple(_table_fingerprint(getattr(self.bivae, n)) for n in FACTORS)

    def _build_handle(self):
        model = _lib.BivaeModel(self.r_mat, self.k, self._check_structure(), self.act_fn, self.likelihood, device=self.device)
        return filled_handle(model, self._fill)

    def _fill(self, model):
        model.set_params(self.bivae.tables)
        model.set_factors(**{n: getattr(self.bivae, n) for n in FACTORS})

    def _pair_values(self, handle, users, items):
        """recom_bivaecf.py:221-225: the pair's probability scaled from [0, 1] to [min_rating, max_rating]"""
        p = handle.score_pairs(users, items).astype(np.float64)
        return p * (self.max_rating - self.min_rating) + self.min_rating

    def _scoring_tables(self):
        """(mu_theta, mu_beta, zeros, zeros): the logits as a factor model"""
        cached = self.__dict__.get("_rank_tables")
        if cached is None or cached[0] is not self.bivae.mu_theta or cached[1] is not self.bivae.mu_beta:
            cached = (self.bivae.mu_theta, self.bivae.mu_beta, np.zeros(len(self.bivae.mu_beta), np.float32),
                      np.zeros(len(self.bivae.mu_theta), np.float32))
            self._rank_tables = cached
        return cached
