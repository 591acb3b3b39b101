"""VAECF on MI355X — constructor, `fit/score/rank` surface and `state_dict` of the reference's `cornac.models.VAECF`
(cornac/models/vaecf/recom_vaecf.py:22-202, vaecf.py:37-149; Liang et al. 2018, "Mult-VAE").  What the reference runs per
batch in torch on densified rows — forward, backward and Adam's dense sweep — and per user in `score()` runs in
libcornac_hip (`_lib.VaecfModel`), in float32 like there, on the sparse binary rows.

Seeded fits follow the reference's CPU run to rounding: with a seed the model calls `torch.manual_seed(seed)`, builds five
`torch.nn.Linear` layers on the CPU in the reference's construction order (encoder fc0, enc_mu, enc_logvar, decoder fc0,
decoder fc1) for the reference's initial bits, and draws each batch's noise on the host, one `torch.randn(B, k)` per batch,
which is what `randn_like(mu)` draws there (torch is the generator here, nothing else of it is used).  Without a seed the
noise comes from the device generator.

Stated departure: `autoencoder_structure` must have length 1 (NotImplementedError otherwise).

Orderings (`rank`, `rank_batch`, `ranking_eval`) come from the decoder's LOGITS c1[i] + <h2(u), D1[i]> through the fused
factor-model scorer: softmax and sigmoid are monotone, so that is the order of `score()`, except where float32
probabilities tie and the logits do not.  `score`, `score_batch` and `rate_batch` return probabilities."""
from collections import OrderedDict

import numpy as np

from . import _lib
from .recommender import HandleScoredRecommender, Recommender, _table_fingerprint, check_table_shapes, filled_handle, float32_tables


class VAECF(HandleScoredRecommender):
    """Variational autoencoder for collaborative filtering.  Parameters are the reference's (recom_vaecf.py:25-79): `k` the
    size of z, `autoencoder_structure` the hidden layer `[h]`, `act_fn` in tanh / sigmoid / relu / relu6 / elu, `likelihood`
    in mult / bern / gaus / pois, `n_epochs`, `batch_size`, `learning_rate` (Adam), `beta` (the KL weight), `seed`;
    `use_gpu` is accepted and ignored (the model always trains on the GPU `device`).  Learned: `vae`, the ten tables as
    float32 arrays on the host under the reference's state_dict names, and `r_mat`, the training CSR."""
    NAMES = _lib.VaecfModel.NAMES

    def __init__(self, name="VAECF", k=10, autoencoder_structure=[20], act_fn="tanh", likelihood="mult", n_epochs=100,
                 batch_size=100, learning_rate=0.001, beta=1.0, trainable=True, verbose=False, seed=None, use_gpu=False,
                 device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.k = k
        self.autoencoder_structure = autoencoder_structure
        self.act_fn = act_fn
        self.likelihood = likelihood
        self.batch_size = batch_size
        self.n_epochs = n_epochs
        self.learning_rate = learning_rate
        self.beta = beta
        self.seed = seed
        self.use_gpu = use_gpu
        self.device = device
        self.ignored_attrs = self.ignored_attrs + ["_vae_handle", "_vae_key", "_rank_tables"]

    # ---- fit --------------------------------------------------------------------------------------
    def _check_structure(self):
        if len(self.autoencoder_structure) != 1:
            raise NotImplementedError("VAECF here supports one hidden layer: autoencoder_structure must have length 1, got %r"
                                      % (self.autoencoder_structure,))
        if self.act_fn not in _lib.VaecfModel.ACTS:
            raise ValueError("Supported act_fn: {}".format(_lib.VaecfModel.ACTS))
        if self.likelihood not in _lib.VaecfModel.LIKELIHOODS:
            raise ValueError("Supported likelihoods: {}".format(_lib.VaecfModel.LIKELIHOODS))
        return int(self.autoencoder_structure[0])

    @staticmethod
    def _initial_tables(n_items, k, h):
        """vaecf.py:46-64: five nn.Linear layers in construction order, from torch's generator as it stands"""
        import torch

        layers = [torch.nn.Linear(*io) for io in ((n_items, h), (h, k), (h, k), (k, h), (h, n_items))]
        out = OrderedDict()
        for q, layer in enumerate(layers):
            out[VAECF.NAMES[2 * q]] = layer.weight.detach().numpy().astype(np.float32).copy()
            out[VAECF.NAMES[2 * q + 1]] = layer.bias.detach().numpy().astype(np.float32).copy()
        return out

    def fit(self, train_set, val_set=None):
        """recom_vaecf.py:109-165; a second fit continues from the model's weights, with a new Adam as there"""
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
        if not hasattr(self, "vae"):
            self.vae = self._initial_tables(n_items, int(self.k), h)
        model = _lib.VaecfModel(self.r_mat, self.k, h, self.act_fn, self.likelihood, device=self.device)
        try:
            model.set_params(self.vae)
            device_seed = int(np.random.SeedSequence().entropy % (1 << 63)) if self.seed is None else 0
            self.loss_history = []
            bs = int(self.batch_size)
            for epoch in range(int(self.n_epochs)):
                eps = None
                if self.seed is not None:   # vaecf.py:79, one draw per batch
                    eps = np.concatenate([torch.randn(min(bs, n_users - u0), int(self.k)).numpy() for u0 in range(0, n_users, bs)])
                total, _ = model.fit_epoch(bs, self.learning_rate, self.beta, eps=eps, seed=device_seed)
                self.loss_history.append(total / n_users)   # (the progress bar's figure, vaecf.py:147)
                if self.verbose:
                    print("%s epoch %d: loss %.6g" % (self.name, epoch + 1, self.loss_history[-1]))
            self.vae = OrderedDict((n, a) for n, a in model.get_params().items())
        except Exception:
            model.close()
            raise
        self._keep_handle(model)   # its tables are self.vae already: kept for scoring
        return self

    # ---- the tables -------------------------------------------------------------------------------
    def state_dict(self):
        """the ten tables under the reference's names and shapes (copies): they load into the reference's VAE"""
        return OrderedDict((n, self.vae[n].copy()) for n in self.NAMES)

    def load_state_dict(self, state):
        """tables (arrays or torch tensors) under the reference's names; shapes must agree with each other"""
        if set(state) != set(self.NAMES):
            raise KeyError("state_dict needs exactly the keys %r" % (self.NAMES,))
        tabs = float32_tables(state, self.NAMES)
        h, n_items = tabs[self.NAMES[0]].shape
        k = tabs[self.NAMES[2]].shape[0]
        check_table_shapes(tabs, _lib.VaecfModel.shapes(n_items, k, h))
        self.vae = tabs
        self.k, self.autoencoder_structure = k, [h]
        self._drop_scorer()

    # ---- prediction (recom_vaecf.py:167-202: decode(mu(x_u)), or its entry for one item) -----------
    _HANDLE_ATTRS = ("_vae_handle", "_vae_key")   # (`_scorer` is the fused factor scorer over h2 that the orderings use)
    _scorer_row_count = Recommender._scorer_row_count
    batch_num_items = Recommender.batch_num_items
    register_exclusions = Recommender.register_exclusions

    def _handle_key(self):
        X = self.r_mat
        return (id(X),) + tuple(_table_fingerprint(a) for a in (X.indptr, X.indices)) + tuple(
            _table_fingerprint(self.vae[n]) for n in self.NAMES)

    def _build_handle(self):
        model = _lib.VaecfModel(self.r_mat, self.k, self._check_structure(), self.act_fn, self.likelihood, device=self.device)
        return filled_handle(model, lambda m: m.set_params(self.vae))

    def _scoring_tables(self):
        """(h2 of every user at z = mu, D1, c1, zeros): the decoder's logits as a factor model"""
        handle = self._handle()
        cached = self.__dict__.get("_rank_tables")
        if cached is None or cached[0] != self._vae_key:
            H2 = handle.encode_users(np.arange(self.num_users, dtype=np.int32))
            cached = (self._vae_key, (H2, self.vae[self.NAMES[8]], self.vae[self.NAMES[9]], np.zeros(self.num_users, np.float32)))
            self._rank_tables = cached
        return cached[1]
