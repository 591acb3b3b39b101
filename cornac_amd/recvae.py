"""RecVAE on MI355X — constructor, `fit/score/rank` surface and `state_dict` of the reference's `cornac.models.RecVAE`
(cornac/models/recvae/recom_recvae.py:23-278, recvae.py:9-117; Shenbin et al. 2020).  What the reference runs per batch in
torch on densified rows — the five-layer encoder, the composite prior, backward and the two Adams' dense sweeps — and per
user in `score()` runs in libcornac_hip (`_lib.RecvaeModel`), in float32 like there, on the sparse rows with their values.

Seeded fits follow the reference's CPU run to rounding: with a seed the model calls `torch.manual_seed(seed)`, builds the
reference's layers on the CPU in its construction order (encoder fc1, ln1 .. fc5, ln5, fc_mu, fc_logvar, then the old
encoder's own set, then the decoder) for the initial bits, and draws per step what the reference draws, in its order: the
dropout mask as `torch.empty(B, n_items).bernoulli_(1 - p)` where the rate is not zero, then the noise as
`torch.zeros(B, latent).normal_(mean=0, std=0.01)` (torch is the generator here, nothing else of it is used).  Between outer
epochs the reference's evaluation scores every user with a positive rating in training mode, which consumes one mask of
`[1, n_items]` and one noise row per user: the same draws are made and thrown away here.  Without a seed masks and noise
come from the device generator, and the batch order from the data set's rng in both cases.

Stated departures, where the reference is odd:
  * scoring mode: the reference never leaves `model.train()`, so its `score()` applies dropout 0.5 and noise and is random.
    Here `score`, `score_batch` and the `rank*` family use evaluation semantics: no dropout, z = mu.  `score(u)` returns the
    decoder's logits, as there (no softmax).
  * KL weight: with `gamma` and `beta` both falsy the reference dies on an unbound name; here `fit` raises ValueError before
    it touches the device.
  * per-epoch evaluation: the reference runs `ranking_eval(NDCG@100)` over the training set after every outer epoch only to
    label the progress bar; here that runs only when `verbose`.
  * `use_gpu` is accepted and ignored (the model always trains on the GPU `device`).

Orderings (`rank`, `rank_batch`, `ranking_eval`) come from decoder.bias[i] + <mu(u), decoder.weight[i]> through the fused
factor-model scorer: the same numbers as `score()` up to the order of a float32 sum."""
from collections import OrderedDict

import numpy as np

from . import _lib
from .recommender import HandleScoredRecommender, Recommender, _table_fingerprint, check_table_shapes, filled_handle, float32_tables


class RecVAE(HandleScoredRecommender):
    """Parameters are the reference's (recom_recvae.py:27-72): `hidden_dim`, `latent_dim`, `batch_size`, `beta` (a scalar KL
    weight, used where `gamma` is falsy), `gamma` (KL weight per unit of a user's rating sum), `lr` (both Adams), `n_epochs`
    outer epochs of `n_enc_epochs` encoder passes, `update_prior` and `n_dec_epochs` decoder passes (`not_alternating`: one
    joint pass, the prior never updated), `seed`.  Learned: `recvae`, the 53 tables as float32 arrays on the host under the
    reference's state_dict names, `r_mat`, the training CSR, and `loss_history`, per pass the mean of the steps'
    negative_elbo."""
    NAMES = _lib.RecvaeModel.NAMES

    def __init__(self, name="RecVae", hidden_dim=600, latent_dim=200, batch_size=500, beta=None, gamma=0.005, lr=5e-4, n_epochs=50,
                 n_enc_epochs=3, n_dec_epochs=1, not_alternating=False, trainable=True, verbose=False, seed=None, use_gpu=True,
                 device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.hidden_dim = hidden_dim
        self.latent_dim = latent_dim
        self.batch_size = batch_size
        self.beta = beta
        self.gamma = gamma
        self.lr = lr
        self.n_epochs = n_epochs
        self.n_enc_epochs = n_enc_epochs
        self.n_dec_epochs = n_dec_epochs
        self.not_alternating = not_alternating
        self.seed = seed
        self.use_gpu = use_gpu
        self.device = device
        self.ignored_attrs = self.ignored_attrs + ["_recvae_handle", "_recvae_key", "_rank_tables"]

    # ---- fit --------------------------------------------------------------------------------------
    @staticmethod
    def _initial_tables(n_items, hidden, latent):
        """recvae.py:16-32, 49-64, 78-84: the reference's layers in construction order, from torch's generator as it stands"""
        import torch

        def encoder():
            tabs = []
            for l in range(1, 6):
                fc = torch.nn.Linear(n_items if l == 1 else hidden, hidden)
                tabs += [fc.weight.detach().numpy(), fc.bias.detach().numpy(), np.ones(hidden), np.zeros(hidden)]   # (LayerNorm draws nothing)
            for _ in range(2):
                fc = torch.nn.Linear(hidden, latent)
                tabs += [fc.weight.detach().numpy(), fc.bias.detach().numpy()]
            return tabs

        enc, old = encoder(), encoder()
        dec = torch.nn.Linear(latent, n_items)
        priors = [np.zeros((1, latent)), np.zeros((1, latent)), np.full((1, latent), 10.0)]   # recvae.py:22-29
        tabs = enc + priors + old + [dec.weight.detach().numpy(), dec.bias.detach().numpy()]
        return OrderedDict((n, np.array(t, np.float32)) for n, t in zip(RecVAE.NAMES, tabs))

    def _model(self, X):
        return _lib.RecvaeModel(X, self.hidden_dim, self.latent_dim, device=self.device)

    def _pass(self, model, train_set, dropout_rate, step_encoder, step_decoder, device_seed):
        """recom_recvae.py:131-145, one pass: the order from the data set, the draws from torch where seeded"""
        X, bs = self.r_mat, int(self.batch_size)
        order = np.concatenate(list(train_set.user_iter(bs, shuffle=True))).astype(np.int32)
        keep = eps = None
        if self.seed is not None:
            import torch

            n_users, n_items = X.shape
            keep = np.ones(X.nnz, np.uint8) if dropout_rate else None
            eps = np.zeros((n_users, int(self.latent_dim)), np.float32)
            for p0 in range(0, n_users, bs):
                users = order[p0:p0 + bs]
                if dropout_rate:   # (F.dropout's mask, recvae.py:68; a rate of 0 draws nothing)
                    mask = torch.empty(len(users), n_items).bernoulli_(1 - dropout_rate).numpy()
                    for b, u in enumerate(users):
                        lo, hi = X.indptr[u], X.indptr[u + 1]
                        keep[lo:hi] = mask[b, X.indices[lo:hi]] != 0
                eps[users] = torch.zeros(len(users), int(self.latent_dim)).normal_(mean=0, std=0.01).numpy()   # recvae.py:89
        steps = model.fit_epoch(order, bs, self.lr, self.gamma, self.beta, dropout_rate, step_encoder, step_decoder, keep=keep, eps=eps,
                                seed=device_seed)
        self.loss_history.append(float(steps[:, 2].mean()))
        if self.verbose:
            print("%s pass %d: negative_elbo %.6g" % (self.name, len(self.loss_history), self.loss_history[-1]))

    def _burn_evaluation_draws(self):
        """recom_recvae.py:222-227: one training-mode score() per user with a rating >= 1 (base_method.py:176-210), each a
        dropout mask of the row and a noise row (recom_recvae.py:261, recvae.py:68, 89)"""
        import torch

        X = self.r_mat
        n_items = X.shape[1]
        for u in range(X.shape[0]):
            if (X.data[X.indptr[u]:X.indptr[u + 1]] >= 1.0).any():
                torch.empty(1, n_items).bernoulli_(0.5)
                torch.zeros(1, int(self.latent_dim)).normal_(mean=0, std=0.01)

    def fit(self, train_set, val_set=None):
        """recom_recvae.py:148-239; a second fit continues from the model's weights, with new Adams as there"""
        Recommender.fit(self, train_set, val_set)
        if not self.trainable:
            if self.verbose:
                print("%s is trained already (trainable = False)" % (self.name))
            return self
        if not self.gamma and not self.beta:
            raise ValueError("RecVAE needs a KL weight: gamma or beta must be set and not zero")
        if self.seed is not None:
            import torch

            torch.manual_seed(self.seed)
        self.r_mat = train_set.matrix
        n_users, n_items = self.r_mat.shape
        if not hasattr(self, "recvae"):
            self.recvae = self._initial_tables(n_items, int(self.hidden_dim), int(self.latent_dim))
        model = self._model(self.r_mat)
        try:
            model.set_params(self.recvae)
            device_seed = int(np.random.SeedSequence().entropy % (1 << 63)) if self.seed is None else 0
            self.loss_history = []
            for epoch in range(int(self.n_epochs)):
                if self.not_alternating:
                    self._pass(model, train_set, 0.5, True, True, device_seed)
                else:
                    for _ in range(int(self.n_enc_epochs)):
                        self._pass(model, train_set, 0.5, True, False, device_seed)
                    model.update_prior()
                    for _ in range(int(self.n_dec_epochs)):
                        self._pass(model, train_set, 0, False, True, device_seed)
                if self.seed is not None and epoch + 1 < int(self.n_epochs):
                    self._burn_evaluation_draws()
                if self.verbose:   # (the training handle scores for the evaluation, then goes on training)
                    params = model.get_params()
                    self.recvae = OrderedDict((n, params[n]) for n in self.NAMES)
                    self._keep_handle(model)
                    from .eval import ranking_eval
                    from .metrics import NDCG

                    print("%s epoch %d: ndcg100 %.6g" % (self.name, epoch + 1, ranking_eval(self, [NDCG(k=100)], train_set, train_set)[0][0]))
            params = model.get_params()
            self.recvae = OrderedDict((n, params[n]) for n in self.NAMES)
        except Exception:
            model.close()
            raise
        self._keep_handle(model)   # its tables are self.recvae already: kept for scoring
        return self

    # ---- the tables -------------------------------------------------------------------------------
    def state_dict(self):
        """the 53 tables under the reference's names and shapes (copies): they load into the reference's VAE"""
        return OrderedDict((n, self.recvae[n].copy()) for n in self.NAMES)

    def load_state_dict(self, state):
        """tables (arrays or torch tensors) under the reference's names; shapes must agree with each other"""
        if set(state) != set(self.NAMES):
            raise KeyError("state_dict needs exactly the keys %r" % (self.NAMES,))
        tabs = float32_tables(state, self.NAMES)
        hidden, n_items = tabs["encoder.fc1.weight"].shape
        latent = tabs["encoder.fc_mu.weight"].shape[0]
        check_table_shapes(tabs, _lib.RecvaeModel.shapes(n_items, hidden, latent))
        self.recvae = tabs
        self.hidden_dim, self.latent_dim = hidden, latent
        self._drop_scorer()

    # ---- prediction (recom_recvae.py:241-278 in evaluation mode: decoder(mu(x_u)), or its entry for one item) -----------
    _HANDLE_ATTRS = ("_recvae_handle", "_recvae_key")   # (`_scorer` is the fused factor scorer over mu that the orderings use)
    _scorer_row_count = Recommender._scorer_row_count
    batch_num_items = Recommender.batch_num_items
    register_exclusions = Recommender.register_exclusions

    def _handle_key(self):
        X = self.r_mat
        return (id(X),) + tuple(_table_fingerprint(a) for a in (X.indptr, X.indices, X.data)) + tuple(
            _table_fingerprint(self.recvae[n]) for n in self.NAMES)

    def _build_handle(self):
        return filled_handle(self._model(self.r_mat), lambda m: m.set_params(self.recvae))

    def _scoring_tables(self):
        """(mu of every user, decoder.weight, decoder.bias, zeros): the decoder's logits as a factor model"""
        handle = self._handle()
        cached = self.__dict__.get("_rank_tables")
        if cached is None or cached[0] != self._recvae_key:
            mu = handle.encode_users(np.arange(self.num_users, dtype=np.int32))
            cached = (self._recvae_key, (mu, self.recvae["decoder.weight"], self.recvae["decoder.bias"], np.zeros(self.num_users, np.float32)))
            self._rank_tables = cached
        return cached[1]
