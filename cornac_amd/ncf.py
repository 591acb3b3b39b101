"""Neural collaborative filtering on MI355X — `GMF`, `MLP` and `NeuMF` with the constructors, the `fit/score/rank` surface
and the `state_dict` of the reference's `cornac.models.GMF / MLP / NeuMF` (cornac/models/ncf/recom_gmf.py, recom_mlp.py,
recom_neumf.py, recom_ncf_base.py:240-293, backend_pt.py:22-175; He et al. 2017).  What the reference runs per batch in
torch — forward, BCE, backward and the optimiser's dense pass over every table — and per user in `score()` runs in
libcornac_hip (`_lib.NcfModel`), in float32 like there.

Seeded fits follow the reference's CPU run of its PyTorch backend to rounding: with a seed the model calls
`torch.manual_seed(seed)`, builds the reference's layers with `torch.nn` on the CPU in its construction order for its initial
bits (for NeuMF: the final logit, GMF's two embeddings and logit and their `normal_`, MLP's embeddings, layers and logit and
their inits, then `normal_` on the final logit's weight), takes each epoch's batches from
`train_set.uir_iter(batch_size, shuffle=True, binary=True, num_zeros=num_neg)` (the reference's sampler, restated draw for
draw in `Dataset`) and hands the whole epoch to the device in one call.  Without a seed the initial draws are the same kind
and the epoch's samples are drawn on the device (`fit_epoch_sampled`): every stored entry once in a permuted order, each
followed by `num_neg` items uniform among those the user has not rated positively.

Stated departures:
  * `backend` is accepted and ignored: the model always has the PyTorch backend's semantics (its initialisation, its
    `weight_decay` form of `reg`, its dense optimiser passes), on the GPU `device`.
  * `early_stopping` other than None raises NotImplementedError at `fit`.
  * `verbose` defaults to True as in the reference, but prints one line per epoch instead of a progress bar.
  * `save` / `load` work (the tables are host arrays); the reference's PyTorch backend raises there.

`score`, `score_batch` and `rate_batch` return probabilities.  GMF's logit is a factor model, sum_f w_f p_uf q_if + b, so its
orderings (`rank`, `rank_batch`, the evaluators) come from the LOGITS through the fused factor-model scorer: the sigmoid is
monotone, so that is the order of `score()`, except where float32 probabilities tie and the logits do not.  MLP and NeuMF
take the per-user flow over `score_users`."""
from collections import OrderedDict

import numpy as np
import scipy.sparse as sp

from . import _lib
from .recommender import HandleScoredRecommender, Recommender, _table_fingerprint, check_table_shapes, filled_handle, float32_tables


def _f32(t):
    return t.detach().numpy().astype(np.float32).copy()


def _gmf_initial(n_users, n_items, f):
    """backend_pt.py:33-44: the layers in construction order, then their normal_ (std 0.01), from torch's generator as it stands"""
    import torch

    ue, ie, logit = torch.nn.Embedding(n_users, f), torch.nn.Embedding(n_items, f), torch.nn.Linear(f, 1)
    for t in (ue.weight, ie.weight, logit.weight):
        torch.nn.init.normal_(t, std=1e-2)
    return OrderedDict(zip(_lib.NcfModel.NAMES("GMF"), (_f32(ue.weight), _f32(ie.weight), _f32(logit.weight), _f32(logit.bias))))


def _mlp_initial(n_users, n_items, layers):
    """backend_pt.py:73-95: embeddings, the Linear layers, the logit; then normal_ / xavier_uniform_ / normal_"""
    import torch

    half = layers[0] // 2
    ue, ie = torch.nn.Embedding(n_users, half), torch.nn.Embedding(n_items, half)
    lin = [torch.nn.Linear(layers[l], layers[l + 1]) for l in range(len(layers) - 1)]
    logit = torch.nn.Linear(layers[-1], 1)
    torch.nn.init.normal_(ue.weight, std=1e-2)
    torch.nn.init.normal_(ie.weight, std=1e-2)
    for layer in lin:
        torch.nn.init.xavier_uniform_(layer.weight)
    torch.nn.init.normal_(logit.weight, std=1e-2)
    tabs = [_f32(ue.weight), _f32(ie.weight)]
    for layer in lin:
        tabs += [_f32(layer.weight), _f32(layer.bias)]
    tabs += [_f32(logit.weight), _f32(logit.bias)]
    return OrderedDict(zip(_lib.NcfModel.NAMES("MLP", layers), tabs))


def _neumf_initial(n_users, n_items, f, layers):
    """backend_pt.py:141-149: the final logit first, then GMF, then MLP, then normal_ on the final logit's weight"""
    import torch

    logit = torch.nn.Linear(f + layers[-1], 1)
    gmf = _gmf_initial(n_users, n_items, f)
    mlp = _mlp_initial(n_users, n_items, layers)
    torch.nn.init.normal_(logit.weight, std=1e-2)
    out = OrderedDict((("logit.weight", _f32(logit.weight)), ("logit.bias", _f32(logit.bias))))
    out.update(("gmf." + n, a) for n, a in gmf.items())
    out.update(("mlp." + n, a) for n, a in mlp.items())
    return out


class _NCF(HandleScoredRecommender):
    """What the three models share (recom_ncf_base.py:25-110): the training loop's arguments, the epoch, the tables.  Learned:
    `params`, the tables as float32 arrays on the host under the reference's state_dict names."""
    KIND = None
    _HANDLE_ATTRS = ("_ncf_handle", "_ncf_key")

    def _init_common(self, num_epochs, batch_size, num_neg, lr, learner, backend, early_stopping, seed, device):
        self.num_epochs = num_epochs
        self.batch_size = batch_size
        self.num_neg = num_neg
        self.lr = lr
        self.learner = learner
        self.backend = backend
        self.early_stopping = early_stopping
        self.seed = seed
        self.device = device
        self.ignored_attrs = self.ignored_attrs + ["_ncf_handle", "_ncf_key", "_rank_tables", "pretrained_gmf", "pretrained_mlp"]

    # ---- the shape ----------------------------------------------------------------------------------
    def _factors(self):
        return 0 if self.KIND == "MLP" else int(self.num_factors)

    def _layers(self):
        return () if self.KIND == "GMF" else tuple(int(x) for x in self.layers)

    def _act(self):
        return "relu" if self.KIND == "GMF" else str(self.act_fn).lower()

    def _names(self):
        return _lib.NcfModel.NAMES(self.KIND, self._layers())

    def _check(self):
        if self.early_stopping is not None:
            raise NotImplementedError("%s here has no early stopping: early_stopping must be None" % self.name)
        if str(self.learner).lower() not in _lib.NcfModel.LEARNERS:
            raise ValueError("Supported learners: {}".format(_lib.NcfModel.LEARNERS))
        if self._act() not in _lib.NcfModel.ACTS:
            raise ValueError("Supported act_fn: {}".format(_lib.NcfModel.ACTS))
        if self.KIND == "NeuMF" and self._layers()[-1] != self._factors():
            raise ValueError("NeuMF: layers[-1] = %d must equal num_factors = %d" % (self._layers()[-1], self._factors()))

    def _initial_tables(self, n_users, n_items):
        if self.KIND == "GMF":
            return _gmf_initial(n_users, n_items, self._factors())
        if self.KIND == "MLP":
            return _mlp_initial(n_users, n_items, self._layers())
        return _neumf_initial(n_users, n_items, self._factors(), self._layers())

    def _new_model(self, X):
        return _lib.NcfModel(self.KIND, X, self._factors(), self._layers(), self._act(), device=self.device)

    # ---- fit ----------------------------------------------------------------------------------------
    def fit(self, train_set, val_set=None):
        """recom_ncf_base.py:111-139, 240-293: every fit starts from new tables and a new optimiser, as there"""
        Recommender.fit(self, train_set, val_set)
        if not self.trainable:
            if self.verbose:
                print("%s is trained already (trainable = False)" % (self.name))
            return self
        self._check()
        import torch

        if self.seed is not None:
            torch.manual_seed(self.seed)
        X = train_set.matrix
        n_users, n_items = X.shape
        params = self._initial_tables(n_users, n_items)
        self._drop_scorer()
        model = self._new_model(X)
        try:
            model.set_params(params)
            learner, bs, nn = str(self.learner).lower(), int(self.batch_size), int(self.num_neg)
            device_seed = int(np.random.SeedSequence().entropy % (1 << 63)) if self.seed is None else 0
            self.loss_history = []
            for epoch in range(int(self.num_epochs)):
                if self.seed is not None:   # the reference's sampler, one epoch of batches handed over as a whole
                    bu, bi, br, ptr = [], [], [], [0]
                    for u, i, r in train_set.uir_iter(bs, shuffle=True, binary=True, num_zeros=nn):
                        bu.append(u); bi.append(i); br.append(r); ptr.append(ptr[-1] + len(u))
                    ptr = np.asarray(ptr, np.int64)
                    _, steps = model.fit_epoch(ptr, np.concatenate(bu), np.concatenate(bi), np.concatenate(br), self.lr, self.reg, learner)
                else:
                    _, steps = model.fit_epoch_sampled(bs, nn, self.lr, self.reg, learner, seed=device_seed, epoch=epoch)
                    ptr = np.minimum(np.arange(len(steps) + 1, dtype=np.int64) * bs, model.nnz) * (1 + nn)
                count = np.diff(ptr).astype(np.float64)
                self.loss_history.append(float((steps * count).sum() / count.sum()))   # recom_ncf_base.py:283-287
                if self.verbose:
                    print("%s epoch %d: loss %.6g" % (self.name, epoch + 1, self.loss_history[-1]))
            self.params = OrderedDict((n, a) for n, a in model.get_params().items())
        except Exception:
            model.close()
            raise
        self._keep_handle(model)   # its tables are self.params already: kept for scoring
        return self

    # ---- the tables ---------------------------------------------------------------------------------
    def state_dict(self):
        """the tables under the reference's names and shapes (copies): they load into the reference's module"""
        return OrderedDict((n, self.params[n].copy()) for n in self._names())

    def _shape_from(self, tabs):
        """(n_users, n_items, num_factors, layers) that the tables' shapes describe"""
        pre = "mlp." if self.KIND == "NeuMF" else ""
        gpre = "gmf." if self.KIND == "NeuMF" else ""
        layers, f = (), 0
        if self.KIND != "GMF":
            layers, l = (tabs[pre + "mlp_model.0.weight"].shape[1],), 0
            while pre + "mlp_model.%d.weight" % (2 * l) in tabs:
                layers += (tabs[pre + "mlp_model.%d.weight" % (2 * l)].shape[0],)
                l += 1
        if self.KIND != "MLP":
            f = tabs[gpre + "user_embedding.weight"].shape[1]
        emb = (gpre if self.KIND != "MLP" else pre)
        return tabs[emb + "user_embedding.weight"].shape[0], tabs[emb + "item_embedding.weight"].shape[0], f, layers

    def load_state_dict(self, state):
        """tables (arrays or torch tensors) under the reference's names; shapes must agree with each other"""
        tabs = float32_tables(state)
        try:
            n_users, n_items, f, layers = self._shape_from(tabs)
        except (KeyError, IndexError):
            raise KeyError("state_dict needs exactly the keys %r" % (self._names(),))
        names = _lib.NcfModel.NAMES(self.KIND, layers)
        if set(tabs) != set(names):
            raise KeyError("state_dict needs exactly the keys %r" % (names,))
        check_table_shapes(tabs, _lib.NcfModel.shapes(self.KIND, n_users, n_items, f, layers))
        if self.KIND != "MLP":
            self.num_factors = f
        if self.KIND != "GMF":
            self.layers = layers
        self.params = OrderedDict((n, tabs[n]) for n in names)
        self._drop_scorer()

    # ---- prediction ---------------------------------------------------------------------------------
    def _handle_key(self):
        return tuple(_table_fingerprint(self.params[n]) for n in self._names())

    def _build_handle(self):
        """scoring needs the tables alone: the handle gets a matrix without entries"""
        n_users, n_items = self._shape_from(self.params)[:2]
        model = self._new_model(sp.csr_matrix((n_users, n_items), dtype=np.float64))
        return filled_handle(model, lambda m: m.set_params(self.params))


class GMF(_NCF):
    """Generalized matrix factorization.  Parameters are the reference's (recom_gmf.py:22-109): `num_factors`, `reg` (torch's
    weight_decay), `num_epochs`, `batch_size`, `num_neg`, `lr`, `learner` in adam / sgd / rmsprop / adagrad, `seed`;
    `backend` is accepted and ignored, `early_stopping` must be None."""
    KIND = "GMF"

    def __init__(self, name="GMF", num_factors=8, reg=0.0, num_epochs=20, batch_size=256, num_neg=4, lr=0.001, learner="adam",
                 backend="tensorflow", early_stopping=None, trainable=True, verbose=True, seed=None, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.num_factors = num_factors
        self.reg = reg
        self._init_common(num_epochs, batch_size, num_neg, lr, learner, backend, early_stopping, seed, device)

    # the orderings go through the fused factor scorer (`_scorer`) on the logits
    _scorer_row_count = Recommender._scorer_row_count
    batch_num_items = Recommender.batch_num_items
    register_exclusions = Recommender.register_exclusions

    def _scoring_tables(self):
        """(P * w, Q, b, zeros): the logit sum_f w_f p_uf q_if + b as a factor model"""
        key = self._handle_key()
        cached = self.__dict__.get("_rank_tables")
        if cached is None or cached[0] != key:
            P, Q, w, b = (self.params[n] for n in self._names())
            cached = (key, (np.ascontiguousarray(P * w.reshape(1, -1), np.float32), Q,
                            np.full(Q.shape[0], b.reshape(-1)[0], np.float32), np.zeros(P.shape[0], np.float32)))
            self._rank_tables = cached
        return cached[1]


class MLP(_NCF):
    """Multi-layer perceptron.  Parameters are the reference's (recom_mlp.py:22-114): `layers` (layers[0] / 2 is the embedding
    size), `act_fn` in sigmoid / tanh / elu / selu / relu / relu6 / leaky_relu, and GMF's training arguments."""
    KIND = "MLP"

    def __init__(self, name="MLP", layers=(64, 32, 16, 8), act_fn="relu", reg=0.0, num_epochs=20, batch_size=256, num_neg=4, lr=0.001,
                 learner="adam", backend="tensorflow", early_stopping=None, trainable=True, verbose=True, seed=None, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.layers = layers
        self.act_fn = act_fn
        self.reg = reg
        self._init_common(num_epochs, batch_size, num_neg, lr, learner, backend, early_stopping, seed, device)


class NeuMF(_NCF):
    """Neural matrix factorization: GMF and MLP under one logit.  Parameters are the reference's (recom_neumf.py:22-134);
    `layers[-1]` must equal `num_factors` (backend_pt.py:139)."""
    KIND = "NeuMF"

    def __init__(self, name="NeuMF", num_factors=8, layers=(64, 32, 16, 8), act_fn="relu", reg=0.0, num_epochs=20, batch_size=256,
                 num_neg=4, lr=0.001, learner="adam", backend="tensorflow", early_stopping=None, trainable=True, verbose=True, seed=None,
                 device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.num_factors = num_factors
        self.layers = layers
        self.act_fn = act_fn
        self.reg = reg
        self.pretrained = False
        self._init_common(num_epochs, batch_size, num_neg, lr, learner, backend, early_stopping, seed, device)
        self.ignored_attrs = self.ignored_attrs + ["alpha"]

    def from_pretrained(self, pretrained_gmf, pretrained_mlp, alpha=0.5):
        """fitted GMF and MLP models to start the next `fit` from: section 3.4.1 of the paper (recom_neumf.py:136-155)"""
        self.pretrained = True
        self.pretrained_gmf = pretrained_gmf
        self.pretrained_mlp = pretrained_mlp
        self.alpha = alpha
        return self

    @staticmethod
    def combine(gmf_tables, mlp_tables, alpha):
        """backend_pt.py:151-163 in float32 on the host: the embedding and layer tables copied, the final logit
        [alpha w_gmf | (1 - alpha) w_mlp] and alpha b_gmf + (1 - alpha) b_mlp"""
        a, b = np.float32(alpha), np.float32(1.0 - alpha)
        out = OrderedDict()
        out["logit.weight"] = np.concatenate([a * gmf_tables["logit.weight"], b * mlp_tables["logit.weight"]], axis=1).astype(np.float32)
        out["logit.bias"] = (a * gmf_tables["logit.bias"] + b * mlp_tables["logit.bias"]).astype(np.float32)
        out.update(("gmf." + n, np.array(t, np.float32)) for n, t in gmf_tables.items())
        out.update(("mlp." + n, np.array(t, np.float32)) for n, t in mlp_tables.items())
        return out

    def _initial_tables(self, n_users, n_items):
        tabs = _NCF._initial_tables(self, n_users, n_items)   # (drawn in either case, as the reference does)
        if self.pretrained:
            tabs = self.combine(self.pretrained_gmf.params, self.pretrained_mlp.params, self.alpha)
            want = _lib.NcfModel.shapes("NeuMF", n_users, n_items, self._factors(), self._layers())
            for n, t in tabs.items():
                if t.shape != want[n]:
                    raise ValueError("pretrained %s has shape %r, expected %r" % (n, t.shape, want[n]))
        return tabs
