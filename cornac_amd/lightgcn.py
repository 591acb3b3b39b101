"""LightGCN on MI355X — `LightGCN` with the constructor, the `fit/score/rank` surface, the early stopping and the
`state_dict` of the reference's `cornac.models.LightGCN` (cornac/models/lightgcn/recom_lightgcn.py, lightgcn.py; He et al.
2020).  What the reference runs per batch through DGL and torch — the propagation over the whole user-item graph, once per
layer, forward and backward, the BPR loss and Adam's dense pass over both tables — runs in libcornac_hip
(`_lib.LightGcnModel`), in float32 like there.

Seeded fits follow the reference's CPU run to rounding: with a seed the model calls `torch.manual_seed(seed)` and draws the
initial tables on the CPU with `xavier_uniform_` on `torch.empty(n, emb_size)`, THE ITEM TABLE FIRST and the user table
second.  That order is an assumption, stated here because DGL is not at hand to consult: the reference fills its
`ParameterDict` in `g.ntypes` order (lightgcn.py:75-82), and DGL keeps a heterograph's node types sorted by name, "item"
before "user".  Each epoch's batches come from `train_set.uij_iter(batch_size, shuffle=True)` (the reference's sampler,
restated draw for draw in `Dataset`) and go to the device in one call; seeded and unseeded fits both use that host sampler.

The graph has `total_users` + `total_items` nodes (lightgcn.py:28): ids that the training set does not hold, such as
validation-only and test-only ones, are nodes without edges.  Their rows get no gradient and stay at their initial values.

Stated departures:
  * `verbose` prints one line per epoch instead of two progress bars.
  * `save` / `load` work (the tables are host arrays).

Learned: `U`, `V` (the final embeddings, the mean of the layers' tables, which `score` and the fused scorer read),
`params` (the layer-0 tables under the reference's names `feature_dict.user`, `feature_dict.item`) and `loss_history`."""
from collections import OrderedDict

import numpy as np
import scipy.sparse as sp

from . import _lib
from .recommender import Recommender, ScoreException, filled_handle, float32_tables

NAMES = ("feature_dict.user", "feature_dict.item")


class GraphRecommender(Recommender):
    """What the two graph models (LightGCN, NGCF) share on the host: the train matrix over all nodes, the epoch loop of `fit`,
    the monitored value of early stopping, the propagation over a given graph after `load_state_dict`, and scoring from the
    learned embeddings `U` and `V` through the fused scorer with zero bases.  A subclass supplies `_initial_params()` (drawn
    with torch on the CPU), `_model(X, params)` (a device model over the matrix X that holds `params`) and `_take(model)`."""

    def _graph_matrix(self, train_set):
        """the train matrix over total_users x total_items (lightgcn.py:22-30), sorted indices"""
        u, i, _ = train_set.uir_tuple
        X = sp.csr_matrix((np.ones(len(u), np.float64), (np.asarray(u, np.int64), np.asarray(i, np.int64))),
                          shape=(self.total_users, self.total_items))
        X.sum_duplicates()
        X.sort_indices()
        return X

    def fit(self, train_set, val_set=None):
        """recom_lightgcn.py:102-194, recom_ngcf.py:106-199: every fit starts from new parameters and a new optimiser, as there"""
        Recommender.fit(self, train_set, val_set)
        if not self.trainable:
            return self
        import torch

        if self.seed is not None:
            torch.manual_seed(self.seed)
        init = self._initial_params()
        model = self._model(self._graph_matrix(train_set), init)
        try:
            n_obs = len(train_set.uir_tuple[0])
            self.loss_history = []
            for epoch in range(int(self.num_epochs)):
                bu, bi, bj, ptr = [], [], [], [0]
                for u, i, j in train_set.uij_iter(batch_size=self.batch_size, shuffle=True):
                    bu.append(u); bi.append(i); bj.append(j); ptr.append(ptr[-1] + len(u))
                ptr = np.asarray(ptr, np.int64)
                losses, _, _ = model.fit_epoch(ptr, np.concatenate(bu), np.concatenate(bi), np.concatenate(bj), self.learning_rate,
                                               self.lambda_reg)
                self.loss_history.append(float((losses * np.diff(ptr)).sum() / n_obs))   # recom_lightgcn.py:175-181
                if self.verbose:
                    print("%s epoch %d: loss %.6g" % (self.name, epoch + 1, self.loss_history[-1]))
                if self.early_stopping is not None:   # the embeddings that the monitored value is computed from
                    self._take(model)
                    if self.early_stop(train_set, val_set, **self.early_stopping):
                        break
            if self.early_stopping is None or not self.loss_history:
                self._take(model)
        finally:
            model.close()
        return self

    def _propagate_over(self, graph):
        """`U` and `V` of `self.params` over `graph`: the train matrix over the tables' users x items, or a Dataset"""
        shape = tuple(len(self.params["feature_dict." + n]) for n in ("user", "item"))
        X = graph if sp.issparse(graph) else None
        if X is None:
            u, i, _ = graph.uir_tuple
            X = sp.csr_matrix((np.ones(len(u)), (u, i)), shape=shape)
        X = sp.csr_matrix(X)
        X.sort_indices()
        if X.shape != shape:
            raise ValueError("the graph is %r, expected %r" % (X.shape, shape))
        model = self._model(X, self.params)
        try:
            self.U, self.V = model.propagate()
        finally:
            model.close()

    def monitor_value(self, train_set, val_set):
        """Recall@20 on the validation set (recom_lightgcn.py:196-227; section 4.1.2 of the paper); None without one"""
        if val_set is None:
            return None
        from .eval import ranking_eval
        from .metrics import Recall

        return ranking_eval(model=self, metrics=[Recall(k=20)], train_set=train_set, test_set=val_set)[0][0]

    # ---- prediction ---------------------------------------------------------------------------------
    def _scoring_tables(self):
        """(U, V, zeros, zeros): the score is the dot product of the final embeddings"""
        key = (id(self.U), id(self.V))
        cached = self.__dict__.get("_zero_bases")
        if cached is None or cached[0] != key:
            cached = (key, np.zeros(len(self.V), np.float32), np.zeros(len(self.U), np.float32))
            self._zero_bases = cached
        return self.U, self.V, cached[1], cached[2]

    def _scorer_row_count(self):
        return len(self.U)

    def score(self, user_idx, item_idx=None):
        """recom_lightgcn.py:229-260"""
        if item_idx is None:
            if not self.knows_user(user_idx):
                raise ScoreException("Can't make score prediction for (user_id=%d)" % user_idx)
            return self._get_scorer().score_user(user_idx)
        if not (self.knows_user(user_idx) and self.knows_item(item_idx)):
            raise ScoreException("Can't make score prediction for (user_id=%d, item_id=%d)" % (user_idx, item_idx))
        return self.V[item_idx, :].dot(self.U[user_idx, :])

    # ANN mixin surface (recom_lightgcn.py:262-290)
    def get_vector_measure(self):
        return "dot"

    def get_user_vectors(self):
        return self.U

    def get_item_vectors(self):
        return self.V


class LightGCN(GraphRecommender):
    """Parameters are the reference's (recom_lightgcn.py:27-100): `emb_size`, `num_epochs`, `learning_rate`, `batch_size`,
    `num_layers`, `early_stopping` ({min_delta, patience} on Recall@20 of the validation set), `lambda_reg`, `seed`; plus
    `device`, the HIP device ordinal."""

    def __init__(self, name="LightGCN", emb_size=64, num_epochs=1000, learning_rate=0.001, batch_size=1024, num_layers=3,
                 early_stopping=None, lambda_reg=1e-4, trainable=True, verbose=False, seed=2020, device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.emb_size = emb_size
        self.num_epochs = num_epochs
        self.learning_rate = learning_rate
        self.batch_size = batch_size
        self.num_layers = num_layers
        self.early_stopping = early_stopping
        self.lambda_reg = lambda_reg
        self.seed = seed
        self.device = device

    def _initial_params(self):
        """lightgcn.py:72-82: xavier_uniform_ on torch.empty(n, emb_size) per node type, in the graph's ntypes order: item, user"""
        import torch

        item = torch.nn.init.xavier_uniform_(torch.empty(self.total_items, int(self.emb_size)))
        user = torch.nn.init.xavier_uniform_(torch.empty(self.total_users, int(self.emb_size)))
        return OrderedDict(zip(NAMES, (user.numpy().astype(np.float32).copy(), item.numpy().astype(np.float32).copy())))

    def _model(self, X, params):
        model = _lib.LightGcnModel(X, int(self.emb_size), int(self.num_layers), device=self.device)
        return filled_handle(model, lambda m: m.set_params(params[NAMES[0]], params[NAMES[1]]))

    def _take(self, model):
        """the layer-0 tables and the final embeddings from the device (recom_lightgcn.py:184-189)"""
        user, item = model.get_params()
        self.params = OrderedDict(zip(NAMES, (user, item)))
        self.U, self.V = model.propagate()
        self._drop_scorer()

    # ---- the tables ---------------------------------------------------------------------------------
    def state_dict(self):
        """the layer-0 tables under the reference's names (copies): they load into the reference's Model"""
        return OrderedDict((n, self.params[n].copy()) for n in NAMES)

    def load_state_dict(self, state, graph=None):
        """layer-0 tables (arrays or torch tensors) under the reference's names.  The final embeddings depend on the graph:
        with `graph` (the train matrix over total_users x total_items, or a Dataset) they are propagated on the device;
        without it `U` and `V` stay as they are."""
        tabs = float32_tables(state)
        if set(tabs) != set(NAMES):
            raise KeyError("state_dict needs exactly the keys %r" % (NAMES,))
        user, item = tabs[NAMES[0]], tabs[NAMES[1]]
        if user.ndim != 2 or item.ndim != 2 or user.shape[1] != item.shape[1]:
            raise ValueError("feature_dict.user %r and feature_dict.item %r, expected [n_users, emb_size] and [n_items, emb_size]"
                             % (user.shape, item.shape))
        self.emb_size = int(user.shape[1])
        self.params = OrderedDict(zip(NAMES, (user, item)))
        if graph is not None:
            self._propagate_over(graph)
        self._drop_scorer()
