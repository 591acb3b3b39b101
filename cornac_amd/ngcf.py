"""NGCF on MI355X — `NGCF` with the constructor, the `fit/score/rank` surface, the early stopping and the `state_dict` of the
reference's `cornac.models.NGCF` (cornac/models/ngcf/recom_ngcf.py, ngcf.py; Wang et al. 2019).  What the reference runs per
batch through DGL and torch — two Linears per edge of the whole user-item graph, per layer, forward and backward, the BPR loss
and Adam over every parameter — runs in libcornac_hip (`_lib.NgcfModel`) as dense work per node, in float32 like there.

With a seed the model calls `torch.manual_seed(seed)` and builds the initial values with torch on the CPU in the reference's
order: per layer a real `nn.Linear` W1 and W2 (their default initialisation consumes draws), `xavier_uniform_` on W1's weight,
then on W2's, with zero biases (ngcf.py:47-60); then `xavier_uniform_` on the tables, THE ITEM TABLE FIRST and the user table
second.  That order is the same stated assumption as lightgcn.py's: the reference fills its `ParameterDict` in `g.ntypes` order
(ngcf.py:141-148), and DGL keeps a heterograph's node types sorted by name.  Each epoch's batches come from
`train_set.uij_iter(batch_size, shuffle=True)` and go to the device in one call.

The graph has `total_users` + `total_items` nodes (ngcf.py:35): ids that the training set does not hold are nodes without
edges.  Unlike LightGCN's, their rows do move: every row feeds the layers' weights.

Stated departures:
  * With any dropout rate above 0 the masks are the device's (a counter-based generator keyed by the seed, csrc/ngcf.hip),
    not torch's CPU stream: a seeded fit is then reproducible but does not follow the reference's seeded run.  With all rates
    0 it follows the reference to rounding.  `seed=None` draws the dropout key from the OS.
  * `verbose` prints one line per epoch instead of two progress bars.
  * `save` / `load` work (the parameters are host arrays).

Learned: `U`, `V` (the concatenated embeddings of all layers in eval mode, which `score` and the fused scorer read), `params`
(every parameter under the reference's state_dict names, in its order) and `loss_history`."""
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from .lightgcn import GraphRecommender
from .recommender import filled_handle, float32_tables


class NGCF(GraphRecommender):
    """Parameters are the reference's (recom_ngcf.py:27-104): `emb_size`, `layer_sizes`, `dropout_rates`, `num_epochs`,
    `learning_rate`, `batch_size`, `early_stopping` ({min_delta, patience} on Recall@20 of the validation set), `lambda_reg`,
    `seed`; plus `device`, the HIP device ordinal.  The graph matrix, the epoch loop of `fit`, the monitored value, the scoring
    through the fused scorer with zero bases and the ANN accessors are `GraphRecommender`'s, shared with LightGCN."""

    def __init__(self, name="NGCF", emb_size=64, layer_sizes=[64, 64, 64], dropout_rates=[0.1, 0.1, 0.1], num_epochs=1000,
                 learning_rate=0.001, batch_size=1024, early_stopping=None, lambda_reg=1e-4, trainable=True, verbose=False, seed=2020,
                 device=0):
        super().__init__(name=name, trainable=trainable, verbose=verbose)
        self.emb_size = emb_size
        self.layer_sizes = layer_sizes
        self.dropout_rates = dropout_rates
        self.num_epochs = num_epochs
        self.learning_rate = learning_rate
        self.batch_size = batch_size
        self.early_stopping = early_stopping
        self.lambda_reg = lambda_reg
        self.seed = seed
        self.device = device

    def _initial_params(self):
        """ngcf.py:40-60, 119-148 in the reference's draw order, under its state_dict names"""
        import torch

        out, din = OrderedDict(), int(self.emb_size)
        for l, dout in enumerate(int(x) for x in self.layer_sizes):
            W1, W2 = torch.nn.Linear(din, dout, bias=True), torch.nn.Linear(din, dout, bias=True)
            torch.nn.init.xavier_uniform_(W1.weight)
            torch.nn.init.constant_(W1.bias, 0)
            torch.nn.init.xavier_uniform_(W2.weight)
            torch.nn.init.constant_(W2.bias, 0)
            for n, lin in (("W1", W1), ("W2", W2)):
                out["layers.%d.%s.weight" % (l, n)] = lin.weight.detach().numpy().astype(np.float32).copy()
                out["layers.%d.%s.bias" % (l, n)] = lin.bias.detach().numpy().astype(np.float32).copy()
            din = dout
        for n, count in (("item", self.total_items), ("user", self.total_users)):
            out["feature_dict." + n] = torch.nn.init.xavier_uniform_(torch.empty(count, self.emb_size)).numpy().astype(np.float32).copy()
        return out

    def _model(self, X, params):
        assert len(self.layer_sizes) == len(self.dropout_rates), "'layer_sizes' and 'dropout_rates' must be of the same size"
        key = int.from_bytes(os.urandom(8), "little") if self.seed is None else int(self.seed)
        model = _lib.NgcfModel(X, int(self.emb_size), list(self.layer_sizes), list(self.dropout_rates), dropout_key=key, device=self.device)
        return filled_handle(model, lambda m: m.set_params(params))

    def _take(self, model):
        """the parameters and the eval-mode embeddings from the device (recom_ngcf.py:189-194)"""
        self.params = model.get_params()
        self.U, self.V = model.propagate()
        self._drop_scorer()

    # ---- the parameters -----------------------------------------------------------------------------
    def state_dict(self):
        """every parameter under the reference's names, in its order (copies): they load into the reference's Model"""
        return OrderedDict((n, a.copy()) for n, a in self.params.items())

    def load_state_dict(self, state, graph=None):
        """parameters (arrays or torch tensors) under the reference's names; the layer sizes are read from them.  The embeddings
        depend on the graph: with `graph` (the train matrix over total_users x total_items, or a Dataset) they are propagated on
        the device; without it `U` and `V` stay as they are."""
        tabs = float32_tables(state)
        n_layers = len([n for n in tabs if n.endswith(".W1.weight")])
        if n_layers < 1 or "feature_dict.user" not in tabs or "feature_dict.item" not in tabs:
            raise KeyError("state_dict needs feature_dict.user, feature_dict.item and at least layers.0.*")
        user, item = tabs["feature_dict.user"], tabs["feature_dict.item"]
        if user.ndim != 2 or item.ndim != 2 or user.shape[1] != item.shape[1]:
            raise ValueError("feature_dict.user %r and feature_dict.item %r, expected [n_users, emb_size] and [n_items, emb_size]"
                             % (user.shape, item.shape))
        sizes = [int(tabs["layers.%d.W1.weight" % l].shape[0]) for l in range(n_layers)]
        shapes = _lib.NgcfModel.param_shapes(user.shape[0], item.shape[0], user.shape[1], sizes)
        if set(tabs) != set(shapes):
            raise KeyError("state_dict needs exactly the keys %r" % (list(shapes),))
        for n, s in shapes.items():
            if tabs[n].shape != s:
                raise ValueError("%s is %r, expected %r" % (n, tabs[n].shape, s))
        self.emb_size, self.layer_sizes = int(user.shape[1]), sizes
        if len(self.dropout_rates) != n_layers:
            self.dropout_rates = [0.0] * n_layers
        self.params = OrderedDict((n, tabs[n]) for n in shapes)
        if graph is not None:
            self._propagate_over(graph)
        self._drop_scorer()
