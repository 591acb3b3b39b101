"""A small stand-in for the DGL names that cornac/models/lightgcn/lightgcn.py uses, so that the reference's own Model,
construct_graph and LightGCN.fit run on the CPU where DGL is not installed (tests/golden/make_lightgcn_golden.py puts this
folder on sys.path; the same arrangement as oracle/tf1_shim for WMF).  This project's own text: a heterograph is a dict of
edge lists, and message passing is a gather, a multiply and an `index_add_`, all torch operations that autograd follows.

Covered: heterograph(data_dict, num_nodes_dict), canonical_etypes and ntypes (both sorted, as DGL keeps them), num_nodes,
edges, in_degrees / out_degrees, edata / ndata / dstdata, multi_update_all with fn.u_mul_e and fn.sum, .to, and NID (named
only in a branch the reference's fit never takes)."""
import torch

from . import function  # noqa: F401

NID = "_ID"


class _EdgeData:
    """g.edata[name] = {etype: tensor} sets that edge type's feature and keeps the others"""

    def __init__(self, graph):
        self.graph, self.store = graph, {}

    def __setitem__(self, name, value):
        slot = self.store.setdefault(name, {})
        for etype, tensor in value.items():
            slot[self.graph._etype_name(etype)] = tensor

    def __getitem__(self, name):
        return self.store[name]


class _NodeData:
    """g.ndata[name] = {ntype: tensor}; reading gives the dict back"""

    def __init__(self):
        self.store = {}

    def __setitem__(self, name, value):
        self.store[name] = dict(value)

    def __getitem__(self, name):
        return self.store[name]


class DGLGraph:
    def __init__(self, data_dict, num_nodes_dict):
        self._edges = {}
        for (src, etype, dst), (u, v) in data_dict.items():
            self._edges[(src, etype, dst)] = (torch.as_tensor(u, dtype=torch.int64), torch.as_tensor(v, dtype=torch.int64))
        self._num = dict(num_nodes_dict)
        self.canonical_etypes = sorted(self._edges, key=lambda c: c[1])
        self.ntypes = sorted(self._num)
        self.edata = _EdgeData(self)
        self.ndata = _NodeData()
        self.dstdata = self.ndata

    def _canonical(self, etype):
        if isinstance(etype, tuple):
            return etype
        return next(c for c in self.canonical_etypes if c[1] == etype)

    def _etype_name(self, etype):
        return self._canonical(etype)[1]

    def num_nodes(self, ntype):
        return self._num[ntype]

    def edges(self, etype):
        return self._edges[self._canonical(etype)]

    def in_degrees(self, nodes, etype):
        c = self._canonical(etype)
        return torch.bincount(self._edges[c][1], minlength=self._num[c[2]])[nodes]

    def out_degrees(self, nodes, etype):
        c = self._canonical(etype)
        return torch.bincount(self._edges[c][0], minlength=self._num[c[0]])[nodes]

    def to(self, device):
        return self

    def multi_update_all(self, funcs, cross_reducer):
        assert cross_reducer == "sum"
        out = {}
        for etype, (message, reduce) in funcs.items():
            src, name, dst = self._canonical(etype)
            u, v = self._edges[(src, name, dst)]
            assert message.out == reduce.msg
            m = self.ndata[message.u][src][u] * self.edata[message.e][name]
            h = torch.zeros(self._num[dst], m.shape[1], dtype=m.dtype).index_add_(0, v, m)
            slot = out.setdefault(reduce.out, {})
            slot[dst] = h if dst not in slot else slot[dst] + h
        for name, value in out.items():
            self.ndata[name] = value


def heterograph(data_dict, num_nodes_dict=None):
    return DGLGraph(data_dict, num_nodes_dict)
