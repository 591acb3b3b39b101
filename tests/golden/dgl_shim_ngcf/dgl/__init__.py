"""A small stand-in for the DGL names that cornac/models/ngcf/ngcf.py uses, so that the reference's own Model, construct_graph
and NGCF.fit run on the CPU where DGL is not installed (tests/golden/make_ngcf_golden.py puts this folder on sys.path; the
same arrangement as tests/golden/dgl_shim for LightGCN).  This project's own text: a heterograph is a dict of edge lists, node
and edge features live in plain dicts, and message passing is a gather and an `index_add_`, torch operations that autograd
follows.

Covered: heterograph(data_dict, num_nodes_dict), canonical_etypes and ntypes (both sorted, as DGL keeps them), num_nodes,
edges(etype=), in_degrees / out_degrees(nodes, etype=), g.nodes[ntype].data, g.edges[etype].data, multi_update_all with
fn.copy_u / fn.copy_e and fn.sum, and .to."""
import torch

from . import function  # noqa: F401


class _Frame:
    def __init__(self):
        self.data = {}


class _View:
    """g.nodes[ntype] / g.edges[etype]: one frame per type, made on first use"""

    def __init__(self, key):
        self.key, self.frames = key, {}

    def __getitem__(self, name):
        return self.frames.setdefault(self.key(name), _Frame())


class DGLGraph:
    def __init__(self, data_dict, num_nodes_dict):
        self._edges = {}
        for (src, etype, dst), (u, v) in data_dict.items():
            self._edges[(src, etype, dst)] = (torch.as_tensor(u, dtype=torch.int64), torch.as_tensor(v, dtype=torch.int64))
        self._num = dict(num_nodes_dict)
        self.canonical_etypes = sorted(self._edges, key=lambda c: c[1])
        self.ntypes = sorted(self._num)
        self.nodes = _View(lambda n: n)
        self.edges = _Edges(self)

    def _canonical(self, etype):
        if isinstance(etype, tuple):
            return etype
        return next(c for c in self.canonical_etypes if c[1] == etype)

    def num_nodes(self, ntype):
        return self._num[ntype]

    def in_degrees(self, nodes, etype):
        c = self._canonical(etype)
        return torch.bincount(self._edges[c][1], minlength=self._num[c[2]])[nodes]

    def out_degrees(self, nodes, etype):
        c = self._canonical(etype)
        return torch.bincount(self._edges[c][0], minlength=self._num[c[0]])[nodes]

    def to(self, device):
        return self

    def multi_update_all(self, funcs, cross_reducer):
        """per edge type: the message (a copy of a source-node or an edge feature) summed into its destination nodes; the
        types' results that share a destination type and an output name are added"""
        assert cross_reducer == "sum"
        out = {}
        for etype, (message, reduce) in funcs.items():
            src, name, dst = c = self._canonical(etype)
            u, v = self._edges[c]
            assert message.out == reduce.msg
            if isinstance(message, function.CopyU):
                m = self.nodes[src].data[message.field][u]
            else:
                m = self.edges[c].data[message.field]
            h = torch.zeros(self._num[dst], m.shape[1], dtype=m.dtype).index_add_(0, v, m)
            slot = out.setdefault(reduce.out, {})
            slot[dst] = h if dst not in slot else slot[dst] + h
        for name, per_type in out.items():
            for ntype, value in per_type.items():
                self.nodes[ntype].data[name] = value


class _Edges(_View):
    """g.edges(etype=..) gives the (sources, destinations) of a type; g.edges[etype].data is that type's feature dict"""

    def __init__(self, graph):
        super().__init__(graph._canonical)
        self.graph = graph

    def __call__(self, etype):
        return self.graph._edges[self.graph._canonical(etype)]


def heterograph(data_dict, num_nodes_dict=None):
    return DGLGraph(data_dict, num_nodes_dict)
