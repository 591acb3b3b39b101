"""A partial `set_params` on the six neural models' device handles (`_lib.VaecfModel`, `BivaeModel`, `RecvaeModel`, `NcfModel` in
its three kinds, `LightGcnModel`, `NgcfModel`): tables that a call does not name keep their bytes, the named ones take the new
bytes, and `reset_optimizer` leaves both state dicts all zero and the step counters at 0.

One handle per model at a small shape of its case table (tens of users and items, hidden sizes of a few units, one NGCF layer;
no table that the device holds transposed is square).  Every table is set to seeded values; then every second name, from the
second on, is set to new values in the model's own calling convention (for LightGCN that is `set_params(None, item)`), then
the other half.  After each call `get_params()` is compared with what the host holds, as uint32 words.  One training epoch
makes the optimiser state non-zero before it is reset."""
import numpy as np
import pytest
import scipy.sparse as sp

import bivae_cases as bc
import lightgcn_cases as lc
import ncf_cases as nc
import ngcf_cases as gc
import recvae_cases as rc
import vaecf_cases as vc
from cornac_amd import _lib

pytestmark = pytest.mark.gpu


def _vaecf():
    c = vc.CASES["al/tanh/mult"]   # 37 x 131, k 5, h 7
    m = _lib.VaecfModel(vc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"])
    return m, _lib.VaecfModel.shapes(c["ni"], c["k"], c["h"]), lambda: m.fit_epoch(c["bs"], 1e-3, 1.0, seed=3)


def _bivae():
    c = bc.CASES["k20"]   # 21 x 19, k 20, h 7
    m = _lib.BivaeModel(bc.case_matrix(c), c["k"], c["h"], c["act"], c["lik"])
    return m, _lib.BivaeModel.shapes(c["nu"], c["ni"], c["k"], c["h"]), lambda: m.fit_epoch(c["bs"], 1e-3, 1.0, seed=3)


def _recvae():
    c = rc.CASES["i63"]   # 37 x 63, hidden 7, latent 5
    m = _lib.RecvaeModel(rc.case_matrix(c), c["h"], c["k"])
    order = np.arange(c["nu"], dtype=np.int32)
    return m, _lib.RecvaeModel.shapes(c["ni"], c["h"], c["k"]), lambda: m.fit_epoch(order, c["bs"], 1e-3, 0.005, None, 0.5, True, True, seed=3)


def _ncf(case):
    def make():
        c = nc.CASES[case]   # 37 x 29, num_factors 5, layers (12, 7, 5)
        m = _lib.NcfModel(c["kind"], sp.csr_matrix((c["nu"], c["ni"]), dtype=np.float64), c["f"], c["layers"], c["act"])
        epoch = nc.epoch_arrays(nc.case_batches(c))
        return m, _lib.NcfModel.shapes(c["kind"], c["nu"], c["ni"], c["f"], c["layers"]), lambda: m.fit_epoch(*epoch, 1e-3, 0.0, "adam")
    return make


class _LightGcnAsDicts:
    """LightGcnModel's tuple-shaped calls under the names "user" and "item" """

    def __init__(self, m):
        self.m, self.close, self.reset_optimizer = m, m.close, m.reset_optimizer

    def set_params(self, params):
        self.m.set_params(params.get("user"), params.get("item"))

    def get_params(self):
        return dict(zip(("user", "item"), self.m.get_params()))

    def get_state(self):
        mu, mi, vu, vi, t = self.m.get_state()
        return {"user": mu, "item": mi}, {"user": vu, "item": vi}, t


def _lightgcn():
    c = lc.CASES["d8"]   # 13 x 10 nodes with the isolated ones, emb_size 8, 3 layers
    m = _lib.LightGcnModel(lc.case_graph(c), c["d"], c["L"])
    epoch = lc.epoch_arrays(lc.case_batches(c))
    tu, ti = lc.totals(c)
    return _LightGcnAsDicts(m), {"user": (tu, c["d"]), "item": (ti, c["d"])}, lambda: m.fit_epoch(*epoch, 1e-3, 1e-4)


def _ngcf():
    c = gc.CASES["lam0"]   # 37 x 29, emb_size 33, one layer of 33
    m = _lib.NgcfModel(gc.case_graph(c), c["emb"], c["layers"], c["drop"], dropout_key=gc.KEY)
    epoch = gc.epoch_arrays(gc.case_batches(c))
    tu, ti = gc.totals(c)
    return m, dict(_lib.NgcfModel.param_shapes(tu, ti, c["emb"], c["layers"])), lambda: m.fit_epoch(*epoch, 1e-3, 0.0)


MODELS = {"VAECF": _vaecf, "BiVAECF": _bivae, "RecVAE": _recvae, "GMF": _ncf("kl/GMF/adam"), "MLP": _ncf("kl/MLP/adam"),
          "NeuMF": _ncf("kl/NeuMF/adam"), "LightGCN": _lightgcn, "NGCF": _ngcf}


def _draw(rs, shapes, names):
    return {n: rs.uniform(-0.5, 0.5, shapes[n]).astype(np.float32) for n in names}


def _same_words(got, want):
    assert set(got) == set(want)
    for n, a in want.items():
        assert got[n].dtype == np.float32 and got[n].shape == a.shape, n
        diff = int((got[n].view(np.uint32) != a.view(np.uint32)).sum())
        assert diff == 0, "%s: %d of %d words differ" % (n, diff, a.size)


@pytest.mark.parametrize("name", list(MODELS))
def test_partial_set_params_and_reset(name):
    m, shapes, train = MODELS[name]()
    try:
        names = list(shapes)
        rs = np.random.RandomState(11)
        held = _draw(rs, shapes, names)
        m.set_params(held)
        _same_words(m.get_params(), held)
        for part in (names[1::2], names[0::2]):
            new = _draw(rs, shapes, part)
            m.set_params(new)
            held.update(new)
            _same_words(m.get_params(), held)
        train()
        state = m.get_state()
        assert any(np.any(a != 0) for d in state[:2] for a in d.values()) and all(int(t) > 0 for t in state[2:]), \
            "the epoch left no optimiser state to reset"
        m.reset_optimizer()
        state = m.get_state()
        for d in state[:2]:
            for n, a in d.items():
                assert not a.view(np.uint32).any(), "%s is not zero after reset_optimizer" % n
        assert all(int(t) == 0 for t in state[2:]), state[2:]
    finally:
        m.close()
