#!/usr/bin/env python3
"""Generates tests/golden/lightgcn_ref.npz by RUNNING THE REFERENCE'S OWN lightgcn.Model, construct_graph AND LightGCN.fit on
the CPU (only possible where the reference's sources are present: oracle/build_ref.py's REF).  cornac/models/lightgcn is
pure Python over torch and DGL; DGL is not installed, so the few DGL names it uses come from the stand-in of
tests/golden/dgl_shim (this project's own text, put on sys.path here).  oracle.ref_loader.load() makes the reference's Dataset
importable, and the model is imported from where it lies.  Nothing of the reference's text enters this repository.

Per case of tests/lightgcn_cases.py the reference's Model.__init__ is wrapped to load the case's tables after its own draws, the train
set's `uij_iter` is replaced on the instance by one that yields the case's batches, torch.optim.Adam is wrapped to keep the
optimiser, Model.loss_fn is wrapped to record each step's three losses, and `fit` runs one epoch of the case's steps.  Stored
for EVERY case, per table in the order (user, item):
    <case>/d_ref, d_ref_m, d_ref_v   max|reference float32 - float64 restatement| of the table and of Adam's exp_avg, exp_avg_sq
    <case>/move                      max|table after - table before|
    <case>/max, max_m, max_v         max|.| of the reference's table and state
    <case>/d_ref_loss                max|reference's step losses - restatement's| over the three losses of every step
and for the FULL_CASES also the tables (<case>/P/<name>), the state (M/, V/), the per-step losses [steps x 3], the final
embeddings (E/) and score(u) of five users.  For the SEEDED case: U and V after the reference's own seeded `fit` (its initial
draws, its sampler over a Dataset built with a seed), and d_ref / move / max of U and V against this project's LightGCN run on
the restatement.  `check_condition` is asserted for every case: a case that breaks it needs another shape, not another rule.

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_lightgcn_golden.py
"""
import importlib
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.join(HERE, "dgl_shim"))

import lightgcn_cases as lc  # noqa: E402
from make_ncf_golden import write_npz  # noqa: E402
from oracle import ref_loader  # noqa: E402


def reference_dataset(Dataset, tu, ti, triplets, seed=1):
    u, i, r = triplets
    ds = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=seed,   # (identity id maps)
                       global_uid_map=OrderedDict((n, n) for n in range(tu)),
                       global_iid_map=OrderedDict((n, n) for n in range(ti)))
    assert (len(ds.uid_map), len(ds.iid_map)) == (tu, ti)
    assert np.array_equal(ds.uir_tuple[0], u) and np.array_equal(ds.uir_tuple[1], i)
    return ds


class Keep:
    """for the length of a fit: the reference's Model loads `init` after its own draws, and the optimiser, the model and the
    steps' losses are kept"""

    def __init__(self, init=None):
        import torch

        self.torch, self.init, self.opts, self.models, self.losses = torch, init, [], [], []
        self.mod = importlib.import_module("cornac.models.lightgcn.lightgcn")

    def __enter__(self):
        torch, keep = self.torch, self
        Model = self.mod.Model   # (wrapped in place: the reference's own super(Model, self) names the module's global)
        self.real_init, self.real_loss, self.real_adam = Model.__init__, Model.loss_fn, torch.optim.Adam

        def init(model, *a, **kw):
            keep.real_init(model, *a, **kw)
            assert list(model.feature_dict.keys()) == ["item", "user"]
            if keep.init is not None:
                with torch.no_grad():
                    model.feature_dict["user"].copy_(torch.tensor(keep.init[0]))
                    model.feature_dict["item"].copy_(torch.tensor(keep.init[1]))
            keep.models.append(model)

        def loss_fn(model, *a, **kw):
            out = keep.real_loss(model, *a, **kw)
            keep.losses.append([float(x.item()) for x in out])
            return out

        class Adam(self.real_adam):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                keep.opts.append(self)

        Model.__init__, Model.loss_fn, torch.optim.Adam = init, loss_fn, Adam
        return self

    def __exit__(self, *exc):
        self.mod.Model.__init__, self.mod.Model.loss_fn, self.torch.optim.Adam = self.real_init, self.real_loss, self.real_adam

    def tables(self):
        fd = self.models[0].feature_dict
        return tuple(fd[n].detach().numpy().copy() for n in lc.TABLES)

    def state(self, key):
        fd, st = self.models[0].feature_dict, self.opts[0].state
        return tuple(st[fd[n]][key].numpy().copy() for n in lc.TABLES)


def dist(ref, mine):
    return np.array([np.abs(a.astype(np.float64) - b).max() for a, b in zip(ref, mine)])


def top(ref):
    return np.array([np.abs(a).max() for a in ref], np.float64)


def reference_model(**kw):
    return importlib.import_module("cornac.models.lightgcn").LightGCN(**kw)


def run_case(ns, name):
    c = lc.CASES[name]
    X = lc.case_graph(c).tocoo()
    tu, ti = lc.totals(c)
    ds = reference_dataset(ns.Dataset, tu, ti, (X.row.astype(np.int64), X.col.astype(np.int64), np.ones(X.nnz)))
    init, batches = lc.case_params(c), lc.case_batches(c)
    model = reference_model(emb_size=c["d"], num_epochs=1, learning_rate=c["lr"], batch_size=1, num_layers=c["L"], lambda_reg=c["lam"],
                            seed=1, verbose=False)
    ds.uij_iter = lambda *a, **kw: iter(batches)
    with Keep(init) as keep:
        model.fit(ds)
    assert len(keep.losses) == len(batches) and len(keep.opts) == 1 and len(keep.models) == 1
    P, M, V = keep.tables(), keep.state("exp_avg"), keep.state("exp_avg_sq")
    run = lc.run_case(name)
    r = run["r"]
    out = {name + "/d_ref": dist(P, r.tables()), name + "/d_ref_m": dist(M, r.tables(r.M)), name + "/d_ref_v": dist(V, r.tables(r.V)),
           name + "/move": np.array([np.abs(a.astype(np.float64) - b).max() for a, b in zip(P, init)]),
           name + "/max": top(P), name + "/max_m": top(M), name + "/max_v": top(V),
           name + "/d_ref_loss": np.array(np.abs(np.array(keep.losses) - run["losses"]).max())}
    share = lc.check_condition(out, name)
    print("%-8s steps %d  d_ref %.2e  move %.2e .. %.2e  share %.4f  loss diff %.2e" % (
        name, len(batches), out[name + "/d_ref"].max(), out[name + "/move"].min(), out[name + "/move"].max(), share,
        float(out[name + "/d_ref_loss"])))
    for rows, a, b in zip(lc.still_rows(name), P, init):   # rows without a gradient stay bit for bit in the reference too
        assert np.array_equal(a[rows], b[rows])
    if name in lc.FULL_CASES:
        for q, n in enumerate(lc.TABLES):
            out["%s/P/%s" % (name, n)], out["%s/M/%s" % (name, n)], out["%s/V/%s" % (name, n)] = P[q], M[q], V[q]
        out[name + "/E/user"], out[name + "/E/item"] = model.U, model.V
        out[name + "/losses"] = np.array(keep.losses, np.float64)
        out[name + "/scores"] = np.array([model.score(int(u)) for u in lc.score_users(c)], np.float32)
    return out


def run_seeded(ns, name):
    """the reference's own seeded fit against this project's model class on the restatement"""
    from cornac_amd import _lib

    c = lc.SEEDED[name]
    ref = reference_model(emb_size=c["d"], num_epochs=c["epochs"], learning_rate=c["lr"], batch_size=c["bs"], num_layers=c["L"],
                          lambda_reg=c["lam"], seed=c["seed"], verbose=False)
    with Keep():
        ref.fit(reference_dataset(ns.Dataset, c["nu"], c["ni"], lc.seeded_triplets(c), seed=c["seed"]))
    real = _lib.LightGcnModel
    _lib.LightGcnModel = lc.FakeLightGcnModel
    try:
        mine = lc.seeded_model(c).fit(lc.seeded_dataset(c))
    finally:
        _lib.LightGcnModel = real
    fake = lc.FakeLightGcnModel.last
    E, E0 = (ref.U, ref.V), Restated(fake)
    out = {name + "/d_ref": dist(E, fake.r.final()), name + "/move": np.array([np.abs(a.astype(np.float64) - b).max() for a, b in zip(E, E0)]),
           name + "/max": top(E), name + "/U": ref.U, name + "/V": ref.V,
           name + "/scores": np.array([ref.score(int(u)) for u in lc.score_users(c)], np.float32)}
    print("%-8s d_ref %.2e  move %.2e .. %.2e  share %.4f" % (name, out[name + "/d_ref"].max(), out[name + "/move"].min(),
                                                               out[name + "/move"].max(), lc.check_condition(out, name)))
    del mine
    return out


def Restated(fake):
    """the final embeddings of the double's INITIAL tables: what U and V moved away from"""
    r = lc.Restatement(fake.X, fake.emb_size, fake.num_layers, *fake.initial)
    return r.final()


def main():
    ns = ref_loader.load()
    out = {"cases": np.array(sorted(lc.CASES) + sorted(lc.SEEDED))}
    for name in sorted(lc.CASES):
        out.update(run_case(ns, name))
    for name in sorted(lc.SEEDED):
        out.update(run_seeded(ns, name))
    path = os.path.join(HERE, "lightgcn_ref.npz")
    write_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
