#!/usr/bin/env python3
"""Generates tests/golden/ncf_ref.npz by RUNNING THE REFERENCE'S OWN GMF / MLP / NeuMF MODULES AND _fit_pt on the CPU (only
possible where the reference's sources are present: oracle/build_ref.py's REF).  cornac/models/ncf is pure Python over torch,
so nothing is compiled: oracle.ref_loader.load() makes the reference's Dataset importable, and the models are imported from
where they lie.  Nothing of their text enters this repository.

Per case of tests/ncf_cases.py the model's `_build_model_pt` is wrapped to load the case's tables, the train set's `uir_iter`
is replaced on the instance by one that yields the case's batches, the `optimizer_dict` entry is wrapped to keep the
optimiser, nn.BCELoss is wrapped to record each step's loss, and `fit` runs one epoch of the case's steps.  Stored for EVERY
case, per table in the order of ncf_cases.NAMES(kind, layers):
    <case>/d_ref, d_ref_s1, d_ref_s2   max|reference float32 - float64 restatement| of the table and of the learner's state
                                       (adam: exp_avg, exp_avg_sq; rmsprop: square_avg; adagrad: sum; otherwise zeros)
    <case>/move                        max|table after - table before|
    <case>/max, max_s1, max_s2         max|.| of the reference's table and state
and for the FULL_CASES also the tables (<case>/P/<name>), the state (S1/, S2/), the per-step losses, score(u) of a few
users and a few score(u, i) from the reference's own _score_pt.  For the SEEDED cases, one small shape per kind: the tables
after the reference's own seeded `fit` (its initial draws, its sampler over a Dataset built with a seed), and d_ref / move /
max against this project's model classes run on the restatement.

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_ncf_golden.py
"""
import importlib
import io
import os
import sys
import zipfile
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ncf_cases as nc  # noqa: E402
from oracle import ref_loader  # noqa: E402

STATE_KEYS = {"adam": ("exp_avg", "exp_avg_sq"), "rmsprop": ("square_avg", None), "adagrad": ("sum", None), "sgd": (None, None)}


def write_npz(path, arrays):
    """np.savez_compressed with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def reference_dataset(Dataset, nu, ni, triplets, seed=1):
    u, i, r = triplets
    ds = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=seed,   # (identity id maps)
                       global_uid_map=OrderedDict((n, n) for n in range(nu)),
                       global_iid_map=OrderedDict((n, n) for n in range(ni)))
    assert (ds.num_users, ds.num_items) == (nu, ni)
    return ds


def reference_model(c, **kw):
    mod = importlib.import_module("cornac.models.ncf")
    args = dict(num_epochs=1, batch_size=1, num_neg=c["nn"], lr=c["lr"], learner=c["learner"], reg=c["reg"], backend="pytorch",
                verbose=False, seed=1)
    args.update(kw)
    if c["kind"] != "MLP":
        args["num_factors"] = c["f"]
    if c["kind"] != "GMF":
        args["layers"], args["act_fn"] = list(c["layers"]), c["act"]
    return getattr(mod, c["kind"])(**args)


class Keep:
    """wraps optimizer_dict[learner] and nn.BCELoss for the length of a fit: keeps the optimiser and the steps' losses"""

    def __init__(self, learner):
        import torch

        self.torch, self.learner, self.kept, self.losses = torch, learner, [], []
        self.backend = importlib.import_module("cornac.models.ncf.backend_pt")

    def __enter__(self):
        torch, keep = self.torch, self
        self.real_opt, self.real_bce = self.backend.optimizer_dict[self.learner], torch.nn.BCELoss

        class Opt(self.real_opt):
            def __init__(self, *a, **kw):
                super().__init__(*a, **kw)
                keep.kept.append(self)

        class BCE(self.real_bce):
            def forward(self, *a, **kw):
                out = super().forward(*a, **kw)
                keep.losses.append(float(out.data.item()))
                return out

        self.backend.optimizer_dict[self.learner], torch.nn.BCELoss = Opt, BCE
        return self

    def __exit__(self, *exc):
        self.backend.optimizer_dict[self.learner], self.torch.nn.BCELoss = self.real_opt, self.real_bce

    def state(self, model, names):
        """(S1, S2) per table name, zeros where the optimiser holds nothing"""
        assert len(self.kept) == 1
        params = dict(model.named_parameters())
        st = self.kept[0].state
        out = []
        for key in STATE_KEYS[self.learner]:
            d = {}
            for n in names:
                s = st.get(params[n], {})
                d[n] = s[key].numpy().copy() if key is not None and key in s else np.zeros(tuple(params[n].shape), np.float32)
            out.append(d)
        return out


def stats(name, names, P, S1, S2, init, mine_P, mine_S1, mine_S2):
    dist = lambda ref, mine: np.array([np.abs(ref[n].astype(np.float64) - mine[n]).max() for n in names])   # noqa: E731
    top = lambda ref: np.array([np.abs(ref[n]).max() for n in names], np.float64)   # noqa: E731
    return {name + "/d_ref": dist(P, mine_P), name + "/d_ref_s1": dist(S1, mine_S1), name + "/d_ref_s2": dist(S2, mine_S2),
            name + "/move": np.array([np.abs(P[n].astype(np.float64) - init[n]).max() for n in names]),
            name + "/max": top(P), name + "/max_s1": top(S1), name + "/max_s2": top(S2)}


def run_case(ns, name):
    import torch

    c = nc.CASES[name]
    names = nc.NAMES(c["kind"], c["layers"])
    rs = np.random.RandomState(1)
    ds = reference_dataset(ns.Dataset, c["nu"], c["ni"], (np.arange(c["nu"]).repeat(2), rs.randint(0, c["ni"], 2 * c["nu"]),
                                                          np.ones(2 * c["nu"])))
    model = reference_model(c)
    init, batches = nc.case_params(c), nc.case_batches(c)
    build = model._build_model_pt

    def build_and_load():
        net = build()
        assert list(net.state_dict()) == list(names)
        net.load_state_dict({n: torch.tensor(a) for n, a in init.items()})
        return net

    model._build_model_pt = build_and_load
    ds.uir_iter = lambda *a, **kw: iter([(u, i, y) for u, i, y in batches])
    with Keep(c["learner"]) as keep:
        model.fit(ds)
    assert len(keep.losses) == len(batches)
    P = {n: a.detach().numpy().copy() for n, a in model.model.state_dict().items()}
    S1, S2 = keep.state(model.model, names)
    for n in nc.UNUSED(c["kind"]):   # grad is None: untouched, no state
        assert np.array_equal(P[n], init[n]) and not S1[n].any() and not S2[n].any()

    run = nc.run_case(name)
    r = run["r"]
    out = stats(name, names, P, S1, S2, init, r.P, r.S1, r.S2)
    out[name + "/loss_diff"] = np.array(np.abs(np.array(keep.losses) - run["losses"]).max())
    print("%-22s steps %d  d_ref %.2e  move %.2e .. %.2e  loss diff %.2e  kink %.2e" % (
        name, len(batches), out[name + "/d_ref"].max(), out[name + "/move"].min(), out[name + "/move"].max(),
        float(out[name + "/loss_diff"]), r.kink_distance))
    if name in nc.FULL_CASES or name == nc.RANK_CASE:
        for n in names:
            out["%s/P/%s" % (name, n)], out["%s/S1/%s" % (name, n)], out["%s/S2/%s" % (name, n)] = P[n], S1[n], S2[n]
        out[name + "/losses"] = np.array(keep.losses, np.float64)
        users, (pu, pi) = nc.score_users(c), nc.score_pairs(c)
        out[name + "/scores"] = np.array([model.score(int(u)) for u in users], np.float32)
        out[name + "/pair_scores"] = np.array([model.score(int(u), int(i))[0] for u, i in zip(pu, pi)], np.float32)
    if name == nc.RANK_CASE:
        out[name + "/all_scores"] = np.array([model.score(int(u)) for u in range(c["nu"])], np.float32)
    return out


def run_seeded(ns, name):
    """the reference's own seeded fit against this project's model class on the restatement"""
    from cornac_amd import _lib

    c = nc.SEEDED[name]
    names = nc.NAMES(c["kind"], c["layers"])
    trip = nc.seeded_triplets(c)
    ref = reference_model(c, num_epochs=c["epochs"], batch_size=c["bs"], seed=c["seed"])
    ref.fit(reference_dataset(ns.Dataset, c["nu"], c["ni"], trip, seed=c["seed"]))
    P = {n: a.detach().numpy().copy() for n, a in ref.model.state_dict().items()}
    assert list(P) == list(names)

    real = _lib.NcfModel
    _lib.NcfModel = nc.FakeNcfModel
    try:
        mine = nc.seeded_model(c).fit(nc.seeded_dataset(c))
    finally:
        _lib.NcfModel = real
    fake = nc.FakeNcfModel.last
    init = fake.initial
    zeros = {n: np.zeros(P[n].shape) for n in names}
    out = stats(name, names, P, zeros, zeros, init, fake.r.P, zeros, zeros)
    for n in names:
        out["%s/P/%s" % (name, n)] = P[n]
    users, (pu, pi) = nc.score_users(c), nc.score_pairs(c)
    out[name + "/scores"] = np.array([ref.score(int(u)) for u in users], np.float32)
    out[name + "/pair_scores"] = np.array([ref.score(int(u), int(i))[0] for u, i in zip(pu, pi)], np.float32)
    print("%-22s d_ref %.2e  move %.2e .. %.2e" % (name, out[name + "/d_ref"].max(), out[name + "/move"].min(), out[name + "/move"].max()))
    del mine
    return out


def main():
    ns = ref_loader.load()
    out = {"cases": np.array(sorted(nc.CASES) + sorted(nc.SEEDED))}
    for name in sorted(nc.CASES):
        out.update(run_case(ns, name))
    for name in sorted(nc.SEEDED):
        out.update(run_seeded(ns, name))
    path = os.path.join(HERE, "ncf_ref.npz")
    write_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
