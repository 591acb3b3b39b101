#!/usr/bin/env python3
"""Generates tests/golden/vaecf_ref.npz by RUNNING THE REFERENCE'S OWN VAE AND learn() (only possible where the reference's
sources are present: oracle/build_ref.py's REF).  cornac/models/vaecf is pure Python over torch, so nothing is compiled:
oracle.ref_loader.load() makes the reference's Dataset importable, and the model is imported from where it lies.  Nothing of
its text enters this repository.

Per case of tests/vaecf_cases.py the reference's VAE gets the case's tables through load_state_dict, torch.randn_like is
wrapped to return the case's noise, torch.optim.Adam is wrapped to keep the optimiser that learn() builds, and learn() runs
the case's epochs on the CPU.  Stored for EVERY case, per table in the order of vaecf_cases.NAMES:
    <case>/d_ref, d_ref_m, d_ref_v   max|reference float32 - float64 restatement| of the table, of Adam's exp_avg, exp_avg_sq
    <case>/move                      max|table after - table before|
    <case>/max, max_m, max_v         max|.| of the reference's table, exp_avg, exp_avg_sq
and for the FULL_CASES also the ten tables (<case>/P/<short>), exp_avg (M/), exp_avg_sq (V/), the per-step losses, score(u)
of a few users and a few score(u, i), from the reference's own VAECF.score.

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_vaecf_golden.py
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

import vaecf_cases as vc  # noqa: E402
from oracle import ref_loader  # noqa: E402


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


def reference_dataset(Dataset, c):
    u, i, r = vc.case_triplets(c)
    ds = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=1,   # (identity id maps)
                       global_uid_map=OrderedDict((n, n) for n in range(c["nu"])),
                       global_iid_map=OrderedDict((n, n) for n in range(c["ni"])))
    assert (ds.num_users, ds.num_items) == (c["nu"], c["ni"])
    X = ds.matrix
    assert X.nnz == len(r) and np.array_equal(X.toarray() != 0, vc.case_matrix(c).toarray() != 0)
    return ds


def run_case(ns, name):
    import torch

    c = vc.CASES[name]
    mod = importlib.import_module("cornac.models.vaecf.vaecf")
    VAECF = importlib.import_module("cornac.models.vaecf.recom_vaecf").VAECF
    ds = reference_dataset(ns.Dataset, c)
    model = VAECF(k=c["k"], autoencoder_structure=[c["h"]], act_fn=c["act"], likelihood=c["lik"], n_epochs=c["epochs"],
                  batch_size=c["bs"], learning_rate=c["lr"], beta=c["beta"], seed=1, verbose=False)
    model.vae = mod.VAE(c["k"], [c["ni"], c["h"]], c["act"], c["lik"])
    init = vc.case_params(c)
    model.vae.load_state_dict({n: torch.tensor(a) for n, a in init.items()})
    assert list(model.vae.state_dict()) == list(vc.NAMES)
    noise, bs = vc.case_noise(c), c["bs"]
    queue = [noise[e, u0:u0 + bs] for e in range(c["epochs"]) for u0 in range(0, c["nu"], bs)]
    losses, kept = [], []
    real_randn_like, real_adam, real_loss = torch.randn_like, torch.optim.Adam, model.vae.loss

    def randn_like(t, *a, **kw):
        e = torch.tensor(queue.pop(0))
        assert e.shape == t.shape
        return e

    class Adam(real_adam):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            kept.append(self)

    def loss(*a, **kw):
        out = real_loss(*a, **kw)
        losses.append(float(out.data.item()))
        return out

    torch.randn_like, torch.optim.Adam, model.vae.loss = randn_like, Adam, loss
    try:
        model.fit(ds)
    finally:
        torch.randn_like, torch.optim.Adam = real_randn_like, real_adam
        del model.vae.loss
    assert not queue and len(kept) == 1 and len(losses) == vc.n_steps(c)
    P = {n: a.detach().numpy().copy() for n, a in model.vae.state_dict().items()}
    state = kept[0].state
    params = dict(model.vae.named_parameters())
    M = {n: state[params[n]]["exp_avg"].numpy().copy() for n in vc.NAMES}
    V = {n: state[params[n]]["exp_avg_sq"].numpy().copy() for n in vc.NAMES}
    assert int(state[params[vc.NAMES[0]]]["step"]) == vc.n_steps(c)

    r, r_losses, _ = vc.run_case(name)
    dist = lambda ref, mine: np.array([np.abs(ref[n].astype(np.float64) - mine[n]).max() for n in vc.NAMES])   # noqa: E731
    top = lambda ref: np.array([np.abs(ref[n]).max() for n in vc.NAMES], np.float64)   # noqa: E731
    out = {name + "/d_ref": dist(P, r.P), name + "/d_ref_m": dist(M, r.M), name + "/d_ref_v": dist(V, r.V),
           name + "/move": np.array([np.abs(P[n].astype(np.float64) - init[n]).max() for n in vc.NAMES]),
           name + "/max": top(P), name + "/max_m": top(M), name + "/max_v": top(V)}
    print("%-16s steps %2d  d_ref %.2e  move %.2e .. %.2e  loss diff %.2e" % (
        name, vc.n_steps(c), out[name + "/d_ref"].max(), out[name + "/move"].min(), out[name + "/move"].max(),
        np.abs(np.array(losses) - r_losses).max()))
    if name in vc.FULL_CASES:
        for n in vc.NAMES:
            out["%s/P/%s" % (name, vc.SHORT[n])], out["%s/M/%s" % (name, vc.SHORT[n])] = P[n], M[n]
            out["%s/V/%s" % (name, vc.SHORT[n])] = V[n]
        out[name + "/losses"] = np.array(losses, np.float64)
        users, (pu, pi) = vc.score_users(c), vc.score_pairs(c)
        out[name + "/scores"] = np.array([model.score(int(u)) for u in users], np.float32)
        out[name + "/pair_scores"] = np.array([model.score(int(u), int(i)) for u, i in zip(pu, pi)], np.float32)
    return out


def main():
    ns = ref_loader.load()
    out = {"cases": np.array(sorted(vc.CASES))}
    for name in sorted(vc.CASES):
        out.update(run_case(ns, name))
    path = os.path.join(HERE, "vaecf_ref.npz")
    write_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
