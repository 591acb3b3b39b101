#!/usr/bin/env python3
"""Generates tests/golden/bivae_ref.npz by RUNNING THE REFERENCE'S OWN BiVAE AND learn() (only possible where the reference's
sources are present: oracle/build_ref.py's REF).  cornac/models/bivaecf is pure Python over torch, so nothing is compiled:
oracle.ref_loader.load() makes the reference's Dataset importable, and the model is imported from where it lies.  Nothing of
its text enters this repository.

Per case of tests/bivae_cases.py the reference's BiVAE gets the case's 12 tables through load_state_dict and the case's theta
and beta directly, torch.randn_like is wrapped to return the case's noise in call order (the draws of the final passes, which
reach no result, get zeros), torch.optim.Adam is wrapped to keep BOTH optimisers that learn() builds, and learn() runs the
case's epochs on the CPU.  Stored for EVERY case, per table in the order of bivae_cases.TABLES (the 12 parameter tables, then
theta, beta, mu_theta, mu_beta):
    <case>/d_ref [16], d_ref_m [12], d_ref_v [12]   max|reference float32 - float64 restatement| of the table, of Adam's exp_avg,
                                                    exp_avg_sq
    <case>/move [12]                                max|table after - table before| (the factor tables are outputs: none)
    <case>/max [16], max_m [12], max_v [12]         max|.| of the reference's table, exp_avg, exp_avg_sq
and for the FULL_CASES also the tables (<case>/P/<short>, <case>/F/<name>), exp_avg (M/), exp_avg_sq (V/), the per-step
losses (per epoch the item steps, then the user steps), score(u) of a few users and a few score(u, i), from the reference's
own BiVAECF.score.

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_bivae_golden.py
"""
import importlib
import os
import sys
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import bivae_cases as bc  # noqa: E402
from make_vaecf_golden import write_npz  # noqa: E402
from oracle import ref_loader  # noqa: E402


def reference_dataset(Dataset, c):
    u, i, r = bc.case_triplets(c)
    ds = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=1,   # (identity id maps)
                       global_uid_map=OrderedDict((n, n) for n in range(c["nu"])),
                       global_iid_map=OrderedDict((n, n) for n in range(c["ni"])))
    assert (ds.num_users, ds.num_items) == (c["nu"], c["ni"])
    X = ds.matrix
    assert X.nnz == len(r) and np.array_equal(X.toarray() != 0, bc.case_matrix(c).toarray() != 0)
    # the reference's item_iter / user_iter walk the ids that occur in the training triplets, so they would skip the case's
    # item that nobody holds; on a real split every id of the matrix occurs and they yield consecutive ranges.  The cases
    # keep the empty row, so the iterators here yield consecutive ranges over ALL ids (what the device does).
    def ranges(n):
        return lambda batch_size=1, shuffle=False: (np.arange(r0, min(r0 + batch_size, n)) for r0 in range(0, n, batch_size))

    ds.item_iter, ds.user_iter = ranges(c["ni"]), ranges(c["nu"])
    return ds


def run_case(ns, name):
    import torch

    c = bc.CASES[name]
    mod = importlib.import_module("cornac.models.bivaecf.bivae")
    BiVAECF = importlib.import_module("cornac.models.bivaecf.recom_bivaecf").BiVAECF
    ds = reference_dataset(ns.Dataset, c)
    model = BiVAECF(k=c["k"], encoder_structure=[c["h"]], act_fn=c["act"], likelihood=c["lik"], n_epochs=c["epochs"],
                    batch_size=c["bs"], learning_rate=c["lr"], beta_kl=c["beta"], seed=1, verbose=False, use_gpu=False)
    model.bivae = mod.BiVAE(k=c["k"], user_encoder_structure=[c["ni"], c["h"]], item_encoder_structure=[c["nu"], c["h"]],
                            act_fn=c["act"], likelihood=c["lik"], cap_priors={"user": False, "item": False},
                            feature_dim={"user": None, "item": None}, batch_size=c["bs"])
    init, factors = bc.case_params(c), bc.case_factors(c)
    model.bivae.load_state_dict({n: torch.tensor(a) for n, a in init.items()})
    assert list(model.bivae.state_dict()) == list(bc.NAMES)
    for n in bc.FACTORS:
        assert tuple(getattr(model.bivae, n).shape) == factors[n].shape
        setattr(model.bivae, n, torch.tensor(factors[n]))
    queue = bc.noise_queue(c)
    n_train = len(queue)
    losses, kept, tail = [], [], []
    real_randn_like, real_adam, real_loss = torch.randn_like, torch.optim.Adam, model.bivae.loss

    def randn_like(t, *a, **kw):
        if not queue:   # the final passes (the reference's learn, after the last epoch): only mu is kept of them
            tail.append(tuple(t.shape))
            return torch.zeros_like(t)
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

    torch.randn_like, torch.optim.Adam, model.bivae.loss = randn_like, Adam, loss
    try:
        model.fit(ds)
    finally:
        torch.randn_like, torch.optim.Adam = real_randn_like, real_adam
        del model.bivae.loss
    si, su = bc.n_steps(c)
    assert not queue and len(kept) == 2 and len(losses) == si + su and n_train == 2 * (si + su)
    assert len(tail) == (si + su) // c["epochs"], "one draw per batch in the final passes"
    P = {n: a.detach().numpy().copy() for n, a in model.bivae.state_dict().items()}
    F = {n: getattr(model.bivae, n).detach().numpy().copy() for n in bc.FACTORS}
    params = dict(model.bivae.named_parameters())
    state = {}
    for opt in kept:
        state.update(opt.state)
    M = {n: state[params[n]]["exp_avg"].numpy().copy() for n in bc.NAMES}
    V = {n: state[params[n]]["exp_avg_sq"].numpy().copy() for n in bc.NAMES}
    assert int(state[params[bc.NAMES[0]]]["step"]) == su and int(state[params[bc.NAMES[6]]]["step"]) == si   # (u_optimizer, i_optimizer)

    r, r_losses, _ = bc.run_case(name)
    dist = lambda ref, mine, names: np.array([np.abs(ref[n].astype(np.float64) - mine[n]).max() for n in names])   # noqa: E731
    top = lambda ref, names: np.array([np.abs(ref[n]).max() for n in names], np.float64)   # noqa: E731
    out = {name + "/d_ref": np.concatenate([dist(P, r.P, bc.NAMES), dist(F, r.F, bc.FACTORS)]),
           name + "/d_ref_m": dist(M, r.M, bc.NAMES), name + "/d_ref_v": dist(V, r.V, bc.NAMES),
           name + "/move": np.array([np.abs(P[n].astype(np.float64) - init[n]).max() for n in bc.NAMES]),
           name + "/max": np.concatenate([top(P, bc.NAMES), top(F, bc.FACTORS)]), name + "/max_m": top(M, bc.NAMES),
           name + "/max_v": top(V, bc.NAMES)}
    tol_share = max(bc.tolerance(out[name + "/d_ref"][q], out[name + "/max"][q]) / out[name + "/move"][q] for q in range(12)
                    if out[name + "/move"][q] > 0)
    print("%-16s steps %3d + %3d  d_ref %.2e (factors %.2e)  move %.2e .. %.2e  tolerance / move %.2e  loss diff %.2e" % (
        name, si, su, out[name + "/d_ref"][:12].max(), out[name + "/d_ref"][12:].max(), out[name + "/move"].min(),
        out[name + "/move"].max(), tol_share, np.abs(np.array(losses) - r_losses).max()))
    if name in bc.FULL_CASES:
        for n in bc.NAMES:
            out["%s/P/%s" % (name, bc.SHORT[n])], out["%s/M/%s" % (name, bc.SHORT[n])] = P[n], M[n]
            out["%s/V/%s" % (name, bc.SHORT[n])] = V[n]
        for n in bc.FACTORS:
            out["%s/F/%s" % (name, n)] = F[n]
        out[name + "/losses"] = np.array(losses, np.float64)
        users, (pu, pi) = bc.score_users(c), bc.score_pairs(c)
        out[name + "/scores"] = np.array([model.score(int(u)) for u in users], np.float32)
        out[name + "/pair_scores"] = np.array([np.ravel(model.score(int(u), int(i)))[0] for u, i in zip(pu, pi)], np.float64)
    return out


def main():
    ns = ref_loader.load()
    out = {"cases": np.array(sorted(bc.CASES))}
    for name in sorted(bc.CASES):
        out.update(run_case(ns, name))
    path = os.path.join(HERE, "bivae_ref.npz")
    write_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    assert os.path.getsize(path) < 300 * 1024


if __name__ == "__main__":
    main()
