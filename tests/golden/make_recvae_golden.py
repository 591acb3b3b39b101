#!/usr/bin/env python3
"""Generates tests/golden/recvae_ref.npz by RUNNING THE REFERENCE'S OWN VAE AND RecVAE.run (only possible where the
reference's sources are present: oracle/build_ref.py's REF).  cornac/models/recvae is pure Python over torch, so nothing is
compiled: oracle.ref_loader.load() makes the reference's Dataset, metrics and evaluation importable, and the model is
imported from where it lies.  Nothing of its text enters this repository.

Per case of tests/recvae_cases.py the reference's VAE gets the case's tables through load_state_dict; what the reference
calls for its draws is wrapped to serve the case's: its module's `F.dropout` (the case's mask where the rate is not zero)
and `Tensor.normal_` (the case's noise); the batches come from a stand-in for the data set that yields the case's orders;
the two torch.optim.Adam are built as RecVAE.fit builds them and kept; RecVAE.run runs each pass on the CPU, with
update_prior where fit calls it.  Stored for EVERY case, per table in the order of recvae_cases.TRAINABLE:
    <case>/d_ref, d_ref_m, d_ref_v   max|reference float32 - float64 restatement| of the table, of Adam's exp_avg, exp_avg_sq
    <case>/move                      max|table after - table before|
    <case>/max, max_m, max_v         max|.| of the reference's table, exp_avg, exp_avg_sq
    <case>/exact                     the restatement leaves the table exactly in place: its gradient is 0 in exact arithmetic
                                     (hidden_dim 1: a LayerNorm of one element passes nothing back).  The reference's float32
                                     run turns such zeros into rounding noise that Adam scales up to a full step, so its
                                     d_ref and move say nothing there; the tests hold these tables bit for bit instead
and for the FULL_CASES also the 53 tables (<case>/P/<q>, q the index in recvae_cases.NAMES), exp_avg (M/), exp_avg_sq (V/),
the steps' (mll, kld, negative_elbo), and in evaluation mode (model.eval(): no dropout, z = mu) the logits of a few users
and a few pairs.  For recvae_cases.SEEDED the reference's own seeded RecVAE.fit runs on the case's data set:
<name>/P/<q> and <name>/order, the users in the order its passes took them.

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_recvae_golden.py
"""
import importlib
import io
import os
import sys
import types
import zipfile
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import recvae_cases as rc  # noqa: E402
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


def reference_dataset(Dataset, c, seed=1):
    u, i, r = rc.case_triplets(c)
    ds = Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=seed,   # (identity id maps)
                       global_uid_map=OrderedDict((n, n) for n in range(c["nu"])),
                       global_iid_map=OrderedDict((n, n) for n in range(c["ni"])))
    assert (ds.num_users, ds.num_items) == (c["nu"], c["ni"])
    X = ds.csr_matrix
    assert X.nnz == len(r) and np.array_equal(X.toarray(), rc.case_matrix(c).toarray())
    return ds


class ServedSet:
    """what RecVAE.run reads of a data set: the matrix, and user batches, here the case's"""

    def __init__(self, X):
        self.csr_matrix, self.order, self.batch = X, None, None

    def user_iter(self, batch_size, shuffle=False):
        assert shuffle
        for p0 in range(0, len(self.order), batch_size):
            self.batch = self.order[p0:p0 + batch_size]
            yield self.batch


def run_case(ns, name):
    import torch

    c = rc.CASES[name]
    mod = importlib.import_module("cornac.models.recvae.recvae")
    RecVAE = importlib.import_module("cornac.models.recvae.recom_recvae").RecVAE
    X = rc.case_matrix(c)
    rec = RecVAE(hidden_dim=c["h"], latent_dim=c["k"], batch_size=c["bs"], beta=c["beta"], gamma=c["gamma"], lr=c["lr"], use_gpu=False)
    vae = mod.VAE(hidden_dim=c["h"], latent_dim=c["k"], input_dim=c["ni"])
    init = rc.case_params(c)
    vae.load_state_dict({n: torch.tensor(a) for n, a in init.items()})
    assert list(vae.state_dict()) == list(rc.NAMES)
    served = ServedSet(X)
    current, losses = {}, []
    restate = rc.Restatement(X, c["h"], c["k"])   # (only for keep_matrix)
    real_F, real_normal = mod.F, torch.Tensor.normal_

    def dropout(x, p=0.5, training=True, inplace=False):
        if not p:
            return real_F.dropout(x, p, training, inplace)
        assert training and current["rate"] == p
        return x * torch.tensor(current["K"][served.batch] / (1.0 - p), dtype=x.dtype)

    def normal_(self, mean=0, std=1, **kw):
        assert (mean, std) == (0, 0.01) and tuple(self.shape) == (len(served.batch), c["k"])
        return self.copy_(torch.tensor(current["eps"][served.batch]))

    shim = types.SimpleNamespace(dropout=dropout, normalize=real_F.normalize, log_softmax=real_F.log_softmax)
    hook = vae.register_forward_hook(lambda m, i, out: losses.append([float(t.detach()) for t in (out[0][0], out[0][1], out[1])]))
    enc_opt = torch.optim.Adam(set(vae.encoder.parameters()), lr=c["lr"])
    dec_opt = torch.optim.Adam(set(vae.decoder.parameters()), lr=c["lr"])
    mod.F, torch.Tensor.normal_ = shim, normal_
    try:
        for q, p in enumerate(rc.case_passes(c)):
            if q == 1 and not c["not_alternating"]:
                vae.update_prior()
            served.order = p["order"].astype(np.int64)
            current.update(rate=p["rate"], eps=p["eps"], K=restate.keep_matrix(p["keep"]) if p["rate"] else None)
            opts = {"enc": [enc_opt], "dec": [dec_opt], "joint": [enc_opt, dec_opt]}[p["kind"]]
            rec.run(model=vae, opts=opts, train_set=served, my_batch_size=c["bs"], n_epochs=1, beta=c["beta"], gamma=c["gamma"],
                    dropout_rate=p["rate"])
    finally:
        mod.F, torch.Tensor.normal_ = real_F, real_normal
        hook.remove()
    assert len(losses) == rc.n_steps(c)
    P = {n: a.detach().numpy().copy() for n, a in vae.state_dict().items()}
    params = dict(vae.named_parameters())
    state = lambda n: (enc_opt if n.startswith("encoder.") else dec_opt).state[params[n]]   # noqa: E731
    M = {n: state(n)["exp_avg"].numpy().copy() for n in rc.TRAINABLE}
    V = {n: state(n)["exp_avg_sq"].numpy().copy() for n in rc.TRAINABLE}
    t_enc, t_dec = int(state(rc.ENC_NAMES[0])["step"]), int(state(rc.DEC_NAMES[0])["step"])

    r, r_losses, _ = rc.run_case(name)
    assert (t_enc, t_dec) == (r.t_enc, r.t_dec)
    dist = lambda ref, mine: np.array([np.abs(ref[n].astype(np.float64) - mine[n]).max() for n in rc.TRAINABLE])   # noqa: E731
    top = lambda ref: np.array([np.abs(ref[n]).max() for n in rc.TRAINABLE], np.float64)   # noqa: E731
    frozen = max(np.abs(P[n].astype(np.float64) - r.P[n]).max() for n in rc.NAMES if n not in rc.TRAINABLE)
    out = {name + "/d_ref": dist(P, r.P), name + "/d_ref_m": dist(M, r.M), name + "/d_ref_v": dist(V, r.V),
           name + "/move": np.array([np.abs(P[n].astype(np.float64) - init[n]).max() for n in rc.TRAINABLE]),
           name + "/max": top(P), name + "/max_m": top(M), name + "/max_v": top(V), name + "/t": np.array([t_enc, t_dec]),
           name + "/exact": np.array([np.array_equal(r.P[n], init[n].astype(np.float64)) for n in rc.TRAINABLE])}
    losses = np.array(losses, np.float64)
    moved = ~out[name + "/exact"]
    ratio = (np.maximum(16 * out[name + "/d_ref"], 4 * np.array([rc.ulp32(t) for t in out[name + "/max"]]))[moved] / out[name + "/move"][moved]).max()
    print("%-12s steps %2d  d_ref %.2e  old/prior diff %.2e  move %.2e .. %.2e  tol/move %.3f %%  loss rel diff %.2e" % (
        name, rc.n_steps(c), out[name + "/d_ref"].max(), frozen, out[name + "/move"][moved].min(), out[name + "/move"].max(), 100 * ratio,
        np.abs((losses - r_losses) / np.where(r_losses == 0, 1, r_losses)).max()))
    if name in rc.FULL_CASES:
        for q, n in enumerate(rc.NAMES):
            out["%s/P/%d" % (name, q)] = P[n]
        for q, n in enumerate(rc.TRAINABLE):
            out["%s/M/%d" % (name, q)], out["%s/V/%d" % (name, q)] = M[n], V[n]
        out[name + "/losses"] = losses
        users, (pu, pi) = rc.score_users(c), rc.score_pairs(c)
        vae.eval()
        dense = lambda u: torch.tensor(X[np.asarray(u)].toarray(), dtype=torch.float32)   # noqa: E731
        with torch.no_grad():
            out[name + "/logits"] = vae(dense(users), calculate_loss=False).numpy().astype(np.float32)
            out[name + "/pair_logits"] = vae(dense(pu), calculate_loss=False).numpy()[np.arange(len(pu)), pi].astype(np.float32)
    return out


def run_seeded(ns, name):
    """the reference's own RecVAE.fit under a seed, nothing wrapped but the data set's user_iter, which is recorded"""
    s = rc.SEEDED[name]
    c = rc.CASES[s["case"]]
    RecVAE = importlib.import_module("cornac.models.recvae.recom_recvae").RecVAE
    ds = reference_dataset(ns.Dataset, c, seed=s["seed"])
    taken, real_iter = [], ds.user_iter

    def user_iter(batch_size=1, shuffle=False):
        for batch in real_iter(batch_size, shuffle):
            taken.append(np.array(batch))
            yield batch

    ds.user_iter = user_iter
    rec = RecVAE(hidden_dim=c["h"], latent_dim=c["k"], batch_size=c["bs"], beta=c["beta"], gamma=c["gamma"], lr=c["lr"], n_epochs=s["n_epochs"],
                 n_enc_epochs=s["n_enc_epochs"], n_dec_epochs=s["n_dec_epochs"], not_alternating=s["not_alternating"], seed=s["seed"],
                 use_gpu=False, verbose=False)
    rec.fit(ds)
    sd = rec.recvae_model.state_dict()
    assert list(sd) == list(rc.NAMES)
    out = {"%s/P/%d" % (name, q): sd[n].detach().numpy().copy() for q, n in enumerate(rc.NAMES)}
    out[name + "/order"] = np.concatenate(taken).astype(np.int32)
    print("%-12s passes %d" % (name, len(out[name + "/order"]) // c["nu"]))
    return out


def main():
    ns = ref_loader.load()
    out = {"cases": np.array(sorted(rc.CASES))}
    for name in sorted(rc.CASES):
        out.update(run_case(ns, name))
    for name in sorted(rc.SEEDED):
        out.update(run_seeded(ns, name))
    path = os.path.join(HERE, "recvae_ref.npz")
    write_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
