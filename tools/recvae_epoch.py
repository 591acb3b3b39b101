#!/usr/bin/env python3
"""RecVAE times: a pass and a step of the device handle (`_lib.RecvaeModel.fit_epoch`) next to the reference's loop on the
same GPU, at the defaults (hidden 600, latent 200, batch 500), at a synthetic ML-20M shape (138 493 users x 26 744 items,
20 M entries) and at the ML-100K shape (943 x 1 682, 80 000 entries) from cornac_amd/synth.py, for the two kinds of pass:
the encoder's (dropout 0.5, the encoder's Adam) and the decoder's (no dropout, the decoder's Adam).

The reference's tree is not needed: the comparison is a plain torch.nn restatement of its loop written for this tool (the
same layers, composite prior, loss and two torch.optim.Adam; per step a CSR row slice of shuffled users, `.toarray()`,
`torch.Tensor(...).to(device)` -- the host densify and upload that the reference's users pay, recom_recvae.py:136 --
forward, backward, step).

Method: both sides are warmed up first (the handle on a 3-batch slice of the users with the same item side, torch for 3
steps); then the two alternate in this one process, --rounds times: one whole pass of the handle (host clock around the
call, which ends in its one device synchronise; update_prior's pass over all users is timed on its own), and enough torch
steps to fill about --window seconds (host clock, a device synchronise before and after).  The torch pass is its step time
x the pass's steps.

Also printed, from the shapes alone: algorithmic bytes per step (24 B per parameter of the tables that step, for Adam's
dense sweep: w, m, v read and written; plus the B x I logits written once, rewritten once in place and read twice in an
encoder step or once in a decoder step) and flops (per encoder step the dense layers forward and twice backward, the
decoder's product forward and once backward, fc1's sparse products left out; per decoder step the encoder forward and the
decoder's product twice), the time each bound asks for at 6.3 TB/s and 157.3 Tflop/s, and the share of the larger one that
the measured step reaches.  No time is a pass/fail condition.

    python tools/recvae_epoch.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="ml100k,ml20m")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--window", type=float, default=1.5)
ap.add_argument("--hidden", type=int, default=600)
ap.add_argument("--latent", type=int, default=200)
ap.add_argument("--batch", type=int, default=500)
args = ap.parse_args()

from cornac_amd import Dataset, RecVAE, _lib, synth  # noqa: E402

HBM, FP32 = 6.3e12, 157.3e12
LOG_W = [float(np.log(w)) for w in (3 / 20, 3 / 4, 1 / 10)]


def swish(x):
    return x * torch.sigmoid(x)


def log_norm(x, mu, lv):
    return -0.5 * (lv + float(np.log(2 * np.pi)) + (x - mu) ** 2 / lv.exp())


class TorchEncoder(torch.nn.Module):
    def __init__(self, n_items, h, k):
        super().__init__()
        self.fc = torch.nn.ModuleList([torch.nn.Linear(n_items if l == 0 else h, h) for l in range(5)])
        self.ln = torch.nn.ModuleList([torch.nn.LayerNorm(h, eps=0.1) for _ in range(5)])
        self.mu, self.lv = torch.nn.Linear(h, k), torch.nn.Linear(h, k)

    def forward(self, x, rate):
        x = torch.nn.functional.dropout(torch.nn.functional.normalize(x), rate, training=True)
        skip, hid = 0.0, x
        for fc, ln in zip(self.fc, self.ln):
            hid = ln(swish(fc(hid) + skip))
            skip = skip + hid
        return self.mu(hid), self.lv(hid)


class TorchRecVAE(torch.nn.Module):
    """the reference's model, written for this tool"""

    def __init__(self, n_items, h, k):
        super().__init__()
        self.encoder, self.old, self.decoder = TorchEncoder(n_items, h, k), TorchEncoder(n_items, h, k), torch.nn.Linear(k, n_items)
        self.old.requires_grad_(False)
        self.register_buffer("pri", torch.tensor([[0.0] * k, [0.0] * k, [10.0] * k]))

    def forward(self, x, rate, gamma):
        mu, lv = self.encoder(x, rate)
        z = mu + torch.zeros_like(mu).normal_(mean=0, std=0.01) * torch.exp(0.5 * lv)
        o = self.decoder(z)
        pm, plv = self.old(x, 0)
        mix = torch.stack([log_norm(z, self.pri[0], self.pri[1]) + LOG_W[0], log_norm(z, pm, plv) + LOG_W[1],
                           log_norm(z, self.pri[0], self.pri[2]) + LOG_W[2]], dim=-1)
        mll = (torch.log_softmax(o, dim=-1) * x).sum(dim=-1).mean()
        kld = ((log_norm(z, mu, lv) - torch.logsumexp(mix, dim=-1)).sum(dim=-1) * (gamma * x.sum(dim=-1))).mean()
        return -(mll - kld)


def torch_steps(vae, opt, X, order, bs, first, count, rate, dev):
    n = X.shape[0]
    for s in range(first, first + count):
        p0 = (s * bs) % max(1, n - bs)
        x = torch.Tensor(X[order[p0:p0 + bs], :].toarray()).to(dev)
        opt.zero_grad()
        loss = vae(x, rate, 0.005)
        loss.backward()
        opt.step()
    return float(loss.detach())


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
dev = torch.device("cuda:0")
h, k, bs = args.hidden, args.latent, args.batch

for shape in args.shapes.split(","):
    n_users, n_items, users, items, ratings = synth.make(shape)
    X = Dataset.from_arrays(users, items, ratings, num_users=n_users, num_items=n_items).matrix
    steps = -(-n_users // bs)
    nb = min(bs, n_users)
    print("%s: %d users x %d items, %d entries; hidden %d, latent %d, batch %d: %d steps per pass" % (
        shape, n_users, n_items, X.nnz, h, k, bs, steps), flush=True)
    enc_params = n_items * h + 4 * h * h + 15 * h + 2 * (k * h + k)
    dec_params = n_items * k + n_items
    dense = 4 * h * h + 2 * h * k            # multiply-adds per row of the dense layers behind fc1
    init = RecVAE._initial_tables(n_items, h, k)
    rs = np.random.RandomState(1)
    warm = _lib.RecvaeModel(X[:3 * nb], h, k)
    warm.set_params(init)
    for enc in (True, False):
        warm.fit_epoch(rs.permutation(warm.n_users), bs, 5e-4, 0.005, None, 0.5 if enc else 0.0, enc, not enc, seed=1)
    warm.close()
    model = _lib.RecvaeModel(X, h, k)
    model.set_params(init)
    t_prior, _ = timed(model.update_prior)
    t_prior, _ = timed(model.update_prior)
    vae = TorchRecVAE(n_items, h, k).to(dev)
    opts = {True: torch.optim.Adam(vae.encoder.parameters(), lr=5e-4), False: torch.optim.Adam(vae.decoder.parameters(), lr=5e-4)}
    print("%s: update_prior (the old encoder's posterior of all %d users) %.3f s" % (shape, n_users, t_prior), flush=True)
    for enc in (True, False):
        kind, rate = ("encoder" if enc else "decoder"), (0.5 if enc else 0.0)
        order = rs.permutation(n_users)
        torch_steps(vae, opts[enc], X, order, bs, 0, 3, rate, dev)
        torch.cuda.synchronize()
        t_probe, _ = timed(lambda: (torch_steps(vae, opts[enc], X, order, bs, 3, 3, rate, dev), torch.cuda.synchronize()))
        n_torch = max(3, min(steps, int(args.window / (t_probe / 3)) + 1))
        ours, theirs, done = [], [], 6
        for _ in range(args.rounds):
            order = rs.permutation(n_users)
            dt, losses = timed(lambda: model.fit_epoch(order, bs, 5e-4, 0.005, None, rate, enc, not enc, seed=1))
            ours.append(dt)
            torch.cuda.synchronize()
            dt, _ = timed(lambda: (torch_steps(vae, opts[enc], X, order, bs, done, n_torch, rate, dev), torch.cuda.synchronize()))
            theirs.append(dt / n_torch)
            done += n_torch
        if enc:
            bytes_step = 24 * enc_params + 4 * 4 * nb * n_items
            flops_step = 2 * nb * (3 * dense + 2 * n_items * k)
        else:
            bytes_step = 24 * dec_params + 3 * 4 * nb * n_items
            flops_step = 2 * nb * (dense + 2 * n_items * k)
        t_bytes, t_flops = bytes_step / HBM, flops_step / FP32
        bound, which = (t_bytes, "bytes") if t_bytes >= t_flops else (t_flops, "flops")
        epoch, step, t_step = float(np.mean(ours)), float(np.mean(ours)) / steps, float(np.mean(theirs))
        print("%s %s pass: handle %.3f s (%s), step %.3f ms, last pass's mean negative_elbo %.5g; torch loop step %.3f ms over %d steps "
              "per window (%s) = pass %.3f s; handle / torch = %.3f" % (
                  shape, kind, epoch, ", ".join("%.3f" % t for t in ours), step * 1e3, losses[:, 2].mean(), t_step * 1e3, n_torch,
                  ", ".join("%.3f ms" % (t * 1e3) for t in theirs), t_step * steps, epoch / (t_step * steps)), flush=True)
        print("%s %s step: %.1f MB algorithmic bytes = %.3f ms at 6.3 TB/s, %.2f Gflop = %.3f ms at 157.3 Tflop/s; the larger bound is "
              "%s; the measured step is %.1f x that bound (%.1f %% of it reached)" % (
                  shape, kind, bytes_step / 1e6, t_bytes * 1e3, flops_step / 1e9, t_flops * 1e3, which, step / bound,
                  100.0 * bound / step), flush=True)
    model.close()
    del vae, opts
