#!/usr/bin/env python3
"""VAECF times: an epoch and a step of the device handle (`_lib.VaecfModel.fit_epoch`) next to the reference's loop on the
same GPU, at a synthetic ML-20M shape (138 493 users x 26 744 items, 20 M entries) from cornac_amd/synth.py, for two
settings: the reference's defaults (k = 10, h = 20, batch 100) and the paper's (k = 200, h = 600, batch 500).

The reference's tree is not needed: the comparison is a plain torch.nn restatement of its loop written for this tool (the
same five Linear layers, loss and torch.optim.Adam; per step a CSR row slice, `.toarray()`, `torch.tensor(..., device)` —
the host densify and upload that the reference's users pay, vaecf.py:130-133 — forward, backward, step, `loss.item()`).

Method: both sides are warmed up first (the handle on a 5-batch slice of the users with the same item side, torch for 5
steps); then the two alternate in this one process, --rounds times: one whole epoch of the handle (host clock around the
call, which ends in its one device synchronise), and enough torch steps to fill about --window seconds (host clock, a
device synchronise before and after).  Every timed window is at least a second unless the whole epoch is shorter.  The
torch epoch is its step time x the epoch's steps.

Also printed per setting, from the shapes alone: algorithmic bytes per step (24 B per parameter for Adam's dense sweep:
w, m, v read and written; plus the B x I logits written once, rewritten once in place and read four times), flops (three
B x h x I products), the time each bound asks for at 6.3 TB/s and 157.3 Tflop/s, which bound is the larger, and the share of
it that the measured step reaches.  Then the time to encode every user and rank a top-10 for all of them through the fused
scorer (`_scoring_tables` + `rank_batch`), the ranking half of `ranking_eval`.  No time is a pass/fail condition.

    python tools/vaecf_epoch.py
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
ap.add_argument("--shape", default="ml20m")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--window", type=float, default=1.5)
ap.add_argument("--settings", default="defaults,paper")
args = ap.parse_args()

from cornac_amd import VAECF, Dataset, _lib, synth  # noqa: E402

SETTINGS = {"defaults": dict(k=10, h=20, bs=100), "paper": dict(k=200, h=600, bs=500)}
HBM, FP32 = 6.3e12, 157.3e12


class TorchVAE(torch.nn.Module):
    """one hidden layer, tanh, multinomial likelihood: the reference's model at its defaults, written for this tool"""

    def __init__(self, n_items, k, h):
        super().__init__()
        self.fc0, self.mu, self.lv = torch.nn.Linear(n_items, h), torch.nn.Linear(h, k), torch.nn.Linear(h, k)
        self.d0, self.d1 = torch.nn.Linear(k, h), torch.nn.Linear(h, n_items)

    def forward(self, x):
        h1 = torch.tanh(self.fc0(x))
        mu, lv = self.mu(h1), self.lv(h1)
        std = torch.exp(0.5 * lv)
        z = mu + torch.randn_like(mu) * std
        p = torch.softmax(self.d1(torch.tanh(self.d0(z))), dim=1)
        ll = torch.sum(x * torch.log(p + 1e-10), dim=1)
        kld = torch.sum(-0.5 * (1 + 2.0 * torch.log(std) - mu.pow(2) - std.pow(2)), dim=1)
        return torch.mean(kld - ll)


def torch_steps(vae, opt, X, bs, first, count, dev):
    n = X.shape[0]
    for s in range(first, first + count):
        u0 = (s * bs) % (n - bs)
        batch = X[u0:u0 + bs, :]
        batch.data = np.ones(len(batch.data))
        x = torch.tensor(batch.toarray(), dtype=torch.float32, device=dev)
        loss = vae(x)
        opt.zero_grad()
        loss.backward()
        opt.step()
        loss.data.item()


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
n_users, n_items, users, items, ratings = synth.make(args.shape)
ds = Dataset.from_arrays(users, items, ratings, num_users=n_users, num_items=n_items)
X = ds.matrix
print("%s: %d users x %d items, %d entries" % (args.shape, n_users, n_items, X.nnz), flush=True)
dev = torch.device("cuda:0")

for name in args.settings.split(","):
    k, h, bs = (SETTINGS[name][q] for q in ("k", "h", "bs"))
    steps = -(-n_users // bs)
    params = 2 * n_items * h + n_items + 3 * k * h + 2 * h + 2 * k
    bytes_step = 24 * params + 6 * 4 * bs * n_items
    flops_step = 3 * 2 * bs * h * n_items
    t_bytes, t_flops = bytes_step / HBM, flops_step / FP32
    init = VAECF._initial_tables(n_items, k, h)
    warm = _lib.VaecfModel(X[:5 * bs], k, h)
    warm.set_params(init)
    warm.fit_epoch(bs, 1e-3, 1.0, seed=1)
    warm.close()
    model = _lib.VaecfModel(X, k, h)
    model.set_params(init)
    vae = TorchVAE(n_items, k, h).to(dev)
    opt = torch.optim.Adam(vae.parameters(), lr=1e-3)
    torch_steps(vae, opt, X, bs, 0, 5, dev)
    torch.cuda.synchronize()
    t_probe, _ = timed(lambda: (torch_steps(vae, opt, X, bs, 5, 5, dev), torch.cuda.synchronize()))
    n_torch = max(5, min(steps, int(args.window / (t_probe / 5)) + 1))
    ours, theirs, done = [], [], 10
    for _ in range(args.rounds):
        dt, (total, _) = timed(lambda: model.fit_epoch(bs, 1e-3, 1.0, seed=1))
        ours.append(dt)
        torch.cuda.synchronize()
        dt, _ = timed(lambda: (torch_steps(vae, opt, X, bs, done, n_torch, dev), torch.cuda.synchronize()))
        theirs.append(dt / n_torch)
        done += n_torch
    model.close()
    epoch, step, t_step = float(np.mean(ours)), float(np.mean(ours)) / steps, float(np.mean(theirs))
    bound, which = (t_bytes, "bytes") if t_bytes >= t_flops else (t_flops, "flops")
    print("%s (k = %d, h = %d, batch %d; %d steps per epoch, %d parameters): handle epoch %.3f s (%s), step %.3f ms, last epoch's mean "
          "loss %.4g; torch loop step %.3f ms over %d steps per window (%s) = epoch %.3f s; handle / torch = %.3f" % (
              name, k, h, bs, steps, params, epoch, ", ".join("%.3f" % t for t in ours), step * 1e3, total / steps, t_step * 1e3,
              n_torch, ", ".join("%.3f ms" % (t * 1e3) for t in theirs), t_step * steps, epoch / (t_step * steps)), flush=True)
    print("%s: per step %.1f MB algorithmic bytes = %.3f ms at 6.3 TB/s, %.2f Gflop = %.3f ms at 157.3 Tflop/s; the larger bound is %s; "
          "the measured step is %.1f x that bound (%.1f %% of it reached)" % (
              name, bytes_step / 1e6, t_bytes * 1e3, flops_step / 1e9, t_flops * 1e3, which, step / bound, 100.0 * bound / step), flush=True)
    del vae, opt

    if name == "defaults":
        m = VAECF(k=k, autoencoder_structure=[h], n_epochs=1, batch_size=bs)
        t_fit, _ = timed(lambda: m.fit(ds))
        everyone = np.arange(n_users)
        t_enc, _ = timed(m._scoring_tables)
        m.rank_batch(everyone[:4096], k=10)
        t_rank, _ = timed(lambda: [m.rank_batch(everyone[b:b + 16384], k=10) for b in range(0, n_users, 16384)])
        print("%s: VAECF.fit of one epoch as a whole %.3f s; h2 of all %d users (encode_users) %.3f s; rank_batch top-10 of all users "
              "through the fused scorer %.3f s" % (name, t_fit, n_users, t_enc, t_rank), flush=True)
