#!/usr/bin/env python3
"""NeuMF times: an epoch and a step of the device handle (`_lib.NcfModel`) next to the reference's loop on the same GPU, at a
synthetic ML-20M shape (138 493 users x 26 744 items, 20 M entries) from cornac_amd/synth.py, for two settings: the
reference's defaults (num_factors 8, layers 64-32-16-8) and a larger one (num_factors 64, layers 256-128-64); batch 256,
num_neg 4 (1 280 samples per step), Adam.

The reference's tree is not needed: the comparison is a plain torch.nn restatement of its loop written for this tool (two
pairs of nn.Embedding, the Linear + ReLU stack, one logit over the concatenation, nn.BCELoss, torch.optim.Adam; per step the
batch's three arrays go to the device, then forward, backward, step and `loss.item()`, as recom_ncf_base.py's loop does).
Both sides take the same pre-drawn batches (`draw_epoch`), so the reference's Python sampler is in neither; its time is
reported separately: `Dataset.uir_iter(num_zeros=4)`, the sampler restated draw for draw, over a 1 M-entry corner, as
seconds per epoch of the full shape at the measured time per sample.

Method: both sides are warmed up first; then they alternate in this one process, --rounds times: --steps steps of the
handle in one `fit_epoch` call (host clock around the call, which ends in its one device synchronise) and enough torch steps
to fill about --window seconds (host clock, a device synchronise before and after).  Then one whole epoch of
`fit_epoch_sampled` (sampling on the device included), host clock.  Printed with them, from the shapes alone: the bytes of
the optimiser's dense sweep per step (24 B per entry under Adam) and its time at 6.3 TB/s.  No time is a pass/fail condition.

    python tools/ncf_epoch.py
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
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--window", type=float, default=1.5)
ap.add_argument("--settings", default="defaults,larger")
ap.add_argument("--no-epoch", action="store_true", help="skip the whole epoch of fit_epoch_sampled")
args = ap.parse_args()

from cornac_amd import Dataset, _lib, synth  # noqa: E402
from cornac_amd.ncf import _neumf_initial  # noqa: E402

SETTINGS = {"defaults": dict(f=8, layers=(64, 32, 16, 8)), "larger": dict(f=64, layers=(256, 128, 64))}
BS, NN, LR, HBM = 256, 4, 1e-3, 6.3e12


class TorchNeuMF(torch.nn.Module):
    """GMF and MLP under one logit; written for this tool"""

    def __init__(self, nu, ni, f, layers):
        super().__init__()
        E = torch.nn.Embedding
        self.gu, self.gi, self.mu, self.mi = E(nu, f), E(ni, f), E(nu, layers[0] // 2), E(ni, layers[0] // 2)
        stack = []
        for a, b in zip(layers[:-1], layers[1:]):
            stack += [torch.nn.Linear(a, b), torch.nn.ReLU()]
        self.mlp, self.logit = torch.nn.Sequential(*stack), torch.nn.Linear(f + layers[-1], 1)

    def forward(self, u, i):
        h = torch.cat([self.gu(u) * self.gi(i), self.mlp(torch.cat([self.mu(u), self.mi(i)], dim=-1))], dim=-1)
        return torch.sigmoid(self.logit(h)).view(-1)


def torch_steps(net, opt, crit, ptr, users, items, labels, first, count, dev):
    n_steps = len(ptr) - 1
    for s in range(first, first + count):
        a, b = ptr[s % n_steps], ptr[s % n_steps + 1]
        u, i = torch.from_numpy(users[a:b]).to(dev), torch.from_numpy(items[a:b]).to(dev)
        y = torch.tensor(labels[a:b], dtype=torch.float).to(dev)
        opt.zero_grad()
        loss = crit(net(u, i), y)
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
epoch_steps = -(-X.nnz // BS)
print("%s: %d users x %d items, %d entries, %d steps of %d samples per epoch" % (args.shape, n_users, n_items, X.nnz, epoch_steps, BS * (1 + NN)),
      flush=True)

# the reference's sampler, restated draw for draw, on a corner of the data
corner = Dataset.from_arrays(users[:1_000_000], items[:1_000_000], ratings[:1_000_000], num_users=n_users, num_items=n_items, seed=1)
it = corner.uir_iter(BS, shuffle=True, binary=True, num_zeros=NN)
next(it)
dt, got = timed(lambda: sum(len(next(it)[0]) for _ in range(200)))
print("the reference's sampler (uir_iter, num_zeros = %d): %.2f us per sample over %d samples = %.0f s per epoch of this shape" % (
    NN, dt / got * 1e6, got, dt / got * X.nnz * (1 + NN)), flush=True)
del corner, it
dev = torch.device("cuda:0")

for name in args.settings.split(","):
    f, layers = SETTINGS[name]["f"], SETTINGS[name]["layers"]
    model = _lib.NcfModel("NeuMF", X, f, layers, "relu")
    torch.manual_seed(1)
    model.set_params(_neumf_initial(n_users, n_items, f, layers))
    entries = sum(int(np.prod(s)) for n, s in _lib.NcfModel.shapes("NeuMF", n_users, n_items, f, layers).items()
                  if n not in _lib.NcfModel.UNUSED("NeuMF"))
    print("%s: %.2f M table entries with a gradient; Adam's dense sweep moves 24 B x that = %.1f MB per step = %.4f ms at 6.3 TB/s" % (
        name, entries / 1e6, 24 * entries / 1e6, 24 * entries / HBM * 1e3), flush=True)
    ptr, su, si, sy = model.draw_epoch(BS, NN, seed=1, epoch=0)
    K = min(args.steps, epoch_steps)
    cut = int(ptr[K])
    ptr, su, si, sy = ptr[:K + 1].copy(), su[:cut].copy(), si[:cut].copy(), sy[:cut].copy()
    model.fit_epoch(ptr[:51], su[:ptr[50]], si[:ptr[50]], sy[:ptr[50]], LR)   # warm-up
    net = TorchNeuMF(n_users, n_items, f, layers).to(dev)
    opt, crit = torch.optim.Adam(net.parameters(), lr=LR), torch.nn.BCELoss()
    su64, si64 = su.astype(np.int64), si.astype(np.int64)
    torch_steps(net, opt, crit, ptr, su64, si64, sy, 0, 5, dev)
    torch.cuda.synchronize()
    t_probe, _ = timed(lambda: (torch_steps(net, opt, crit, ptr, su64, si64, sy, 5, 5, dev), torch.cuda.synchronize()))
    n_torch, done = max(5, int(args.window / (t_probe / 5)) + 1), 10
    ours, theirs = [], []
    for _ in range(args.rounds):
        dt, (total, _) = timed(lambda: model.fit_epoch(ptr, su, si, sy, LR))
        ours.append(dt / K)
        torch.cuda.synchronize()
        dt, _ = timed(lambda: (torch_steps(net, opt, crit, ptr, su64, si64, sy, done, n_torch, dev), torch.cuda.synchronize()))
        theirs.append(dt / n_torch)
        done += n_torch
    ms = lambda ts: ", ".join("%.4f ms" % (t * 1e3) for t in ts)   # noqa: E731
    step, tstep = float(np.mean(ours)), float(np.mean(theirs))
    print("%s (num_factors %d, layers %s): handle step %.4f ms over %d steps per call (%s), last call's mean loss %.4g = epoch %.2f s at %d "
          "steps; torch loop step %.4f ms over %d steps per window (%s) = epoch %.2f s; handle / torch = %.3f" % (
              name, f, "-".join(str(x) for x in layers), step * 1e3, K, ms(ours), total / K, step * epoch_steps, epoch_steps, tstep * 1e3,
              n_torch, ms(theirs), tstep * epoch_steps, step / tstep), flush=True)
    del net, opt
    torch.cuda.empty_cache()
    if not args.no_epoch:
        dt, (total, _) = timed(lambda: model.fit_epoch_sampled(BS, NN, LR, seed=2, epoch=1))
        print("%s: one whole epoch of fit_epoch_sampled (device sampling included) %.2f s = %.4f ms per step, mean loss %.4g" % (
            name, dt, dt / epoch_steps * 1e3, total / epoch_steps), flush=True)
    model.close()
