#!/usr/bin/env python3
"""BiVAECF times: an epoch, an item step and a user step of the device handle (`_lib.BivaeModel.fit_epoch`) next to the
reference's loop on the same GPU, at a synthetic ML-20M shape (138 493 users x 26 744 items, 20 M entries) from
cornac_amd/synth.py, for two settings: the reference's defaults (k = 10, h = 20, batch 100) and a larger one (k = 50,
h = 100, batch 500; a guess at a realistic setting, not the reference's).

The reference's tree is not needed: the comparison is a plain torch.nn restatement of its loop written for this tool (two
encoders of three Linear layers each, the bilinear decoder against the other side's table, the Poisson loss, two
torch.optim.Adam; per step a CSR row slice of X or of its transpose, `.toarray()`, `torch.tensor(..., device)` — the host
densify and upload that the reference's users pay — forward, backward, step, `loss.item()`, and the second forward whose
sample and mean are stored).

Method: both sides are warmed up first (the handle for one epoch on a 5-batch corner of the matrix, torch for 3 steps per
side); then the two alternate in this one process, --rounds times: one whole epoch of the handle (host clock around the
call, which ends in its one device synchronise; the split into the item pass and the user pass comes from the handle's
stream events), and enough torch steps per side to fill about --window seconds (host clock, a device synchronise before
and after).  The torch epoch is its step times x the epoch's steps.

Also printed per setting and side, from the shapes alone, the fused decode's bounds per step: N x k x 4 bytes of the other
side's table plus the [S x B x k] and [S x B] partials written and read once, at 6.3 TB/s; 4 B N k flops at 157.3 Tflop/s
plus B N exponentials.  Set the kernel's own time from a `rocprofv3 --kernel-trace --stats` run of this tool (with
--handle-only, which skips the torch loop) against them.  No time is a pass/fail condition.

    python tools/bivaecf_epoch.py
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
ap.add_argument("--settings", default="defaults,larger")
ap.add_argument("--handle-only", action="store_true", help="one warm-up and one epoch of the handle per setting, no torch loop")
args = ap.parse_args()

from cornac_amd import BiVAECF, Dataset, _lib, synth  # noqa: E402

SETTINGS = {"defaults": dict(k=10, h=20, bs=100), "larger": dict(k=50, h=100, bs=500)}
HBM, FP32 = 6.3e12, 157.3e12


class TorchEncoder(torch.nn.Module):
    """one side of the bilateral VAE: one hidden layer, tanh, std = sigmoid(.); written for this tool"""

    def __init__(self, n_in, k, h):
        super().__init__()
        self.fc0, self.mu, self.std = torch.nn.Linear(n_in, h), torch.nn.Linear(h, k), torch.nn.Linear(h, k)

    def forward(self, x):
        h1 = torch.tanh(self.fc0(x))
        mu, std = self.mu(h1), torch.sigmoid(self.std(h1))
        return mu + torch.randn_like(mu) * std, mu, std


def torch_steps(enc, opt, M, own, other, mean, bs, first, count, dev):
    """`count` steps of one side: rows of M (X or its transpose), `other` the constant table, `own` / `mean` this side's"""
    n = M.shape[0]
    for s in range(first, first + count):
        r0 = (s * bs) % max(1, n - bs)
        batch = M[r0:r0 + bs, :]
        batch.data = np.ones(len(batch.data))
        x = torch.tensor(batch.toarray(), dtype=torch.float32, device=dev)
        z, mu, std = enc(x)
        p = torch.sigmoid(z.mm(other.t()))
        ll = torch.sum(x * torch.log(p + 1e-10) - p, dim=1)
        kld = torch.sum(-0.5 * (1 + 2.0 * torch.log(std) - mu.pow(2) - std.pow(2)), dim=1)
        loss = torch.mean(kld - ll)
        opt.zero_grad()
        loss.backward()
        opt.step()
        loss.data.item()
        with torch.no_grad():
            z, mu, _ = enc(x)
            own[r0:r0 + len(x)] = z
            mean[r0:r0 + len(x)] = mu


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def start(model, n_users, n_items, k, h):
    init = BiVAECF._initial_tables(n_users, n_items, k, h)
    model.set_params(init.tables)
    model.set_factors(theta=init.theta, beta=init.beta)


print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
n_users, n_items, users, items, ratings = synth.make(args.shape)
ds = Dataset.from_arrays(users, items, ratings, num_users=n_users, num_items=n_items)
X = ds.matrix
XT = X.T.tocsr()
print("%s: %d users x %d items, %d entries" % (args.shape, n_users, n_items, X.nnz), flush=True)
dev = torch.device("cuda:0")

for name in args.settings.split(","):
    k, h, bs = (SETTINGS[name][q] for q in ("k", "h", "bs"))
    steps_i, steps_u = -(-n_items // bs), -(-n_users // bs)
    corner = X[:5 * bs, :5 * bs]
    warm = _lib.BivaeModel(corner, k, h)
    start(warm, corner.shape[0], corner.shape[1], k, h)
    warm.fit_epoch(bs, 1e-3, 1.0, seed=1)
    warm.close()
    model = _lib.BivaeModel(X, k, h)
    start(model, n_users, n_items, k, h)
    for side, N in (("item", n_users), ("user", n_items)):
        S = -(-N // _lib.BIVAE_RANGE)
        by = 4 * N * k + 2 * 4 * S * bs * (k + 1)
        fl = 4 * bs * N * k
        print("%s, %s step's fused decode (B = %d against N = %d, S = %d ranges): %.2f MB = %.4f ms at 6.3 TB/s; %.3f Gflop = %.4f ms at "
              "157.3 Tflop/s; %.2f M exponentials" % (name, side, bs, N, S, by / 1e6, by / HBM * 1e3, fl / 1e9, fl / FP32 * 1e3, bs * N / 1e6),
              flush=True)
    if args.handle_only:
        dt, out = timed(lambda: model.fit_epoch(bs, 1e-3, 1.0, seed=1))
        ti, tu = model.last_timing()
        print("%s (k = %d, h = %d, batch %d): handle epoch %.3f s; item pass %.3f s = %.3f ms per step (%d steps), user pass %.3f s = %.3f ms "
              "per step (%d steps)" % (name, k, h, bs, dt, ti, ti / steps_i * 1e3, steps_i, tu, tu / steps_u * 1e3, steps_u), flush=True)
        model.close()
        continue
    enc_u, enc_i = TorchEncoder(n_items, k, h).to(dev), TorchEncoder(n_users, k, h).to(dev)
    opt_u, opt_i = torch.optim.Adam(enc_u.parameters(), lr=1e-3), torch.optim.Adam(enc_i.parameters(), lr=1e-3)
    theta, beta = torch.randn(n_users, k, device=dev) * 0.1, torch.randn(n_items, k, device=dev) * 0.01
    mu_theta, mu_beta = torch.zeros_like(theta), torch.zeros_like(beta)
    sides = {"item": (enc_i, opt_i, XT, beta, theta, mu_beta), "user": (enc_u, opt_u, X, theta, beta, mu_theta)}
    n_torch, done = {}, {}
    for side, a in sides.items():
        torch_steps(*a, bs, 0, 3, dev)
        torch.cuda.synchronize()
        t_probe, _ = timed(lambda: (torch_steps(*a, bs, 3, 3, dev), torch.cuda.synchronize()))
        n_torch[side] = max(3, min(steps_i if side == "item" else steps_u, int(args.window / (t_probe / 3)) + 1))
        done[side] = 6
    ours, ours_i, ours_u, theirs = [], [], [], {"item": [], "user": []}
    for _ in range(args.rounds):
        dt, (li, lu, _) = timed(lambda: model.fit_epoch(bs, 1e-3, 1.0, seed=1))
        ti, tu = model.last_timing()
        ours.append(dt)
        ours_i.append(ti / steps_i)
        ours_u.append(tu / steps_u)
        for side, a in sides.items():
            torch.cuda.synchronize()
            dt, _ = timed(lambda: (torch_steps(*a, bs, done[side], n_torch[side], dev), torch.cuda.synchronize()))
            theirs[side].append(dt / n_torch[side])
            done[side] += n_torch[side]
    model.close()
    epoch, t_i, t_u = float(np.mean(ours)), float(np.mean(theirs["item"])), float(np.mean(theirs["user"]))
    torch_epoch = t_i * steps_i + t_u * steps_u
    ms = lambda ts: ", ".join("%.3f ms" % (t * 1e3) for t in ts)   # noqa: E731
    print("%s (k = %d, h = %d, batch %d; %d item steps + %d user steps per epoch): handle epoch %.3f s (%s), item step %.3f ms (%s), user "
          "step %.3f ms (%s), last epoch's mean losses %.4g / %.4g; torch loop item step %.3f ms over %d steps per window (%s), user step "
          "%.3f ms over %d steps per window (%s) = epoch %.3f s; handle / torch = %.3f" % (
              name, k, h, bs, steps_i, steps_u, epoch, ", ".join("%.3f" % t for t in ours), np.mean(ours_i) * 1e3, ms(ours_i),
              np.mean(ours_u) * 1e3, ms(ours_u), li / steps_i, lu / steps_u, t_i * 1e3, n_torch["item"], ms(theirs["item"]), t_u * 1e3,
              n_torch["user"], ms(theirs["user"]), torch_epoch, epoch / torch_epoch), flush=True)
    del enc_u, enc_i, opt_u, opt_i, theta, beta, mu_theta, mu_beta, sides
    torch.cuda.empty_cache()
