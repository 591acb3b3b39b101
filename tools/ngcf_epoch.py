#!/usr/bin/env python3
"""NGCF times: a step and an epoch of the device handle (`_lib.NgcfModel`) next to the reference's loop on the same GPU, at
the ML-100K shape and at the synthetic ML-20M shape of cornac_amd/synth.py, with the defaults (emb_size 64, layers
[64, 64, 64], dropout 0.1 each, batches of 1 024 triplets).

The reference's tree and DGL are not needed: the comparison is a plain torch restatement of its loop IN ITS OWN PER-EDGE FORM,
written for this tool: per layer and edge type a gather of both end points' rows, two `nn.Linear`s per edge, the edge norm, an
`index_add_` into the destinations, the self loop's Linear per node, LeakyReLU, dropout, F.normalize; then the concatenation,
the batch's rows, softplus and the squared norms, autograd and torch.optim.Adam over every parameter; per step the batch's
arrays go to the device and `loss.item()` comes back, as recom_ngcf.py's loop does.  Both sides take the same pre-drawn
triplets.  At the ML-20M shape that form holds several edge tensors of 20 M x 64 floats per layer for autograd; where it does
not fit (or does not run) the tool says so and the baseline of that shape is "not measured".

Method: both sides are warmed up first; then they alternate in this one process, --rounds times: --steps steps of the handle in
one `fit_epoch` call (host clock around the call, which ends in its one device synchronise) and --torch-steps torch steps (host
clock, a device synchronise before and after).  An epoch's time is the step's times the epoch's steps.  Then the forward pass
alone: `propagate()` on the host clock.  No time is a pass/fail condition.

    python tools/ngcf_epoch.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="ml100k,ml20m")
ap.add_argument("--rounds", type=int, default=2)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--torch-steps", type=int, default=3)
ap.add_argument("--no-torch", action="store_true", help="the handle alone")
args = ap.parse_args()

from cornac_amd import _lib, synth  # noqa: E402

D, LAYERS, DROP, BS, LR, LAM = 64, [64, 64, 64], [0.1, 0.1, 0.1], 1024, 1e-3, 1e-4


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


class EdgeForm(torch.nn.Module):
    """the reference's layer stack per edge, over one edge list in each direction"""

    def __init__(self, X, params, dev):
        super().__init__()
        nu, ni = X.shape
        coo = X.tocoo()
        du, di = np.diff(X.indptr).astype(np.float32), np.bincount(X.indices, minlength=ni).astype(np.float32)
        self.nu, self.ni = nu, ni
        self.u = torch.from_numpy(coo.row.astype(np.int64)).to(dev)
        self.i = torch.from_numpy(coo.col.astype(np.int64)).to(dev)
        self.norm = torch.from_numpy(np.power(du[coo.row] * di[coo.col], -0.5).astype(np.float32)).to(dev).unsqueeze(1)
        self.W1, self.W2 = torch.nn.ModuleList(), torch.nn.ModuleList()
        din = D
        for l, dout in enumerate(LAYERS):
            for mods, n in ((self.W1, "W1"), (self.W2, "W2")):
                lin = torch.nn.Linear(din, dout)
                with torch.no_grad():
                    lin.weight.copy_(torch.from_numpy(params["layers.%d.%s.weight" % (l, n)]))
                    lin.bias.copy_(torch.from_numpy(params["layers.%d.%s.bias" % (l, n)]))
                mods.append(lin)
            din = dout
        self.user = torch.nn.Parameter(torch.from_numpy(params["feature_dict.user"]))
        self.item = torch.nn.Parameter(torch.from_numpy(params["feature_dict.item"]))

    def forward(self):
        F = torch.nn.functional
        hu, hi, us, its = self.user, self.item, [self.user], [self.item]
        for l in range(len(LAYERS)):
            W1, W2 = self.W1[l], self.W2[l]
            to_i = self.norm * (W1(hu[self.u]) + W2(hu[self.u] * hi[self.i]))   # user_item edges
            to_u = self.norm * (W1(hi[self.i]) + W2(hi[self.i] * hu[self.u]))   # item_user edges
            nu_ = W1(hu).index_add(0, self.u, to_u)
            ni_ = W1(hi).index_add(0, self.i, to_i)
            hu = F.normalize(F.dropout(F.leaky_relu(nu_, 0.2), DROP[l], self.training), dim=1, p=2)
            hi = F.normalize(F.dropout(F.leaky_relu(ni_, 0.2), DROP[l], self.training), dim=1, p=2)
            us.append(hu)
            its.append(hi)
        return torch.cat(us, 1), torch.cat(its, 1)


def torch_steps(net, opt, ptr, users, pos, neg, first, count, dev):
    n_steps = len(ptr) - 1
    for s in range(first, first + count):
        a, b = ptr[s % n_steps], ptr[s % n_steps + 1]
        u, i, j = (torch.from_numpy(x[a:b]).to(dev) for x in (users, pos, neg))
        U, V = net()
        ue, pe, ne = U[u], V[i], V[j]
        bpr = torch.nn.functional.softplus((ue * ne).sum(1) - (ue * pe).sum(1)).mean()
        reg = 0.5 * (torch.norm(ue) ** 2 + torch.norm(pe) ** 2 + torch.norm(ne) ** 2) / len(u)
        loss = bpr + LAM * reg
        opt.zero_grad()
        loss.backward()
        opt.step()
        loss.cpu().item()


print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
dev = torch.device("cuda:0")
for shape in args.shapes.split(","):
    n_users, n_items, users, items, ratings = synth.make(shape)
    X = sp.csr_matrix((np.ones(len(users), np.float32), (users, items)), shape=(n_users, n_items))
    X.sum_duplicates()
    X.sort_indices()
    nnz, N = int(X.nnz), n_users + n_items
    epoch_steps = -(-nnz // BS)
    print("%s: %d users x %d items, %d entries, %d steps of %d triplets per epoch" % (shape, n_users, n_items, nnz, epoch_steps, BS), flush=True)
    rs = np.random.RandomState(1)
    K = min(args.steps, epoch_steps)
    order = rs.permutation(nnz)[:K * BS]
    coo_u = np.repeat(np.arange(n_users), np.diff(X.indptr))
    su, si, sj = coo_u[order].astype(np.int32), X.indices[order].astype(np.int32), rs.randint(0, n_items, len(order)).astype(np.int32)
    ptr = np.minimum(np.arange(K + 1, dtype=np.int64) * BS, len(order))
    params = {}
    for n, s in _lib.NgcfModel.param_shapes(n_users, n_items, D, LAYERS).items():
        params[n] = np.zeros(s, np.float32) if len(s) == 1 else (rs.uniform(-1, 1, s) * np.sqrt(6.0 / (s[0] + s[1]))).astype(np.float32)

    model = _lib.NgcfModel(X, D, LAYERS, DROP, dropout_key=1)
    model.set_params(params)
    model.fit_epoch(ptr[:3], su[:ptr[2]], si[:ptr[2]], sj[:ptr[2]], LR, LAM)   # warm-up
    have_torch = not args.no_torch
    if have_torch:
        try:
            net = EdgeForm(X, params, dev).to(dev)
            opt = torch.optim.Adam(net.parameters(), lr=LR)
            su64, si64, sj64 = (x.astype(np.int64) for x in (su, si, sj))
            torch_steps(net, opt, ptr, su64, si64, sj64, 0, 1, dev)
            torch.cuda.synchronize()
        except Exception as e:   # a measurement aid: say so and time the handle alone
            print("%s: the per-edge torch loop does not run here (%s: %s): baseline not measured" % (shape, type(e).__name__, str(e)[:200]), flush=True)
            have_torch = False
            net = opt = None
            torch.cuda.empty_cache()
    ours, theirs, done = [], [], 1
    for _ in range(args.rounds):
        dt, (losses, _, _) = timed(lambda: model.fit_epoch(ptr, su, si, sj, LR, LAM))
        ours.append(dt / K)
        if have_torch:
            torch.cuda.synchronize()
            dt, _ = timed(lambda: (torch_steps(net, opt, ptr, su64, si64, sj64, done, args.torch_steps, dev), torch.cuda.synchronize()))
            theirs.append(dt / args.torch_steps)
            done += args.torch_steps
    ms = lambda ts: ", ".join("%.3f ms" % (t * 1e3) for t in ts)   # noqa: E731
    step = float(np.mean(ours))
    line = "%s (emb_size %d, layers %r, batch %d): handle step %.3f ms over %d steps per call (%s), last call's mean loss %.4g = epoch %.2f s at %d steps" % (
        shape, D, LAYERS, BS, step * 1e3, K, ms(ours), float(losses.mean()), step * epoch_steps, epoch_steps)
    if have_torch:
        tstep = float(np.mean(theirs))
        line += "; per-edge torch loop step %.3f ms over %d steps per window (%s) = epoch %.2f s; handle / torch = %.4f" % (
            tstep * 1e3, args.torch_steps, ms(theirs), tstep * epoch_steps, step / tstep)
        del net, opt
        torch.cuda.empty_cache()
    else:
        line += "; per-edge torch loop: not measured"
    print(line, flush=True)
    model.propagate()
    t_prop = min(timed(model.propagate)[0] for _ in range(3))
    # the dense part's traffic per step, counted from the buffers it reads and writes (floats per node, d = 64 throughout):
    # forward per layer: P1, P2 read, Z, Y, E slice written (5 d); backward: gz (Y, Z, GE, gin read, GZ written: 5 d),
    # weight gradients (GZ, P1, P2 read: 3 d), back (GZ, X, S read, T, R written: 5 d); Adam over the tables (g, w, m, v: 7 d / L)
    dense_bytes = N * 4 * (18 * D * len(LAYERS) + 7 * D)
    print("%s: propagate (forward, eval mode, with its download) %.3f ms; dense part's traffic %.1f MB per step = %.3f ms at 4 TB/s" % (
        shape, t_prop * 1e3, dense_bytes / 1e6, dense_bytes / 4e12 * 1e3), flush=True)
    model.close()
