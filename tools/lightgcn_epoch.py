#!/usr/bin/env python3
"""LightGCN times: a step and an epoch of the device handle (`_lib.LightGcnModel`) next to the reference's loop on the same
GPU, at the ML-100K shape and at the synthetic ML-20M shape (138 493 users x 26 744 items, 20 M entries) of
cornac_amd/synth.py, with emb_size 64, 3 layers and batches of 1 024 triplets.

The reference's tree and DGL are not needed: the comparison is a plain torch restatement of its loop written for this tool
(the normalised adjacency as one sparse tensor, `torch.sparse.mm` per hop, the mean over the layers, the batch's rows, softplus
and the squared norms, autograd, torch.optim.Adam; per step the batch's three arrays go to the device, then forward,
backward, step and `loss.item()`, as recom_lightgcn.py's loop does).  Both sides take the same pre-drawn triplets (uniform
negatives), so the reference's Python sampler is in neither; its time is reported separately: `Dataset.uij_iter`, the sampler
restated draw for draw, over a corner of the data, as seconds per epoch of the full shape at the measured time per triplet.

Method: both sides are warmed up first; then they alternate in this one process, --rounds times: --steps steps of the handle in
one `fit_epoch` call (host clock around the call, which ends in its one device synchronise) and enough torch steps to fill
about --window seconds (host clock, a device synchronise before and after).  An epoch's time is the step's times the epoch's
steps.  Then the hops alone: `propagate()` calls on the host clock (L hops and a download each; the download is timed on its
own with L = 0 and taken off), as gathered bytes per second = edges x emb_size x 4 B per hop, next to the 8.6 TB/s that
MI355X_MICROARCH.md gives for uniformly gathered rows of a 38 MB table in the Infinity Cache.  No time is a pass/fail condition.

    python tools/lightgcn_epoch.py
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
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--window", type=float, default=2.0)
ap.add_argument("--no-torch", action="store_true", help="the handle alone")
args = ap.parse_args()

from cornac_amd import Dataset, _lib, synth  # noqa: E402

D, L, BS, LR, LAM, GUIDE = 64, 3, 1024, 1e-3, 1e-4, 8.6e12


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


def torch_adjacency(X, dev):
    """[[0, R], [R^T, 0]] with (deg_u deg_i)^-1/2, as one sparse CSR tensor"""
    nu, ni = X.shape
    du, di = np.diff(X.indptr).astype(np.float32), np.bincount(X.indices, minlength=ni).astype(np.float32)
    w = np.power(du.repeat(np.diff(X.indptr)) * di[X.indices], -0.5).astype(np.float32)
    R = sp.csr_matrix((w, X.indices, X.indptr), shape=X.shape)
    A = sp.bmat([[None, R], [R.T, None]], format="csr")
    return torch.sparse_csr_tensor(torch.from_numpy(A.indptr.astype(np.int64)), torch.from_numpy(A.indices.astype(np.int64)),
                                   torch.from_numpy(A.data), size=A.shape).to(dev)


def torch_steps(A, E0, opt, nu, ptr, users, pos, neg, first, count, dev):
    n_steps = len(ptr) - 1
    for s in range(first, first + count):
        a, b = ptr[s % n_steps], ptr[s % n_steps + 1]
        u, i, j = (torch.from_numpy(x[a:b]).to(dev) for x in (users, pos, neg))
        h, total = E0, E0
        for _ in range(L):
            h = torch.sparse.mm(A, h)
            total = total + h
        E = total / (L + 1)
        ue, pe, ne = E[u], E[nu + i], E[nu + j]
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
    nnz = int(X.nnz)
    epoch_steps = -(-nnz // BS)
    table_mb = (n_users + n_items) * D * 4 / 1e6
    print("%s: %d users x %d items, %d entries, %d steps of %d triplets per epoch; both tables %.1f MB; longest row %d edges" % (
        shape, n_users, n_items, nnz, epoch_steps, BS, table_mb, max(int(np.diff(X.indptr).max()), int(np.bincount(X.indices).max()))), flush=True)

    # the reference's sampler, restated draw for draw, on a corner of the data
    cut = min(len(users), 1_000_000)
    corner = Dataset.from_arrays(users[:cut], items[:cut], ratings[:cut], num_users=n_users, num_items=n_items, seed=1)
    it = corner.uij_iter(BS, shuffle=True)
    next(it)
    n_batches = min(40, -(-cut // BS) - 2)
    dt, got = timed(lambda: sum(len(next(it)[0]) for _ in range(n_batches)))
    print("%s: the reference's sampler (uij_iter): %.2f us per triplet over %d triplets = %.1f s per epoch of this shape" % (
        shape, dt / got * 1e6, got, dt / got * nnz), flush=True)
    del corner, it

    rs = np.random.RandomState(1)
    K = min(args.steps, epoch_steps)
    order = rs.permutation(nnz)[:K * BS]
    coo_u = np.repeat(np.arange(n_users), np.diff(X.indptr))
    su, si, sj = coo_u[order].astype(np.int32), X.indices[order].astype(np.int32), rs.randint(0, n_items, len(order)).astype(np.int32)
    ptr = np.minimum(np.arange(K + 1, dtype=np.int64) * BS, len(order))
    bound = np.sqrt(6.0 / (n_users + D)), np.sqrt(6.0 / (n_items + D))
    user0 = rs.uniform(-bound[0], bound[0], (n_users, D)).astype(np.float32)
    item0 = rs.uniform(-bound[1], bound[1], (n_items, D)).astype(np.float32)

    model = _lib.LightGcnModel(X, D, L)
    model.set_params(user0, item0)
    model.fit_epoch(ptr[:4], su[:ptr[3]], si[:ptr[3]], sj[:ptr[3]], LR, LAM)   # warm-up
    have_torch = not args.no_torch
    if have_torch:
        try:
            A = torch_adjacency(X, dev)
            E0 = torch.nn.Parameter(torch.from_numpy(np.concatenate([user0, item0])).to(dev))
            opt = torch.optim.Adam([E0], lr=LR)
            su64, si64, sj64 = (x.astype(np.int64) for x in (su, si, sj))
            torch_steps(A, E0, opt, n_users, ptr, su64, si64, sj64, 0, 2, dev)
            torch.cuda.synchronize()
            t_probe, _ = timed(lambda: (torch_steps(A, E0, opt, n_users, ptr, su64, si64, sj64, 2, 3, dev), torch.cuda.synchronize()))
            n_torch, done = max(3, int(args.window / (t_probe / 3)) + 1), 5
        except Exception as e:   # a measurement aid: say so and time the handle alone
            print("%s: the torch loop does not run here (%s: %s)" % (shape, type(e).__name__, e), flush=True)
            have_torch = False
    ours, theirs = [], []
    for _ in range(args.rounds):
        dt, (losses, _, _) = timed(lambda: model.fit_epoch(ptr, su, si, sj, LR, LAM))
        ours.append(dt / K)
        if have_torch:
            torch.cuda.synchronize()
            dt, _ = timed(lambda: (torch_steps(A, E0, opt, n_users, ptr, su64, si64, sj64, done, n_torch, dev), torch.cuda.synchronize()))
            theirs.append(dt / n_torch)
            done += n_torch
    ms = lambda ts: ", ".join("%.3f ms" % (t * 1e3) for t in ts)   # noqa: E731
    step = float(np.mean(ours))
    line = "%s (emb_size %d, %d layers, batch %d): handle step %.3f ms over %d steps per call (%s), last call's mean loss %.4g = epoch %.2f s at %d steps" % (
        shape, D, L, BS, step * 1e3, K, ms(ours), float(losses.mean()), step * epoch_steps, epoch_steps)
    if have_torch:
        tstep = float(np.mean(theirs))
        line += "; torch loop step %.3f ms over %d steps per window (%s) = epoch %.2f s; handle / torch = %.3f" % (
            tstep * 1e3, n_torch, ms(theirs), tstep * epoch_steps, step / tstep)
        del A, E0, opt
        torch.cuda.empty_cache()
    print(line, flush=True)

    # the hops alone
    flat = _lib.LightGcnModel(X, D, 0)
    flat.set_params(user0, item0)
    flat.propagate()
    model.propagate()
    reps = 5
    t_copy = min(timed(flat.propagate)[0] for _ in range(reps))
    t_prop = min(timed(model.propagate)[0] for _ in range(reps))
    hop = max(t_prop - t_copy, 1e-9) / L
    gathered = 2 * nnz * D * 4
    print("%s: propagate %.3f ms, its download alone %.3f ms: a hop %.3f ms gathers %.1f MB = %.2f TB/s (MI355X_MICROARCH.md: %.1f TB/s for "
          "uniformly gathered rows of a 38 MB table; these tables: %.1f MB); %d hops per step = %.3f ms of the step's %.3f ms" % (
              shape, t_prop * 1e3, t_copy * 1e3, hop * 1e3, gathered / 1e6, gathered / hop / 1e12, GUIDE / 1e12, table_mb, 2 * L, 2 * L * hop * 1e3,
              step * 1e3), flush=True)
    flat.close()
    model.close()
