#!/usr/bin/env python3
"""EASE times: the fit (Gram matrix, inverse, weights, each stage on its own, then `EASE.fit` as a whole) and one scoring
batch, at a synthetic shape with ML-20M's item side (138 493 users x 26 744 items, 20 M entries, ratings 1..5) from
cornac_amd/synth.py.  --shape ml100k runs the small shape.

Prints the box's device_probe line first, then: the handle's creation (X to the device, its CSC built on the host, the
5.7 GB table allocated and zeroed), the three stages through the ABI (host-clock times around calls that end in a device
synchronise; the inverse as 2 n^3 flops per second), the copy of B to the host, `EASE.fit` as a whole, and score_batch for
--users users (mean and range of --repeats calls after a warm-up; the copy of the scores to the host included).  --every N
keeps every N-th rating.  --check compares, on the first --check-n users' ratings, the device's Gram matrix and scores with
the float64 restatement (tests/ease_cases.py) bit for bit and its weights with NumPy's formula.  No time is a pass/fail
condition, and the reference's own NumPy/SciPy path is not timed here.

    python tools/ease_epoch.py --check
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="ml20m")
ap.add_argument("--lamb", type=float, default=500.0)
ap.add_argument("--users", type=int, default=256)
ap.add_argument("--every", type=int, default=1)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--check", action="store_true")
ap.add_argument("--check-n", type=int, default=120)
args = ap.parse_args()

from cornac_amd import EASE, Dataset, _lib, synth  # noqa: E402


def timed(f):
    t0 = time.perf_counter()
    out = f()
    return time.perf_counter() - t0, out


print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
n_users, n_items, users, items, ratings = synth.make(args.shape)
users, items, ratings = users[::args.every], items[::args.every], ratings[::args.every]
ds = Dataset.from_arrays(users, items, ratings, num_users=n_users, num_items=n_items)
X = ds.matrix
print("%s: %d users x %d items, %d ratings; table %d x %d float64 = %.2f GB" % (
    args.shape, n_users, n_items, X.nnz, n_items, n_items, n_items * n_items * 8 / 1e9), flush=True)

t_create, model = timed(lambda: _lib.EaseModel(X))
t_gram, _ = timed(model.gram)
t_inv, _ = timed(lambda: model.invert(args.lamb))
t_w, _ = timed(lambda: model.weights(True))
t_copy, B = timed(model.get_table)
model.close()
print("stages: create %.3f s; gram %.3f s; invert %.3f s = %.2f Tflop/s (2 n^3); weights %.3f s; B to the host %.3f s (finite %s, "
      "%.1f %% of its entries > 0)" % (t_create, t_gram, t_inv, 2.0 * n_items ** 3 / t_inv / 1e12, t_w, t_copy,
                                        bool(np.isfinite(B).all()), 100.0 * float((B > 0).mean())), flush=True)
del B

m = EASE(lamb=args.lamb, verbose=False)
t_fit, _ = timed(lambda: m.fit(ds))
batch = np.arange(min(args.users, n_users))
m.score_batch(batch)   # (warms the kernel up at this shape)
t_score = []
for _ in range(args.repeats):
    dt, scores = timed(lambda: m.score_batch(batch))
    t_score.append(dt)
print("EASE.fit as a whole (handle, fit, B to the host): %.3f s; score_batch of %d users: %.4f s (%.4f .. %.4f over %d calls) = "
      "%.1f M outputs/s (finite %s)" % (t_fit, len(batch), float(np.mean(t_score)), min(t_score), max(t_score), args.repeats,
                                        scores.size / float(np.mean(t_score)) / 1e6, bool(np.isfinite(scores).all())), flush=True)

if args.check:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ease_cases as ec

    keep = users < args.check_n
    Xc = sp.csr_matrix((ratings[keep], (users[keep], items[keep])), shape=(args.check_n, n_items))
    Xc = Xc[:, np.unique(Xc.indices)[:300]].tocsr()   # (at most 300 of the items these users rated)
    Xc.sort_indices()
    dev = _lib.EaseModel(Xc)
    dev.gram()
    G = dev.get_table()
    dev.fit(args.lamb, True)
    Bd = dev.get_table()
    sd = dev.score_users(np.arange(8))
    dev.close()
    want = ec.numpy_formula(Xc, args.lamb, True)
    print("first %d users, %d items: Gram matrix equal to the restatement bit for bit: %s; B differs from NumPy's formula by %.3g "
          "(CEILING %.3g); scores equal to the restatement bit for bit: %s" % (
              args.check_n, Xc.shape[1], ec.same_bits(G, ec.gram(Xc)), np.abs(Bd - want).max(),
              ec.ceiling(ec.gram(Xc), args.lamb, want), ec.same_bits(sd, np.array([ec.score_user(Xc, Bd, u) for u in range(8)]))),
          flush=True)
