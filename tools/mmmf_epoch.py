#!/usr/bin/env python3
"""MMMF hogwild epoch times at the ML-20M shape (cornac_amd/synth.py CONFIGS["ml20m"]) beside BPR's unowned fused epoch on
the same data, tables and k, in one process.

Per k (default 10 and 64), on one handle:
  (a) start tables (BPR's _init rule): --reps rounds, each one BPR epoch (hogwild_enqueue, FORM_FUSED | HOG_NO_OWNERSHIP)
      and one MMMF epoch (mmmf_hogwild_enqueue), alternating, after one warm-up round;
  train --train-epochs MMMF epochs at --lr / --reg;
  (b) the same rounds on the trained tables.
The timed epochs run at lr = 0, so the tables stay what they were and every repetition does the same work: a violator
still issues all its atomics (of 0.0), a correct triplet none, BPR all of them.  Two clocks per epoch: the handle's HIP
events around the SGD kernel (kernel_timing) and a host clock from the enqueue to the end of sync() (which adds the bias
pad / unpad passes and the counter fetch).  Printed: median and min..max of each, and the `correct` share of the MMMF
epochs' non-skipped samples.  No time is a pass/fail condition.

    python tools/mmmf_epoch.py --ks 10,64
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="ml20m")
ap.add_argument("--scale", type=float, default=1.0)
ap.add_argument("--ks", default="10,64")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--train-epochs", type=int, default=20)
ap.add_argument("--lr", type=float, default=0.05)
ap.add_argument("--reg", type=float, default=0.01)
args = ap.parse_args()

from cornac_amd import _lib, synth  # noqa: E402

print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
n_users, n_items, users, items, _ = synth.make(args.shape, args.scale)
indptr, indices = synth.csr_from_sorted(users, items, n_users)
nnz = len(indices)
BPR_FLAGS = _lib.FORM_FUSED | _lib.HOG_NO_OWNERSHIP


def summary(xs):
    return "%.3f ms (%.3f .. %.3f)" % (float(np.median(xs)), min(xs), max(xs))


def timed(tr, enqueue):
    """one epoch: (kernel ms by HIP events, wall ms enqueue -> sync, correct, skipped)"""
    tr.kernel_timing(True)
    t0 = time.perf_counter()
    enqueue()
    correct, skipped = tr.sync()
    wall = (time.perf_counter() - t0) * 1e3
    ms, _ = tr.kernel_timing(False)
    return ms, wall, correct, skipped


def rounds(tr, label, k):
    bpr = lambda: tr.hogwild_enqueue(nnz, 0.0, 0.0, True, _lib.NEG_UNIFORM, BPR_FLAGS)  # noqa: E731
    mmmf = lambda: tr.mmmf_hogwild_enqueue(nnz, 0.0, 0.0)  # noqa: E731
    res = {"bpr": [], "mmmf": []}
    for r in range(args.reps + 1):
        for name, fn in (("bpr", bpr), ("mmmf", mmmf)):
            out = timed(tr, fn)
            if r:  # (round 0 warms up: code objects, the padded bias table)
                res[name].append(out)
    share = np.mean([c / max(1, nnz - s) for _, _, c, s in res["mmmf"]])
    for name in ("mmmf", "bpr"):
        print("%s k=%-3d %-14s %-5s kernel %s, epoch %s = %.0f M samples/s%s" % (
            args.shape, k, label, name.upper(), summary([x[0] for x in res[name]]), summary([x[1] for x in res[name]]),
            nnz / np.median([x[1] for x in res[name]]) / 1e3, ", correct share %.3f" % share if name == "mmmf" else ""), flush=True)


for k in (int(x) for x in args.ks.split(",")):
    rs = np.random.RandomState(11)
    U0 = ((rs.uniform(0, 1, (n_users, k)).astype(np.float32) - 0.5) / k)
    V0 = ((rs.uniform(0, 1, (n_items, k)).astype(np.float32) - 0.5) / k)
    tr = _lib.BprTrainer(indptr, indices, n_users, n_items, n_users, n_items, k)
    try:
        tr.set_factors(U0, V0, np.zeros(n_items, np.float32))
        tr.seed_hogwild(2024)
        rounds(tr, "start tables", k)
        t0 = time.perf_counter()
        correct, skipped = tr.mmmf_fit_epochs(args.train_epochs, args.lr, args.reg, _lib.MODE_HOGWILD)
        print("%s k=%-3d trained %d MMMF epochs (lr %g, reg %g) in %.2f s: correct share %.3f over them" % (
            args.shape, k, args.train_epochs, args.lr, args.reg, time.perf_counter() - t0,
            correct / max(1, args.train_epochs * nnz - skipped)), flush=True)
        rounds(tr, "trained tables", k)
    finally:
        tr.close()
