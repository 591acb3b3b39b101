#!/usr/bin/env python3
"""KNN times: the similarity table and one scoring batch, at the ML-100K shape (both models) and at ML-20M's item side
(ItemKNN: 26 744 items over 138 493 users), on cornac_amd/synth.py's interaction sets with ratings 1..5.

Prints the box's device_probe line first, then per shape and model: the host preparation (mean centring, NumPy), the
similarity on the device including the copy of the table back to the host (entries, and products per second of the
row-by-row product: the sum over the rows' entries of the length of the entry's column), then score_batch for --users
users at k = --k (items x users outputs per second).  Both are host-clock times around calls that end in a device
synchronise: the first similarity run on its own, then the mean and the range of --repeats runs after a warm-up.  --every N keeps every N-th rating; --rows-per-pass forces the
pass size (0: chosen from the free device memory).  --check compares the table and the scores of the first --check-n
users' worth of ratings with the float64 restatement of the reference's loops (tests/knn_cases.py): the table bit for
bit, the scores within the restatement's derived bound.  No time is a pass/fail condition, and the reference's own
loops are not timed here.

    python tools/knn_epoch.py --check
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
ap.add_argument("--shapes", default="ml100k:user,ml100k:item,ml20m:item")
ap.add_argument("--k", type=int, default=50)
ap.add_argument("--users", type=int, default=64)
ap.add_argument("--every", type=int, default=1)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--rows-per-pass", type=int, default=0)
ap.add_argument("--check", action="store_true")
ap.add_argument("--check-n", type=int, default=120)
args = ap.parse_args()

from cornac_amd import Dataset, ItemKNN, UserKNN, _lib, synth  # noqa: E402

print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
for spec in args.shapes.split(","):
    shape, model = spec.split(":")
    n_users, n_items, users, items, ratings = synth.make(shape)
    users, items, ratings = users[::args.every], items[::args.every], ratings[::args.every]
    ds = Dataset.from_arrays(users, items, ratings, num_users=n_users, num_items=n_items)
    cls = UserKNN if model == "user" else ItemKNN
    m = cls(k=args.k, similarity="cosine", mean_centered=True, verbose=False)
    m._similarity = lambda W: W   # (first the host preparation alone: fit() then holds the weight matrix)
    t0 = time.perf_counter()
    m.fit(ds)
    prep = time.perf_counter() - t0
    W = m.sim_mat.tocsr()
    col_len = np.diff(W.T.tocsr().indptr)
    products = int(col_len[W.indices].sum())
    sim = _lib.KnnSimilarity(W)
    t0 = time.perf_counter()
    table = sim.run(args.rows_per_pass)   # (the first run loads the code objects: reported on its own)
    first = time.perf_counter() - t0
    t_sim = []
    for _ in range(args.repeats):
        del table
        t0 = time.perf_counter()
        table = sim.run(args.rows_per_pass)
        t_sim.append(time.perf_counter() - t0)
    sim.close()
    m.sim_mat = table
    m.invalidate_scorer()
    batch = np.arange(min(args.users, n_users))
    m.score_batch(batch)   # (builds the scorer, its tables go to the device once; warms the kernel up at this shape)
    t_score = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        scores = m.score_batch(batch)
        t_score.append(time.perf_counter() - t0)
    dt_sim, dt_score = float(np.mean(t_sim)), float(np.mean(t_score))
    line = ("%-7s %-4s %9d ratings: preparation %.2f s; similarity %d x %d, %d entries (%.1f %% dense): first run %.3f s, then "
            "%.4f s (%.4f .. %.4f over %d runs) = %.2f G products/s, the copy of the table to the host included; score_batch of %d "
            "users at k = %d: %.4f s (%.4f .. %.4f) = %.1f M outputs/s (finite %s)") % (
        shape, model, len(ratings), prep, table.shape[0], table.shape[1], table.nnz,
        100.0 * table.nnz / (table.shape[0] * table.shape[1]), first, dt_sim, min(t_sim), max(t_sim), args.repeats,
        products / dt_sim / 1e9, len(batch), args.k, dt_score, min(t_score), max(t_score), scores.size / dt_score / 1e6,
        bool(np.isfinite(scores).all()))
    if args.check:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import knn_cases as kc

        keep = users < args.check_n
        X = sp.csr_matrix((ratings[keep], (users[keep], items[keep])), shape=(args.check_n, n_items))
        X = X[:, np.unique(X.indices)].tocsr()   # (the items these users rated)
        Wc, mean, rat = kc.prepare(X, model, similarity="cosine", mean_centered_=True)
        sim = _lib.KnnSimilarity(Wc)
        got = sim.run(7)
        sim.close()
        want = kc.similarity(Wc)
        N, Q, user_mode = kc.tables(model, want, rat)
        sc = _lib.KnnScorer(N, Q, user_mode)
        dev = sc.score_users(np.arange(8), args.k)
        sc.close()
        ref = np.array([kc.score_row(N, Q, u, user_mode, args.k) for u in range(8)])
        line += " | first %d users: table equal to the restatement bit for bit: %s; scores differ by %.3g (bound %.3g)" % (
            args.check_n, kc.same_csr(got, want), np.abs(dev - ref).max(), kc.score_tolerance(args.k, 5.0, 0.0))
    print(line, flush=True)
