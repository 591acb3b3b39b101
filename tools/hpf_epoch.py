#!/usr/bin/env python3
"""HPF iteration times at the ML-20M shape (cornac_amd/synth.py CONFIGS, ratings of bench.synth_ratings, stored by user as
HPF needs them): k = 5, 16 and 64, hierarchical and plain PF.

Prints the box's device_probe line first, then one line per configuration: the first fit (plans + first iteration), the
mean of --iters further iterations, the form taken (hpf_form) and the fraction of the memory roofline by ALGORITHMIC bytes
of one iteration: per rating 4 B index + 4 B rating on each side and 4 B of the item side's permutation; per table element
8 B times 13 (the expected-log step reads four tables and writes two, the two sum passes read their own expected-log row
and write the shape, the column sums read shape and rate, the rate step reads the shape, writes the rate and reads it back
for the row sum) — against --peak-gbs (the MI355X's 8 TB/s HBM3E by default).  The gathered rows of the other side's
expected-log table are not counted: they are meant to come from the L2.  --every N keeps every N-th rating; --check
compares 1 iteration on the first --check-n ratings with the float64 restatement of the reference's loop
(tests/hpf_cases.py; at this shape a column sum has 138 493 terms, which the restatement adds one after the other like the
reference, so the two orders differ by about sqrt(n) 2^-53 ~ 1e-13, more than on the tests' small shapes).  With the
profiling build (CORNAC_HIP_PROFILE=1) CORNAC_HIP_HPF_STORE_DK=1 switches the item pass from computing dk again to reading
what the user pass stored.  No time is a pass/fail condition.

    python tools/hpf_epoch.py --check
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
ap.add_argument("--shapes", default="ml20m")
ap.add_argument("--ks", default="5,16,64")
ap.add_argument("--variants", default="hier,pf")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--every", type=int, default=1)
ap.add_argument("--peak-gbs", type=float, default=8000.0)
ap.add_argument("--check", action="store_true")
ap.add_argument("--check-n", type=int, default=20000)
args = ap.parse_args()

from bench import synth_ratings  # noqa: E402
from cornac_amd import _lib, synth  # noqa: E402

print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
for shape in args.shapes.split(","):
    n_users, n_items, nnz, zipf_a, seed = synth.CONFIGS[shape]
    rid, cid, val = synth_ratings(n_users, n_items, nnz, zipf_a, seed)
    order = np.argsort(rid, kind="stable")[::args.every]
    rid, cid, val = (np.ascontiguousarray(x[order]) for x in (rid, cid, np.asarray(val, np.float32)))
    for k in (int(x) for x in args.ks.split(",")):
        gbytes = (20 * len(val) + 13 * 8 * (n_users + n_items) * k) / 1e9
        for variant in args.variants.split(","):
            hier = variant == "hier"
            rs = np.random.RandomState(11)
            shp, scale = (100., 0.003) if hier else (0.3, 1 / 0.3)
            tables = [rs.gamma(shp, scale, (rows, k)).astype(np.float32).astype(np.float64)
                      for rows in (n_users, n_users, n_items, n_items)]
            tr = _lib.MfTrainer(rid, cid, val, n_users, n_items, k)
            tr.hpf_set_tables(*tables)
            t0 = time.perf_counter()
            tr.hpf_fit(1, hier)
            first = time.perf_counter() - t0
            t0 = time.perf_counter()
            tr.hpf_fit(args.iters, hier)
            dt = (time.perf_counter() - t0) / max(args.iters, 1)
            group, split = tr.hpf_form()
            Gs = tr.hpf_get_tables()[0]
            tr.close()
            line = ("%-8s k=%-3d %-4s %10d ratings: first fit %.2f s, iteration %.4f s = %.0f M ratings/s, %.2f GB -> %.1f %% of "
                    "%.0f GB/s (group %d, %d rows split; G_s finite %s, mean %.4g)") % (
                shape, k, variant, len(val), first, dt, len(val) / dt / 1e6, gbytes, 100.0 * gbytes / dt / args.peak_gbs,
                args.peak_gbs, group, split, bool(np.isfinite(Gs).all()), Gs.mean())
            if args.check:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import hpf_cases as hc

                n = min(args.check_n, len(val))
                r_, c_, v_ = rid[:n], cid[:n], val[:n]
                tr = _lib.MfTrainer(r_, c_, v_, n_users, n_items, k)
                tr.hpf_set_tables(*tables)
                tr.hpf_fit(1, hier)
                got = tr.hpf_get_tables()
                tr.close()
                want = hc.hpf_fit(r_, c_, v_, *tables, 1, hier)
                line += " | first %d ratings, 1 iteration vs the restatement: max relative difference %.3g" % (
                    n, hc.max_rel_diff(got, want))
            print(line, flush=True)
