#!/usr/bin/env python3
"""PMF epoch times at the ML-20M and Netflix Prize shapes (cornac_amd/synth.py CONFIGS, ratings of bench.synth_ratings):
k = 10 and 128, stored sorted by user and sorted by item, several ratings per wave pass (k <= 32) and one per wave.

The one-per-wave form of a small k is a switch of the profile build only (CORNAC_HIP_PMF_ONE_PER_WAVE; make -C
cornac_amd/csrc PROFILE=1, CORNAC_HIP_PROFILE=1): the tool starts itself once per form as a fresh child process.
Prints the box's device_probe line first, then one line per configuration: the first fit (schedule + first epoch) and
the mean of --epochs further epochs.  --every N keeps every N-th rating; --check compares 1 epoch of the first
--check-n ratings with the restatement of the reference's loop (tests/pmf_cases.py).

    CORNAC_HIP_PROFILE=1 python tools/pmf_epoch.py --shapes ml20m,netflix
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="ml20m,netflix")
ap.add_argument("--ks", default="10,128")
ap.add_argument("--orders", default="by_user,by_item")
ap.add_argument("--forms", default="grouped,one_per_wave")
ap.add_argument("--variant", default="non_linear")
ap.add_argument("--epochs", type=int, default=2)
ap.add_argument("--every", type=int, default=1)
ap.add_argument("--check", action="store_true")
ap.add_argument("--check-n", type=int, default=20000)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

if args.child is None:
    # parent: the probe line, then one child per form (the switch is read from the environment when the library loads)
    from cornac_amd import _lib

    print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
    for form in args.forms.split(","):
        env = dict(os.environ)
        if form == "one_per_wave":
            if not _lib.PROFILE:
                print("one_per_wave: needs the profile build (CORNAC_HIP_PROFILE=1) — skipped", flush=True)
                continue
            env["CORNAC_HIP_PMF_ONE_PER_WAVE"] = "1"
        rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", form] + sys.argv[1:], env=env)
        if rc != 0:
            sys.exit(rc)
    sys.exit(0)

from bench import synth_ratings  # noqa: E402
from cornac_amd import _lib, synth  # noqa: E402

lr, reg, gamma = 0.001, 0.001, 0.9
for shape in args.shapes.split(","):
    n_users, n_items, nnz, zipf_a, seed = synth.CONFIGS[shape]
    rid, cid, val = synth_ratings(n_users, n_items, nnz, zipf_a, seed)
    val = np.asarray(val, np.float32)
    if args.variant == "non_linear":
        val = ((val - np.float32(1.0)) / np.float32(4.0)).astype(np.float32)
    for k in (int(x) for x in args.ks.split(",")):
        if args.child == "one_per_wave" and k > 32:
            continue   # one rating per wave is the only form there: timed under "grouped"
        rs = np.random.RandomState(11)
        U0, V0 = rs.normal(0, 0.001, (n_users, k)), rs.normal(0, 0.001, (n_items, k))
        for name in args.orders.split(","):
            order = np.arange(nnz) if name == "by_user" else np.argsort(cid, kind="stable")
            order = order[::args.every]
            r_, c_, v_ = (np.ascontiguousarray(x[order]) for x in (rid, cid, val))
            tr = _lib.MfTrainer(r_, c_, v_, n_users, n_items, k)
            tr.pmf_set_factors(U0, V0)
            t0 = time.perf_counter()
            tr.pmf_fit(1, lr, reg, gamma, args.variant)
            first = time.perf_counter() - t0
            t0 = time.perf_counter()
            loss = tr.pmf_fit(args.epochs, lr, reg, gamma, args.variant)
            dt = (time.perf_counter() - t0) / max(args.epochs, 1)
            form, group = tr.pmf_form()
            tr.close()
            line = "%-8s k=%-3d %-8s %-12s %10d ratings: first fit %.2f s, epoch %.3f s = %.1f M ratings/s (form %d, %d per pass, loss %.6g)" % (
                shape, k, name, args.child, len(v_), first, dt, len(v_) / dt / 1e6, form, group, loss[-1])
            if args.check:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import pmf_cases as pc

                n = min(args.check_n, len(v_))
                tr = _lib.MfTrainer(r_[:n], c_[:n], v_[:n], n_users, n_items, k)
                tr.pmf_set_factors(U0, V0)
                tr.pmf_fit(1, lr, reg, gamma, args.variant)
                Ud, Vd = tr.pmf_get_factors()
                tr.close()
                Ur, Vr, _, _ = pc.pmf_fit(r_[:n], c_[:n], v_[:n], U0, V0, 1, reg, lr, gamma, args.variant)
                line += " | first %d ratings vs the restatement: bit-equal %s" % (n, pc.bits_equal(Ud, Ur) and pc.bits_equal(Vd, Vr))
            print(line, flush=True)
