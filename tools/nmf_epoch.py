#!/usr/bin/env python3
"""NMF epoch times at the ML-20M and Netflix Prize shapes (cornac_amd/synth.py CONFIGS, ratings of bench.synth_ratings,
stored by user as NMF needs them): k = 15 and 128, both modes, with and without biases.

Prints the box's device_probe line first, then one line per configuration: the first fit (plans + first epoch), the
mean of --epochs further epochs, the forms taken (nmf_form) and the fraction of the memory roofline by ALGORITHMIC bytes:
per rating and pass (user side, item side) 4 B index + 4 B rating + 4 B r_pred, plus one read and one write of each of
the two tables and four accumulators — against --peak-gbs (the MI355X's 8 TB/s HBM3E by default).  The gathered rows of
the other side's table are not counted: they are meant to come from the L2.  --every N keeps every N-th rating; --check
compares 1 epoch on the first --check-n ratings with the restatement of the reference's loop (tests/nmf_cases.py): bits
in deterministic mode, the free-order bound otherwise.  No time is a pass/fail condition.

    python tools/nmf_epoch.py --shapes ml20m,netflix --check
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
ap.add_argument("--shapes", default="ml20m,netflix")
ap.add_argument("--ks", default="15,128")
ap.add_argument("--modes", default="deterministic,hogwild")
ap.add_argument("--bias", default="0,1")
ap.add_argument("--epochs", type=int, default=3)
ap.add_argument("--every", type=int, default=1)
ap.add_argument("--peak-gbs", type=float, default=8000.0)
ap.add_argument("--check", action="store_true")
ap.add_argument("--check-n", type=int, default=20000)
args = ap.parse_args()

from bench import synth_ratings  # noqa: E402
from cornac_amd import _lib, synth  # noqa: E402

print("device_probe: " + json.dumps(dict(_lib.device_probe(0, 2 << 30), **_lib.device_info(0))), flush=True)
MODES = {"deterministic": _lib.MODE_DETERMINISTIC, "hogwild": _lib.MODE_HOGWILD}
hyper = (0.005, 0.06, 0.06, 0.02, 0.02)
for shape in args.shapes.split(","):
    n_users, n_items, nnz, zipf_a, seed = synth.CONFIGS[shape]
    rid, cid, val = synth_ratings(n_users, n_items, nnz, zipf_a, seed)
    order = np.argsort(rid, kind="stable")[::args.every]
    rid, cid, val = (np.ascontiguousarray(x[order]) for x in (rid, cid, np.asarray(val, np.float32)))
    mu = float(val.mean())
    for k in (int(x) for x in args.ks.split(",")):
        rs = np.random.RandomState(11)
        U0, V0 = rs.uniform(0, 1, (n_users, k)).astype(np.float32), rs.uniform(0, 1, (n_items, k)).astype(np.float32)
        gbytes = (2 * 12 * len(val) + 2 * 4 * 3 * (n_users + n_items) * k) / 1e9
        for mode in args.modes.split(","):
            for use_bias in (bool(int(b)) for b in args.bias.split(",")):
                tr = _lib.MfTrainer(rid, cid, val, n_users, n_items, k)
                tr.nmf_set_factors(U0, V0)
                fit = lambda n: tr.nmf_fit(n, *hyper, mu if use_bias else 0.0, use_bias, MODES[mode])  # noqa: E731
                t0 = time.perf_counter()
                fit(1)
                first = time.perf_counter() - t0
                t0 = time.perf_counter()
                loss = fit(args.epochs)
                dt = (time.perf_counter() - t0) / max(args.epochs, 1)
                forms = tr.nmf_form()
                tr.close()
                line = ("%-8s k=%-3d %-13s %-5s %10d ratings: first fit %.2f s, epoch %.4f s = %.0f M ratings/s, %.2f GB -> %.1f %% of "
                        "%.0f GB/s (sum %d, bias %d, %d rows split; loss %.6g)") % (
                    shape, k, mode, "bias" if use_bias else "plain", len(val), first, dt, len(val) / dt / 1e6, gbytes,
                    100.0 * gbytes / dt / args.peak_gbs, args.peak_gbs, forms[0], forms[1], forms[2], loss[-1] if len(loss) else 0.0)
                if args.check:
                    sys.path.insert(0, os.path.join(ROOT, "tests"))
                    import nmf_cases as nc

                    n = min(args.check_n, len(val))
                    r_, c_, v_ = rid[:n], cid[:n], val[:n]
                    tr = _lib.MfTrainer(r_, c_, v_, n_users, n_items, k)
                    tr.nmf_set_factors(U0, V0)
                    tr.nmf_fit(1, *hyper, mu if use_bias else 0.0, use_bias, MODES[mode])
                    got = tr.nmf_get_factors()
                    tr.close()
                    dtype = np.float32 if mode == "deterministic" else np.float64
                    want = nc.nmf_fit(r_, c_, v_, U0, V0, None, None, 1, *hyper, mu if use_bias else 0.0, use_bias, dtype=dtype)
                    if mode == "deterministic":
                        line += " | first %d ratings vs the restatement: bit-equal %s" % (
                            n, all(nc.bits_equal(a, b) for a, b in zip(got, want[:4])))
                    else:
                        du, di = np.bincount(r_, minlength=n_users), np.bincount(c_, minlength=n_items)
                        line += " | first %d ratings vs the float64 restatement: U at %.3f, V at %.3f of the free-order bound" % (
                            n, nc.free_order_excess(got[0], want[0], du, k)[0], nc.free_order_excess(got[1], want[1], di, k)[0])
                print(line, flush=True)
