#!/usr/bin/env python3
"""Generates tests/golden/ease_ref.npz by RUNNING THE REFERENCE'S OWN EASE (only possible where the reference's sources are
present: oracle/build_ref.py's REF).  cornac/models/ease/recom_ease.py is pure Python over NumPy and SciPy, so nothing is
compiled: oracle.ref_loader.load() makes the reference's Recommender and Dataset importable, and the model is imported from
where it lies.  Nothing of its text enters this repository.

Per case of tests/ease_cases.py (A, Ai, R, T): the training triplets as the reference's Dataset indexes them (<case>/u, i, r)
and, for A, Ai and R, the Gram matrix <case>/G = U.T.dot(U).toarray() exactly as recom_ease.py:78 computes it.  Per
configuration (<case>/<lamb>): B of a fit with posB=False (the clamp of posB=True is exact, the tests compute it), score(u) of
ten users and twenty score(u, i), without (scores, pair_scores) and with posB (scores_pos, pair_scores_pos).

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_ease_golden.py
"""
import importlib
import io
import os
import sys
import zipfile
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ease_cases as ec  # noqa: E402
from oracle import ref_loader  # noqa: E402


def write_npz(path, arrays):
    """np.savez_compressed with fixed member times: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def reference_dataset(Dataset, c):
    ds = Dataset.build(list(zip(c["u"].tolist(), c["i"].tolist(), c["r"].tolist())), seed=1,   # (identity id maps)
                       global_uid_map=OrderedDict((n, n) for n in range(c["nu"])),
                       global_iid_map=OrderedDict((n, n) for n in range(c["ni"])))
    assert (ds.num_users, ds.num_items) == (c["nu"], c["ni"])
    assert all(np.array_equal(a, c[n]) for a, n in zip(ds.uir_tuple, "uir")), "the reference indexes the case as it is"
    return ds


def run_case(Dataset, cname):
    c = ec.case(cname)
    ds = reference_dataset(Dataset, c)
    u, i, r = ds.uir_tuple
    out = {cname + "/u": np.asarray(u, np.int32), cname + "/i": np.asarray(i, np.int32), cname + "/r": np.asarray(r, np.float64)}
    if cname in ec.GRAM_CASES:
        X = ds.matrix
        out[cname + "/G"] = X.T.dot(X).toarray()   # recom_ease.py:78
    return ds, out


def run_config(EASE, ds, name):
    cname, lamb = ec.CONFIGS[name]
    c = ec.case(cname)
    users, (pu, pi) = ec.score_users(c), ec.score_pairs(c)
    out = {}
    for posB, tag in ((False, ""), (True, "_pos")):
        m = EASE(lamb=lamb, posB=posB, verbose=False).fit(ds)
        if not posB:
            out[name + "/B"] = np.array(m.B, np.float64)
        out[name + "/scores" + tag] = np.array([np.asarray(m.score(int(u))).ravel() for u in users])
        out[name + "/pair_scores" + tag] = np.array([float(np.asarray(m.score(int(u), int(i))).ravel()[0]) for u, i in zip(pu, pi)])
    return out


def main():
    ns = ref_loader.load()
    EASE = importlib.import_module("cornac.models.ease.recom_ease").EASE
    out = {"configs": np.array(sorted(ec.CONFIGS))}
    datasets = {}
    for cname in sorted({v[0] for v in ec.CONFIGS.values()}):
        datasets[cname], arrays = run_case(ns.Dataset, cname)
        out.update(arrays)
    for name in sorted(ec.CONFIGS):
        out.update(run_config(EASE, datasets[ec.CONFIGS[name][0]], name))
    path = os.path.join(HERE, "ease_ref.npz")
    write_npz(path, out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
