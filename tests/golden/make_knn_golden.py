#!/usr/bin/env python3
"""Generates tests/golden/knn_ref.npz by RUNNING THE REFERENCE'S OWN UserKNN / ItemKNN over its own compiled extension (only
possible where the reference's sources are present: oracle/build_ref.py's REF).  The fixture travels; this script's build
products do not.

cornac/models/knn/similarity.pyx is cythonised and compiled straight from where it lies into a temporary directory that is
removed afterwards; nothing of its text enters this repository.  Flags: those of the reference's setup.py (:128-138: -O3
-ffast-math -std=c++11 -fopenmp); include paths: numpy's (setup.py:289-296) and the directory of similarity.h.  The result
is registered as cornac.models.knn.similarity next to oracle.ref_loader.load(), which makes the reference's own
recom_knn.py, Recommender and Dataset importable; the models run with seed=1, i.e. on one thread.

Run it as a process of its own: loading a -ffast-math extension switches the process to flush-to-zero.

Per configuration of tests/knn_cases.CONFIGS: the training triplets as the reference's Dataset indexes them (u, i, r), the
similarity table before amplification (sim_indptr, sim_indices, sim0_data) and after it (sim_data, only where amplify !=
1), mean_arr, the mean-centred ratings the scorer reads (rat_*: iu_mat for UserKNN, ui_mat for ItemKNN), score(u) of ten
users at k in {1, 3, 5, 20, 50} (scores [5, 10, num_items]) and twenty score(u, i) per k (pair_scores [5, 20]).

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_knn_golden.py
"""
import importlib.machinery
import importlib.util
import io
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import knn_cases as kc  # noqa: E402
from oracle import build_ref, ref_loader  # noqa: E402

REF = build_ref.REF


def build_extension(tmp):
    src_dir = os.path.join(REF, "cornac", "models", "knn")
    cpp = os.path.join(tmp, "similarity.cpp")
    so = os.path.join(tmp, "similarity" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", "-o", cpp, os.path.join(src_dir, "similarity.pyx")],
                          cwd=REF)
    subprocess.check_call(["g++", "-O3", "-ffast-math", "-std=c++11", "-fopenmp", "-fPIC", "-shared", "-w",
                           "-I", sysconfig.get_paths()["include"], "-I", np.get_include(), "-I", src_dir, cpp, "-o", so])
    return so


def load_models(so):
    ns = ref_loader.load()
    name = "cornac.models.knn.similarity"
    spec = importlib.machinery.ModuleSpec(name, importlib.machinery.ExtensionFileLoader(name, so), origin=so)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    knn = importlib.import_module("cornac.models.knn.recom_knn")
    return ns.Dataset, knn


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


def run_config(Dataset, knn, name):
    cname, model, kw = kc.CONFIGS[name]
    c = kc.case(cname)
    from collections import OrderedDict

    ds = Dataset.build(list(zip(c["u"].tolist(), c["i"].tolist(), c["r"].tolist())), seed=1,   # (identity id maps)
                       global_uid_map=OrderedDict((n, n) for n in range(c["nu"])),
                       global_iid_map=OrderedDict((n, n) for n in range(c["ni"])))
    assert (ds.num_users, ds.num_items) == (c["nu"], c["ni"])
    assert all(np.array_equal(a, c[n]) for a, n in zip(ds.uir_tuple, "uir")), "the reference indexes the case as it is"
    cls = knn.UserKNN if model == "user" else knn.ItemKNN
    amp = kw.get("amplify", 1.0)
    m = cls(k=20, verbose=False, seed=1, **kw)
    amplify, knn._amplify = knn._amplify, lambda mat, alpha=1.0: mat     # first the table as compute_similarity leaves it
    try:
        m.fit(ds)
    finally:
        knn._amplify = amplify
    sim0 = m.sim_mat.copy()
    m.sim_mat = amplify(m.sim_mat, amp)
    assert sim0.has_sorted_indices and np.array_equal(sim0.indices, m.sim_mat.indices)
    key = name + "/"
    u, i, r = ds.uir_tuple
    rat = m.iu_mat if model == "user" else m.ui_mat
    out = {key + "u": np.asarray(u, np.int32), key + "i": np.asarray(i, np.int32), key + "r": np.asarray(r, np.float64),
           key + "sim_indptr": sim0.indptr.astype(np.int32), key + "sim_indices": sim0.indices.astype(np.int32),
           key + "sim0_data": sim0.data, key + "mean_arr": m.mean_arr,
           key + "rat_indptr": rat.indptr.astype(np.int32), key + "rat_indices": rat.indices.astype(np.int32),
           key + "rat_data": rat.data}
    if amp != 1.0:
        out[key + "sim_data"] = m.sim_mat.data
    users, (pu, pi) = kc.score_users(c), kc.score_pairs(c)
    scores = np.zeros((len(kc.KS), len(users), ds.num_items))
    pairs = np.zeros((len(kc.KS), len(pu)))
    for a, k in enumerate(kc.KS):
        m.k = k
        for b, user in enumerate(users):
            scores[a, b] = m.score(int(user))
        for b, (user, item) in enumerate(zip(pu, pi)):
            pairs[a, b] = m.score(int(user), int(item))
    out[key + "scores"], out[key + "pair_scores"] = scores, pairs
    return out


def main():
    tmp = tempfile.mkdtemp(prefix="knn_ref_")
    try:
        Dataset, knn = load_models(build_extension(tmp))
        out = {"configs": np.array(sorted(kc.CONFIGS)), "ks": np.array(kc.KS, np.int64)}
        for name in sorted(kc.CONFIGS):
            out.update(run_config(Dataset, knn, name))
        path = os.path.join(HERE, "knn_ref.npz")
        write_npz(path, out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
