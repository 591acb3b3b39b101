#!/usr/bin/env python3
"""Generates tests/golden/mmmf_ref.npz by RUNNING THE REFERENCE'S OWN MMMF LOOP (only possible where the reference's sources
are present: oracle/build_ref.py's REF).  The fixture travels; this script's build products do not.

cornac/models/mmmf/recom_mmmf.pyx is cythonised and compiled, straight from where it lies, into a temporary directory that
is removed afterwards; nothing of its text enters this repository.  Flags: -O2 -ffp-contract=off, WITHOUT -ffast-math and
WITHOUT OpenMP: the fixture pins the SOURCE's IEEE semantics on one thread — every float operation separately rounded, the
score summed in index order — which is the contract of the device's deterministic mode (the reasoning of
make_nmf_golden.py).  The extension subclasses the reference's BPR and cimports RNGVector / has_non_zero from
cornac/models/bpr/recom_bpr: it is loaded beside the compiled recom_bpr that oracle/ref_loader.py provides (RNGVector is
integer work, has_non_zero an inline function compiled into this extension).

`_fit_sgd` is called once per epoch, as BPR.fit does (recom_bpr.pyx:189-206), with two RNGVector engines, num_threads = 1.

Four cases on 60 users x 40 items x 600 unique interactions: k = 5 with 3 epochs and k = 15 with 2 epochs, each in float32
and float64; lr = 0.05, reg = 0.01, start tables by BPR's _init rule ((uniform - 0.5) / k, zero biases).  Per case: the CSR,
the start tables, the hyper-parameters, the two mt19937 seeds, U, V, B after the run and (correct, skipped) per epoch.

    python tests/golden/make_mmmf_golden.py
"""
import importlib.machinery
import importlib.util
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import build_ref, ref_loader  # noqa: E402
from oracle import oracle as orc  # noqa: E402

REF = build_ref.REF
CASES = [(5, 3, "f32"), (5, 3, "f64"), (15, 2, "f32"), (15, 2, "f64")]
NU, NI, NNZ, LR, REG = 60, 40, 600, 0.05, 0.01
SEED_POS, SEED_NEG = 20240, 20241  # RNGVector(1, rows, seed) arguments


def case_name(k, kind):
    return "k%d_%s" % (k, kind)


def interactions():
    rs = np.random.RandomState(7)
    cells = np.sort(rs.choice(NU * NI, NNZ, replace=False))
    users, items = cells // NI, cells % NI
    indptr = np.zeros(NU + 1, np.int32)
    np.cumsum(np.bincount(users, minlength=NU), out=indptr[1:])
    return indptr, items.astype(np.int32), users.astype(np.int32)


def start_tables(k):
    rs = np.random.RandomState(100 + k)
    U = ((rs.uniform(0.0, 1.0, (NU, k)).astype(np.float32) - 0.5) / k).astype(np.float32)
    V = ((rs.uniform(0.0, 1.0, (NI, k)).astype(np.float32) - 0.5) / k).astype(np.float32)
    return U, V, np.zeros(NI, np.float32)


def build_extension(tmp):
    rel = "cornac/models/mmmf/recom_mmmf"
    pyx = os.path.join(REF, rel + ".pyx")
    cpp = os.path.join(tmp, "recom_mmmf.cpp")
    so = os.path.join(tmp, "recom_mmmf" + sysconfig.get_config_var("EXT_SUFFIX"))
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", "-I", REF, "-o", cpp, pyx], cwd=REF)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-std=c++11",
                           "-DNPY_NO_DEPRECATED_API=NPY_1_7_API_VERSION", "-I", sysconfig.get_paths()["include"],
                           "-I", np.get_include(), "-I", os.path.join(REF, "cornac", "utils", "external"),
                           "-I", os.path.join(REF, os.path.dirname(rel)), cpp, "-o", so])
    return so


def load_extension(so, tmp):
    """as cornac.models.mmmf.recom_mmmf, beside the reference's compiled recom_bpr"""
    build_ref.build(verbose=False)
    ns = ref_loader.load()
    ref_loader._stub_pkg("cornac.models.mmmf", tmp)
    name = "cornac.models.mmmf.recom_mmmf"
    spec = importlib.machinery.ModuleSpec(name, importlib.machinery.ExtensionFileLoader(name, so), origin=so)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module, ns


def main():
    tmp = tempfile.mkdtemp(prefix="mmmf_ref_")
    try:
        ext, ns = load_extension(build_extension(tmp), tmp)
        indptr, indices, user_ids = interactions()
        neg_ids = np.arange(NI, dtype=np.int32)
        out = {"cases": np.array([case_name(k, kind) for k, _, kind in CASES]), "indptr": indptr, "indices": indices,
               "hyper": np.array([LR, REG], np.float64),
               "mt_seeds": np.array([orc.rngvector_seed(SEED_POS), orc.rngvector_seed(SEED_NEG)], np.int64)}
        for k, epochs, kind in CASES:
            dt = np.float32 if kind == "f32" else np.float64
            U0, V0, B0 = start_tables(k)
            U, V, B = (a.astype(dt) for a in (U0, V0, B0))
            model = ext.MMMF(k=k, max_iter=epochs, learning_rate=LR, lambda_reg=REG, num_threads=1, seed=1)
            model.num_users, model.num_items = NU, NI
            rng_pos, rng_neg = ns.RNGVector(1, NNZ - 1, SEED_POS), ns.RNGVector(1, NI - 1, SEED_NEG)
            stats = [model._fit_sgd(rng_pos, rng_neg, 1, user_ids, indices, neg_ids, indptr, U, V, B) for _ in range(epochs)]
            key = case_name(k, kind) + "/"
            out.update({key + "U0": U0, key + "V0": V0, key + "B0": B0, key + "U": U, key + "V": V, key + "B": B,
                        key + "epochs": np.int64(epochs), key + "stats": np.array(stats, np.int64)})
            print(key, stats)
        path = os.path.join(HERE, "mmmf_ref.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
