#!/usr/bin/env python3
"""Generates tests/golden/nmf_ref.npz by RUNNING THE REFERENCE'S OWN NMF LOOP (only possible where the reference's sources
are present: oracle/build_ref.py's REF).  The fixture travels; this script's build products do not.

cornac/models/nmf/recom_nmf.pyx is cythonised and compiled, straight from where it lies, into a temporary directory that
is removed afterwards; nothing of its text enters this repository.  Flags: -O2 -ffp-contract=off, WITHOUT -ffast-math and
WITHOUT OpenMP.  The fixture pins the SOURCE's IEEE semantics on one thread — the contract of the device's deterministic
mode: every float operation separately rounded, the sums in rating order.  -ffast-math would let the compiler reassociate
the row sums and the dot product and replace the division, so the recorded bits would belong to one compiler version, not
to the algorithm; OpenMP would turn the prange loops into threads whose unsynchronised `+=` on the row sums make the
result depend on timing (without -fopenmp the pragmas are ignored and the loops run in index order, which `num_threads=1`
asks for as well).  -ffp-contract=off keeps a host with fused multiply-add from contracting r_pred + U * V.  (The
reference's setup.py, :155-160, gives this extension no extra compile arguments at all, so its own build takes the
compiler's defaults too.)

The extension's module body imports names from the reference's package (`..recommender`, `...exception`, `...utils`,
`...utils.init_utils`) and tqdm's trange; stand-in modules written here meet them, so nothing else of the reference is
loaded.  `_fit_sgd` is called on an instance built among those stand-ins, with num_threads = 1.

Four cases on 60 users x 40 items x 600 ratings (unique cells, CSR order, tests/nmf_cases.random_case): use_bias False /
True at k = 5 with 3 epochs and at k = 15 with 2 epochs.  Per case: rid, cid, val (float32), U0, V0, the hyper-parameters,
mu, and the loop's U, V, Bu, Bi.

    python tests/golden/make_nmf_golden.py
"""
import importlib.machinery
import importlib.util
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import nmf_cases  # noqa: E402
from oracle import build_ref  # noqa: E402

REF = build_ref.REF
CASES = [(False, 5, 3), (True, 5, 3), (False, 15, 2), (True, 15, 2)]


def case_name(use_bias, k):
    return "%s_k%d" % ("bias" if use_bias else "plain", k)


def build_extension(tmp):
    pyx = os.path.join(REF, "cornac", "models", "nmf", "recom_nmf.pyx")
    cpp = os.path.join(tmp, "recom_nmf.cpp")
    so = os.path.join(tmp, "recom_nmf" + sysconfig.get_config_var("EXT_SUFFIX"))
    # --cplus: the reference declares this extension with language="c++" (it cimports libcpp.bool)
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", "-o", cpp, pyx], cwd=REF)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-std=c++11",
                           "-DNPY_NO_DEPRECATED_API=NPY_1_7_API_VERSION", "-I", sysconfig.get_paths()["include"],
                           "-I", np.get_include(), cpp, "-o", so])
    return so


class _Progress:
    """trange(max_iter, disable=...) as the loop uses it"""

    def __init__(self, n, **kwargs):
        self.n = n

    def __iter__(self):
        return iter(range(self.n))

    def set_postfix(self, *args, **kwargs):
        pass

    def update(self, n=1):
        pass

    def close(self):
        pass


def load_extension(so):
    """as cornac.models.nmf.recom_nmf, among stand-ins for the names its module body imports"""
    def mod(name, package=False, **names):
        m = types.ModuleType(name)
        if package:
            m.__path__ = []
        m.__dict__.update(names)
        sys.modules[name] = m
        return m

    def not_used(*args, **kwargs):
        raise AssertionError("the golden cases pass every table and never score: nothing is drawn or predicted")

    class Recommender:
        def __init__(self, name, trainable=True, verbose=False):
            self.name, self.trainable, self.verbose = name, trainable, verbose

    for name in ("cornac", "cornac.models", "cornac.models.nmf"):
        mod(name, package=True)
    mod("cornac.models.recommender", Recommender=Recommender, ANNMixin=type("ANNMixin", (), {}), MEASURE_DOT="dot")
    mod("cornac.exception", ScoreException=type("ScoreException", (Exception,), {}))
    mod("cornac.utils", package=True, fast_dot=not_used, get_rng=not_used)
    mod("cornac.utils.init_utils", uniform=not_used, zeros=not_used)
    mod("tqdm", package=True)
    mod("tqdm.auto", trange=_Progress)
    name = "cornac.models.nmf.recom_nmf"
    spec = importlib.machinery.ModuleSpec(name, importlib.machinery.ExtensionFileLoader(name, so), origin=so)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def main():
    tmp = tempfile.mkdtemp(prefix="nmf_ref_")
    try:
        ext = load_extension(build_extension(tmp))
        out = {"cases": np.array([case_name(b, k) for b, k, _ in CASES])}
        for use_bias, k, epochs in CASES:
            c = nmf_cases.random_case(60, 40, 600, k, epochs=epochs, seed=9)
            model = ext.NMF(k=k, max_iter=epochs, learning_rate=c["lr"], lambda_u=c["lambda_u"], lambda_v=c["lambda_v"],
                            lambda_bu=c["lambda_bu"], lambda_bi=c["lambda_bi"], use_bias=use_bias, num_threads=1, seed=1)
            assert model.num_threads == 1
            model.num_users, model.num_items = c["nu"], c["ni"]
            model.global_mean = c["mu"] if use_bias else 0.0
            U, V = c["U"].copy(), c["V"].copy()
            Bu, Bi = np.zeros(c["nu"], np.float32), np.zeros(c["ni"], np.float32)
            user_counts = np.bincount(c["rid"], minlength=c["nu"]).astype(np.int32)
            item_counts = np.bincount(c["cid"], minlength=c["ni"]).astype(np.int32)
            model._fit_sgd(c["rid"].copy(), c["cid"].copy(), c["val"].copy(), user_counts, item_counts, U, V, Bu, Bi)
            key = case_name(use_bias, k) + "/"
            hyper = np.array([c["lr"], c["lambda_u"], c["lambda_v"], c["lambda_bu"], c["lambda_bi"], model.global_mean], np.float64)
            out.update({key + "rid": c["rid"], key + "cid": c["cid"], key + "val": c["val"], key + "U0": c["U"], key + "V0": c["V"],
                        key + "hyper": hyper, key + "epochs": np.int64(epochs), key + "use_bias": np.bool_(use_bias),
                        key + "U": U, key + "V": V, key + "Bu": Bu, key + "Bi": Bi})
        path = os.path.join(HERE, "nmf_ref.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
