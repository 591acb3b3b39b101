#!/usr/bin/env python3
"""Generates tests/golden/pmf_ref.npz by RUNNING THE REFERENCE'S OWN PMF LOOP (only possible where the reference's sources
are present: oracle/build_ref.py's REF).  The fixture travels; this script's build products do not.

cornac/models/pmf/cython/pmf.pyx is cythonised and compiled, straight from where it lies, into a temporary directory that
is removed afterwards; nothing of its text enters this repository.  Flags: the reference's setup.py gives this extension
no extra compile arguments (setup.py:161-165, unlike the -ffast-math extensions around it), so the compiler's defaults
apply: -O2 here, with -ffp-contract=off added so that the recorded bits are the source's IEEE semantics on any host (baseline
x86-64 has no fused multiply-add to contract into anyway).  The extension's relative imports (`...utils.get_rng`,
`...utils.init_utils.normal`) are met by stand-in modules built here at run time; every case passes its own U and V as
init_params, so nothing is drawn.

Four cases: both variants x {k = 5, 3 epochs | k = 10, 2 epochs} on 60 users x 40 items x 600 ratings in shuffled order
(tests/pmf_cases.random_case).  Per case: uid, iid, rat (float32, as handed to the loop), U0, V0, the three
hyper-parameters, and the loop's U, V and loss.

    python tests/golden/make_pmf_golden.py
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

import pmf_cases  # noqa: E402
from oracle import build_ref  # noqa: E402

REF = build_ref.REF
CASES = [("linear", 5, 3), ("linear", 10, 2), ("non_linear", 5, 3), ("non_linear", 10, 2)]


def build_extension(tmp):
    pyx = os.path.join(REF, "cornac", "models", "pmf", "cython", "pmf.pyx")
    cpp = os.path.join(tmp, "pmf.cpp")
    so = os.path.join(tmp, "pmf" + sysconfig.get_config_var("EXT_SUFFIX"))
    # --cplus: the reference declares this extension with language="c++" (which decides the sigmoid's exp overload)
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", "-o", cpp, pyx], cwd=REF)
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-w", "-std=c++11",
                           "-DNPY_NO_DEPRECATED_API=NPY_1_7_API_VERSION", "-I", sysconfig.get_paths()["include"],
                           "-I", np.get_include(), cpp, "-o", so])
    return so


def load_extension(so):
    """as cornac.models.pmf.pmf, among stand-ins for the two names its module body imports"""
    def pkg(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m

    for name in ("cornac", "cornac.models", "cornac.models.pmf"):
        pkg(name)
    utils = pkg("cornac.utils")
    utils.get_rng = lambda seed: np.random.RandomState(seed)
    init_utils = types.ModuleType("cornac.utils.init_utils")

    def normal(*args, **kwargs):
        raise AssertionError("the golden cases pass U and V: nothing is drawn")

    init_utils.normal = normal
    sys.modules["cornac.utils.init_utils"] = init_utils
    name = "cornac.models.pmf.pmf"
    spec = importlib.machinery.ModuleSpec(name, importlib.machinery.ExtensionFileLoader(name, so), origin=so)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main():
    tmp = tempfile.mkdtemp(prefix="pmf_ref_")
    try:
        pmf = load_extension(build_extension(tmp))
        out = {"cases": np.array(["%s_k%d" % (v, k) for v, k, _ in CASES])}
        for variant, k, epochs in CASES:
            c = pmf_cases.random_case(60, 40, 600, k, epochs=epochs, seed=9)
            rat = pmf_cases.ratings_for(variant, c["stars"])
            fn = pmf.pmf_linear if variant == "linear" else pmf.pmf_non_linear
            res = fn(c["uid"], c["iid"], rat, n_users=c["nu"], n_items=c["ni"], n_ratings=len(rat), k=k, n_epochs=epochs,
                     lambda_reg=c["lambda_reg"], learning_rate=c["learning_rate"], gamma=c["gamma"],
                     init_params={"U": c["U"].copy(), "V": c["V"].copy()}, verbose=False, seed=None)
            key = "%s_k%d/" % (variant, k)
            out.update({key + "uid": c["uid"], key + "iid": c["iid"], key + "rat": rat, key + "U0": c["U"], key + "V0": c["V"],
                        key + "hyper": np.array([c["lambda_reg"], c["learning_rate"], c["gamma"]], np.float64),
                        key + "epochs": np.int64(epochs), key + "U": np.asarray(res["U"]).copy(),
                        key + "V": np.asarray(res["V"]).copy(), key + "loss": np.asarray(res["loss"]).copy()})
        path = os.path.join(HERE, "pmf_ref.npz")
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
