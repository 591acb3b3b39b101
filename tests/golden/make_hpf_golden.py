#!/usr/bin/env python3
"""Generates tests/golden/hpf_ref.npz by RUNNING THE REFERENCE'S OWN HPF EXTENSION (only possible where the reference's
sources are present: oracle/build_ref.py's REF).  The fixture travels; this script's build products do not.

cornac/models/hpf/cython/hpf.pyx is cythonised and compiled together with cornac/models/hpf/cpp/cpp_hpf.cpp, straight from
where they lie, into a temporary directory that is removed afterwards; nothing of their text enters this repository.
Include paths: the three of the reference's setup.py (:182-186: the cpp directory, its bundled Eigen and Eigen's
unsupported modules, which hold the digamma).  Flags: -O2, WITHOUT -ffast-math (the reference's setup.py gives this
extension no extra compile arguments).  The module body imports `...utils.get_rng` and `...utils.init_utils.gamma`;
stand-in modules written here meet them (a RandomState per seed; RandomState.gamma cast to float32), so nothing else of
the reference is loaded.  The extension's `hpf` / `pf` functions are called as recom_hpf.py:136-167 calls them: the
triplets of the CSC matrix from scipy.sparse.find, as a float64 [n, 3] array.

Given-tables cases (tests/hpf_cases.GOLDEN_GIVEN), hierarchical and plain PF each: 60 users x 40 items x 600 ratings at
k = 5 with 5 iterations, 300 x 200 x 5000 at k = 15 with 3 iterations.  Per case: rid, cid, val (float32), the four start
tables, the four tables after the iterations and, under "it1/", after ONE iteration from the same start (the yardstick of
the device's one-iteration checks).
Seeded cases (GOLDEN_SEEDED), one per variant, init_params all None: the triplets, the seed, k, the iterations and the six
outputs (Z, W, G_s, G_r, L_s, L_r) — they pin the init draws.

The archive is written with fixed member times, so the same inputs give the same bytes.

    python tests/golden/make_hpf_golden.py
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
import types
import zipfile

import numpy as np
import scipy.sparse as sp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import hpf_cases as hc  # noqa: E402
from oracle import build_ref  # noqa: E402

REF = build_ref.REF
TABLES = ("G_s", "G_r", "L_s", "L_r")


def build_extension(tmp):
    pyx = os.path.join(REF, "cornac", "models", "hpf", "cython", "hpf.pyx")
    src = os.path.join(REF, "cornac", "models", "hpf", "cpp", "cpp_hpf.cpp")
    cpp = os.path.join(tmp, "hpf.cpp")
    so = os.path.join(tmp, "hpf" + sysconfig.get_config_var("EXT_SUFFIX"))
    includes = [os.path.join(REF, "cornac", "models", "hpf", "cpp"), os.path.join(REF, "cornac", "utils", "external", "eigen", "Eigen"),
                os.path.join(REF, "cornac", "utils", "external", "eigen", "unsupported", "Eigen")]
    subprocess.check_call([sys.executable, "-m", "cython", "--cplus", "-3", "-o", cpp, pyx], cwd=REF)
    cmd = ["g++", "-O2", "-fPIC", "-shared", "-w", "-std=c++11", "-I", sysconfig.get_paths()["include"]]
    for inc in includes:
        cmd += ["-I", inc]
    subprocess.check_call(cmd + [cpp, src, "-o", so])
    return so


def load_extension(so):
    """as cornac.models.hpf.hpf, among stand-ins for the two names its module body imports"""
    def mod(name, package=False, **names):
        m = types.ModuleType(name)
        if package:
            m.__path__ = []
        m.__dict__.update(names)
        sys.modules[name] = m
        return m

    def get_rng(seed):
        assert isinstance(seed, int), "the golden cases are seeded"
        return np.random.RandomState(seed)

    def gamma(shape, scale=1.0, size=None, random_state=None, dtype=np.float32):
        return random_state.gamma(shape, scale, size).astype(dtype)

    for name in ("cornac", "cornac.models", "cornac.models.hpf"):
        mod(name, package=True)
    mod("cornac.utils", package=True, get_rng=get_rng)
    mod("cornac.utils.init_utils", gamma=gamma)
    name = "cornac.models.hpf.hpf"
    spec = importlib.machinery.ModuleSpec(name, importlib.machinery.ExtensionFileLoader(name, so), origin=so)
    module = importlib.util.module_from_spec(spec)
    sys.modules[name] = module
    spec.loader.exec_module(module)
    return module


def triplets(case):
    """recom_hpf.py:136-145: the CSC matrix's (row, column, value) from scipy.sparse.find, values through float32"""
    X = sp.csc_matrix((case["val"], (case["rid"], case["cid"])), shape=(case["nu"], case["ni"]))
    rid, cid, val = sp.find(X)
    val = np.array(val, dtype="float32")
    rid, cid = np.array(rid, dtype="int32"), np.array(cid, dtype="int32")
    return np.concatenate((np.concatenate(([rid], [cid]), axis=0).T, val.reshape((len(val), 1))), axis=1)


def run(ext, case, k, iters, hierarchical, seed, init):
    fn = ext.hpf if hierarchical else ext.pf
    saved = sys.stdout
    sys.stdout = io.StringIO()   # the extension prints its progress
    try:
        return fn(triplets(case), case["nu"], case["ni"], k, iters, seed, init)
    finally:
        sys.stdout = saved


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


def main():
    tmp = tempfile.mkdtemp(prefix="hpf_ref_")
    try:
        ext = load_extension(build_extension(tmp))
        out = {"given": np.array(sorted(hc.GOLDEN_GIVEN)), "seeded": np.array(sorted(hc.GOLDEN_SEEDED))}
        for name, (make, k, iters, hier) in sorted(hc.GOLDEN_GIVEN.items()):
            c = make(k, hier)
            key = name + "/"
            out.update({key + "rid": c["rid"], key + "cid": c["cid"], key + "val": c["val"], key + "iters": np.int64(iters),
                        key + "hierarchical": np.bool_(hier)})
            for t, a in zip(TABLES, c["tables"]):
                out[key + t + "0"] = a
            for sub, n in (("", iters), ("it1/", 1)):
                res = run(ext, c, k, n, hier, 1, dict(zip(TABLES, (a.copy() for a in c["tables"]))))
                for t in TABLES:
                    out[key + sub + t] = np.asarray(res[t], np.float64)
        for name, (k, iters, seed, hier) in sorted(hc.GOLDEN_SEEDED.items()):
            c = hc.small_case(k, hier)
            res = run(ext, c, k, iters, hier, seed, dict.fromkeys(TABLES))
            key = name + "/"
            out.update({key + "rid": c["rid"], key + "cid": c["cid"], key + "val": c["val"], key + "iters": np.int64(iters),
                        key + "seed": np.int64(seed), key + "k": np.int64(k), key + "hierarchical": np.bool_(hier),
                        key + "nu": np.int64(c["nu"]), key + "ni": np.int64(c["ni"])})
            for t in ("Z", "W") + TABLES:
                out[key + t] = np.asarray(res[t], np.float64)
        path = os.path.join(HERE, "hpf_ref.npz")
        write_npz(path, out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
