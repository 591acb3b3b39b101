"""The PMF checks' reference and inputs, in ONE place: tests/test_pmf_cpu.py holds the restatement below against the
golden that the reference's own compiled loop wrote (tests/golden/make_pmf_golden.py), tests/test_pmf_gpu.py holds the
device against the restatement.

`pmf_fit` restates both loops of cornac/models/pmf/cython/pmf.pyx (:78-104 linear, :137-166 non-linear) with the types of
the C that Cython generates:
  * U, V, the RMSProp caches, s, e, we, sg and eps = 1e-8 are double;
  * lambda_reg, learning_rate and gamma are C floats (np.float32 here), promoted to double in every product;
  * (1 - gamma) is evaluated in float before it meets the double g * g;
  * rat[r] is float32, promoted;
  * s is summed over the factors in index order from 0.0;
  * `float sigmoid(float z)`: s rounded to float, 1 above 6, 0 below -6, else 1.0 / (1.0 + exp(-z)) rounded to float.  The
    reference builds this extension as C++ (setup.py:161-165, `language="c++"`), where `exp` of a float argument is the
    FLOAT overload: libm's expf(-z), a float, then the addition and the division in double.  (Compiled as C it would be
    the double exp; the golden is the C++ build's, like the reference's own binary.)  `expf` here is the host's libm's.
The factors of one row do not depend on each other inside a step, so the element-wise part runs as NumPy array
arithmetic (IEEE double + - * / sqrt, correctly rounded: the same bits as a scalar loop); the three sums over the factors
are strictly sequential (np.add.accumulate).
"""
import ctypes
import ctypes.util

import numpy as np

F32 = np.float32
F64 = np.float64
VARIANTS = ("linear", "non_linear")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]


def sigmoid_f32(z):
    """cdef float sigmoid(float z), pmf.pyx:27-37 (z: np.float32)"""
    if z > F32(6.0):
        return F32(1.0)
    if z < F32(-6.0):
        return F32(0.0)
    return F32(1.0 / (1.0 + float(F32(_libm.expf(float(-z))))))


def _seq_sum(terms):
    """((0.0 + t[0]) + t[1]) + ... in index order"""
    return float(np.add.accumulate(np.concatenate(([0.0], terms)))[-1])


def pmf_fit(uid, iid, rat, U, V, n_epochs, lambda_reg=0.001, learning_rate=0.001, gamma=0.9, variant="non_linear",
            caches=None):
    """n_epochs of the reference's loop over (uid, iid, rat) in the given order, from copies of U and V.
    Returns (U, V, loss [n_epochs], (cache_u, cache_v)); `caches` continues from an earlier call's."""
    assert variant in VARIANTS
    U, V = np.array(U, F64, order="C"), np.array(V, F64, order="C")
    rat = np.asarray(rat)
    assert rat.dtype == F32
    reg32, lr32, gamma32 = F32(lambda_reg), F32(learning_rate), F32(gamma)
    omg32 = F32(1) - gamma32                    # int - float: float arithmetic
    assert omg32.dtype == F32
    reg, lr, gam, omg = F64(reg32), F64(lr32), F64(gamma32), F64(omg32)   # the promotions, exact
    eps = 1e-8
    cache_u, cache_v = (np.zeros_like(U), np.zeros_like(V)) if caches is None else (caches[0].copy(), caches[1].copy())
    loss = np.full(n_epochs, 0.0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for epoch in range(n_epochs):
            for r in range(len(rat)):
                Uu, Vi, cu, cv = U[uid[r]], V[iid[r]], cache_u[uid[r]], cache_v[iid[r]]   # views
                val = float(rat[r])
                s = _seq_sum(Uu * Vi)
                if variant == "non_linear":
                    sg = float(sigmoid_f32(F32(s)))
                    e = val - sg
                    w = e * sg * (1. - sg)
                else:
                    e = val - s
                    w = e
                g = w * Vi - reg * Uu
                cu[:] = gam * cu + omg * (g * g)
                Uu += lr * (g / (np.sqrt(cu) + eps))
                g = w * Uu - reg * Vi                       # the already updated U, the not yet updated V
                cv[:] = gam * cv + omg * (g * g)
                Vi += lr * (g / (np.sqrt(cv) + eps))
                loss[epoch] += e * e + reg * (_seq_sum(Uu * Uu) + _seq_sum(Vi * Vi))
    return U, V, loss, (cache_u, cache_v)


# ---- inputs ------------------------------------------------------------------------------------------------------------
HYPER = dict(lambda_reg=0.01, learning_rate=0.005, gamma=0.9)


def ratings_for(variant, stars):
    """what the reference's loop receives for ratings 1..5: float32, mapped to [0, 1] for the non-linear variant"""
    stars = np.asarray(stars, F32)
    return ((stars - F32(1.0)) / F32(4.0)).astype(F32) if variant == "non_linear" else stars


def random_case(nu, ni, nnz, k, epochs=3, seed=0, std=0.3):
    """nnz ratings 1..5 on random cells (repeats allowed) in shuffled order; normal(0, std) tables"""
    rs = np.random.RandomState(seed * 1000 + k)
    uid = rs.randint(0, nu, nnz).astype(np.int32)
    iid = rs.randint(0, ni, nnz).astype(np.int32)
    stars = rs.randint(1, 6, nnz).astype(F32)
    U, V = rs.normal(0, std, (nu, k)), rs.normal(0, std, (ni, k))
    return dict(uid=uid, iid=iid, stars=stars, U=U, V=V, nu=nu, ni=ni, k=k, epochs=epochs, **HYPER)


def base_case(k=5):
    """48 users x 32 items x 256 ratings, 3 epochs"""
    return random_case(48, 32, 256, k, seed=1)


def threshold_case(nnz):
    """around the dataflow kernel's size threshold (4096 ratings): 200 users x 150 items, k = 5, 2 epochs"""
    return random_case(200, 150, nnz, 5, epochs=2, seed=2)


def order_case(order, k=10):
    """300 users x 200 items x 5000 ratings, 2 epochs: item 3 holds 20 % of the ratings (a long shared- or owned-row
    chain), user 299 has a single rating, (u, i) pairs repeat (1000 ratings of item 3 among 299 users; random repeats
    elsewhere).  order: "user" / "item" = stored sorted by that side (stable), "shuffled" = as drawn"""
    rs = np.random.RandomState(77)
    n = 5000
    uid = rs.randint(0, 299, n).astype(np.int32)
    iid = rs.randint(0, 200, n).astype(np.int32)
    hot = rs.permutation(n)[:1000]
    iid[hot] = 3
    cold = np.setdiff1d(np.arange(n), hot)
    uid[cold[17]] = 299
    stars = rs.randint(1, 6, n).astype(F32)
    if order != "shuffled":
        p = np.argsort(uid if order == "user" else iid, kind="stable")
        uid, iid, stars = uid[p], iid[p], stars[p]
    assert (iid == 3).sum() >= 1000 and (uid == 299).sum() == 1
    assert len(np.unique(uid.astype(np.int64) * 200 + iid)) < n
    U, V = rs.normal(0, 0.3, (300, k)), rs.normal(0, 0.3, (200, k))
    return dict(uid=uid, iid=iid, stars=stars, U=U, V=V, nu=300, ni=200, k=k, epochs=2, **HYPER)


def saturation_case():
    """non-linear only: tables wide enough that |s| > 6 on both sides, ratings exactly 0 and 1 (handed over as they are)"""
    c = random_case(48, 32, 256, 5, seed=3, std=1.6)
    c["rat01"] = (c["stars"] > 3).astype(F32)
    s = np.einsum("nk,nk->n", c["U"][c["uid"]], c["V"][c["iid"]])
    assert (s > 6).sum() >= 5 and (s < -6).sum() >= 5
    return c


def run_reference(case, variant, rat=None, epochs=None, caches=None, U=None, V=None):
    rat = ratings_for(variant, case["stars"]) if rat is None else rat
    return pmf_fit(case["uid"], case["iid"], rat, case["U"] if U is None else U, case["V"] if V is None else V,
                   case["epochs"] if epochs is None else epochs, case["lambda_reg"], case["learning_rate"], case["gamma"],
                   variant, caches=caches)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def max_abs_diff(a, b):
    return float(np.max(np.abs(np.asarray(a, F64) - np.asarray(b, F64)))) if np.size(a) else 0.0
