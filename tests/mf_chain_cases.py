"""The inputs and the reference of the deterministic MF dataflow checks, in ONE place: tests/test_mf_chain_cases_cpu.py
holds the cases to what they claim (the oracle alone), tests/test_mf_chain_gpu.py holds the device against the oracle.

Index arrays: those of tests/pmf_cases.py (random_case / threshold_case / order_case), so MF's dataflow launch is
exercised on the shapes PMF's is.  Tables: float32 normal(0, 0.1), zero biases; mu = the float32 mean of the stars;
lr 0.01, reg 0.02, 2 epochs.

Reference: oracle_mf_fit of the strict oracle build on one thread — the sequential loop of backend_cpu.pyx:58-83 with
every float32 operation separately rounded in index order.  The device states the same expression tree with
contraction off, so U, V, Bu and Bi are compared BIT FOR BIT; loss_per_epoch at rtol 2e-4 (the device sums err^2 in
fp64 tree order, the reference sequentially in fp32; the bound of tests/test_mf_gpu.py).
"""
import functools

import numpy as np

import pmf_cases as pc

F32 = np.float32
LR, REG, EPOCHS = 0.01, 0.02, 2
LOSS_RTOL = 2e-4
FORM_NONE, FORM_CHAIN, FORM_LEVELS = 0, 1, 2

K_CHAIN = (1, 64, 65, 128, 129, 192, 193, 256)   # the register slices R = 1 | 2 | 3 | 4 of the dataflow kernel
K_LEVELS = 257                                    # above the dataflow kernel's k bound
ORDERS = ("user", "item", "shuffled")
ORDER_K = (10, 130)
OWN_USER = {"user": 1, "item": 0}                 # the side the waves must own on a sorted store

# (kind, k, use_bias) of every case the GPU tests run
ALL_CASES = ([("edge", k, True) for k in K_CHAIN + (K_LEVELS,)] + [("edge", 10, False), ("nnz4095", 5, True), ("nnz4096", 5, True)] +
             [("order_" + o, k, True) for o in ORDERS for k in ORDER_K])


@functools.lru_cache(maxsize=None)
def case(kind, k):
    """edge: 64 users x 48 items x 4096 ratings, shuffled, the smallest shape that takes the dataflow launch;
    nnzN: 200 x 150 x N ratings around the size threshold; order_X: pmf_cases.order_case (300 x 200 x 5000, a
    1000-rating item, a single-rating user)"""
    if kind == "edge":
        idx = pc.random_case(64, 48, 4096, k, epochs=EPOCHS, seed=5)
    elif kind.startswith("nnz"):
        assert k == 5
        idx = pc.threshold_case(int(kind[3:]))
    else:
        assert kind.startswith("order_")
        idx = pc.order_case(kind[6:], k)
    nu, ni = idx["nu"], idx["ni"]
    rs = np.random.RandomState(4242 + k)
    U, V = rs.normal(0, 0.1, (nu, k)).astype(F32), rs.normal(0, 0.1, (ni, k)).astype(F32)
    stars = np.ascontiguousarray(idx["stars"], F32)
    c = dict(uid=idx["uid"].astype(np.int64), iid=idx["iid"].astype(np.int64), stars=stars, U=U, V=V, nu=nu, ni=ni, k=k,
             mu=float(stars.mean(dtype=F32)))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(kind, k, use_bias=True, epochs=EPOCHS):
    """(U, V, Bu, Bi, loss [epochs]) of the sequential loop, read-only"""
    from oracle import oracle as orc

    c = case(kind, k)
    U, V = c["U"].copy(), c["V"].copy()
    Bu, Bi = np.zeros(c["nu"], F32), np.zeros(c["ni"], F32)
    loss = np.zeros(epochs, F32)
    ran = orc.lib().oracle_mf_fit(c["uid"].copy(), c["iid"].copy(), c["stars"].copy(), len(c["stars"]), U, V, Bu, Bi, k, LR,
                                  REG, c["mu"], epochs, 1, int(use_bias), 0, loss.ctypes.data)
    assert ran == epochs
    out = (U, V, Bu, Bi, loss)
    for a in out:
        a.setflags(write=False)
    return out


def owns_users(uid, iid):
    """the ownership rule of mf_build_chain (csrc/mf.hip), restated: an adjacency share above 30 % picks the side whose
    ratings are adjacent in the stored order, else the side with the longer hottest row"""
    n = len(uid)
    adj_u, adj_i = int((uid[1:] == uid[:-1]).sum()), int((iid[1:] == iid[:-1]).sum())
    if max(adj_u, adj_i) * 10 > n * 3:
        return adj_u > adj_i
    return int(np.bincount(uid).max()) > int(np.bincount(iid).max())


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def max_abs_diff(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)))) if np.size(a) else 0.0
