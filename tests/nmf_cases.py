"""The NMF checks' reference and inputs, in ONE place: tests/test_nmf_cpu.py holds the restatement below against the golden
that the reference's own compiled loop wrote (tests/golden/make_nmf_golden.py), tests/test_nmf_gpu.py holds the device
against the restatement.

`nmf_fit` restates NMF._fit_sgd (cornac/models/nmf/recom_nmf.pyx:182-267) on one thread with the types of the C that
Cython generates for `floating` = float: every table, hyper-parameter, r, r_pred, error and eps = 1e-9 is a float, every
operation a separately rounded float + - * /:
  * r_pred = ((mu + Bu[u]) + Bi[i]), then + U[u,f] * V[i,f] for f = 0..k-1 in index order (:228-230);
  * the bias steps see the biases the earlier ratings left (:236-238);
  * the four row sums start from zero and grow in rating order (:241-245);
  * U_den += ((count * lambda_u) * U) + eps with the integer count converted to float, U *= U_num / U_den, all users
    before the items (:248-259).
The factors of one row do not depend on each other inside a step, so the element-wise part runs as NumPy array arithmetic
(IEEE, correctly rounded: the same bits as a scalar loop); the sum over the factors is strictly sequential
(np.add.accumulate).  `dtype=np.float64` runs the same code in double FROM THE SAME INPUTS (the hyper-parameters are the
float32 values, promoted): the exact-arithmetic yardstick of the free-order checks.  The loss is
sum error^2 + lambda_u sum U^2 + lambda_v sum V^2 over the pre-update tables, the terms in `dtype`, summed in double (the
reference sums them into a float; no check leans on that rounding).
"""
import functools

import numpy as np

F32 = np.float32
F64 = np.float64
LAMBDAS = dict(lambda_u=0.06, lambda_v=0.06, lambda_bu=0.02, lambda_bi=0.02)
HYPER = dict(lr=0.005, **LAMBDAS)


def nmf_fit(rid, cid, val, U, V, Bu, Bi, n_epochs, lr=0.005, lambda_u=0.06, lambda_v=0.06, lambda_bu=0.02, lambda_bi=0.02,
            mu=0.0, use_bias=False, dtype=F32, details=False):
    """n_epochs of the reference's loop over (rid, cid, val) in the given order (a CSR: rid non-decreasing), from copies of
    the tables.  Returns (U, V, Bu, Bi, loss [n_epochs]); details=True adds a dict of the LAST epoch's r_pred, error,
    magnitude (|mu| + |Bu| + |Bi| + sum |U V|, summed like r_pred) and the tables that epoch started from."""
    T = dtype
    U, V = np.array(U, T, order="C"), np.array(V, T, order="C")
    Bu = np.zeros(U.shape[0], T) if Bu is None else np.array(Bu, T)
    Bi = np.zeros(V.shape[0], T) if Bi is None else np.array(Bi, T)
    rid, cid = np.asarray(rid, np.int64), np.asarray(cid, np.int64)
    assert np.asarray(val).dtype == F32 and (np.diff(rid) >= 0).all()
    val = np.asarray(val).astype(T)
    lr, lu, lv, lbu, lbi, mu, eps = (T(F32(x)) for x in (lr, lambda_u, lambda_v, lambda_bu, lambda_bi, mu, 1e-9))
    cnt_u = np.bincount(rid, minlength=U.shape[0]).astype(T)[:, None]
    cnt_i = np.bincount(cid, minlength=V.shape[0]).astype(T)[:, None]
    loss = np.zeros(n_epochs, F64)
    info = {}
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for epoch in range(n_epochs):
            Un, Ud, Vn, Vd = np.zeros_like(U), np.zeros_like(U), np.zeros_like(V), np.zeros_like(V)
            preds, errs, mags = np.zeros(len(val), T), np.zeros(len(val), T), np.zeros(len(val), T)
            for j in range(len(val)):
                u, i, r = rid[j], cid[j], val[j]
                Uu, Vi = U[u], V[i]
                r_pred = np.add.accumulate(np.concatenate(([mu + Bu[u] + Bi[i]], Uu * Vi)), dtype=T)[-1]
                error = r - r_pred
                preds[j], errs[j] = r_pred, error
                if details:   # the same sum over the terms' magnitudes: r_pred itself where no term is negative
                    mags[j] = np.add.accumulate(np.concatenate(([abs(mu) + abs(Bu[u]) + abs(Bi[i])], np.abs(Uu * Vi))), dtype=T)[-1]
                if use_bias:
                    Bu[u] += lr * (error - lbu * Bu[u])
                    Bi[i] += lr * (error - lbi * Bi[i])
                Un[u] += r * Vi
                Ud[u] += r_pred * Vi
                Vn[i] += r * Uu
                Vd[i] += r_pred * Uu
            if details:   # of the LAST epoch, before its update: what the conditioning of the two denominators needs
                info = dict(r_pred=preds, error=errs, magnitude=mags, U=U.copy(), V=V.copy())
            loss[epoch] = (errs * errs).astype(F64).sum() + (lu * U * U).astype(F64).sum() + (lv * V * V).astype(F64).sum()
            Ud += cnt_u * lu * U + eps
            U *= Un / Ud
            Vd += cnt_i * lv * V + eps
            V *= Vn / Vd
    assert all(a.dtype == T for a in (U, V, Bu, Bi))
    return (U, V, Bu, Bi, loss, info) if details else (U, V, Bu, Bi, loss)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _tables(rs, nu, ni, k):
    return rs.uniform(0, 1, (nu, k)).astype(F32), rs.uniform(0, 1, (ni, k)).astype(F32)


def _csr(cells, ni, rs):
    """unique cells in CSR order (by user, then item) with ratings 1..5"""
    cells = np.sort(np.asarray(cells, np.int64))
    assert len(np.unique(cells)) == len(cells)
    return (cells // ni).astype(np.int32), (cells % ni).astype(np.int32), rs.randint(1, 6, len(cells)).astype(F32)


def _case(rid, cid, val, U, V, nu, ni, k, epochs):
    for a in (rid, cid, val, U, V):
        a.setflags(write=False)
    return dict(rid=rid, cid=cid, val=val, U=U, V=V, nu=nu, ni=ni, k=k, epochs=epochs, mu=float(F32(val.mean())), **HYPER)


@functools.lru_cache(maxsize=None)
def random_case(nu, ni, nnz, k, epochs=2, seed=0):
    """nnz ratings 1..5 on unique random cells of nu x ni, stored as the CSR; uniform(0, 1) tables"""
    rs = np.random.RandomState(seed * 1000 + k)
    rid, cid, val = _csr(rs.permutation(nu * ni)[:nnz], ni, rs)
    U, V = _tables(rs, nu, ni, k)
    return _case(rid, cid, val, U, V, nu, ni, k, epochs)


def base_case(k=15):
    """48 users x 32 items x 256 ratings, 3 epochs: below the dataflow threshold"""
    return random_case(48, 32, 256, k, epochs=3, seed=1)


def chain_case(k=15):
    """128 users x 48 items x 4096 ratings, 2 epochs: the smallest size the bias pass takes as one dataflow launch
    (64 x 48 full holds 3072 ratings only)"""
    c = random_case(128, 48, 4096, k, epochs=2, seed=5)
    assert len(c["val"]) >= 4096
    return c


def threshold_case(nnz, k=5):
    """around the dataflow launch's size threshold (4096 ratings): 200 users x 150 items, 2 epochs"""
    return random_case(200, 150, nnz, k, epochs=2, seed=2)


def wide_case(k=15):
    """300 users x 200 items x 5000 ratings, 1 epoch (the second shape of the free-order bound's CPU check)"""
    return random_case(300, 200, 5000, k, epochs=1, seed=3)


@functools.lru_cache(maxsize=None)
def long_rows_case(k=15):
    """1200 users x 200 items x 6000 ratings, 2 epochs: item 3 is rated by 1000 users (four pieces of the free-order
    plan), user 0 rates every item that has ratings (199: all but item 11), user 1199 rates one item, user 7 and item 11
    have no ratings"""
    nu, ni, n = 1200, 200, 6000
    rs = np.random.RandomState(4242 + k)
    cells = set(0 * ni + i for i in range(ni) if i != 11)                       # user 0
    hot = rs.permutation(np.setdiff1d(np.arange(1, nu - 1), [7]))[:999]         # + user 0 = 1000 raters of item 3
    cells |= set(int(u) * ni + 3 for u in hot)
    cells.add(1199 * ni + 50)
    for c in rs.permutation(nu * ni):
        if len(cells) >= n:
            break
        u, i = divmod(int(c), ni)
        if u in (0, 7, 1199) or i in (3, 11):
            continue
        cells.add(int(c))
    rid, cid, val = _csr(sorted(cells), ni, rs)
    U, V = _tables(rs, nu, ni, k)
    return _case(rid, cid, val, U, V, nu, ni, k, 2)


def run_reference(case, use_bias=False, epochs=None, dtype=F32, U=None, V=None, Bu=None, Bi=None, details=False):
    return nmf_fit(case["rid"], case["cid"], case["val"], case["U"] if U is None else U, case["V"] if V is None else V,
                   Bu, Bi, case["epochs"] if epochs is None else epochs, case["lr"], case["lambda_u"], case["lambda_v"],
                   case["lambda_bu"], case["lambda_bi"], case["mu"] if use_bias else 0.0, use_bias, dtype=dtype, details=details)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype == F32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def max_abs_diff(a, b):
    return float(np.max(np.abs(np.asarray(a, F64) - np.asarray(b, F64)))) if np.size(a) else 0.0


# ---- the free-order (hogwild) bounds, from the float64 run of one epoch ----------------------------------------------
def free_order_condition(case, info64):
    """(cond_U [nu, k], cond_V [ni, k]) >= 1: how much larger a denominator's sum is when r_pred is replaced by the sum of
    its terms' magnitudes.  r_pred's rounding error is (k + 2) 2^-24 of THAT sum, so it is (k + 2) 2^-24 of r_pred only
    while no term is negative — always without biases (mu = Bu = Bi = 0, non-negative tables: the condition is exactly 1,
    bit for bit, and the bound below is the plain one).  With use_bias the biases go negative wherever the start
    over-predicts and r_pred cancels.  Used on ONE case only, long rows at k = 257 with biases, where the plain bound is
    out of reach of every summation order in float32, the reference's own included (tests/test_nmf_cpu.py); every other
    case is held to the plain bound."""
    rid, cid = np.asarray(case["rid"], np.int64), np.asarray(case["cid"], np.int64)
    U, V = np.asarray(info64["U"], F64), np.asarray(info64["V"], F64)
    p, m = np.asarray(info64["r_pred"], F64), np.asarray(info64["magnitude"], F64)
    eps = F64(F32(1e-9))
    out = []
    for own, other, rows, cols, lam in ((U, V, rid, cid, case["lambda_u"]), (V, U, cid, rid, case["lambda_v"])):
        reg = np.bincount(rows, minlength=len(own)).astype(F64)[:, None] * F64(F32(lam)) * own + eps
        den, mag = np.zeros_like(own), np.zeros_like(own)
        np.add.at(den, rows, p[:, None] * other[cols])
        np.add.at(mag, rows, m[:, None] * other[cols])
        out.append(np.maximum(1.0, (mag + reg) / np.abs(den + reg)))
    return out


def free_order_excess(got, want64, deg, k, cond=None):
    """max over the elements with a nonzero float64 value of |got - want| / (|want| cond (2 deg + 2 k + 16) 2^-24): <= 1
    passes.  First-order bound of two deg-term sums of non-negative terms, each carrying r_pred's own (k + 2)-term error,
    plus the final multiply and divide.  cond: None everywhere but on the one case free_order_condition names.  Also returns how many elements were checked (all with want != 0)."""
    got, want64 = np.asarray(got, F64), np.asarray(want64, F64)
    bound = (2.0 * np.asarray(deg, F64)[:, None] + 2 * k + 16) * 2.0 ** -24 * np.abs(want64) * (1.0 if cond is None else cond)
    nz = want64 != 0
    ratio = np.abs(got - want64)[nz] / bound[nz]
    return (float(ratio.max()) if nz.any() else 0.0), int(nz.sum())


def free_order_loss_bound(case, k, info64, U, V):
    """2 (k + 3) 2^-24 sum |e| (r + r_pred)  +  the same relative factor on the regulariser"""
    e, p = np.abs(info64["error"]), np.abs(info64["r_pred"])
    rel = 2.0 * (k + 3) * 2.0 ** -24
    reg = F64(F32(case["lambda_u"])) * (np.asarray(U, F64) ** 2).sum() + F64(F32(case["lambda_v"])) * (np.asarray(V, F64) ** 2).sum()
    return rel * float((e * (case["val"].astype(F64) + p)).sum()) + rel * float(reg)
