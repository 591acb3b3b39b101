"""TEST INFRASTRUCTURE ONLY — the VEBPR update of one quadruple (cornac/models/bpr/recom_vebpr.pyx inner loop), as the hogwild
kernel states it (csrc/vebpr.inc vebpr_hogwild_kernel), in float64.  All deltas of a quadruple (u, i, v, j) come from the
values BEFORE it; v < 0 = the user has no views:

    x_ij = u.(i - j)   x_iv = u.(i - v)   x_vj = u.(v - j)      each clamped to [-50, 50];  d = 1 / (1 + exp(x))
    no view: d_iv = d_vj = 0, al = be = 0;   else al = alpha, be = 1 - alpha
    dU  = -lr (-d_ij (i - j) - al d_iv (i - v) - be d_vj (v - j) + reg u)
    dVi = -lr (-d_ij u - al d_iv u + reg i)
    dVv = -lr ( al d_iv u - be d_vj u + reg v)        (only with a view)
    dVj = -lr ( d_ij u + be d_vj u + reg j)

v == i (the view item drawn is the purchased one): the hogwild kernel adds BOTH dVi and dVv atomically onto the one row,
and so does this step — the deterministic kernel, like the reference's loop, lets the second plain store win.

`jacobi` sums the deltas every quadruple of an epoch would make from the START tables; `sequential` applies them one after
another in a given order; `step_f32` is one quadruple in the device's number format (sizes tolerances, never a reference).

FAULTS names deliberately wrong variants of the update: tests/test_vebpr_step_cpu.py feeds them to the checks of
tests/vebpr_step_cases.py to prove that those checks would notice.  The heavy loops run in C (oracle/cornac_oracle.c
oracle_vebpr_jacobi_f64, oracle_vebpr_apply_seq_f64, the faults included); `deltas` states the same update in numpy.
"""
import numpy as np

# (the order is the fault number of oracle_vebpr_apply_seq_f64, from 1)
FAULTS = ("alpha_beta_swapped", "view_row_sign_of_d_vj", "view_delta_without_view", "reg_from_other_row",
          "item_from_new_user", "d_iv_from_v_minus_i", "last_lane_left_out")


def _rows(quad, U, V, dtype):
    u, i, v, j = quad
    has_v = v >= 0
    return has_v, U[u].astype(dtype), V[i].astype(dtype), V[np.where(has_v, v, i)].astype(dtype), V[j].astype(dtype)


def scores(quad, U, V, dtype=np.float64):
    """(x_ij, x_iv, x_vj) of every quadruple, clamped, from the given tables; the last two are 0 without a view"""
    has_v, Uu, Vi, Vv, Vj = _rows(quad, U, V, dtype)
    lim = dtype(50)
    x = [np.clip((Uu * d).sum(axis=1, dtype=dtype), -lim, lim) for d in (Vi - Vj, Vi - Vv, Vv - Vj)]
    return x[0], np.where(has_v, x[1], dtype(0)), np.where(has_v, x[2], dtype(0))


def deltas(quad, U, V, lr, reg, alpha, dtype=np.float64):
    """(x [n, 3], dU [n, k], dVi, dVv, dVj) of every quadruple, all from the given tables; dVv is 0 without a view"""
    has_v, Uu, Vi, Vv, Vj = _rows(quad, U, V, dtype)
    lr, reg, one = dtype(lr), dtype(reg), dtype(1)
    x_ij, x_iv, x_vj = scores(quad, U, V, dtype)
    hv = has_v[:, None]
    zero = np.zeros((len(has_v), 1), dtype)
    d_ij = (one / (one + np.exp(x_ij))).astype(dtype)[:, None]
    d_iv = np.where(hv, (one / (one + np.exp(x_iv))).astype(dtype)[:, None], zero)
    d_vj = np.where(hv, (one / (one + np.exp(x_vj))).astype(dtype)[:, None], zero)
    al = np.where(hv, dtype(alpha), zero)
    be = np.where(hv, one - dtype(alpha), zero)
    dU = -lr * (-d_ij * (Vi - Vj) - al * d_iv * (Vi - Vv) - be * d_vj * (Vv - Vj) + reg * Uu)
    dVi = -lr * (-d_ij * Uu - al * d_iv * Uu + reg * Vi)
    dVv = np.where(hv, -lr * (al * d_iv * Uu - be * d_vj * Uu + reg * Vv), zero)
    dVj = -lr * (d_ij * Uu + be * d_vj * Uu + reg * Vj)
    return np.stack([x_ij, x_iv, x_vj], axis=1), dU, dVi, dVv, dVj


def jacobi(quad, tables, lr, reg, alpha):
    """Every quadruple's deltas from the start tables, summed per row (in C: oracle_vebpr_jacobi_f64).  Returns a dict with,
    for each of "U", "V": sum (the summed delta, the table's shape), touches (per row: the deltas that land on it — a
    quadruple with v == i touches that row twice) and path (per row: sum over those deltas of |delta|, Euclidean over the
    row), and x [n, 3] (the float64 scores x_ij, x_iv, x_vj; the last two 0 without a view)."""
    from oracle import oracle as orc

    return orc.vebpr_jacobi_f64(quad, tables, lr, reg, alpha)


def sequential(quad, tables, lr, reg, alpha, order=None, fault=None, drop=None, double=None):
    """The same deltas applied one quadruple after another, in `order` (indices into the quadruples; default: as given).
    Returns float64 (U, V).  fault: one of FAULTS.  drop / double = (table, row): that row's LAST update is left out /
    applied twice.  The loop runs in C (oracle_vebpr_apply_seq_f64)."""
    from oracle import oracle as orc

    U, V = (np.array(t, np.float64) for t in tables[:2])
    order = np.arange(len(quad[0])) if order is None else np.asarray(order)
    assert drop is None or double is None
    mark = None if drop is None and double is None else ((drop[0], drop[1], -1.0) if drop is not None else (double[0], double[1], 1.0))
    orc.vebpr_apply_seq_f64(quad, order, U, V, lr, reg, alpha, 0 if fault is None else 1 + FAULTS.index(fault), mark)
    return U, V


def step_f32(quad, tables, lr, reg, alpha):
    """One step of every quadruple in float32 from the start tables, rounded like the device: float32 products and sums,
    float32 sigmoids, float32 deltas, ONE float32 add onto the row.  Returns (x32 [n, 3], new U rows [n, k], new V[i] rows,
    new V[v] rows (V[i] unchanged without a view), new V[j] rows) — meaningful for quadruples whose rows no other
    quadruple touches and whose v is not their i."""
    U, V = (np.asarray(t, np.float32) for t in tables[:2])
    u, i, v, j = quad
    x, dU, dVi, dVv, dVj = deltas(quad, U, V, lr, reg, alpha, np.float32)
    assert dU.dtype == dVv.dtype == np.float32 and x.dtype == np.float32
    return x, U[u] + dU, V[i] + dVi, V[np.where(v >= 0, v, i)] + dVv, V[j] + dVj


def score_error_bound(quad, tables):
    """An a-priori bound of |float32 score - exact score| per quadruple and score [n, 3], for ANY order of summation and
    with or without fused multiply-adds: k products u (a - b), each carrying at most k + 2 roundings of relative size
    2^-24 (the subtraction, the product, at most k additions), so |err| <= ((1 + 2^-24)^(k + 2) - 1) sum |u_f (a_f - b_f)|
    <= 1.001 (k + 2) 2^-24 sum |...| for k <= 256.  On top of it 2^-20 for the sign decision itself, which the device
    makes as 1 / (1 + __expf(x)) < 0.5: a float32 x within a few ulp(1) of 0 gives exactly 0.5 there.  0 for the two view
    scores of a quadruple without a view, and for x_iv where v == i: every product is exactly 0 and the sigmoid exactly
    0.5 on the device too."""
    U, V = tables[:2]
    has_v, Uu, Vi, Vv, Vj = _rows(quad, U, V, np.float64)
    k = U.shape[1]
    assert k <= 256
    mag = np.stack([np.abs(Uu * d).sum(axis=1) for d in (Vi - Vj, Vi - Vv, Vv - Vj)], axis=1)
    mag[~has_v, 1:] = 0.0
    return np.where(mag > 0, 1.001 * (k + 2) * 2.0 ** -24 * mag + 2.0 ** -20, 0.0)
