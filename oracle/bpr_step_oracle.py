"""TEST INFRASTRUCTURE ONLY — the BPR update of one triplet (cornac/models/bpr/recom_bpr.pyx inner loop), as the hogwild
kernels implement it, in float64 numpy.  All five deltas of a triplet (u, i, j) come from the values BEFORE it:

    x = U[u].(V[i] - V[j]) + B[i] - B[j]          z = 1 / (1 + exp(x))
    U[u] += lr (z (V[i] - V[j]) - reg U[u])
    V[i] += lr (z U[u] - reg V[i])                B[i] += lr (z - reg B[i])       (biases: use_bias only)
    V[j] += lr (-z U[u] - reg V[j])               B[j] += lr (-z - reg B[j])

`jacobi` sums the deltas every triplet of a launch would make from the START tables; `sequential` applies them one after
another in a given order; `step_f32` is one triplet in the device's number format (sizes tolerances, never a reference).

FAULTS names deliberately wrong variants of the update: tests/test_bpr_step_cpu.py feeds them to the checks of
tests/bpr_step_cases.py to prove that those checks would notice.
"""
import numpy as np

FAULTS = ("bias_reg_dropped", "reg_from_other_row", "item_from_new_user", "lr_twice_on_neg", "bias_sign_in_score",
          "last_lane_left_out")


def scores(trip, U, V, B, dtype=np.float64, fault=None):
    """x of every triplet, from the given tables"""
    u, i, j = trip
    Uu, d = U[u].astype(dtype), V[i].astype(dtype) - V[j].astype(dtype)
    prod = Uu * d
    if fault == "last_lane_left_out":
        prod = prod[:, :-1]
    bi, bj = B[i].astype(dtype), B[j].astype(dtype)
    return prod.sum(axis=1, dtype=dtype) + ((bi + bj) if fault == "bias_sign_in_score" else (bi - bj))


def deltas(trip, U, V, B, lr, reg, use_bias=True, dtype=np.float64, fault=None):
    """(x, z, dU [n, k], dVi, dVj, dBi [n], dBj) of every triplet, all from the given tables"""
    u, i, j = trip
    lr, reg = dtype(lr), dtype(reg)
    Uu, Vi, Vj = U[u].astype(dtype), V[i].astype(dtype), V[j].astype(dtype)
    bi, bj = B[i].astype(dtype), B[j].astype(dtype)
    d = Vi - Vj
    x = scores(trip, U, V, B, dtype, fault)
    z = (dtype(1) / (dtype(1) + np.exp(x))).astype(dtype)
    zc = z[:, None]
    dU = lr * (zc * d - reg * Uu)
    u_item = Uu + dU if fault == "item_from_new_user" else Uu
    dVi = lr * (zc * u_item - reg * (Vj if fault == "reg_from_other_row" else Vi))
    dVj = lr * (-zc * u_item - reg * Vj)
    if fault == "lr_twice_on_neg":
        dVj = lr * dVj
    if use_bias:
        breg = dtype(0) if fault == "bias_reg_dropped" else reg
        dBi, dBj = lr * (z - breg * bi), lr * (-z - breg * bj)
    else:
        dBi = dBj = np.zeros_like(z)
    return x, z, dU, dVi, dVj, dBi, dBj


def jacobi(trip, tables, lr, reg, use_bias=True):
    """Every triplet's deltas from the start tables, summed per row (in C: oracle_bpr_jacobi_f64).  Returns a dict with,
    for each of "U", "V", "B": sum (the summed delta, the table's shape), touches (per row) and path (per row: sum over
    its triplets of |delta|, Euclidean over the row), and x, z (the float64 scores and their sigmoids)."""
    from oracle import oracle as orc

    return orc.bpr_jacobi_f64(trip, tables, lr, reg, use_bias)


def sequential(trip, tables, lr, reg, use_bias=True, order=None, fault=None, drop=None, double=None):
    """The same deltas applied one triplet after another, in `order` (indices into the triplets; default: as given).
    Returns float64 (U, V, B).  drop / double = (table, row): that row's LAST update is left out / applied twice.
    Without a fault the loop runs in C (oracle_bpr_apply_seq_f64), with one here, through `deltas`."""
    U, V, B = (np.array(t, np.float64) for t in tables)
    u, i, j = trip
    order = np.arange(len(u)) if order is None else np.asarray(order)
    if fault is None and drop is None and double is None:
        from oracle import oracle as orc

        orc.bpr_apply_seq_f64(trip, order, U, V, B, lr, reg, use_bias)
        return U, V, B
    last = {}
    for t in order:
        s = slice(t, t + 1)
        tr = (u[s], i[s], j[s])
        _, _, dU, dVi, dVj, dBi, dBj = deltas(tr, U, V, B, lr, reg, use_bias, np.float64, fault)
        U[u[t]] += dU[0]
        V[i[t]] += dVi[0]
        V[j[t]] += dVj[0]
        B[i[t]] += dBi[0]
        B[j[t]] += dBj[0]
        if drop is not None or double is not None:
            last[("U", int(u[t]))] = dU[0]
            last[("V", int(i[t]))] = dVi[0]
            last[("V", int(j[t]))] = dVj[0]
            last[("B", int(i[t]))] = dBi[0]
            last[("B", int(j[t]))] = dBj[0]
    for key, sign in ((drop, -1.0), (double, 1.0)):
        if key is not None:
            {"U": U, "V": V, "B": B}[key[0]][key[1]] += sign * last[(key[0], int(key[1]))]
    return U, V, B


def step_f32(trip, tables, lr, reg, use_bias=True):
    """One step of every triplet in float32 from the start tables, rounded like the device: float32 products and sum,
    float32 z, float32 deltas, ONE float32 add onto the row.  Returns (x32, new U rows [n, k], new V[i] rows, new V[j]
    rows, new B[i], new B[j]) — meaningful for triplets whose rows no other triplet touches."""
    U, V, B = (np.asarray(t, np.float32) for t in tables)
    u, i, j = trip
    x, _, dU, dVi, dVj, dBi, dBj = deltas(trip, U, V, B, lr, reg, use_bias, np.float32)
    assert dU.dtype == np.float32 and x.dtype == np.float32
    return x, U[u] + dU, V[i] + dVi, V[j] + dVj, B[i] + dBi.astype(np.float32), B[j] + dBj.astype(np.float32)


def score_error_bound(trip, tables):
    """An a-priori bound of |float32 score - exact score| per triplet, for ANY order of summation and with or without
    fused multiply-adds: k products of (u, vi - vj) plus two biases are k + 2 terms, each carrying at most (k + 3)
    roundings of relative size 2^-24 (the subtraction, the product, at most k + 1 additions):
    |err| <= (k + 3) 2^-24 (sum |u_f (vi_f - vj_f)| + |b_i| + |b_j|), to first order; doubled to cover the higher orders
    and the sign decision z < 0.5 <=> exp(x) > 1 made through __expf."""
    U, V, B = tables
    u, i, j = trip
    k = U.shape[1]
    mag = np.abs(U[u].astype(np.float64) * (V[i].astype(np.float64) - V[j].astype(np.float64))).sum(axis=1)
    mag += np.abs(B[i].astype(np.float64)) + np.abs(B[j].astype(np.float64))
    return 2.0 * (k + 3) * 2.0 ** -24 * mag
