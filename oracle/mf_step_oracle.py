"""TEST INFRASTRUCTURE ONLY — the MF update of one rating (cornac/models/mf/backend_cpu.pyx inner loop), as the hogwild
kernels implement it (csrc/mf.hip mf_hogwild_rowwise_kernel, the generic kernel, csrc/mf_blocks.inc mf_blocks_kernel), in
float64 numpy.  All four deltas of a rating (u, i, r) come from the values BEFORE it:

    err = r - (mu + Bu[u] + Bi[i] + U[u].V[i])
    U[u] += lr (err V[i] - reg U[u])      V[i] += lr (err U[u] - reg V[i])
    Bu[u] += lr (err - reg Bu[u])         Bi[i] += lr (err - reg Bi[i])        (biases: use_bias only)

`jacobi` sums the deltas every rating of a launch would make from the START tables; `sequential` applies them one after
another in a given order; `step_f32` is one rating in the device's number format (sizes tolerances, never a reference).
A rating is (u, i, r); a set of tables is (U, V, Bu, Bi).

Split rows (csrc/mf.hip mf_build_split, mf_split_id; csrc/mf_blocks.inc mf_virtual_merge_kernel) are restated here too:
`split_plan`, `split_id`, `step_inflight`, `align_merge`; `launch` is a whole launch with copies — the copies start equal
to their rows, the ratings (item ids >= n_items name copies) are applied, the copies are folded back — and `fold` turns the
Jacobi sums of the copies into the reference of the merged row.  `ownership` restates mf_build_ownership.

FAULTS names deliberately wrong variants: tests/test_mf_step_cpu.py feeds them to the checks of tests/mf_step_cases.py to
prove that those checks would notice.  MERGE_FAULTS are the ones that live in the copies' reset and merge: they change
nothing where no row is split.
"""
import heapq

import numpy as np

TABLES = ("U", "V", "Bu", "Bi")
MERGE_FAULTS = ("merge_plain_sum", "merge_mean", "copies_not_reset")
FAULTS = ("item_from_new_user", "reg_from_other_row", "bias_reg_dropped", "mu_left_out", "err_sign_on_item",
          "last_lane_left_out") + MERGE_FAULTS


def errors(rat, tables, mu, dtype=np.float64, fault=None):
    """err of every rating, from the given tables"""
    u, i, r = rat
    U, V, Bu, Bi = tables
    prod = U[u].astype(dtype) * V[i].astype(dtype)
    if fault == "last_lane_left_out":
        prod = prod[:, :-1]
    m = dtype(0) if fault == "mu_left_out" else dtype(mu)
    return np.asarray(r).astype(dtype) - ((m + Bu[u].astype(dtype) + Bi[i].astype(dtype)) + prod.sum(axis=1, dtype=dtype))


def deltas(rat, tables, lr, reg, mu, use_bias=True, dtype=np.float64, fault=None):
    """(err, dU [n, k], dV, dBu [n], dBi) of every rating, all from the given tables"""
    u, i, _ = rat
    U, V, Bu, Bi = tables
    lr, reg = dtype(lr), dtype(reg)
    Uu, Vi, bu, bi = U[u].astype(dtype), V[i].astype(dtype), Bu[u].astype(dtype), Bi[i].astype(dtype)
    err = errors(rat, tables, mu, dtype, fault)
    ec = err[:, None]
    dU = lr * (ec * Vi - reg * Uu)
    u_item = Uu + dU if fault == "item_from_new_user" else Uu
    dV = lr * ((-ec if fault == "err_sign_on_item" else ec) * u_item - reg * (Uu if fault == "reg_from_other_row" else Vi))
    if use_bias:
        dBu = lr * (err - reg * bu)
        dBi = lr * (err - (dtype(0) if fault == "bias_reg_dropped" else reg) * bi)
    else:
        dBu = dBi = np.zeros_like(err)
    return err, dU, dV, dBu, dBi


def jacobi(rat, tables, lr, reg, mu, use_bias=True, err_floor=None):
    """Every rating's deltas from the start tables, summed per row (in C: oracle_mf_jacobi_f64).  Returns a dict with, for
    each of "U", "V", "Bu", "Bi": sum (the summed delta, the table's shape), touches (per row) and path (per row: sum over
    its ratings of lr (max(|err|, E) |other row| + reg |own row|), Euclidean norms; E = err_floor, default the rms error of
    the ratings), and err (float64, per rating), sse (their sum of squares), E."""
    from oracle import oracle as orc

    if err_floor is None:
        e = orc.mf_jacobi_f64(rat, tables, 0.0, 0.0, mu, use_bias, 0.0)["err"]
        err_floor = float(np.sqrt(np.mean(e * e)))
    out = orc.mf_jacobi_f64(rat, tables, lr, reg, mu, use_bias, err_floor)
    out["sse"], out["E"] = float(np.sum(out["err"] ** 2)), err_floor
    return out


def sequential(rat, tables, lr, reg, mu, use_bias=True, order=None, fault=None, drop=None, double=None):
    """The same deltas applied one rating after another, in `order` (indices into the ratings; default: as given).
    Returns float64 (U, V, Bu, Bi).  drop / double = (table, row): that row's LAST update is left out / applied twice.
    Without a fault the loop runs in C (oracle_mf_apply_seq_f64), with one here, through `deltas`."""
    T = [np.array(t, np.float64) for t in tables]
    u, i, r = rat
    order = np.arange(len(u)) if order is None else np.asarray(order)
    if fault in (None,) + MERGE_FAULTS and drop is None and double is None:
        from oracle import oracle as orc

        orc.mf_apply_seq_f64(rat, order, *T, lr, reg, mu, use_bias)
        return tuple(T)
    last = {}
    for t in order:
        s = slice(t, t + 1)
        _, dU, dV, dBu, dBi = deltas((u[s], i[s], r[s]), T, lr, reg, mu, use_bias, np.float64, fault)
        for tab, row, d in (("U", u[t], dU), ("V", i[t], dV), ("Bu", u[t], dBu), ("Bi", i[t], dBi)):
            T[TABLES.index(tab)][row] += d[0]
            last[(tab, int(row))] = d[0]
    for key, sign in ((drop, -1.0), (double, 1.0)):
        if key is not None:
            T[TABLES.index(key[0])][key[1]] += sign * last[(key[0], int(key[1]))]
    return tuple(T)


def step_f32(rat, tables, lr, reg, mu, use_bias=True):
    """One step of every rating in float32 from the start tables, rounded like the device: float32 products and sum,
    float32 deltas, ONE float32 add onto the row.  Returns (err32, new U rows [n, k], new V rows, new Bu, new Bi) —
    meaningful for ratings whose rows no other rating touches."""
    T = [np.asarray(t, np.float32) for t in tables]
    u, i, _ = rat
    err, dU, dV, dBu, dBi = deltas(rat, T, lr, reg, mu, use_bias, np.float32)
    assert dU.dtype == np.float32 and err.dtype == np.float32
    return err, T[0][u] + dU, T[1][i] + dV, T[2][u] + dBu.astype(np.float32), T[3][i] + dBi.astype(np.float32)


def error_bound(rat, tables, mu):
    """An a-priori bound of |float32 err - exact err| per rating, for ANY order of summation and with or without fused
    multiply-adds: mu, two biases and k products are k + 3 terms, each carrying at most k + 3 roundings of relative size
    2^-24 (its product, at most k + 2 additions), and the subtraction from r rounds once more:
    |error| <= (k + 4) 2^-24 (|mu| + |bu| + |bi| + sum |u_f v_f| + |r|) to first order; doubled to cover the higher orders."""
    u, i, r = rat
    U, V, Bu, Bi = tables
    k = U.shape[1]
    mag = np.abs(U[u].astype(np.float64) * V[i].astype(np.float64)).sum(axis=1)
    mag += abs(mu) + np.abs(Bu[u].astype(np.float64)) + np.abs(Bi[i].astype(np.float64)) + np.abs(np.asarray(r, np.float64))
    return 2.0 * (k + 4) * 2.0 ** -24 * mag


# ---- split rows ---------------------------------------------------------------------------------------------------------------
def step_inflight(n_items, k, cus=256, blocks_per_cu=8):
    """csrc/mf.hip mf_launch_fused, form 3: (workgroups of the throttled launch, ratings it keeps in flight together)"""
    per_wave = 32 if k <= 4 else 16 if k <= 8 else 8 if k <= 32 else 4 if k <= 64 else 2 if k <= 192 else 1
    per_wg = 4 * per_wave
    want = max(256, 4 * n_items)
    grid = max(1, min(cus * blocks_per_cu, -(-want // per_wg)))
    return grid, grid * per_wg


def split_per_copy(nnz, inflight=None):
    """the `per_copy` of mf_build_split: a copy per 32 ratings in flight for a step handle (form 3; inflight =
    step_inflight), 0.1 % of the ratings from 2^20 ratings on, 0 (nothing is split) below"""
    if inflight is not None:
        return (max(1, min(nnz, inflight)) + 31) // 32
    return 1000 if nnz >= 1 << 20 else 0


def split_plan(cid, n_items, per_copy):
    """mf_build_split restated: (split_item, split_ptr) — item i is split when cnt_i x per_copy > nnz, into
    min(256, ceil(cnt_i x per_copy / nnz)) copies"""
    n = len(cid)
    cnt = np.bincount(cid, minlength=n_items).astype(np.int64)
    items = np.flatnonzero(cnt * per_copy > n)
    w = np.minimum(256, (cnt[items] * per_copy + n - 1) // n)
    return items.astype(np.int32), np.concatenate([[0], np.cumsum(w)]).astype(np.int32)


def split_id(s, item, split_item, split_ptr, n_items):
    """mf_split_id restated, for arrays: the row a rating of `item` at COO position `s` updates — the item, or the copy
    (id n_items + v) a hash of the position names"""
    s, item = np.asarray(s, np.int64), np.asarray(item, np.int64)
    of = np.full(n_items, -1, np.int64)
    of[split_item] = np.arange(len(split_item))
    j = of[item]
    x = ((s & 0xFFFFFFFF) * 0x85EBCA6B + 0x165667B1) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x9E3779B1) & 0xFFFFFFFF
    x ^= x >> 13
    ptr = np.asarray(split_ptr, np.int64)
    jj = np.maximum(j, 0)
    w = ptr[jj + 1] - ptr[jj] if len(split_item) else np.ones_like(j)
    return np.where(j < 0, item, n_items + (ptr[jj] if len(split_item) else 0) + x % np.maximum(w, 1))


def align_merge(D):
    """the "align" merge of the copies' deltas D [W, k] (or [W] for a bias, merged on its own as a scalar):
    S x min(1, sum |d_w|^2 / |S|^2) with S = sum d_w (mf_virtual_merge_kernel)"""
    D = np.asarray(D, np.float64)
    S = D.sum(axis=0)
    n2, w2 = float(np.sum(S * S)), float(np.sum(D * D))
    return S * (min(1.0, w2 / n2) if n2 > 0 else 1.0)


def _merge(D, fault):
    if fault == "merge_plain_sum":
        return np.asarray(D, np.float64).sum(axis=0)
    if fault == "merge_mean":
        return np.asarray(D, np.float64).mean(axis=0)
    return align_merge(D)


def extend(tables, split, copies=None):
    """the tables with the copies' rows after the items' (id n_items + v): every copy equal to its row, or `copies` =
    (Vx, Bix) as they are"""
    U, V, Bu, Bi = tables
    items, ptr = split
    of = np.repeat(items, np.diff(ptr))
    Vx, Bix = (V[of], Bi[of]) if copies is None else copies
    return U, np.concatenate([V, Vx.astype(V.dtype)]), Bu, np.concatenate([Bi, Bix.astype(Bi.dtype)])


def launch(rat, tables, split, lr, reg, mu, use_bias=True, order=None, fault=None, drop=None, double=None, copies=None):
    """One launch over ratings whose item ids name copies (>= n_items) where the row is split, in float64: the copies
    start equal to their rows (fault copies_not_reset: from `copies`, what the previous launch left), the ratings are
    applied one after another, every split row becomes row + the merge of its copies' deltas.  Returns ((U, V, Bu, Bi) at
    the tables' shapes, (Vx, Bix): what the copies hold afterwards — the merged rows).  drop / double name rows of the
    EXTENDED tables."""
    n_items = len(tables[1])
    items, ptr = split
    ext = extend(tables, split, copies if fault == "copies_not_reset" else None)
    U, Vx, Bu, Bix = sequential(rat, ext, lr, reg, mu, use_bias, order, fault, drop, double)
    V, Bi = Vx[:n_items].copy(), Bix[:n_items].copy()
    for j, it in enumerate(items):
        lo, hi = n_items + ptr[j], n_items + ptr[j + 1]
        V[it] += _merge(Vx[lo:hi] - V[it], fault)
        Bi[it] += _merge(Bix[lo:hi] - Bi[it], fault)
    of = np.repeat(items, np.diff(ptr))
    return (U, V, Bu, Bi), (V[of], Bi[of])


def fold(jac, split, n_items):
    """the Jacobi sums over the extended tables -> the reference at the tables' own shapes: a split row's delta is the
    align merge of its copies' sums, its touches and its path the sums of theirs"""
    items, ptr = split
    out = {key: v for key, v in jac.items() if key not in ("V", "Bi")}
    for tab in ("V", "Bi"):
        out[tab] = {key: v[:n_items].copy() for key, v in jac[tab].items()}
        for j, it in enumerate(items):
            lo, hi = n_items + ptr[j], n_items + ptr[j + 1]
            out[tab]["sum"][it] = align_merge(jac[tab]["sum"][lo:hi])
            out[tab]["touches"][it] = jac[tab]["touches"][lo:hi].sum()
            out[tab]["path"][it] = jac[tab]["path"][lo:hi].sum()
    return out


# ---- user-row ownership of the fused kernel -------------------------------------------------------------------------------------
def _hash_key24(x):
    """the integer whose float is csrc/mf.hip hash_key (x >> 8 of the mixed position: 24 bits, exact in float32)"""
    x = np.asarray(x, np.int64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x >> 8


def ownership(rid, cid_ext, n_users, n_waves):
    """mf_build_ownership restated: (wave_ptr, own_u, own_i) as MfTrainer.debug_ownership() returns them.  Users with more
    than nnz / W / 2 ratings are shared (own_u = ~u, their ratings dealt round-robin over the waves); the others go whole,
    heaviest first, to the least loaded wave (LPT); inside a wave the ratings stand in the order of a hash of their COO
    position (stable: shared ones first, then the wave's users as they arrived).  cid_ext: the item ids after split_id."""
    rid = np.asarray(rid, np.int64)
    nnz, W = len(rid), int(n_waves)
    deg = np.bincount(rid, minlength=n_users)
    cap = max(1, nnz // W // 2)
    n_shared = int(deg[deg > cap].sum())
    blk = -(-n_shared // W)
    load = [max(0, min(blk, n_shared - w * blk)) if blk > 0 else 0 for w in range(W)]
    excl = np.flatnonzero((deg > 0) & (deg <= cap))
    excl = excl[np.argsort(-deg[excl], kind="stable")]
    heap = [(load[w], w) for w in range(W)]
    heapq.heapify(heap)
    owner = np.full(n_users, -1, np.int64)
    for usr in excl:
        ld, w = heapq.heappop(heap)
        owner[usr] = w
        heapq.heappush(heap, (ld + int(deg[usr]), w))
    arrival = np.zeros(n_users, np.int64)
    arrival[excl] = np.arange(len(excl))
    pos = np.argsort(rid, kind="stable")  # COO positions grouped by user
    usr = rid[pos]
    shared = deg[usr] > cap
    sp = np.cumsum(shared) - 1
    wave = np.where(shared, sp % W, owner[usr])
    order = np.lexsort((np.arange(nnz), np.where(shared, sp, arrival[usr]), ~shared, _hash_key24(pos), wave))
    wave_ptr = np.concatenate([[0], np.cumsum(np.bincount(wave, minlength=W))]).astype(np.int64)
    return wave_ptr, np.where(shared, ~usr, usr)[order].astype(np.int32), np.asarray(cid_ext)[pos][order].astype(np.int32)


def same_user_batches(own, unr):
    """batches of `unr` consecutive ratings of one wave's 64-rating tiles that name the same exclusive user twice: where
    the owned kernel sums the deltas of a batch before its one plain store (csrc/mf.hip, "exclusive users")"""
    wave_ptr, own_u, _ = own
    idx = np.arange(len(own_u))
    wave = np.searchsorted(wave_ptr, idx, side="right") - 1
    batch = (idx - wave_ptr[wave]) // unr
    o = np.lexsort((own_u, batch, wave))
    same = (wave[o][1:] == wave[o][:-1]) & (batch[o][1:] == batch[o][:-1]) & (own_u[o][1:] == own_u[o][:-1]) & (own_u[o][1:] >= 0)
    return len(np.unique(np.stack([wave[o][1:][same], batch[o][1:][same]]), axis=1).T)
