"""Inputs of the WMF step tests, in ONE place: tests/test_wmf_gpu.py runs them on the device, tests/test_wmf_cpu.py checks
— in the reference alone — that every one of them is a fair test (few ill-conditioned elements, the clip exercised but
not dominant, the tables move) and that the tolerance T below is tied to them.

A case is a dict: R (CSC), U, V (float32), batches (list of item-id arrays), lu, lv, a, b, lr, k.  Cases whose user
count depends on the device take its compute-unit count (`cus`); the CPU tests use MI355X_CUS.

The user side of a step runs one of three implementations, chosen from ld = round_up(k, 32):
  lds      ld <= 96   wmf_user_step_lds_kernel       ws   ld == 128   wmf_user_step_ws_kernel
  unfused  ld >= 160  wmf_pred / wmf_fixup / wmf_grad_v / wmf_update_u
"""
import numpy as np
import scipy.sparse as sp

from oracle.wmf_oracle import WmfOracle

MI355X_CUS = 256

# T: the bound of |device - float64 oracle| on the elements the oracle does not flag as ill-conditioned (flagged ones are
# compared at 2 lr).  Rule: the largest error of the FLOAT32 oracle against the float64 oracle over the unflagged elements
# of all cases below, times 4 (the device sums in another order: MFMA k-pairs, split-K and dv_part float atomics,
# v_rcp_f32 / v_sqrt_f32 at 1 ulp in the wave-specialised sweep), rounded up to one significant digit.
# Measured (31 cases of at most 9 steps, up to 70 023 users): float32 oracle 3.1e-6 in U (k = 1024), 6.7e-6 in V (k = 64)
# ->  T = 3e-5 (at T = 1e-5 and 2e-5 the rule gives 3e-5 as well).  The device (MI355X): 2.5e-6 in U, 5.3e-6 in V; losses
# within 4.5e-6 (relative) of the float64 loss.  Largest flagged shares 1.6e-4 of U, 1.4e-3 of V; largest clipped shares 0.03 of
# dU, 0.22 of dV.  tests/test_wmf_cpu.py asserts float32-oracle error <= T / 4 for every case and that T follows the rule.
T = 3e-5


def path_of(k):
    ld = (k + 31) // 32 * 32
    return "lds" if ld <= 96 else "ws" if ld == 128 else "unfused"


def random_inputs(seed, nu, ni, k, std=0.2):
    """the generator of test_steps_match_oracle: nnz distinct cells with ratings 1..5, normal tables"""
    rs = np.random.RandomState(seed)
    nnz = min(nu * ni // 3, max(6000, 4 * nu))
    keys = rs.permutation(nu * ni)[:nnz]
    u, i = keys // ni, keys % ni
    R = sp.csc_matrix((rs.randint(1, 6, nnz).astype(np.float32), (u, i)), shape=(nu, ni))
    U = rs.normal(0, std, (nu, k)).astype(np.float32)
    V = rs.normal(0, std, (ni, k)).astype(np.float32)
    return rs, R, U, V


def legacy_case(nu, ni, k, bs):
    """test_steps_match_oracle's inputs (three shuffled epochs, a = 1, b = 0.01)"""
    rs, R, U, V = random_inputs(nu + k, nu, ni, k)
    batches = []
    for _ in range(3):
        perm = rs.permutation(ni)
        batches += [perm[s:s + bs] for s in range(0, ni, bs)]
    return dict(R=R, U=U, V=V, batches=batches, lu=0.02, lv=0.03, a=1.0, b=0.01, lr=0.005, k=k)


def _epochs(rs, ni, bs, steps):
    out = []
    while len(out) < steps:
        perm = rs.permutation(ni)
        out += [perm[s:s + bs] for s in range(0, ni, bs)]
    return out[:steps]


def k_edge_case(k, cus=MI355X_CUS):
    """300 users x 1 200 items, the k / ld boundaries of the dispatch.  The batches are shuffled epochs over the first 300
    items: the other rows of V stay untouched, and every touched row is touched two or three times — a row touched once
    moves by lr_t m / sqrt(v), which does not depend on the size of its gradient, so a wrong dV would show only its sign"""
    rs, R, U, V = random_inputs(1000 + k, 300, 1200, k, std=0.2 if k <= 256 else 0.1)
    return dict(R=R, U=U, V=V, batches=_epochs(rs, 300, 128, 8 if k <= 256 else 6), lu=0.02, lv=0.03, a=1.0, b=0.01, lr=0.005, k=k)


def scale_case(k, nu, ni=200, steps=6, a=0.03, b=0.001, seed=0):
    """tens of thousands of users: several user tiles per workgroup (fused paths), split-K chunks above the minimum
    (unfused); weights small enough that V's gradient, a sum over all users, is not clipped away"""
    rs, R, U, V = random_inputs(seed + nu + k, nu, ni, k)
    return dict(R=R, U=U, V=V, batches=_epochs(rs, ni, 128, steps), lu=0.02, lv=0.03, a=a, b=b, lr=0.005, k=k)


def lds_scale_users(cus, exact=False):
    """more user tiles than the LDS-fused kernel has workgroups (2 per CU): 35 tiles over -> per_wg = 2, a ragged last tile
    and trailing workgroups with no tile; `exact`: one user over one tile per workgroup"""
    return 128 * 2 * cus + (1 if exact else 128 * 35 + 7)


def batch_edge_case(k, b=0.01):
    """700 users x 300 items; item 0 rated by every user, items 1..5 empty, explicit zeros in items 6..9.  Batches: 127, 128,
    1 (a short batch after a full one), 2, only empty columns, a ragged last batch, the full column again"""
    rs, R, U, V = random_inputs(2000 + k, 700, 300, k)
    R = R.tolil()
    R[:, 0] = rs.randint(1, 6, (700, 1)).astype(np.float32)
    R[:, 1:6] = 0
    R = R.tocsc()
    R.eliminate_zeros()
    for it in range(6, 10):   # explicit zeros: stored entries that stay "unobserved"
        lo, hi = R.indptr[it], R.indptr[it + 1]
        R.data[lo:hi:3] = 0.0
    perm = rs.permutation(np.arange(6, 300))
    batches = [np.concatenate([[0], perm[:126]]), perm[100:228], perm[5:6], perm[[7, 250]], np.array([3, 1, 5, 2, 4]),
               np.concatenate([perm[200:290], [2, 0, 4]]), perm[:128], perm[128:165]]
    return dict(R=R, U=U, V=V, batches=batches, lu=0.02, lv=0.03, a=0.7, b=b, lr=0.005, k=k)


def fixup_pattern_matrix(rs, ni=140):
    """421 users (three 128-row tiles + 37 rows) x `ni` items; item c < 128 is column c of the first batch and holds
      tile 0: c % 11 entries (0, 1, 4, 5, 7, 8, 9, 10 among them), rows 0 and 127 included;
      tile 1: exactly 8 entries, first and last row included — 128 (every row) for c = 5;
      tile 2: 9 entries, the first on the tile's first row (the ninth entry after tile 1's eight);
      tile 3 (ragged): c % 3 entries, the last existing row first, then the tile's first row;
      explicit zeros at position c % 8 of tile 1's eight entries where c % 8 is 0, 3, 4 or 7 (the positions the two
      threads of a column split between them).  Items >= 128 are random columns.  Returns (data, indices, indptr) sorted."""
    nu = 421
    data, indices, indptr = [], [], [0]
    for c in range(ni):
        rows = []
        if c < 128:
            n0 = c % 11
            t0 = [0, 127][:n0] if c % 2 == 0 else [127, 0][:n0]
            t0 += list(rs.permutation(np.arange(1, 127))[:max(0, n0 - 2)])
            t1 = list(range(128, 256)) if c == 5 else [128, 255] + list(128 + rs.permutation(np.arange(1, 127))[:6])
            t2 = [256] + list(256 + rs.permutation(np.arange(1, 128))[:8])
            t3 = [420, 384][:c % 3]
            rows = sorted(t0) + sorted(t1) + sorted(t2) + sorted(t3)
            vals = rs.randint(1, 6, len(rows)).astype(np.float32)
            if c != 5 and c % 8 in (0, 3, 4, 7):
                vals[len(t0) + c % 8] = 0.0
        else:
            rows = sorted(rs.permutation(nu)[:rs.randint(0, 40)])
            vals = rs.randint(1, 6, len(rows)).astype(np.float32)
        data += list(vals)
        indices += list(rows)
        indptr.append(len(indices))
    return np.array(data, np.float32), np.array(indices, np.int32), np.array(indptr, np.int64)


def fixup_pattern_case(k, unsorted=False):
    """the hand-built count edges of the wave-specialised fix-up (8 prefetched entries per column and tile, two threads a
    column), the same matrix on the other two paths; `unsorted`: the rows of every column handed over in shuffled order"""
    rs = np.random.RandomState(77)
    data, indices, indptr = fixup_pattern_matrix(rs)
    nu, ni = 421, len(indptr) - 1
    if unsorted:
        ps = np.random.RandomState(5)
        for c in range(ni):
            p = ps.permutation(indptr[c + 1] - indptr[c]) + indptr[c]
            data[indptr[c]:indptr[c + 1]], indices[indptr[c]:indptr[c + 1]] = data[p], indices[p]
    R = sp.csc_matrix((data, indices, indptr), shape=(nu, ni))   # (this constructor keeps the order it is given)
    U = rs.normal(0, 0.2, (nu, k)).astype(np.float32)
    V = rs.normal(0, 0.2, (ni, k)).astype(np.float32)
    first = np.arange(128)
    batches = [first, np.arange(128, ni), first[::-1].copy(), np.concatenate([np.arange(100, ni), [5]]), first, first[:77]]
    return dict(R=R, U=U, V=V, batches=batches, lu=0.02, lv=0.03, a=0.6, b=0.01, lr=0.005, k=k)


def model_case(k):
    """cornac_amd.WMF on conftest.synth_dataset with init_params: the batches are the model's own item_iter order"""
    from conftest import synth_dataset

    ds = synth_dataset(400, 300, 9000, seed=11)
    rs = np.random.RandomState(k)
    U = rs.normal(0, 0.2, (ds.num_users, k)).astype(np.float32)
    V = rs.normal(0, 0.2, (ds.num_items, k)).astype(np.float32)
    kw = dict(k=k, lambda_u=0.02, lambda_v=0.03, a=0.6, b=0.01, learning_rate=0.005, batch_size=100, max_iter=3)
    batches = [np.asarray(x) for _ in range(kw["max_iter"]) for x in ds.item_iter(kw["batch_size"], shuffle=True)]
    return dict(R=ds.csc_matrix, U=U, V=V, batches=batches, lu=0.02, lv=0.03, a=0.6, b=0.01, lr=0.005, k=k, model_kw=kw,
                dataset=lambda: synth_dataset(400, 300, 9000, seed=11))


K_EDGES = (1, 31, 32, 33, 64, 65, 80, 96, 97, 128, 129, 160, 200, 256, 257, 1024)

# every case the device is compared on at T: name -> builder(cus)
CASES = {}
for _k in K_EDGES:
    CASES["k%d" % _k] = lambda cus, k=_k: k_edge_case(k)
CASES.update({
    "lds_scale_k96": lambda cus: scale_case(96, lds_scale_users(cus)),
    "lds_scale_k40": lambda cus: scale_case(40, lds_scale_users(cus)),
    "lds_scale_exact_k96": lambda cus: scale_case(96, lds_scale_users(cus, exact=True), steps=3),
    "unfused_scale_k200": lambda cus: scale_case(200, 70000),                   # chunk 144, 487 K-chunks, the last of 16 users
    "unfused_scale_chunk_plus_one_k200": lambda cus: scale_case(200, 32 * 300 + 1, a=0.06, b=0.002),   # chunk 32, 300 chunks + 1 user
    "unfused_b0_k200": lambda cus: batch_edge_case(200, b=0.0),
})
for _k in (80, 128, 200):
    CASES["batch_edges_k%d" % _k] = lambda cus, k=_k: batch_edge_case(k)
    CASES["fixup_pattern_k%d" % (96 if _k == 80 else _k)] = lambda cus, k=(96 if _k == 80 else _k): fixup_pattern_case(k)
CASES["fixup_pattern_unsorted_k128"] = lambda cus: fixup_pattern_case(128, unsorted=True)
CASES["model_k80"] = lambda cus: model_case(80)
CASES["model_k200"] = lambda cus: model_case(200)

# cases above 60 000 users: the float64 oracle takes seconds on each
BIG = ("lds_scale_k96", "lds_scale_k40", "lds_scale_exact_k96", "unfused_scale_k200")


def run_oracle(case, dtype=np.float64, cls=WmfOracle):
    o = cls(case["U"], case["V"], case["R"], case["lu"], case["lv"], case["a"], case["b"], case["lr"], dtype=dtype)
    losses = np.array(o.fit_batches(case["batches"]))
    return o, losses


def compare(o, U, V, lr, what=""):
    """|U - o.U|, |V - o.V| against the float64 oracle `o`: T on the unflagged elements, 2 lr on the flagged ones (NaN fails
    both).  Returns the largest unflagged errors (U, V) after asserting."""
    worst = []
    for name, got, want, flag in (("U", U, o.U, o.flagged(T)[0]), ("V", V, o.V, o.flagged(T)[1])):
        err = np.abs(got.astype(np.float64) - want)
        assert np.isfinite(got).all(), "%s %s: non-finite values" % (what, name)
        e_un = float(err[~flag].max()) if (~flag).any() else 0.0
        e_fl = float(err[flag].max()) if flag.any() else 0.0
        print("%s %s: unflagged max err %.3g (T = %g), flagged %d of %d, max err %.3g" % (what, name, e_un, T, flag.sum(),
                                                                                          flag.size, e_fl))
        assert e_un <= T, "%s %s: %g over T = %g on an unflagged element" % (what, name, e_un, T)
        assert e_fl <= 2 * lr, "%s %s: %g over 2 lr on a flagged element" % (what, name, e_fl)
        worst.append(e_un)
    return worst
