"""The float64 VBPR reference (oracle/vbpr_oracle.py:steps_f64) pinned on the CPU, and the cases the device tests of
tests/test_vbpr_gpu.py run against it: the shape matrix (SHAPES), the hand-written row schedule (SCHEDULE) and the
float32 drift that the device tolerance rests on."""
import numpy as np
import pytest

from oracle.vbpr_oracle import TABLES, steps_f64
from test_oracle_golden import _vbpr_case

# the device tests' bound on every table (A-C of tests/test_vbpr_gpu.py): 7-20 x the float32 drift measured below
DEVICE_TOL = 2e-5
LR, LW, LB, LE = 0.01, 0.01, 0.01, 1e-3

# name: (n_users, n_items, n_feat, k, k2, batch_size, n_total) — and the device path each case is there for
SHAPES = {
    # 1 x 1 objective; scalar sweep (width 1); n_feat < one K tile; scalar feature paths; 256 item-table slices
    "b1_k1": (50, 40, 5, 1, 1, 1, 9),
    # second N tile of the proj GEMM (k2 > 128); fpb 7; K tail; scalar features; ragged last batch (10).  (B > 128 at
    # k2 = 129 does not pass the feature-gradient LDS check: the second M tile is the b513 case's)
    "k2_129": (300, 200, 4095, 3, 129, 117, 1180),
    # score lane loop twice (k > 64); fpb 8 x 128 = 1024 feat-Adam outputs; ragged (50)
    "k65_k2_127": (200, 150, 64, 65, 127, 100, 950),
    # vectorised sweep with 3 units per row (64-bit division); fpb 4 x 256 = 1024 outputs; ragged (51)
    "k12_k2_255": (100, 80, 256, 12, 255, 61, 600),
    # kMaxK2 at the largest batch the LDS check accepts; ragged (1)
    "k2_256_b61": (100, 80, 128, 64, 256, 61, 610),
    # second pass of the pair-scatter loop over a (B > 256); 5 M tiles of the proj GEMM; ragged (383)
    "b513": (120, 90, 20, 4, 3, 513, 5000),
    # tables much larger than a batch: sweep-dominated, sparse recurrence
    "sparse_50k": (2000, 50000, 16, 8, 10, 100, 1200),
    # item tables above 64 KB of LDS; 5000-feature gather slices
    "nfeat_20k": (1000, 300, 20000, 16, 10, 16, 160),
}


def xavier(shape, rs):
    limit = np.sqrt(3.0) * np.sqrt(2.0 / np.sum(shape))
    return rs.uniform(-limit, limit, shape).astype(np.float32)


def random_params(n_users, n_items, n_feat, k, k2, rs):
    return {"Bi": rs.normal(0, 0.1, n_items).astype(np.float32), "Gu": xavier((n_users, k), rs),
            "Gi": xavier((n_items, k), rs), "Tu": xavier((n_users, k2), rs), "E": xavier((n_feat, k2), rs),
            "Bp": xavier((n_feat, 1), rs).ravel()}


def split(u, i, j, batch_size):
    return [(u[a:a + batch_size], i[a:a + batch_size], j[a:a + batch_size]) for a in range(0, len(u), batch_size)]


def shape_case(name, seed=0):
    """features, initial tables and uniformly drawn triplets (i != j) of one SHAPES case"""
    nu, ni, nf, k, k2, B, n = SHAPES[name]
    rs = np.random.RandomState(seed)
    F = rs.uniform(0, 1, (ni, nf)).astype(np.float32)
    P = random_params(nu, ni, nf, k, k2, rs)
    u = rs.randint(0, nu, n).astype(np.int32)
    i = rs.randint(0, ni, n).astype(np.int32)
    j = ((i + 1 + rs.randint(0, ni - 1, n)) % ni).astype(np.int32)
    return dict(F=F, P=P, u=u, i=i, j=j, batch_size=B, batches=split(u, i, j, B), dims=(nu, ni, nf, k, k2))


# the row schedule: 6 users, 10 items, batch 4, 14 steps, written by hand (tests/test_vbpr_gpu.py, case B).  User 0 is in
# every batch, user 1 recurs at gaps of 1, 2, 3 and 4 steps, item 8 is only in the first batch, item 2 is i in batch 4
# and j in batch 5, user 2 is three of batch 7's four triplets, (3, 4, 4) is an i == j triplet, the last batch is
# ragged, and user 5 / item 9 are never touched
SCHEDULE = [
    [(0, 0, 8), (1, 1, 2), (3, 3, 4), (4, 5, 6)],
    [(0, 1, 3), (1, 0, 5), (4, 6, 7), (3, 2, 0)],
    [(0, 4, 6), (3, 7, 1), (4, 0, 3), (2, 5, 2)],
    [(0, 2, 7), (1, 3, 6), (2, 1, 4), (4, 7, 5)],
    [(0, 2, 5), (3, 6, 0), (4, 1, 7), (2, 3, 4)],
    [(0, 7, 2), (2, 0, 6), (3, 4, 1), (4, 5, 3)],
    [(0, 3, 0), (1, 6, 4), (4, 7, 1), (3, 5, 0)],
    [(2, 1, 0), (2, 4, 5), (2, 6, 3), (0, 7, 6)],
    [(0, 0, 1), (3, 2, 3), (4, 4, 6), (3, 5, 7)],
    [(0, 6, 2), (3, 4, 4), (4, 1, 5), (2, 7, 3)],
    [(0, 5, 1), (1, 2, 6), (4, 3, 0), (3, 7, 4)],
    [(0, 0, 7), (2, 6, 1), (4, 2, 5), (3, 3, 4)],
    [(0, 4, 2), (3, 1, 6), (4, 5, 0), (2, 7, 3)],
    [(0, 3, 5), (4, 6, 1)],
]
SCHEDULE_DIMS = (6, 10, 8, 4, 3)  # n_users, n_items, n_feat, k, k2
SCHEDULE_BATCH = 4


def schedule_case(seed=3):
    nu, ni, nf, k, k2 = SCHEDULE_DIMS
    rs = np.random.RandomState(seed)
    F = rs.uniform(0, 1, (ni, nf)).astype(np.float32)
    P = random_params(nu, ni, nf, k, k2, rs)
    u, i, j = (np.array([t[c] for b in SCHEDULE for t in b], np.int32) for c in range(3))
    return dict(F=F, P=P, u=u, i=i, j=j, batch_size=SCHEDULE_BATCH, batches=split(u, i, j, SCHEDULE_BATCH),
                dims=SCHEDULE_DIMS)


def row_sets(batches):
    """per batch: the users and the items it touches"""
    return [(set(u.tolist()), set(i.tolist()) | set(j.tolist())) for u, i, j in batches]


def schedule_classes(batches, n_users, n_items):
    """the row classes the schedule test needs, derived from the batches (so an edit cannot silently drop one)"""
    sets = row_sets(batches)
    n = len(batches)
    users_in = [[t for t in range(n) if r in sets[t][0]] for r in range(n_users)]
    items_in = [[t for t in range(n) if r in sets[t][1]] for r in range(n_items)]
    gaps = set()
    for ts in users_in + items_in:
        gaps |= set(np.diff(ts).tolist())
    return {
        "in every batch": [r for r, ts in enumerate(users_in + items_in) if len(ts) == n],
        "gaps 1-4": sorted(g for g in gaps if g <= 4),
        "first batch only": [r for r, ts in enumerate(users_in + items_in) if ts == [0]],
        "i at t, j at t+1": [int(r) for t in range(n - 1)
                             for r in set(batches[t][1].tolist()) & set(batches[t + 1][2].tolist())],
        "user 3x in a batch": [t for t, (u, _, _) in enumerate(batches) if np.bincount(u).max() >= 3],
        "i == j": [t for t, (_, i, j) in enumerate(batches) if (i == j).any()],
        "ragged last": [n - 1] if len(batches[-1][0]) < len(batches[0][0]) else [],
        "untouched users": [r for r, ts in enumerate(users_in) if not ts],
        "untouched items": [r for r, ts in enumerate(items_in) if not ts],
    }


def lookahead_rows(batches):
    """(table, row, t) for rows of batch t + 1 that batch t does not touch but an earlier batch did: their step-t update
    is the device's gradient-free look-ahead update, and their moments are non-zero so that it moves them"""
    sets = row_sets(batches)
    out = []
    for t in range(1, len(batches) - 1):
        seen_u = set().union(*(s[0] for s in sets[:t]))
        seen_i = set().union(*(s[1] for s in sets[:t]))
        out += [("Gu", r, t) for r in sorted((sets[t + 1][0] - sets[t][0]) & seen_u)]
        out += [("Gi", r, t) for r in sorted((sets[t + 1][1] - sets[t][1]) & seen_i)]
    return out


def torch_adam_steps(features, params, batches, lr, lambda_w, lambda_b, lambda_e, dtype):
    """the same steps with torch.optim.Adam in `dtype` (VBPROracle.fit's body over explicit batches)"""
    import torch

    F = torch.tensor(np.asarray(features), dtype=dtype)
    P = {n: torch.tensor(np.asarray(params[n], np.float64).reshape(-1, 1) if n == "Bp" else np.asarray(params[n]),
                         dtype=dtype, requires_grad=True) for n in TABLES}
    Bi, Gu, Gi, Tu, E, Bp = (P[n] for n in TABLES)
    opt = torch.optim.Adam([P[n] for n in TABLES], lr=lr)

    def l2(*ts):
        return sum(t.pow(2).sum() for t in ts) / 2

    nll = []
    for u, i, j in batches:
        bu, bi, bj = (torch.as_tensor(np.asarray(x, np.int64)) for x in (u, i, j))
        gu, tu = Gu[bu], Tu[bu]
        beta_i, beta_j = Bi[bi], Bi[bj]
        gi, gj = Gi[bi], Gi[bj]
        feat_diff = F[bi] - F[bj]
        X = (beta_i - beta_j + (gu * (gi - gj)).sum(dim=1) + (tu * feat_diff.mm(E)).sum(dim=1) + feat_diff.mm(Bp))
        ll = torch.nn.functional.logsigmoid(X).sum()
        loss = -ll + (l2(gu, gi, gj, tu) * lambda_w + l2(beta_i) * lambda_b + l2(beta_j) * lambda_b / 10
                      + l2(E, Bp) * lambda_e)
        opt.zero_grad()
        loss.backward()
        opt.step()
        nll.append(-float(ll.detach()))
    return {n: P[n].detach().numpy().reshape(-1) if n == "Bp" else P[n].detach().numpy() for n in TABLES}, nll


def max_err(a, b):
    return max(float(np.abs(np.asarray(a[n], np.float64).reshape(-1) - np.asarray(b[n], np.float64).reshape(-1)).max())
               for n in TABLES)


def test_steps_f64_reproduces_the_reference_golden():
    """the batches VBPROracle draws for vbpr_small, run through the float64 steps: within 1e-4 of what the real
    reference learned in float32"""
    from oracle.vbpr_oracle import VBPROracle

    fx, ds, kw = _vbpr_case()
    o = VBPROracle(**kw)
    F = np.asarray(ds.item_image.features[: len(ds.iid_map)], np.float32)
    o.init(len(ds.uid_map), len(ds.iid_map), F)
    init = {"Bi": o.beta_item, "Gu": o.gamma_user, "Gi": o.gamma_item, "Tu": o.theta_user, "E": o.emb_matrix,
            "Bp": o.beta_prime}
    o.fit(ds, record_batches=True)
    assert len(o.batches) == kw["n_epochs"] * -(-len(fx["users"]) // kw["batch_size"])
    got, nll = steps_f64(F, init, o.batches, kw["learning_rate"], kw["lambda_w"], kw["lambda_b"], kw["lambda_e"])
    for n in TABLES:
        err = np.abs(got[n].reshape(-1) - fx[n].astype(np.float64).reshape(-1)).max()
        assert err <= 1e-4, (n, err)
    assert len(nll) == len(o.batches) and np.all(np.isfinite(nll))


def test_steps_f64_adam_matches_torch_optim_adam():
    """ragged batches of varying sizes with duplicate users and items and one i == j triplet: the hand-written dense
    Adam is torch.optim.Adam in float64 (to 1e-12), NLL included"""
    rs = np.random.RandomState(11)
    nu, ni, nf, k, k2 = 7, 9, 13, 3, 5
    F = rs.uniform(0, 1, (ni, nf))
    P = random_params(nu, ni, nf, k, k2, rs)
    batches = []
    for n in (5, 1, 8, 3, 6, 2, 7):
        u = rs.randint(0, 4, n)
        i = rs.randint(0, 6, n)
        j = (i + 1 + rs.randint(0, 5, n)) % 6
        batches.append((u, i, j))
    u, i, j = batches[3]
    j[1] = i[1]  # the i == j triplet
    assert any(np.bincount(b[0]).max() > 1 for b in batches) and any(np.bincount(b[1]).max() > 1 for b in batches)
    got, nll = steps_f64(F, P, batches, 0.02, 0.03, 0.02, 0.005)
    want, want_nll = torch_adam_steps(F, P, batches, 0.02, 0.03, 0.02, 0.005, dtype=__import__("torch").float64)
    assert max_err(got, want) <= 1e-12
    assert np.allclose(nll, want_nll, rtol=1e-12, atol=0)
    # untouched rows (user >= 4, item >= 6) never move: m = v = 0 leaves p exactly where it was
    assert np.array_equal(got["Gu"][4:], P["Gu"][4:].astype(np.float64))
    assert np.array_equal(got["Gi"][6:], P["Gi"][6:].astype(np.float64))


def _drift_cases():
    return [("shape", n) for n in SHAPES] + [("schedule", None)]


@pytest.mark.parametrize("kind,name", _drift_cases())
def test_float32_drift_of_the_device_cases(kind, name):
    """the device cases' data through torch's float32 step (autograd + torch.optim.Adam, what the reference runs): within
    1e-5 of the float64 steps on every table, NLL within rtol 1e-6 — the float32 drift the device's 2e-5 rests on; and
    every table moves by more than 1e-3, so the device comparison is not one of unmoved tables"""
    import torch

    c = shape_case(name) if kind == "shape" else schedule_case()
    want, want_nll = steps_f64(c["F"], c["P"], c["batches"], LR, LW, LB, LE)
    got, nll = torch_adam_steps(c["F"], c["P"], c["batches"], LR, LW, LB, LE, dtype=torch.float32)
    assert max_err(got, want) <= 1e-5, max_err(got, want)
    assert np.allclose(nll, want_nll, rtol=1e-6, atol=0)
    for n in TABLES:
        assert np.abs(want[n].reshape(-1) - np.asarray(c["P"][n], np.float64).reshape(-1)).max() >= 1e-3, n


@pytest.mark.parametrize("kind,name", [("schedule", None), ("shape", "k65_k2_127"), ("shape", "b513")])
def test_a_withheld_lookahead_update_is_visible(kind, name):
    """withholding ONE gradient-free update of one look-ahead row (in batch t + 1, not in batch t, touched before)
    shifts the result by at least 10 x the device tolerance: a device that missed or doubled it would fail"""
    c = shape_case(name) if kind == "shape" else schedule_case()
    base, _ = steps_f64(c["F"], c["P"], c["batches"], LR, LW, LB, LE)
    rows = lookahead_rows(c["batches"])
    tables = sorted({r[0] for r in rows})  # (every item of the b513 case is in every batch: users only)
    assert tables == (["Gu"] if name == "b513" else ["Gi", "Gu"])
    for table in tables:
        skip = next(r for r in rows if r[0] == table)
        got, _ = steps_f64(c["F"], c["P"], c["batches"], LR, LW, LB, LE, skip=skip)
        assert max_err(got, base) >= 10 * DEVICE_TOL, (skip, max_err(got, base))


def test_schedule_has_every_row_class():
    """the hand-written schedule holds every row class the device test is for"""
    c = schedule_case()
    nu, ni = SCHEDULE_DIMS[:2]
    classes = schedule_classes(c["batches"], nu, ni)
    assert classes["gaps 1-4"] == [1, 2, 3, 4]
    for name, rows in classes.items():
        assert rows, name
    assert len(c["batches"]) >= 13 and all(len(b[0]) == SCHEDULE_BATCH for b in c["batches"][:-1])
