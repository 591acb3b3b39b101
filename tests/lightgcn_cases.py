"""The LightGCN checks' reference, inputs and tolerances, in ONE place: tests/test_lightgcn_cpu.py holds the float64 restatement
below against the golden that the reference's own lightgcn.Model, construct_graph and LightGCN.fit wrote
(tests/golden/make_lightgcn_golden.py, over the DGL stand-in of tests/golden/dgl_shim), tests/test_lightgcn_gpu.py holds the
device against the restatement and against the same golden.

`Restatement` restates one step of cornac/models/lightgcn/recom_lightgcn.py:168-179 in float64 NumPy / SciPy with the
gradients written out by hand (no autograd): E = P(E0) with P = 1 / (L + 1) sum_k A^k over the normalised adjacency A (its
weights are the reference's float32 values, lightgcn.py:31-39), the BPR loss with torch's softplus, the gradient rows
    da = (s (n - p) + lambda a) / B,  dp = (-s a + lambda p) / B,  dn = (s a + lambda n) / B,   s = sigmoid(<a, n> - <a, p>)
summed per node, dL/dE0 = P(G) because P is linear and symmetric, and torch's dense Adam over both tables.

Cases pass explicit graphs, batches and tables, drawn from numpy.random.RandomState and never from torch.  In every case
user 0 appears in the first step only, in every step of five triplets or more a third of the positives are item 1, and in
every step of two triplets or more some item is a positive and a negative (a case of one-triplet steps ends with a triplet
whose positive is its negative).  Nodes without edges are the
LAST users and items; no batch names such a user, and the d8 case draws its isolated item as a negative.

Tolerance of the device against the restatement, per table (E0_user, E0_item, Adam's m and v of each): NCF's rule unchanged,
    max(16 * d_ref, 4 units in the last float32 place of max|table|)
where d_ref = max|reference float32 - restatement| is read from the golden.  For the two parameter tables that tolerance must
stay under 1 % of the table's recorded movement (`check_condition`); a row that the restatement leaves exactly in place is
compared bit for bit."""
import numpy as np
import scipy.sparse as sp

from ncf_cases import tolerance, ulp32  # noqa: F401  (the rule itself: one definition)

PIECE = 512           # the device's piece length (_lib.LightGcnModel.PIECE); the hub case is sized against it
TABLES = ("user", "item")
N_SCORE_USERS = 5


def _c(nu, ni, d, L, steps, iso_u=0, iso_i=0, lam=1e-4, lr=1e-3, seed=0, density=0.2, hub=False):
    assert len(steps) >= 3
    return dict(nu=nu, ni=ni, d=d, L=L, steps=tuple(steps), iso_u=iso_u, iso_i=iso_i, lam=lam, lr=lr, seed=seed, density=density, hub=hub)


# nu x ni: the connected part; iso_u / iso_i: users / items without edges, appended
CASES = {
    "d1": _c(5, 7, 1, 1, (1, 1, 1), seed=1, density=0.4),
    "d8": _c(11, 9, 8, 3, (5, 5, 5), iso_u=2, iso_i=1, seed=2, density=0.3),
    "d33": _c(37, 29, 33, 2, (64, 64, 17), seed=3),
    "d64": _c(37, 29, 64, 3, (65, 65, 30), iso_u=3, iso_i=2, seed=4),
    "d65": _c(300, 200, 65, 3, (1024, 1024, 500), seed=5, density=0.05),
    "d256": _c(37, 29, 256, 1, (64, 64, 5), seed=6),
    "l0": _c(37, 29, 8, 0, (64, 64, 17), seed=7),
    "l4reg": _c(300, 200, 64, 4, (1024, 1024, 500), lam=1e-2, seed=8, density=0.05),
    "lam0": _c(37, 29, 33, 2, (64, 64, 17), lam=0.0, seed=9),
    # item 0 is held by every one of the 1 100 users: its row spans three pieces of 512 edges
    "hub": _c(1100, 40, 16, 3, (256, 256, 100), seed=10, density=0.08, hub=True),
}
FULL_CASES = ("d8", "d64", "hub", "l4reg")   # the golden holds tables, state, losses, final embeddings and scores for these
RANK_CASE = "d64"                            # the users' top scores are distinct (checked on the CPU)
REPEAT_CASES = ("hub", "d65")
# the reference's own seeded fit (its initial draws, its sampler over a Dataset built with a seed)
SEEDED = {"seeded": dict(nu=23, ni=19, d=5, L=2, bs=16, epochs=3, lr=0.01, lam=1e-4, seed=11)}


def totals(c):
    return c["nu"] + c.get("iso_u", 0), c["ni"] + c.get("iso_i", 0)


def case_graph(c):
    """the train matrix over all users x all items (CSR, sorted indices, values 1): every connected user and item has an edge"""
    rs = np.random.RandomState(1000 + c["seed"])
    nu, ni = c["nu"], c["ni"]
    held = rs.rand(nu, ni) < c["density"]
    held[np.arange(nu), rs.randint(0, ni, nu)] = True
    held[rs.randint(0, nu, ni), np.arange(ni)] = True
    if c["hub"]:
        held[:, 0] = True
    tu, ti = totals(c)
    u, i = np.nonzero(held)
    X = sp.csr_matrix((np.ones(len(u)), (u, i)), shape=(tu, ti))
    X.sort_indices()
    return X


def case_batches(c):
    """the steps' (users, positives, negatives)"""
    rs = np.random.RandomState(4000 + c["seed"])
    nu, ni, out = c["nu"], c["ni"], []
    ti = totals(c)[1]
    for s, n in enumerate(c["steps"]):
        users = rs.randint(0 if s == 0 else 1, nu, n)   # connected users only
        if s == 0:
            users[0] = 0   # user 0: the first step only
        pos, neg = rs.randint(0, ni, n), rs.randint(0, ti, n)
        if n >= 5:
            pos[rs.permutation(n)[:-(-n // 3)]] = 1
        if c["iso_i"] and n >= 2:
            neg[1] = ti - 1            # an item without edges as a negative
        if n >= 2 or s == len(c["steps"]) - 1:
            neg[n - 1] = pos[0]        # an item that is a positive and a negative in one step
        out.append((users.astype(np.int64), pos.astype(np.int64), neg.astype(np.int64)))
    return out


def epoch_arrays(batches):
    """(step_ptr, users, pos, neg) as fit_epoch takes an epoch"""
    ptr = np.concatenate([[0], np.cumsum([len(b[0]) for b in batches])]).astype(np.int64)
    return (ptr,) + tuple(np.concatenate([b[q] for b in batches]) for q in range(3))


def case_params(c):
    """float32 layer-0 tables (user, item), uniform within xavier_uniform_'s bound for their shapes"""
    rs = np.random.RandomState(2000 + c["seed"])
    tu, ti = totals(c)
    return tuple((rs.uniform(-1.0, 1.0, (n, c["d"])) * np.sqrt(6.0 / (n + c["d"]))).astype(np.float32) for n in (tu, ti))


def score_users(c):
    return np.unique(np.linspace(0, c["nu"] - 1, N_SCORE_USERS).astype(np.int64))


# ---- the restatement -------------------------------------------------------------------------------------------------------
def edge_weights(X):
    """lightgcn.py:31-39 per stored entry of the CSR X: float32(pow(float32(deg_u) * float32(deg_i), -0.5))"""
    X = sp.csr_matrix(X)
    du = np.diff(X.indptr).astype(np.float32)
    di = np.bincount(X.indices, minlength=X.shape[1]).astype(np.float32)
    prod = (du.repeat(np.diff(X.indptr)) * di[X.indices]).astype(np.float32)
    return np.power(prod.astype(np.float64), -0.5).astype(np.float32)


def adjacency(X):
    """A = [[0, R], [R^T, 0]] over users then items, float64 holding the float32 weights"""
    X = sp.csr_matrix(X)
    X.sort_indices()
    R = sp.csr_matrix((edge_weights(X).astype(np.float64), X.indices, X.indptr), shape=X.shape)
    return sp.bmat([[None, R], [R.T, None]], format="csr")


class Restatement:
    """the layer-0 tables W [users | items], Adam's M and V and the step counter t, all float64 / int; `step` is one batch"""

    def __init__(self, X, d, L, user=None, item=None):
        self.nu, self.ni = (int(x) for x in X.shape)
        self.d, self.L = int(d), int(L)
        self.A = adjacency(X)
        n = self.nu + self.ni
        self.W, self.M, self.V = np.zeros((n, self.d)), np.zeros((n, self.d)), np.zeros((n, self.d))
        self.t = 0
        self.set_params(user, item)

    def set_params(self, user=None, item=None):
        if user is not None:
            assert np.shape(user) == (self.nu, self.d)
            self.W[:self.nu] = np.array(user, np.float64)
        if item is not None:
            assert np.shape(item) == (self.ni, self.d)
            self.W[self.nu:] = np.array(item, np.float64)

    def P(self, T):
        """1 / (L + 1) sum_{k = 0..L} A^k T"""
        total, h = T.copy(), T
        for _ in range(self.L):
            h = self.A @ h
            total = total + h
        return total / (self.L + 1)

    def losses(self, E, users, pos, neg, lam):
        a, p, n = E[users], E[self.nu + pos], E[self.nu + neg]
        x = (a * n).sum(1) - (a * p).sum(1)
        bpr = float(np.mean(np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))))
        reg = float(0.5 * ((a * a).sum() + (p * p).sum() + (n * n).sum()) / len(users))
        return bpr + lam * reg, bpr, reg

    def gradient(self, E, users, pos, neg, lam):
        """dL/dE, zero outside the batch's rows"""
        a, p, n = E[users], E[self.nu + pos], E[self.nu + neg]
        B = len(users)
        s = 1.0 / (1.0 + np.exp(-((a * n).sum(1) - (a * p).sum(1))))[:, None]
        G = np.zeros_like(E)
        np.add.at(G, users, (s * (n - p) + lam * a) / B)
        np.add.at(G, self.nu + pos, (-s * a + lam * p) / B)
        np.add.at(G, self.nu + neg, (s * a + lam * n) / B)
        return G

    def step(self, users, pos, neg, lr, lam):
        """one batch; returns (loss, bpr, reg)"""
        users, pos, neg = (np.asarray(x, np.int64) for x in (users, pos, neg))
        E = self.P(self.W)
        out = self.losses(E, users, pos, neg, lam)
        g = self.P(self.gradient(E, users, pos, neg, lam))
        self.t += 1
        b1, b2 = 0.9, 0.999
        self.M = b1 * self.M + (1 - b1) * g
        self.V = b2 * self.V + (1 - b2) * g ** 2
        self.W = self.W - lr / (1 - b1 ** self.t) * self.M / (np.sqrt(self.V) / np.sqrt(1 - b2 ** self.t) + 1e-8)
        return out

    def fit_epoch(self, step_ptr, users, pos, neg, lr, lam):
        out = np.array([self.step(users[a:b], pos[a:b], neg[a:b], lr, lam) for a, b in zip(step_ptr[:-1], step_ptr[1:])])
        return out[:, 0], out[:, 1], out[:, 2]

    def tables(self, T=None):
        T = self.W if T is None else T
        return T[:self.nu], T[self.nu:]

    def final(self):
        return self.tables(self.P(self.W))


def new_restatement(c, params=None):
    user, item = params if params is not None else (None, None)
    return Restatement(case_graph(c), c["d"], c["L"], user, item)


_RUNS = {}


def run_case(name):
    """the restatement over the whole case, computed once: dict(r: the Restatement after the last step, losses [steps x 3], init)"""
    if name not in _RUNS:
        c = CASES[name]
        init = case_params(c)
        r = new_restatement(c, init)
        losses = np.array([r.step(u, i, j, c["lr"], c["lam"]) for u, i, j in case_batches(c)])
        _RUNS[name] = dict(r=r, losses=losses, init=init)
    return _RUNS[name]


def still_rows(name):
    """per table: the rows that the restatement leaves exactly in place (no gradient ever reaches them)"""
    run = run_case(name)
    return tuple(np.flatnonzero((np.asarray(a, np.float64) == b).all(axis=1)) for a, b in zip(run["init"], run["r"].tables()))


# ---- tolerances ------------------------------------------------------------------------------------------------------------
def check_condition(golden, name):
    """for the two parameter tables the device's tolerance stays under 1 % of the recorded movement.  Returns the worst share."""
    worst = 0.0
    for q, n in enumerate(TABLES):
        d_ref, move, top = (float(golden["%s/%s" % (name, kind)][q]) for kind in ("d_ref", "move", "max"))
        assert move > 0.0, (name, n)
        tol = tolerance(d_ref, top)
        worst = max(worst, tol / move)
        assert tol < 0.01 * move, "%s %s: tolerance %.3g is not under 1 %% of the movement %.3g" % (name, n, tol, move)
    return worst


def loss_tolerance(golden, name, top):
    return max(16.0 * float(golden[name + "/d_ref_loss"]), 4.0 * ulp32(float(top)))


# ---- the seeded case ---------------------------------------------------------------------------------------------------------
def seeded_triplets(c):
    """(users, items, ratings) of the seeded case's data: every user and item at least once, ratings 1..5"""
    rs = np.random.RandomState(7000 + c["seed"])
    held = rs.rand(c["nu"], c["ni"]) < 0.25
    held[np.arange(c["nu"]), rs.randint(0, c["ni"], c["nu"])] = True
    held[rs.randint(0, c["nu"], c["ni"]), np.arange(c["ni"])] = True
    u, i = np.nonzero(held)
    order = rs.permutation(len(u))
    return u[order].astype(np.int64), i[order].astype(np.int64), rs.randint(1, 6, len(u)).astype(np.float64)


def seeded_model(c, **over):
    import cornac_amd

    kw = dict(emb_size=c["d"], num_epochs=c["epochs"], learning_rate=c["lr"], batch_size=c["bs"], num_layers=c["L"], lambda_reg=c["lam"],
              seed=c["seed"], verbose=False)
    kw.update(over)
    return cornac_amd.LightGCN(**kw)


def seeded_dataset(c):
    """the seeded case's data as this project's Dataset, built as the golden's generator builds the reference's"""
    from collections import OrderedDict

    from cornac_amd import Dataset

    u, i, r = seeded_triplets(c)
    return Dataset.build(list(zip(u.tolist(), i.tolist(), r.tolist())), seed=c["seed"],
                         global_uid_map=OrderedDict((n, n) for n in range(c["nu"])),
                         global_iid_map=OrderedDict((n, n) for n in range(c["ni"])))


# ---- a device double ---------------------------------------------------------------------------------------------------------
class FakeLightGcnModel:
    """_lib.LightGcnModel served by the restatement (float32 in, float32 out); counts what was built"""
    PIECE, MAX_STEP, NAMES = PIECE, 16384, TABLES
    built = 0
    last = None

    def __init__(self, X, emb_size=64, num_layers=3, device=0):
        assert sp.issparse(X)
        self.X = sp.csr_matrix(X)
        assert self.X.has_sorted_indices
        self.n_users, self.n_items = (int(x) for x in X.shape)
        self.emb_size, self.num_layers = int(emb_size), int(num_layers)
        self.nnz = int(self.X.nnz)
        self.r = Restatement(self.X, emb_size, num_layers)
        self.device, self.closed, self.epochs, self.propagated = device, False, [], 0
        FakeLightGcnModel.built += 1
        FakeLightGcnModel.last = self

    def set_params(self, user=None, item=None):
        if not hasattr(self, "initial"):
            self.initial = (np.array(user, np.float32), np.array(item, np.float32))
        self.r.set_params(user, item)

    def get_params(self):
        return tuple(a.astype(np.float32) for a in self.r.tables())

    def get_state(self):
        return tuple(a.astype(np.float32) for a in self.r.tables(self.r.M) + self.r.tables(self.r.V)) + (self.r.t,)

    def reset_optimizer(self):
        self.r.M[...] = 0
        self.r.V[...] = 0
        self.r.t = 0

    def fit_epoch(self, step_ptr, users, pos, neg, lr, lambda_reg):
        step_ptr = np.asarray(step_ptr, np.int64)
        assert np.diff(step_ptr).min() >= 1 and np.diff(step_ptr).max() <= self.MAX_STEP
        self.epochs.append((step_ptr.copy(), np.array(users), np.array(pos), np.array(neg)))
        return self.r.fit_epoch(step_ptr, np.asarray(users), np.asarray(pos), np.asarray(neg), float(lr), float(lambda_reg))

    def propagate(self):
        """from what get_params returns: the float32 tables (the device holds nothing finer)"""
        self.propagated += 1
        f32 = np.concatenate(self.get_params()).astype(np.float64)
        return tuple(a.astype(np.float32) for a in self.r.tables(self.r.P(f32)))

    def close(self):
        self.closed = True
