"""The VAECF checks' reference, inputs and tolerances, in ONE place: tests/test_vaecf_cpu.py holds the float64 restatement
below against the golden that the reference's own VAE / learn wrote (tests/golden/make_vaecf_golden.py),
tests/test_vaecf_gpu.py holds the device against the restatement and against the same golden.

`Restatement` restates one Adam step of cornac/models/vaecf/vaecf.py:127-144 in float64 NumPy, with the gradients written
out by hand (no autograd): forward, the likelihood's dL/dp, dL/do, the chain through both layers, the KL terms, and
torch.optim.Adam's dense update of all ten tables.  Its sums are float64 (about 1e-16 relative whatever the order), which
is 10^8 times finer than the float32 effects the tests measure, so BLAS's summation order does not matter.

Cases draw their initial weights and their noise from numpy.random.RandomState, never from torch, so another torch build
changes nothing.

Tolerance of the device against the restatement, per table (parameters, Adam's m and v alike):
    max(16 * d_ref, 4 units in the last float32 place of max|table|)
where d_ref = max|reference float32 - restatement| is read from the golden (16 is this project's factor over the
reference's own distance, as for EASE and HPF).  For every parameter table that tolerance must stay under 1 % of the
table's recorded movement: `check_condition`."""
import numpy as np
import scipy.sparse as sp

NAMES = ("encoder.fc0.weight", "encoder.fc0.bias", "enc_mu.weight", "enc_mu.bias", "enc_logvar.weight", "enc_logvar.bias",
         "decoder.fc0.weight", "decoder.fc0.bias", "decoder.fc1.weight", "decoder.fc1.bias")
SHORT = dict(zip(NAMES, ("W1", "b1", "Wm", "bm", "Wv", "bv", "D0", "c0", "D1", "c1")))
ACTS = ("tanh", "sigmoid", "relu", "relu6", "elu")
LIKELIHOODS = ("mult", "bern", "gaus", "pois")
EPS = 1e-10
N_SCORE_USERS = 5
N_PAIRS = 12


def shapes(ni, k, h):
    return dict(zip(NAMES, ((h, ni), (h,), (k, h), (k,), (k, h), (k,), (h, k), (h,), (ni, h), (ni,))))


# ---- the case table --------------------------------------------------------------------------------------------------------
def _c(nu, ni, k, h, bs, epochs, act="tanh", lik="mult", lr=1e-3, beta=1.0, seed=0, dscale=1.0):
    return dict(nu=nu, ni=ni, k=k, h=h, bs=bs, epochs=epochs, act=act, lik=lik, lr=lr, beta=beta, seed=seed, dscale=dscale)


CASES = {
    # item counts 1, 63, 64, 65, 257, 1031; h 1, 20, 64, 65; k 1, 10, 33; batches 1, 16, 100; the user count is never a
    # multiple of the batch, and every case runs past an epoch's end, so Adam's t persists
    "i1": _c(5, 1, 1, 1, 2, 2, lik="bern", seed=1),          # (one item: "mult" has p = 1 and no gradient)
    "b1": _c(5, 9, 1, 1, 1, 2, seed=8),                      # batch size 1, ten steps
    "i63": _c(37, 63, 10, 20, 16, 2, seed=2),
    "i64": _c(21, 64, 33, 64, 16, 2, act="sigmoid", lik="bern", seed=3),
    "i65": _c(23, 65, 10, 65, 16, 2, act="elu", lik="pois", seed=4),
    "i257": _c(250, 257, 10, 20, 100, 2, seed=5),
    "i1031": _c(45, 1031, 33, 65, 16, 2, act="relu", lik="gaus", seed=6),
    # decoder weights scaled so that a held item has p < 1e-6 and EPS = 1e-10 shows in -x / (p + EPS)
    "sat": _c(37, 131, 5, 7, 16, 2, seed=7, dscale=8.0),
}
for _a in ACTS:   # all five activations x all four likelihoods at one small shape, 9 steps
    for _l in LIKELIHOODS:
        CASES["al/%s/%s" % (_a, _l)] = _c(37, 131, 5, 7, 16, 3, act=_a, lik=_l, seed=20 + 4 * ACTS.index(_a) + LIKELIHOODS.index(_l))
FULL_CASES = ("i257", "al/tanh/mult", "sat")   # the golden holds tables, moments, losses and scores for these
# max over the ten tables of |restatement - the reference's float32 table|, measured by
# tests/test_vaecf_cpu.py::test_restatement_against_the_references_tables (for orientation: the feasibility trial, 9 steps at
# 37 x 131, gave 6.5e-8 to 9.2e-8; the saturated case's larger figure is float32's own, through 1 / (p + EPS) at p ~ 1e-8)
RESTATEMENT_VS_REFERENCE = {"i257": 6.54e-08, "al/tanh/mult": 8.81e-08, "sat": 4.65e-07}


def n_steps(c):
    return c["epochs"] * -(-c["nu"] // c["bs"])


def case_matrix(c):
    """users x items CSR with sorted indices.  Where the shape allows (>= 8 items): item 1 is held by nobody, item 2 only
    by users 0 and 1 (the first batch, or the first two), user 3 holds one item, and one stored value is 0.0 (it counts
    as 1); the other stored values are ratings 1..5."""
    rs = np.random.RandomState(1000 + c["seed"])
    nu, ni = c["nu"], c["ni"]
    held = rs.rand(nu, ni) < min(0.5, max(0.08, 6.0 / ni))
    if ni >= 8:
        held[:, 1] = False
        held[:, 2] = False
        held[0, 2] = held[1, 2] = True
        held[3, :] = False
        held[3, 5] = True
    for u in range(nu):
        if not held[u].any():
            held[u, rs.randint(ni)] = True
    rows, cols = np.nonzero(held)
    vals = rs.randint(1, 6, len(rows)).astype(np.float64)
    if ni >= 8:
        vals[len(vals) // 2] = 0.0
    X = sp.csr_matrix((vals, (rows, cols)), shape=(nu, ni))
    X.sort_indices()
    assert X.nnz == len(rows), "the stored zero stays stored"
    return X


def case_triplets(c):
    X = case_matrix(c).tocoo()
    return X.row.astype(np.int64), X.col.astype(np.int64), X.data.astype(np.float64)


def case_params(c):
    """float32 tables drawn as nn.Linear would scale them (uniform in +- 1 / sqrt(fan_in)), from RandomState"""
    rs = np.random.RandomState(2000 + c["seed"])
    out = {}
    for n, sh in shapes(c["ni"], c["k"], c["h"]).items():
        layer = n.rsplit(".", 1)[0]
        fan_in = shapes(c["ni"], c["k"], c["h"])[layer + ".weight"][1]
        out[n] = rs.uniform(-1.0, 1.0, sh).astype(np.float32) / np.float32(np.sqrt(fan_in))
    if c["dscale"] != 1.0:
        out["decoder.fc1.weight"] = (out["decoder.fc1.weight"] * np.float32(c["dscale"])).astype(np.float32)
    return out


def case_noise(c):
    """[epochs, n_users, k] float32: epoch e's reparameterisation noise, row = user"""
    return np.random.RandomState(3000 + c["seed"]).standard_normal((c["epochs"], c["nu"], c["k"])).astype(np.float32)


def score_users(c):
    return np.unique(np.linspace(0, c["nu"] - 1, N_SCORE_USERS).astype(np.int64))


def score_pairs(c, seed=5):
    rs = np.random.RandomState(seed)
    return rs.randint(0, c["nu"], N_PAIRS).astype(np.int64), rs.randint(0, c["ni"], N_PAIRS).astype(np.int64)


def dataset(name):
    from cornac_amd import Dataset

    c = CASES[name]
    u, i, r = case_triplets(c)
    return Dataset.from_arrays(u, i, r, num_users=c["nu"], num_items=c["ni"])


# ---- the restatement -------------------------------------------------------------------------------------------------------
def activation(name, a):
    """(f(a), f'(a))"""
    if name == "tanh":
        t = np.tanh(a)
        return t, 1.0 - t * t
    if name == "sigmoid":
        s = 1.0 / (1.0 + np.exp(-a))
        return s, s * (1.0 - s)
    if name == "relu":
        return np.maximum(a, 0.0), (a > 0).astype(np.float64)
    if name == "relu6":
        return np.clip(a, 0.0, 6.0), ((a > 0) & (a < 6)).astype(np.float64)
    if name == "elu":
        return np.where(a > 0, a, np.expm1(np.minimum(a, 0.0))), np.where(a > 0, 1.0, np.exp(np.minimum(a, 0.0)))
    raise ValueError(name)


def probabilities(o, lik):
    if lik == "mult":
        e = np.exp(o - o.max(axis=1, keepdims=True))
        return e / e.sum(axis=1, keepdims=True)
    return 1.0 / (1.0 + np.exp(-o))


class Restatement:
    """the ten tables, Adam's m and v and its step counter t, all float64 / int; `step` is one batch"""

    def __init__(self, X, k, h, act, lik, params=None):
        X = sp.csr_matrix(X)
        self.B = sp.csr_matrix((np.ones(len(X.data)), X.indices, X.indptr), shape=X.shape).toarray()   # stored zeros count
        self.nu, self.ni = X.shape
        self.k, self.h, self.act, self.lik = k, h, act, lik
        sh = shapes(self.ni, k, h)
        self.P = {n: np.zeros(sh[n]) for n in NAMES}
        self.M = {n: np.zeros(sh[n]) for n in NAMES}
        self.V = {n: np.zeros(sh[n]) for n in NAMES}
        self.t = 0
        if params is not None:
            self.set_params(params)

    def set_params(self, params):
        for n, a in params.items():
            if a is not None:
                assert np.shape(a) == self.P[n].shape, n
                self.P[n] = np.array(a, np.float64)

    def forward(self, x, eps):
        P = self.P
        a1 = x @ P[NAMES[0]].T + P[NAMES[1]]
        h1, d1 = activation(self.act, a1)
        mu = h1 @ P[NAMES[2]].T + P[NAMES[3]]
        lv = h1 @ P[NAMES[4]].T + P[NAMES[5]]
        std = np.exp(0.5 * lv)
        z = mu + (0.0 if eps is None else eps * std)
        a2 = z @ P[NAMES[6]].T + P[NAMES[7]]
        h2, d2 = activation(self.act, a2)
        o = h2 @ P[NAMES[8]].T + P[NAMES[9]]
        return dict(h1=h1, d1=d1, mu=mu, lv=lv, std=std, z=z, h2=h2, d2=d2, o=o, p=probabilities(o, self.lik))

    def step(self, u0, nb, eps, lr, beta):
        """one batch: users u0 .. u0 + nb, noise eps [nb, k]; returns the batch-mean loss"""
        x, P = self.B[u0:u0 + nb], self.P
        eps = np.asarray(eps, np.float64)
        f = self.forward(x, eps)
        p, mu, lv, std = f["p"], f["mu"], f["lv"], f["std"]
        kl = -0.5 * np.sum(1.0 + lv - mu ** 2 - std ** 2, axis=1)
        if self.lik == "mult":
            ll, g = x * np.log(p + EPS), -x / (p + EPS)
        elif self.lik == "bern":
            ll, g = x * np.log(p + EPS) + (1 - x) * np.log(1 - p + EPS), -(x / (p + EPS) - (1 - x) / (1 - p + EPS))
        elif self.lik == "gaus":
            ll, g = -(x - p) ** 2, 2.0 * (p - x)
        else:
            ll, g = x * np.log(p + EPS) - p, -(x / (p + EPS) - 1.0)
        loss = float(np.mean(beta * kl - ll.sum(axis=1)))
        g = g / nb
        go = p * (g - np.sum(g * p, axis=1, keepdims=True)) if self.lik == "mult" else g * p * (1.0 - p)
        G = {}
        G[NAMES[8]], G[NAMES[9]] = go.T @ f["h2"], go.sum(axis=0)
        ga2 = (go @ P[NAMES[8]]) * f["d2"]
        G[NAMES[6]], G[NAMES[7]] = ga2.T @ f["z"], ga2.sum(axis=0)
        gz = ga2 @ P[NAMES[6]]
        gmu = gz + beta * mu / nb
        glv = gz * eps * std / 2.0 - beta * (1.0 - std ** 2) / (2.0 * nb)
        G[NAMES[2]], G[NAMES[3]] = gmu.T @ f["h1"], gmu.sum(axis=0)
        G[NAMES[4]], G[NAMES[5]] = glv.T @ f["h1"], glv.sum(axis=0)
        ga1 = (gmu @ P[NAMES[2]] + glv @ P[NAMES[4]]) * f["d1"]
        G[NAMES[0]], G[NAMES[1]] = ga1.T @ x, ga1.sum(axis=0)
        self.t += 1
        b1, b2 = 0.9, 0.999
        for n in NAMES:   # torch.optim.Adam, dense: every entry of every table, whatever its gradient
            self.M[n] = b1 * self.M[n] + (1 - b1) * G[n]
            self.V[n] = b2 * self.V[n] + (1 - b2) * G[n] ** 2
            self.P[n] = self.P[n] - lr / (1 - b1 ** self.t) * self.M[n] / (np.sqrt(self.V[n]) / np.sqrt(1 - b2 ** self.t) + 1e-8)
        return loss

    def fit_epoch(self, bs, lr, beta, eps):
        """eps [n_users, k]; returns the per-step losses"""
        return np.array([self.step(u0, min(bs, self.nu - u0), eps[u0:u0 + bs], lr, beta) for u0 in range(0, self.nu, bs)])

    def h2(self, users):
        return self.forward(self.B[np.asarray(users, np.int64)], None)["h2"]

    def logits(self, users):
        return self.forward(self.B[np.asarray(users, np.int64)], None)["o"]

    def scores(self, users):
        return self.forward(self.B[np.asarray(users, np.int64)], None)["p"]


def run_case(name):
    """the restatement over the whole case: (Restatement after the last step, per-step losses, the initial tables)"""
    c = CASES[name]
    init = case_params(c)
    r = Restatement(case_matrix(c), c["k"], c["h"], c["act"], c["lik"], init)
    noise = case_noise(c)
    losses = np.concatenate([r.fit_epoch(c["bs"], c["lr"], c["beta"], noise[e]) for e in range(c["epochs"])])
    return r, losses, init


# ---- tolerances ------------------------------------------------------------------------------------------------------------
def ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else float(np.spacing(np.float32(0)))


def tolerance(d_ref, table):
    return max(16.0 * float(d_ref), 4.0 * ulp32(float(np.abs(table).max(initial=0.0))))


def check_condition(golden, name):
    """for every parameter table the device's tolerance stays under 1 % of the recorded movement (a table that the case
    leaves exactly in place has movement 0 and d_ref 0, and is held to 4 ulp: nothing to compare the 1 % with)"""
    worst = 0.0
    for q, n in enumerate(NAMES):
        d_ref, move, top = (float(golden["%s/%s" % (name, kind)][q]) for kind in ("d_ref", "move", "max"))
        if move == 0.0:
            assert d_ref == 0.0, (name, n)
            continue
        tol = max(16.0 * d_ref, 4.0 * ulp32(top))
        worst = max(worst, tol / move)
        assert tol < 0.01 * move, "%s %s: tolerance %.3g is not under 1 %% of the movement %.3g" % (name, n, tol, move)
    return worst


# ---- a device double ---------------------------------------------------------------------------------------------------------
class FakeVaecfModel:
    """_lib.VaecfModel served by the restatement (float32 in, float32 out); counts what was built"""
    NAMES, ACTS, LIKELIHOODS = NAMES, ACTS, LIKELIHOODS
    built = 0
    last = None

    @staticmethod
    def shapes(n_items, k, h):
        return shapes(n_items, k, h)

    def __init__(self, X, k, h, act_fn="tanh", likelihood="mult", device=0):
        assert sp.issparse(X) and act_fn in ACTS and likelihood in LIKELIHOODS
        self.r = Restatement(X, int(k), int(h), act_fn, likelihood)
        self.n_users, self.n_items, self.k, self.h = self.r.nu, self.r.ni, int(k), int(h)
        self.device, self.closed, self.epochs, self.noise = device, False, 0, []
        FakeVaecfModel.built += 1
        FakeVaecfModel.last = self

    def set_params(self, params):
        self.r.set_params(params)

    def get_params(self):
        return {n: self.r.P[n].astype(np.float32) for n in NAMES}

    def get_state(self):
        return ({n: self.r.M[n].astype(np.float32) for n in NAMES}, {n: self.r.V[n].astype(np.float32) for n in NAMES}, self.r.t)

    def reset_optimizer(self):
        for n in NAMES:
            self.r.M[n][...] = 0
            self.r.V[n][...] = 0
        self.r.t = 0

    def fit_epoch(self, batch_size, lr, beta, eps=None, seed=0):
        if eps is None:
            eps = np.random.RandomState((int(seed) + self.r.t) % 2 ** 32).standard_normal((self.n_users, self.k)).astype(np.float32)
        self.noise.append(None if eps is None else np.array(eps))
        self.epochs += 1
        steps = self.r.fit_epoch(int(batch_size), float(lr), float(beta), np.asarray(eps, np.float32))
        return float(steps.sum()), steps

    def _f32(self):
        """prediction sees what get_params returns: the float32 tables (the device holds nothing finer)"""
        return Restatement(sp.csr_matrix(self.r.B), self.k, self.h, self.r.act, self.r.lik, self.get_params())

    def encode_users(self, users):
        return self._f32().h2(users).astype(np.float32).reshape(len(users), self.h)

    def score_users(self, users):
        return self._f32().scores(users).astype(np.float32).reshape(len(users), self.n_items)

    def score_pairs(self, users, items):
        users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
        return self._f32().scores(users)[np.arange(len(users)), items].astype(np.float32)

    def close(self):
        self.closed = True
