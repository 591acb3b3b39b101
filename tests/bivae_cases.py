"""The BiVAECF checks' reference, inputs and tolerances, in ONE place: tests/test_bivaecf_cpu.py holds the float64 restatement
below against the golden that the reference's own BiVAE / learn wrote (tests/golden/make_bivae_golden.py),
tests/test_bivaecf_gpu.py holds the device against the restatement and against the same golden.

`Restatement` restates one item step and one user step of cornac/models/bivaecf/bivae.py:194-256 in float64 NumPy, with the
gradients written out by hand (no autograd): the encoder's forward, z = mu + eps sigmoid(.), the bilinear decoder against
the other side's table (a constant), the likelihood's dL/dp and dL/do, the chain back through z, the sigmoid, mu and the KL
terms, torch.optim.Adam's dense update of the side's six tables under the side's own step counter, and the second forward
whose sample and mean go to the side's factor tables.  Its sums are float64 (about 1e-16 relative whatever the order),
10^8 times finer than the float32 effects the tests measure.

Cases draw their initial tables and their noise from numpy.random.RandomState, never from torch, so another torch build
changes nothing.  The matrices are vaecf_cases.case_matrix's: an item nobody holds (an EMPTY ROW of the item side), an
item held by the first two users only, a user with one item, a stored 0.0 that counts as 1.

Tolerance of the device against the restatement, per table (parameters, Adam's m and v, and the four factor tables):
    max(16 * d_ref, 4 units in the last float32 place of max|table|)
where d_ref = max|reference float32 - restatement| is read from the golden.  For every parameter table that tolerance
must stay under 1 % of the table's recorded movement: `check_condition`."""
import numpy as np
import scipy.sparse as sp

from vaecf_cases import activation, case_matrix, ulp32

NAMES = ("user_encoder.fc0.weight", "user_encoder.fc0.bias", "user_mu.weight", "user_mu.bias", "user_std.weight", "user_std.bias",
         "item_encoder.fc0.weight", "item_encoder.fc0.bias", "item_mu.weight", "item_mu.bias", "item_std.weight", "item_std.bias")
SHORT = dict(zip(NAMES, ("uW1", "ub1", "uWm", "ubm", "uWs", "ubs", "iW1", "ib1", "iWm", "ibm", "iWs", "ibs")))
FACTORS = ("theta", "beta", "mu_theta", "mu_beta")
TABLES = NAMES + FACTORS   # the order of the golden's 16-entry arrays
ACTS = ("tanh", "sigmoid", "relu", "relu6", "elu")
LIKELIHOODS = ("bern", "gaus", "pois")
EPS = 1e-10
N_SCORE_USERS = 5
N_PAIRS = 12


def shapes(nu, ni, k, h):
    side = lambda n: ((h, n), (h,), (k, h), (k,), (k, h), (k,))   # noqa: E731
    return dict(zip(NAMES, side(ni) + side(nu)))


def factor_shapes(nu, ni, k):
    return dict(zip(FACTORS, ((nu, k), (ni, k), (nu, k), (ni, k))))


# ---- the case table --------------------------------------------------------------------------------------------------------
def _c(nu, ni, k, h, bs, epochs, act="tanh", lik="pois", lr=1e-3, beta=1.0, seed=0, fscale=1.0):
    return dict(nu=nu, ni=ni, k=k, h=h, bs=bs, epochs=epochs, act=act, lik=lik, lr=lr, beta=beta, seed=seed, fscale=fscale)


CASES = {
    # the other side's table length 1, 63, 64, 65, 257, 1031 on EACH side (i*: items, u*: users), rectangular both ways;
    # 1031 is past two of the dense pass's ranges (512 rows), on the user side in i1031 and on the item side in u1031;
    # k 1, 10, 33, 65 (and 20, 130 for the dense kernel's other widths); h 1, 20, 65; batches 1, 16, 100 (100 also above
    # the side's count: one short batch); neither count is a multiple of the batch except at batch 1; two epochs, so both
    # step counters and the sampled theta and beta carry over
    "i1": _c(5, 1, 1, 1, 2, 2, lik="bern", seed=1),
    "u1": _c(1, 5, 1, 1, 2, 2, seed=9),
    "b1": _c(5, 9, 1, 1, 1, 2, seed=8),
    "i63": _c(37, 63, 10, 20, 16, 2, seed=2),
    "i64": _c(21, 64, 33, 20, 24, 2, act="sigmoid", lik="bern", seed=3),
    "i65": _c(23, 65, 65, 65, 16, 2, act="elu", lik="gaus", seed=4),
    "i257": _c(250, 257, 10, 20, 100, 2, seed=5),
    "i1031": _c(45, 1031, 33, 65, 16, 2, act="relu", lik="gaus", seed=6),
    "u63": _c(63, 37, 10, 20, 16, 2, lik="bern", seed=10),
    "u64": _c(64, 21, 1, 20, 100, 2, lik="gaus", seed=11),
    "u65": _c(65, 23, 10, 1, 16, 2, act="relu6", seed=12),
    "u257": _c(257, 250, 33, 20, 100, 2, lik="bern", seed=13),
    "u1031": _c(1031, 45, 10, 20, 100, 2, seed=14),
    "k20": _c(21, 19, 20, 7, 16, 2, seed=15),
    "k130": _c(21, 19, 130, 7, 16, 2, lik="bern", seed=16),
    # theta scaled so that in the item pass some held entry has p < 1e-6 and EPS = 1e-10 shows in x / (p + EPS)
    "sat": _c(37, 131, 5, 7, 16, 2, seed=7, fscale=16.0),
}
for _a in ACTS:   # all five activations x all three likelihoods at one small shape
    for _l in LIKELIHOODS:
        CASES["al/%s/%s" % (_a, _l)] = _c(37, 131, 5, 7, 16, 2, act=_a, lik=_l, seed=20 + 3 * ACTS.index(_a) + LIKELIHOODS.index(_l))
FULL_CASES = ("i257", "al/tanh/pois", "sat")   # the golden holds tables, moments, losses and scores for these
# max over the 12 tables of |restatement - the reference's float32 table|, measured by
# tests/test_bivaecf_cpu.py::test_restatement_against_the_references_tables
RESTATEMENT_VS_REFERENCE = {"i257": 3.25e-08, "al/tanh/pois": 1.02e-07, "sat": 9.63e-08}


def n_steps(c):
    """(item steps, user steps) of the whole case"""
    return c["epochs"] * -(-c["ni"] // c["bs"]), c["epochs"] * -(-c["nu"] // c["bs"])


def case_triplets(c):
    X = case_matrix(c).tocoo()
    return X.row.astype(np.int64), X.col.astype(np.int64), X.data.astype(np.float64)


def case_params(c):
    """float32 tables drawn as nn.Linear would scale them (uniform in +- 1 / sqrt(fan_in)), from RandomState"""
    rs = np.random.RandomState(2000 + c["seed"])
    sh = shapes(c["nu"], c["ni"], c["k"], c["h"])
    out = {}
    for n in NAMES:
        fan_in = sh[n.rsplit(".", 1)[0] + ".weight"][1]
        out[n] = rs.uniform(-1.0, 1.0, sh[n]).astype(np.float32) / np.float32(np.sqrt(fan_in))
    return out


def case_factors(c):
    """theta as kaiming_uniform_(a = sqrt 5) scales it (uniform in +- 1 / sqrt(k)), times the case's fscale; beta 0.01 x
    normal; the two mean tables zero (bivae.py:48-53)"""
    rs = np.random.RandomState(2500 + c["seed"])
    theta = rs.uniform(-1.0, 1.0, (c["nu"], c["k"])).astype(np.float32) / np.float32(np.sqrt(c["k"])) * np.float32(c["fscale"])
    beta = (0.01 * rs.standard_normal((c["ni"], c["k"]))).astype(np.float32)
    return dict(theta=theta.astype(np.float32), beta=beta, mu_theta=np.zeros((c["nu"], c["k"]), np.float32),
                mu_beta=np.zeros((c["ni"], c["k"]), np.float32))


def case_noise(c):
    """(item [epochs, 2, n_items, k], user [epochs, 2, n_users, k]) float32: plane 0 is the training forward's noise, plane 1
    that of the forward after the step, row = id"""
    rs = np.random.RandomState(3000 + c["seed"])
    return (rs.standard_normal((c["epochs"], 2, c["ni"], c["k"])).astype(np.float32),
            rs.standard_normal((c["epochs"], 2, c["nu"], c["k"])).astype(np.float32))


def noise_queue(c):
    """the case's noise in the order the reference draws it: per epoch the item batches, then the user batches, two draws
    per batch"""
    ni, nu = case_noise(c)
    out = []
    for e in range(c["epochs"]):
        for noise, n in ((ni, c["ni"]), (nu, c["nu"])):
            for r0 in range(0, n, c["bs"]):
                out += [noise[e, 0, r0:r0 + c["bs"]], noise[e, 1, r0:r0 + c["bs"]]]
    return out


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
def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def likelihood(lik, x, p):
    """(LL per entry, -dLL/dp) of bivae.py:136-140"""
    if lik == "bern":
        return x * np.log(p + EPS) + (1 - x) * np.log(1 - p + EPS), -(x / (p + EPS) - (1 - x) / (1 - p + EPS))
    if lik == "gaus":
        return -(x - p) ** 2, 2.0 * (p - x)
    if lik == "pois":
        return x * np.log(p + EPS) - p, -(x / (p + EPS) - 1.0)
    raise ValueError(lik)


class Restatement:
    """the 12 tables, Adam's m and v, the two step counters `t` and the four factor tables `F`, all float64 / int"""
    SIDES = {"user": (0, "beta", "theta", "mu_theta"), "item": (6, "theta", "beta", "mu_beta")}   # first table, constant, z, mean

    def __init__(self, X, k, h, act, lik, params=None, factors=None):
        X = sp.csr_matrix(X)
        self.B = sp.csr_matrix((np.ones(len(X.data)), X.indices, X.indptr), shape=X.shape).toarray()   # stored zeros count
        self.nu, self.ni = X.shape
        self.k, self.h, self.act, self.lik = k, h, act, lik
        sh = shapes(self.nu, self.ni, k, h)
        self.P = {n: np.zeros(sh[n]) for n in NAMES}
        self.M = {n: np.zeros(sh[n]) for n in NAMES}
        self.V = {n: np.zeros(sh[n]) for n in NAMES}
        self.F = {n: np.zeros(s) for n, s in factor_shapes(self.nu, self.ni, k).items()}
        self.t = {"user": 0, "item": 0}
        self.set_params(params or {})
        self.set_factors(**(factors or {}))

    def set_params(self, params):
        for n, a in params.items():
            if a is not None:
                assert np.shape(a) == self.P[n].shape, n
                self.P[n] = np.array(a, np.float64)

    def set_factors(self, theta=None, beta=None, mu_theta=None, mu_beta=None):
        for n, a in zip(FACTORS, (theta, beta, mu_theta, mu_beta)):
            if a is not None:
                assert np.shape(a) == self.F[n].shape, n
                self.F[n] = np.array(a, np.float64)

    def rows(self, side):
        return self.B if side == "user" else self.B.T

    def encode(self, side, x, eps):
        W1, b1, Wm, bm, Ws, bs = (self.P[NAMES[self.SIDES[side][0] + q]] for q in range(6))
        h1, d1 = activation(self.act, x @ W1.T + b1)
        mu, s = h1 @ Wm.T + bm, sigmoid(h1 @ Ws.T + bs)
        return dict(h1=h1, d1=d1, mu=mu, s=s, z=mu + (0.0 if eps is None else eps * s))

    def loss_and_gradients(self, side, r0, nb, eps, beta):
        """the batch-mean loss of bivae.py:134-152 and its gradients by hand, keyed by table name"""
        first, const = self.SIDES[side][:2]
        x, T = self.rows(side)[r0:r0 + nb], self.F[const]
        f = self.encode(side, x, eps)
        mu, s, z = f["mu"], f["s"], f["z"]
        p = sigmoid(z @ T.T)
        kl = -0.5 * np.sum(1.0 + 2.0 * np.log(s) - mu ** 2 - s ** 2, axis=1)
        ll, g = likelihood(self.lik, x, p)
        loss = float(np.mean(beta * kl - ll.sum(axis=1)))
        gz = (g / nb * p * (1.0 - p)) @ T
        gmu = gz + beta * mu / nb
        gas = (gz * eps + beta * (s - 1.0 / s) / nb) * s * (1.0 - s)
        Wm, Ws = self.P[NAMES[first + 2]], self.P[NAMES[first + 4]]
        ga1 = (gmu @ Wm + gas @ Ws) * f["d1"]
        G = (ga1.T @ x, ga1.sum(axis=0), gmu.T @ f["h1"], gmu.sum(axis=0), gas.T @ f["h1"], gas.sum(axis=0))
        return loss, {NAMES[first + q]: G[q] for q in range(6)}, p

    def step(self, side, r0, nb, eps1, eps2, lr, beta):
        """one batch of `side`: ids r0 .. r0 + nb, noise eps1 (the training forward) and eps2 (the forward after the step),
        each [nb, k]; returns the batch-mean loss"""
        eps1, eps2 = np.asarray(eps1, np.float64), np.asarray(eps2, np.float64)
        loss, G, _ = self.loss_and_gradients(side, r0, nb, eps1, beta)
        self.t[side] += 1
        t, b1, b2 = self.t[side], 0.9, 0.999
        for n, g in G.items():   # torch.optim.Adam, dense: every entry of the side's tables, whatever its gradient
            self.M[n] = b1 * self.M[n] + (1 - b1) * g
            self.V[n] = b2 * self.V[n] + (1 - b2) * g ** 2
            self.P[n] = self.P[n] - lr / (1 - b1 ** t) * self.M[n] / (np.sqrt(self.V[n]) / np.sqrt(1 - b2 ** t) + 1e-8)
        f = self.encode(side, self.rows(side)[r0:r0 + nb], eps2)
        _, _, zname, mname = self.SIDES[side]
        self.F[zname][r0:r0 + nb], self.F[mname][r0:r0 + nb] = f["z"], f["mu"]
        return loss

    def fit_epoch(self, bs, lr, beta, eps_item, eps_user):
        """eps_item [2, n_items, k], eps_user [2, n_users, k]; returns the per-step losses, item steps first"""
        out = []
        for side, n, eps in (("item", self.ni, eps_item), ("user", self.nu, eps_user)):
            for r0 in range(0, n, bs):
                out.append(self.step(side, r0, min(bs, n - r0), eps[0][r0:r0 + bs], eps[1][r0:r0 + bs], lr, beta))
        return np.array(out)

    def infer_means(self):
        for side in ("item", "user"):
            self.F[self.SIDES[side][3]] = self.encode(side, self.rows(side), None)["mu"]

    def logits(self, users):
        return self.F["mu_theta"][np.asarray(users, np.int64)] @ self.F["mu_beta"].T

    def scores(self, users):
        return sigmoid(self.logits(users))


def run_case(name):
    """the restatement over the whole case, final passes included: (Restatement, per-step losses [epochs x (item steps,
    then user steps)], the initial tables)"""
    c = CASES[name]
    init = case_params(c)
    r = Restatement(case_matrix(c), c["k"], c["h"], c["act"], c["lik"], init, case_factors(c))
    ni, nu = case_noise(c)
    losses = np.concatenate([r.fit_epoch(c["bs"], c["lr"], c["beta"], ni[e], nu[e]) for e in range(c["epochs"])])
    r.infer_means()
    return r, losses, init


# ---- tolerances ------------------------------------------------------------------------------------------------------------
def tolerance(d_ref, top):
    return max(16.0 * float(d_ref), 4.0 * ulp32(float(top)))


def check_condition(golden, name):
    """for every parameter table the device's tolerance stays under 1 % of the recorded movement (a table that the case
    leaves exactly in place has movement 0 and d_ref 0, and is held to 4 ulp: nothing to compare the 1 % with)"""
    worst = 0.0
    for q, n in enumerate(NAMES):
        d_ref, move, top = (float(golden["%s/%s" % (name, kind)][q]) for kind in ("d_ref", "move", "max"))
        if move == 0.0:
            assert d_ref == 0.0, (name, n)
            continue
        tol = tolerance(d_ref, top)
        worst = max(worst, tol / move)
        assert tol < 0.01 * move, "%s %s: tolerance %.3g is not under 1 %% of the movement %.3g" % (name, n, tol, move)
    return worst


# ---- a device double ---------------------------------------------------------------------------------------------------------
class FakeBivaeModel:
    """_lib.BivaeModel served by the restatement (float32 in, float32 out); counts what was built"""
    NAMES, FACTORS, ACTS, LIKELIHOODS = NAMES, FACTORS, ACTS, LIKELIHOODS
    built = 0
    last = None

    @staticmethod
    def shapes(n_users, n_items, k, h):
        return shapes(n_users, n_items, k, h)

    @staticmethod
    def factor_shapes(n_users, n_items, k):
        return factor_shapes(n_users, n_items, k)

    def __init__(self, X, k, h, act_fn="tanh", likelihood="pois", device=0):
        assert sp.issparse(X) and act_fn in ACTS and likelihood in LIKELIHOODS
        self.r = Restatement(X, int(k), int(h), act_fn, likelihood)
        self.n_users, self.n_items, self.k, self.h = self.r.nu, self.r.ni, int(k), int(h)
        self.device, self.closed, self.epochs, self.noise, self.inferred = device, False, 0, [], 0
        FakeBivaeModel.built += 1
        FakeBivaeModel.last = self

    def set_params(self, params):
        self.r.set_params(params)

    def get_params(self):
        return {n: self.r.P[n].astype(np.float32) for n in NAMES}

    def set_factors(self, theta=None, beta=None, mu_theta=None, mu_beta=None):
        self.r.set_factors(theta, beta, mu_theta, mu_beta)

    def get_factors(self):
        return {n: self.r.F[n].astype(np.float32) for n in FACTORS}

    def get_state(self):
        return ({n: self.r.M[n].astype(np.float32) for n in NAMES}, {n: self.r.V[n].astype(np.float32) for n in NAMES},
                self.r.t["user"], self.r.t["item"])

    def reset_optimizer(self):
        for n in NAMES:
            self.r.M[n][...] = 0
            self.r.V[n][...] = 0
        self.r.t = {"user": 0, "item": 0}

    def fit_epoch(self, batch_size, lr, beta_kl, eps_item=None, eps_user=None, seed=0):
        self.noise.append((None if eps_item is None else np.array(eps_item), None if eps_user is None else np.array(eps_user)))
        rs = np.random.RandomState((int(seed) + self.r.t["item"]) % 2 ** 32)
        if eps_item is None:
            eps_item = rs.standard_normal((2, self.n_items, self.k)).astype(np.float32)
        if eps_user is None:
            eps_user = rs.standard_normal((2, self.n_users, self.k)).astype(np.float32)
        self.epochs += 1
        steps = self.r.fit_epoch(int(batch_size), float(lr), float(beta_kl), np.asarray(eps_item, np.float32), np.asarray(eps_user, np.float32))
        n_item = -(-self.n_items // int(batch_size))
        return float(steps[:n_item].sum()), float(steps[n_item:].sum()), steps

    def infer_means(self):
        self.inferred += 1
        self.r.infer_means()

    def _f32(self):
        """prediction sees what get_factors returns: the float32 tables (the device holds nothing finer)"""
        return sigmoid(self.r.F["mu_theta"].astype(np.float32).astype(np.float64) @ self.r.F["mu_beta"].astype(np.float32).astype(np.float64).T)

    def score_users(self, users):
        return self._f32()[np.asarray(users, np.int64)].astype(np.float32).reshape(len(users), self.n_items)

    def score_pairs(self, users, items):
        return self._f32()[np.asarray(users, np.int64), np.asarray(items, np.int64)].astype(np.float32)

    def close(self):
        self.closed = True
