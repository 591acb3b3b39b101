"""The RecVAE checks' reference, inputs and tolerances, in ONE place: tests/test_recvae_cpu.py holds the float64 restatement
below against the golden that the reference's own VAE / RecVAE.run wrote (tests/golden/make_recvae_golden.py),
tests/test_recvae_gpu.py holds the device against the restatement and against the same golden.

`Restatement` restates one step of cornac/models/recvae/recom_recvae.py:131-145 over recvae.py:9-117 in float64 NumPy, with
every gradient written out by hand (no autograd): the likelihood's dL/do, the mixture prior's gradient in z, the paths into mu
and logvar both directly and through z, LayerNorm's backward, swish's derivative, the dense skip sums, and the two
torch.optim.Adam with their own step counters.  Its sums are float64 (about 1e-16 relative whatever the order), which is 10^8
times finer than the float32 effects the tests measure.

Cases draw their weights, masks, noise and batch orders from numpy.random.RandomState, never from torch, so another torch
build changes nothing.  Every case runs encoder pass -> update_prior -> decoder pass -> encoder pass (`not_alternating`: three
joint passes and no update_prior): the old encoder then differs from the new one, both step counters persist, and the
encoder's m carries across the decoder pass.  The user count is never a multiple of the batch size.

Tolerance of the device against the restatement, per table (parameters, Adam's m and v alike):
    max(16 * d_ref, 4 units in the last float32 place of max|table|)
where d_ref = max|reference float32 - restatement| is read from the golden (16 is this project's factor over the
reference's own distance, as for EASE, HPF and VAECF).  For every parameter table that tolerance must stay under 1 % of the
table's recorded movement: `check_condition`."""
import numpy as np
import scipy.sparse as sp

ENCODER = tuple("%s%d.%s" % (kind, l, p) for l in range(1, 6) for kind in ("fc", "ln") for p in ("weight", "bias")) + (
    "fc_mu.weight", "fc_mu.bias", "fc_logvar.weight", "fc_logvar.bias")
PRIORS = ("prior.mu_prior", "prior.logvar_prior", "prior.logvar_uniform_prior")
NAMES = tuple("encoder." + n for n in ENCODER) + PRIORS + tuple("prior.encoder_old." + n for n in ENCODER) + (
    "decoder.weight", "decoder.bias")
ENC_NAMES = tuple("encoder." + n for n in ENCODER)
DEC_NAMES = ("decoder.weight", "decoder.bias")
TRAINABLE = ENC_NAMES + DEC_NAMES
LOG_W = np.log(np.array([3 / 20, 3 / 4, 1 / 10]))
LN_EPS = 0.1
N_SCORE_USERS = 5
N_PAIRS = 12


def shapes(ni, h, k):
    enc = tuple(s for l in range(1, 6) for s in ((h, ni if l == 1 else h), (h,), (h,), (h,))) + ((k, h), (k,), (k, h), (k,))
    return dict(zip(NAMES, enc + ((1, k),) * 3 + enc + ((ni, k), (ni,))))


# ---- the case table --------------------------------------------------------------------------------------------------------
def _c(nu, ni, h, k, bs, gamma=0.005, beta=None, lr=1e-3, seed=0, not_alternating=False, mu_scale=1.0, wide=10.0):
    return dict(nu=nu, ni=ni, h=h, k=k, bs=bs, gamma=gamma, beta=beta, lr=lr, seed=seed, not_alternating=not_alternating,
                mu_scale=mu_scale, wide=wide)


CASES = {
    # items 1, 63, 64, 65, 257, 1031; hidden 1, 7, 64, 65; latent 1, 5, 33; batches 1, 16, 100
    "i1": _c(5, 1, 1, 1, 2, seed=1),                        # one item; LayerNorm of one element
    "b1": _c(5, 9, 1, 1, 1, seed=2),                        # batch size 1, hidden 1: the encoder's matrices stay in place
    "i63": _c(37, 63, 7, 5, 16, seed=3),
    "i64": _c(21, 64, 64, 33, 16, beta=0.3, gamma=None, seed=4),   # the scalar KL weight
    "i65": _c(23, 65, 65, 5, 16, seed=5),
    "i257": _c(250, 257, 7, 5, 100, seed=6),
    "i1031": _c(45, 1031, 65, 33, 16, seed=7),
    "joint": _c(37, 131, 7, 5, 16, seed=8, not_alternating=True),
    "joint/beta": _c(37, 131, 7, 5, 16, beta=0.2, gamma=0, seed=9, not_alternating=True),
    # fc_mu scaled so that |z| reaches the hundreds, against a wide prior of logvar about 4: the posterior term lies
    # thousands below the wide one, and where |z| > 107 all three lie below float32's exp underflow (-104), so that only a
    # max-shifted logsumexp is finite (test_recvae_cpu.py::test_far_case_underflows_unshifted counts such entries)
    # (lr 0.01: fc_mu's entries are near 100, where 16 float32 ulp are 1e-4, and 9 steps of 1e-3 would move them 6e-3)
    "far": _c(37, 131, 7, 5, 16, lr=1e-2, seed=10, mu_scale=300.0, wide=4.0),
}
FULL_CASES = ("i257", "joint", "i63")   # the golden holds tables, moments, losses and logits for these
SEEDED = {   # the reference's own seeded RecVAE.fit, recorded in the golden (its NDCG@100 needs more than 100 items)
    "seed1": dict(case="i257", seed=11, n_epochs=1, n_enc_epochs=2, n_dec_epochs=1, not_alternating=False),
    "seed2": dict(case="i257", seed=12, n_epochs=2, n_enc_epochs=1, n_dec_epochs=1, not_alternating=False),
}


def case_matrix(c):
    """users x items CSR with sorted indices.  Where the shape allows (>= 8 items): item 1 is held by nobody, item 2 only by
    users 0 and 1 (the first pass's first batch, or its first two), user 3 holds one item, and one stored value is 0.0; the
    other stored values are ratings 1..5."""
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
        z = len(vals) // 2
        while rows[z] in (0, 1, 3):
            z += 1
        vals[z] = 0.0
    X = sp.csr_matrix((vals, (rows, cols)), shape=(nu, ni))
    X.sort_indices()
    assert X.nnz == len(rows), "the stored zero stays stored"
    return X


def case_triplets(c):
    X = case_matrix(c).tocoo()
    return X.row.astype(np.int64), X.col.astype(np.int64), X.data.astype(np.float64)


def case_params(c):
    """float32 tables: the Linear ones as nn.Linear would scale them (uniform in +- 1 / sqrt(fan_in)), LayerNorm's weights
    around 1 and biases around 0, the prior tables away from the reference's 0, 0, 10 (the wide one around the case's `wide`);
    from RandomState"""
    rs = np.random.RandomState(2000 + c["seed"])
    sh = shapes(c["ni"], c["h"], c["k"])
    out = {}
    for n in NAMES:
        if n in PRIORS:
            out[n] = (rs.uniform(-0.2, 0.2, sh[n]) + (c["wide"] if n == PRIORS[2] else 0.0)).astype(np.float32)
        elif ".ln" in n:
            out[n] = (rs.uniform(-0.1, 0.1, sh[n]) + (1.0 if n.endswith("weight") else 0.0)).astype(np.float32)
        else:
            fan_in = sh[n.rsplit(".", 1)[0] + ".weight"][1]
            out[n] = rs.uniform(-1.0, 1.0, sh[n]).astype(np.float32) / np.float32(np.sqrt(fan_in))
    if c["mu_scale"] != 1.0:
        for n in ("encoder.fc_mu.weight", "encoder.fc_mu.bias"):
            out[n] = (out[n] * np.float32(c["mu_scale"])).astype(np.float32)
    return out


def case_passes(c):
    """the case's passes: dicts of kind ("enc", "dec", "joint"), dropout rate, order [nu], keep [nnz] uint8 (None without
    dropout) and eps [nu, k] float32, the noise itself.  Pass 0 opens with users 0 and 1 (the holders of item 2, whose entries
    it keeps), and where the shape allows it drops every entry of user 4."""
    X = case_matrix(c)
    rs = np.random.RandomState(3000 + c["seed"])
    kinds = ("joint",) * 3 if c["not_alternating"] else ("enc", "dec", "enc")
    out = []
    for q, kind in enumerate(kinds):
        order = rs.permutation(c["nu"]).astype(np.int32)
        if q == 0:
            rest = [u for u in order if u not in (0, 1)]
            order = np.array([0, 1] + rest, np.int32)
        rate = 0.0 if kind == "dec" else 0.5
        keep = None
        if rate:
            keep = (rs.rand(X.nnz) < 1.0 - rate).astype(np.uint8)
            if q == 0 and c["nu"] > 4 and c["ni"] >= 8:
                keep[X.indptr[4]:X.indptr[5]] = 0
                keep[X.indices == 2] = 1
        eps = (0.01 * rs.standard_normal((c["nu"], c["k"]))).astype(np.float32)
        out.append(dict(kind=kind, rate=rate, order=order, keep=keep, eps=eps))
    return out


def n_steps(c):
    return 3 * -(-c["nu"] // c["bs"])


def score_users(c):
    return np.unique(np.linspace(0, c["nu"] - 1, N_SCORE_USERS).astype(np.int64))


def score_pairs(c, seed=5):
    rs = np.random.RandomState(seed)
    return rs.randint(0, c["nu"], N_PAIRS).astype(np.int64), rs.randint(0, c["ni"], N_PAIRS).astype(np.int64)


def dataset(name, seed=None):
    from cornac_amd import Dataset

    c = CASES[name]
    u, i, r = case_triplets(c)
    return Dataset.from_arrays(u, i, r, num_users=c["nu"], num_items=c["ni"], seed=seed)


# ---- the restatement -------------------------------------------------------------------------------------------------------
def sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def log_norm_pdf(x, mu, lv):
    return -0.5 * (lv + np.log(2 * np.pi) + (x - mu) ** 2 / np.exp(lv))


class Restatement:
    """the 53 tables, the two Adams' m and v over the 26 trainable ones and their counters, all float64 / int"""

    def __init__(self, X, hidden, latent, params=None):
        X = sp.csr_matrix(X)
        self.csr = X
        self.X = X.toarray().astype(np.float64)
        self.Xn = self.X / np.maximum(np.sqrt((self.X ** 2).sum(axis=1, keepdims=True)), 1e-12)   # F.normalize
        self.nu, self.ni = X.shape
        self.h, self.k = int(hidden), int(latent)
        sh = shapes(self.ni, self.h, self.k)
        self.P = {n: np.zeros(sh[n]) for n in NAMES}
        self.M = {n: np.zeros(sh[n]) for n in TRAINABLE}
        self.V = {n: np.zeros(sh[n]) for n in TRAINABLE}
        self.t_enc = self.t_dec = 0
        if params is not None:
            self.set_params(params)

    def set_params(self, params):
        for n, a in params.items():
            if a is not None:
                assert np.shape(a) == self.P[n].shape, n
                self.P[n] = np.array(a, np.float64)

    def update_prior(self):
        for n in ENCODER:
            self.P["prior.encoder_old." + n] = self.P["encoder." + n].copy()

    def reset_optimizer(self):
        for n in TRAINABLE:
            self.M[n][...] = 0
            self.V[n][...] = 0
        self.t_enc = self.t_dec = 0

    # -- forward ----------------------------------------------------------------------------------
    def encoder(self, prefix, x):
        """recvae.py:70-75 on the already normalised and dropped-out rows x; keeps what the backward needs"""
        P = self.P
        f = dict(x=x, pre=[], sg=[], xhat=[], rstd=[], hid=[])
        skip = 0.0
        for l in range(1, 6):
            inp = x if l == 1 else f["hid"][-1]
            pre = inp @ P["%sfc%d.weight" % (prefix, l)].T + P["%sfc%d.bias" % (prefix, l)] + skip
            sg = sigmoid(pre)
            s = pre * sg
            d = s - s.mean(axis=1, keepdims=True)
            rstd = 1.0 / np.sqrt((d * d).mean(axis=1, keepdims=True) + LN_EPS)
            xhat = d * rstd
            hid = xhat * P["%sln%d.weight" % (prefix, l)] + P["%sln%d.bias" % (prefix, l)]
            skip = skip + hid
            for key, val in (("pre", pre), ("sg", sg), ("xhat", xhat), ("rstd", rstd), ("hid", hid)):
                f[key].append(val)
        f["mu"] = f["hid"][-1] @ P[prefix + "fc_mu.weight"].T + P[prefix + "fc_mu.bias"]
        f["lv"] = f["hid"][-1] @ P[prefix + "fc_logvar.weight"].T + P[prefix + "fc_logvar.bias"]
        return f

    def mixture(self, z, post_mu, post_lv):
        """recvae.py:37-46: the three log densities plus log weights [.., 3], their max-shifted logsumexp"""
        P = self.P
        a = np.stack([log_norm_pdf(z, P[PRIORS[0]], P[PRIORS[1]]), log_norm_pdf(z, post_mu, post_lv),
                      log_norm_pdf(z, P[PRIORS[0]], P[PRIORS[2]])], axis=-1) + LOG_W
        mx = a.max(axis=-1, keepdims=True)
        e = np.exp(a - mx)
        return a, mx[..., 0] + np.log(e.sum(axis=-1)), e / e.sum(axis=-1, keepdims=True)

    def forward(self, users, keep_rows, scale, eps, gamma, beta):
        """recvae.py:94-111 for the listed users: keep_rows [nb, ni] (None: no dropout), eps [nb, k] the noise"""
        users = np.asarray(users, np.int64)
        x = self.X[users]
        xin = self.Xn[users] if keep_rows is None else self.Xn[users] * keep_rows * scale
        f = self.encoder("encoder.", xin)
        old = self.encoder("prior.encoder_old.", self.Xn[users])
        mu, lv = f["mu"], f["lv"]
        std = np.exp(0.5 * lv)
        z = mu + eps * std
        o = z @ self.P["decoder.weight"].T + self.P["decoder.bias"]
        mx = o.max(axis=1, keepdims=True)
        lse = mx + np.log(np.exp(o - mx).sum(axis=1, keepdims=True))
        w = gamma * x.sum(axis=1) if gamma else np.full(len(users), float(beta))
        a, P_z, resp = self.mixture(z, old["mu"], old["lv"])
        mll = float(((o - lse) * x).sum(axis=1).mean())
        kld = float(((log_norm_pdf(z, mu, lv) - P_z).sum(axis=1) * w).mean())
        f.update(raw=x, std=std, z=z, o=o, lse=lse, w=w, resp=resp, post_mu=old["mu"], post_lv=old["lv"], eps=eps,
                 mll=mll, kld=kld, loss=-(mll - kld))
        return f

    # -- backward ---------------------------------------------------------------------------------
    def gradients(self, f, encoder=True, decoder=True):
        """dL/dtable for L = negative_elbo of the forward pass f, by hand"""
        P, G = self.P, {}
        nb = len(f["raw"])
        x, z, mu, lv, w = f["raw"], f["z"], f["mu"], f["lv"], f["w"][:, None] / nb
        go = (np.exp(f["o"] - f["lse"]) * x.sum(axis=1, keepdims=True) - x) / nb   # -d mll / d o
        if decoder:
            G["decoder.weight"], G["decoder.bias"] = go.T @ z, go.sum(axis=0)
        if not encoder:
            return G
        iv = np.exp(-lv)
        q_z = -(z - mu) * iv                                        # d log N(z; mu, lv) / dz; in mu it is -q_z
        q_lv = -0.5 * (1.0 - (z - mu) ** 2 * iv)
        means = (P[PRIORS[0]], f["post_mu"], P[PRIORS[0]])
        lvs = (P[PRIORS[1]], f["post_lv"], P[PRIORS[2]])
        p_z = sum(f["resp"][..., j] * (-(z - means[j]) / np.exp(lvs[j])) for j in range(3))   # d logsumexp / dz
        gz = go @ P["decoder.weight"] + w * (q_z - p_z)
        gmu = gz - w * q_z
        glv = gz * f["eps"] * f["std"] * 0.5 + w * q_lv
        h5 = f["hid"][4]
        G["encoder.fc_mu.weight"], G["encoder.fc_mu.bias"] = gmu.T @ h5, gmu.sum(axis=0)
        G["encoder.fc_logvar.weight"], G["encoder.fc_logvar.bias"] = glv.T @ h5, glv.sum(axis=0)
        g_hid = gmu @ P["encoder.fc_mu.weight"] + glv @ P["encoder.fc_logvar.weight"]
        later = 0.0   # the sum of dL/dpre over the layers above: every hidden layer feeds all of them through the skips
        for l in range(5, 0, -1):
            q = l - 1
            xhat, rstd, pre, sg = f["xhat"][q], f["rstd"][q], f["pre"][q], f["sg"][q]
            G["encoder.ln%d.weight" % l], G["encoder.ln%d.bias" % l] = (g_hid * xhat).sum(axis=0), g_hid.sum(axis=0)
            gx = g_hid * P["encoder.ln%d.weight" % l]
            gs = rstd * (gx - gx.mean(axis=1, keepdims=True) - xhat * (gx * xhat).mean(axis=1, keepdims=True))
            gpre = gs * (sg * (1.0 + pre * (1.0 - sg)))
            inp = f["x"] if l == 1 else f["hid"][q - 1]
            G["encoder.fc%d.weight" % l], G["encoder.fc%d.bias" % l] = gpre.T @ inp, gpre.sum(axis=0)
            later = later + gpre
            if l > 1:
                g_hid = gpre @ P["encoder.fc%d.weight" % l] + later
        return G

    def _adam(self, names, G, lr, t):
        b1, b2 = 0.9, 0.999
        for n in names:   # torch.optim.Adam, dense: every entry of every table, whatever its gradient
            self.M[n] = b1 * self.M[n] + (1 - b1) * G[n]
            self.V[n] = b2 * self.V[n] + (1 - b2) * G[n] ** 2
            self.P[n] = self.P[n] - lr / (1 - b1 ** t) * self.M[n] / (np.sqrt(self.V[n]) / np.sqrt(1 - b2 ** t) + 1e-8)

    def step(self, users, keep_rows, scale, eps, lr, gamma, beta, step_encoder, step_decoder):
        f = self.forward(users, keep_rows, scale, np.asarray(eps, np.float64), gamma, beta)
        G = self.gradients(f, step_encoder, step_decoder)
        if step_encoder:
            self.t_enc += 1
            self._adam(ENC_NAMES, G, lr, self.t_enc)
        if step_decoder:
            self.t_dec += 1
            self._adam(DEC_NAMES, G, lr, self.t_dec)
        return f["mll"], f["kld"], f["loss"]

    def keep_matrix(self, keep):
        """[nu, ni] 0 / 1 from the per-entry bytes (entries not stored are 0 in x whatever the mask says)"""
        return sp.csr_matrix((np.asarray(keep, np.float64), self.csr.indices, self.csr.indptr), shape=self.csr.shape).toarray()

    def fit_epoch(self, order, bs, lr, gamma, beta, rate, step_encoder, step_decoder, keep, eps):
        """one pass; returns the steps' (mll, kld, negative_elbo) [steps, 3]"""
        order = np.asarray(order, np.int64)
        K = self.keep_matrix(keep) if rate else None
        out = []
        for p0 in range(0, self.nu, bs):
            users = order[p0:p0 + bs]
            out.append(self.step(users, None if K is None else K[users], 1.0 / (1.0 - rate), np.asarray(eps)[users], lr, gamma, beta,
                                 step_encoder, step_decoder))
        return np.array(out, np.float64)

    # -- evaluation mode --------------------------------------------------------------------------
    def encode(self, users, prefix="encoder."):
        f = self.encoder(prefix, self.Xn[np.asarray(users, np.int64)])
        return f["mu"], f["lv"]

    def logits(self, users):
        return self.encode(users)[0] @ self.P["decoder.weight"].T + self.P["decoder.bias"]


def run_passes(r, c, passes=None, upto=None):
    """the case's schedule on a Restatement or a device model of the same interface: the steps' losses [steps, 3]"""
    losses = []
    for q, p in enumerate(case_passes(c) if passes is None else passes):
        if upto is not None and q >= upto:
            break
        if q == 1 and not c["not_alternating"]:
            r.update_prior()
        losses.append(r.fit_epoch(p["order"], c["bs"], c["lr"], c["gamma"], c["beta"], p["rate"], p["kind"] != "dec", p["kind"] != "enc",
                                  keep=p["keep"], eps=p["eps"]))
    return np.concatenate(losses)


_RUNS = {}


def run_case(name):
    """the restatement over the whole case, computed once and shared (leave it unchanged): (Restatement after the last step,
    the steps' losses, the initial tables)"""
    if name not in _RUNS:
        c = CASES[name]
        init = case_params(c)
        r = Restatement(case_matrix(c), c["h"], c["k"], init)
        _RUNS[name] = (r, run_passes(r, c), init)
    return _RUNS[name]


# ---- tolerances ------------------------------------------------------------------------------------------------------------
def ulp32(x):
    return float(np.spacing(np.float32(abs(x)))) if x else float(np.spacing(np.float32(0)))


def tolerance(d_ref, table):
    return max(16.0 * float(d_ref), 4.0 * ulp32(float(np.abs(table).max(initial=0.0))))


def table_tolerance(golden, name, q, kind, table):
    """the tolerance of trainable table q of a case; kind "" (the parameters), "_m" or "_v".  0 (bit for bit) where the
    restatement leaves the table exactly in place."""
    if golden[name + "/exact"][q]:
        return 0.0
    return tolerance(golden["%s/d_ref%s" % (name, kind)][q], table)


def check_condition(golden, name):
    """for every trainable table the device's tolerance stays under 1 % of the recorded movement.  A table whose gradient is
    0 in exact arithmetic (`exact` in the golden: everything below ln5.bias at hidden_dim 1) is left out: the reference's
    float32 run moves it by rounding noise that Adam scales up to full steps, so neither its d_ref nor its movement means
    anything, and the device is held to the restatement bit for bit there instead (`table_tolerance` gives 0)."""
    worst = 0.0
    for q, n in enumerate(TRAINABLE):
        d_ref, move, top = (float(golden["%s/%s" % (name, kind)][q]) for kind in ("d_ref", "move", "max"))
        if golden[name + "/exact"][q]:
            continue
        tol = max(16.0 * d_ref, 4.0 * ulp32(top))
        worst = max(worst, tol / move)
        assert tol < 0.01 * move, "%s %s: tolerance %.3g is not under 1 %% of the movement %.3g" % (name, n, tol, move)
    return worst


# ---- a device double ---------------------------------------------------------------------------------------------------------
class FakeRecvaeModel:
    """_lib.RecvaeModel served by the restatement (float32 in, float32 out); records what was called"""
    NAMES, TRAINABLE, ENCODER, PRIORS = NAMES, TRAINABLE, ENCODER, PRIORS
    MAX_HIDDEN, MAX_LATENT, MAX_BATCH = 1024, 256, 1024
    built = 0
    last = None

    @staticmethod
    def shapes(n_items, hidden, latent):
        return shapes(n_items, hidden, latent)

    def __init__(self, X, hidden, latent, device=0):
        assert sp.issparse(X)
        self.r = Restatement(X, int(hidden), int(latent))
        self.n_users, self.n_items, self.hidden, self.latent, self.nnz = self.r.nu, self.r.ni, int(hidden), int(latent), X.nnz
        self.device, self.closed, self.calls = device, False, []
        FakeRecvaeModel.built += 1
        FakeRecvaeModel.last = self

    def set_params(self, params):
        self.r.set_params(params)

    def get_params(self):
        return {n: self.r.P[n].astype(np.float32) for n in NAMES}

    def get_state(self):
        return ({n: self.r.M[n].astype(np.float32) for n in TRAINABLE}, {n: self.r.V[n].astype(np.float32) for n in TRAINABLE},
                self.r.t_enc, self.r.t_dec)

    def reset_optimizer(self):
        self.r.reset_optimizer()

    def update_prior(self):
        self.calls.append(("update_prior",))
        self.r.update_prior()

    def prior_posterior(self):
        mu, lv = self.r.encode(np.arange(self.n_users), "prior.encoder_old.")
        return mu.astype(np.float32), lv.astype(np.float32)

    def fit_epoch(self, order, batch_size, lr, gamma, beta, dropout_rate, step_encoder, step_decoder, keep=None, eps=None, seed=0):
        rs = np.random.RandomState((int(seed) + self.r.t_enc + self.r.t_dec) % 2 ** 32)
        self.calls.append(("fit_epoch", np.array(order), float(dropout_rate), bool(step_encoder), bool(step_decoder),
                           None if keep is None else np.array(keep), None if eps is None else np.array(eps)))
        if keep is None and dropout_rate:
            keep = (rs.rand(self.nnz) < 1.0 - dropout_rate).astype(np.uint8)
        if eps is None:
            eps = (0.01 * rs.standard_normal((self.n_users, self.latent))).astype(np.float32)
        return self.r.fit_epoch(order, int(batch_size), float(lr), gamma, beta, float(dropout_rate), bool(step_encoder), bool(step_decoder),
                                keep, np.asarray(eps, np.float32))

    def _f32(self):
        """prediction sees what get_params returns: the float32 tables (the device holds nothing finer)"""
        return Restatement(self.r.csr, self.hidden, self.latent, self.get_params())

    def encode_users(self, users, with_logvar=False):
        mu, lv = self._f32().encode(users)
        mu, lv = mu.astype(np.float32).reshape(len(users), self.latent), lv.astype(np.float32).reshape(len(users), self.latent)
        return (mu, lv) if with_logvar else mu

    def score_users(self, users):
        return self._f32().logits(users).astype(np.float32).reshape(len(users), self.n_items)

    def score_pairs(self, users, items):
        users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
        return self._f32().logits(users)[np.arange(len(users)), items].astype(np.float32)

    def close(self):
        self.closed = True
