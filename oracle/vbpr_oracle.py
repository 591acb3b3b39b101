"""TEST INFRASTRUCTURE ONLY — oracle of the VBPR path (cornac/models/vbpr/recom_vbpr.py:116-275).

VBPR's arithmetic lives in a third-party dependency, PyTorch (`torch>=0.4.1`,
cornac/models/vbpr/requirements.txt): minibatch autograd + `torch.optim.Adam` over ALL tables.
torch (CPU) is present on every box this repo runs on, so the oracle restates `_fit_torch` with the
same torch operations in the same order; the sampler (`Dataset.uij_iter`, cornac/data/dataset.py:490-526)
is restated in cornac_amd/data.py and validated draw-for-draw against the reference's
(tests/test_oracle_vs_reference.py).  The reference's own tests never touch VBPR ("parity unpinned" by
its test-suite); this oracle is pinned against the live reference here
(tests/test_oracle_vs_reference.py::test_vbpr_oracle_matches_live_reference) and by goldens the real
reference produced (tests/golden/vbpr_small.npz).
"""
import numpy as np


def xavier_uniform(shape, rng):
    # cornac/utils/init_utils.py:116-144
    std = np.sqrt(2.0 / np.sum(shape))
    limit = np.sqrt(3.0) * std
    return rng.uniform(-limit, limit, shape).astype(np.float32)


class VBPROracle:
    def __init__(self, k=10, k2=10, n_epochs=50, batch_size=100, learning_rate=0.005, lambda_w=0.01, lambda_b=0.01,
                 lambda_e=0.0, seed=None):
        self.k, self.k2, self.n_epochs, self.batch_size = k, k2, n_epochs, batch_size
        self.lr, self.lambda_w, self.lambda_b, self.lambda_e, self.seed = learning_rate, lambda_w, lambda_b, lambda_e, seed

    def init(self, n_users, n_items, features):
        rng = np.random.RandomState(self.seed)  # get_rng(seed), recom_vbpr.py:117
        self.beta_item = np.zeros(n_items)       # zeros() -> float64 like the reference (init_utils.zeros default)
        self.gamma_user = xavier_uniform((n_users, self.k), rng)
        self.gamma_item = xavier_uniform((n_items, self.k), rng)
        self.theta_user = xavier_uniform((n_users, self.k2), rng)
        self.emb_matrix = xavier_uniform((features.shape[1], self.k2), rng)
        self.beta_prime = xavier_uniform((features.shape[1], 1), rng)

    def fit(self, train_set, batches=None, record_batches=False):
        import torch

        train_set.reset()  # Recommender.fit re-seeds the dataset RNG (recommender.py:327)
        F_np = np.asarray(train_set.item_image.features[: len(train_set.iid_map)]).astype(np.float32)
        self.init(len(train_set.uid_map), len(train_set.iid_map), F_np)
        dt = torch.float
        F = torch.tensor(F_np, dtype=dt)
        Bi = torch.tensor(self.beta_item, dtype=dt, requires_grad=True)
        Gu = torch.tensor(self.gamma_user, dtype=dt, requires_grad=True)
        Gi = torch.tensor(self.gamma_item, dtype=dt, requires_grad=True)
        Tu = torch.tensor(self.theta_user, dtype=dt, requires_grad=True)
        E = torch.tensor(self.emb_matrix, dtype=dt, requires_grad=True)
        Bp = torch.tensor(self.beta_prime, dtype=dt, requires_grad=True)
        opt = torch.optim.Adam([Bi, Gu, Gi, Tu, E, Bp], lr=self.lr)

        def l2(*ts):
            return sum(t.pow(2).sum() for t in ts) / 2

        self.batches, self.losses = [], []
        for epoch in range(self.n_epochs):
            it = batches[epoch] if batches is not None else train_set.uij_iter(self.batch_size, shuffle=True)
            for bu, bi, bj in it:
                if record_batches:
                    self.batches.append((np.array(bu), np.array(bi), np.array(bj)))
                gu, tu = Gu[bu], Tu[bu]
                beta_i, beta_j = Bi[bi], Bi[bj]
                gi, gj = Gi[bi], Gi[bj]
                gamma_diff = gi - gj
                feat_diff = F[bi] - F[bj]
                X = (beta_i - beta_j + (gu * gamma_diff).sum(dim=1) + (tu * feat_diff.mm(E)).sum(dim=1)
                     + feat_diff.mm(Bp))
                ll = torch.nn.functional.logsigmoid(X).sum()
                reg = (l2(gu, gi, gj, tu) * self.lambda_w + l2(beta_i) * self.lambda_b
                       + l2(beta_j) * self.lambda_b / 10 + l2(E, Bp) * self.lambda_e)
                loss = -ll + reg
                opt.zero_grad()
                loss.backward()
                opt.step()
                self.losses.append(float(loss.data.item()))
        self.beta_item = Bi.data.numpy().copy()
        self.gamma_user, self.gamma_item = Gu.data.numpy().copy(), Gi.data.numpy().copy()
        self.theta_user = Tu.data.numpy().copy()
        self.emb_matrix, self.beta_prime = E.data.numpy().copy(), Bp.data.numpy().copy()
        self.theta_item = F.mm(E).data.numpy()
        self.visual_bias = F.mm(Bp).data.numpy().ravel()
        return self


def timed_steps(features, params, u, i, j, batch_size, lr=0.005, lambda_w=0.01, lambda_b=0.01, lambda_e=0.0,
                budget_s=5.0, max_steps=None, return_params=False):
    """The same minibatch step as VBPROracle.fit (recom_vbpr.py:228-262), run over consecutive slices of pre-sampled
    (u, i, j) until `budget_s` seconds have passed (or `max_steps` steps are done) — bench.py's CPU baseline for the
    VBPR leg and the full-size parity test's checker.  `params` maps Bi, Gu, Gi, Tu, E, Bp to arrays.  Returns
    (steps done, seconds[, the updated tables])."""
    import time

    import torch

    dt = torch.float
    F = torch.tensor(np.asarray(features, np.float32), dtype=dt)
    P = {n: torch.tensor(np.asarray(params[n], np.float32).reshape(-1, 1) if n == "Bp" else
                         np.asarray(params[n], np.float32), dtype=dt, requires_grad=True)
         for n in ("Bi", "Gu", "Gi", "Tu", "E", "Bp")}
    Bi, Gu, Gi, Tu, E, Bp = (P[n] for n in ("Bi", "Gu", "Gi", "Tu", "E", "Bp"))
    opt = torch.optim.Adam([Bi, Gu, Gi, Tu, E, Bp], lr=lr)

    def l2(*ts):
        return sum(t.pow(2).sum() for t in ts) / 2

    n, t0 = 0, time.time()
    while (n + 1) * batch_size <= len(u) and time.time() - t0 < budget_s and (max_steps is None or n < max_steps):
        a = n * batch_size
        bu, bi, bj = (torch.as_tensor(np.asarray(x[a:a + batch_size], np.int64)) for x in (u, i, j))
        gu, tu = Gu[bu], Tu[bu]
        beta_i, beta_j = Bi[bi], Bi[bj]
        gi, gj = Gi[bi], Gi[bj]
        feat_diff = F[bi] - F[bj]
        X = (beta_i - beta_j + (gu * (gi - gj)).sum(dim=1) + (tu * feat_diff.mm(E)).sum(dim=1) + feat_diff.mm(Bp))
        loss = -torch.nn.functional.logsigmoid(X).sum() + (l2(gu, gi, gj, tu) * lambda_w + l2(beta_i) * lambda_b
                                                         + l2(beta_j) * lambda_b / 10 + l2(E, Bp) * lambda_e)
        opt.zero_grad()
        loss.backward()
        opt.step()
        n += 1
    if return_params:
        return n, time.time() - t0, {name: t.detach().numpy().copy() for name, t in P.items()}
    return n, time.time() - t0


TABLES = ("Bi", "Gu", "Gi", "Tu", "E", "Bp")


def steps_f64(features, params, batches, lr, lambda_w, lambda_b, lambda_e, skip=None):
    """The minibatch step of VBPROracle.fit (recom_vbpr.py:242-262) in float64 over an explicit list of batches — the
    checker of the device's step at shapes and schedules the sampler never produces (ragged, tiny, i == j, ...).

    `batches` is a list of (u, i, j) arrays of any lengths; each batch is one Adam step and all of them form ONE
    continuing sequence (a device handle keeps Adam's step count across calls, so several calls equal one run over the
    concatenated list).  The gradient is torch autograd's; Adam is written out (torch.optim.Adam's single-tensor formula,
    dense: every row's moments decay, and a row with m = v = 0 stays exactly where it is) so that `skip = (table, row,
    t)` can withhold the update of one row of one table at batch index t (0-based) — the sensitivity control of the
    device tests.  `params` maps Bi, Gu, Gi, Tu, E, Bp to arrays (Bp of n_feat entries in any shape).
    Returns ({name: float64 table, Bp as a vector}, [NLL of every step]) with NLL = -sum logsigmoid(X) over the B x B
    broadcast entries (the device's `sum_nll`)."""
    import torch

    dt = torch.float64
    F = torch.tensor(np.asarray(features, np.float64))
    P = {n: torch.tensor(np.asarray(params[n], np.float64).reshape(-1, 1) if n == "Bp" else
                         np.asarray(params[n], np.float64), dtype=dt) for n in TABLES}
    M = {n: torch.zeros_like(P[n]) for n in TABLES}
    V = {n: torch.zeros_like(P[n]) for n in TABLES}
    b1, b2, eps = 0.9, 0.999, 1e-8

    def l2(*ts):
        return sum(t.pow(2).sum() for t in ts) / 2

    nll = []
    for t, (u, i, j) in enumerate(batches):
        bu, bi, bj = (torch.as_tensor(np.asarray(x, np.int64)) for x in (u, i, j))
        L = {n: P[n].clone().requires_grad_(True) for n in TABLES}
        Bi, Gu, Gi, Tu, E, Bp = (L[n] for n in TABLES)
        gu, tu = Gu[bu], Tu[bu]
        beta_i, beta_j = Bi[bi], Bi[bj]
        gi, gj = Gi[bi], Gi[bj]
        feat_diff = F[bi] - F[bj]
        # [B] + [B, 1]: the reference's B x B broadcast score
        X = (beta_i - beta_j + (gu * (gi - gj)).sum(dim=1) + (tu * feat_diff.mm(E)).sum(dim=1) + feat_diff.mm(Bp))
        ll = torch.nn.functional.logsigmoid(X).sum()
        loss = -ll + (l2(gu, gi, gj, tu) * lambda_w + l2(beta_i) * lambda_b + l2(beta_j) * lambda_b / 10
                      + l2(E, Bp) * lambda_e)
        grads = torch.autograd.grad(loss, [L[n] for n in TABLES])
        nll.append(-float(ll.detach()))
        step = t + 1
        step_size = lr / (1 - b1 ** step)
        bc2_sqrt = (1 - b2 ** step) ** 0.5
        for n, g in zip(TABLES, grads):
            p, m, v = P[n], M[n], V[n]
            keep = None
            if skip is not None and skip[0] == n and skip[2] == t:
                keep = (p[skip[1]].clone(), m[skip[1]].clone(), v[skip[1]].clone())
            m.lerp_(g, 1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            p.addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(eps), value=-step_size)
            if keep is not None:
                p[skip[1]], m[skip[1]], v[skip[1]] = keep
    return {n: (P[n].reshape(-1) if n == "Bp" else P[n]).numpy().copy() for n in TABLES}, nll
